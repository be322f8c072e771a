"""GPU parity for the Buckler prover's device work (rg_buckler_encode_dev: buckler.hip
embed_kernel after the cyclic InvNTT; rg_buckler_eval_circuit[_dev]: circuit_kernel) at the inputs
where the kernels can be wrong while test_gpu_buckler.py passes: every limb count with and
without a spare top bit and the 64-bit single-word moduli (synth_util.ALL), and extremal data
instead of random data.  Bit-exact against the C oracle, which test_oracle_polyops_synthetic.py
pins on these moduli and inputs.

Encode / RandEncode: witness rows whose InvNTT is all q - 1 or all 0 besides q - 1 everywhere and
a random row; per row the draws that make the fix-up coeff[0] -= r land on 0 (r = coeff[0]), do
nothing (r = 0), wrap (r = q - 1, r = coeff[0] + 1); batch 1 (InvNTT in place in the output row,
src == nullptr) and batch 4 (through scratch); the output is poisoned first, so the zero fill
above rank, the slot of r and the row past the batch are all checked.

evalCircuit: witnesses all q - 1 and all 0, a public witness alternating 0 / q - 1, coefficients 0
and q - 1, a pair of terms cancelling through exactly q, an empty constraint, a constant; batchConst
0, raw 1, q - 1 and random; one lane (rank 1), a partly filled workgroup, a full one, one lane of
a second.  A second circuit of two cancelling constraints takes pOut's accumulation through
exactly q, the one place where an unreduced q would reach the output."""
import numpy as np
import pytest

import ringo
from ringo import buckler
from tests import synth_util as su

pytestmark = pytest.mark.gpu

POISON = 0x5a5a5a5a5a5a5a5a


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to("cuda")


def _h(t):
    return t.cpu().numpy().view(np.uint64)


def _label(r):
    return "none" if r is None else hex(su.from_limbs(r[None])[0])


@pytest.mark.parametrize("rank,emb", [(8, 9), (256, 512), (4096, 8192), (256, 256)])
@pytest.mark.parametrize("name", su.ALL)
def test_encode_coeff0_edges(name, rank, emb):
    import torch
    q = su.modulus(name)
    F = ringo.Field(q)
    cf = su.cfield(name)
    L = F.L
    rng = np.random.default_rng(rank + emb)
    enc = buckler.NewEncoder(F, rank, emb)
    rows = su.encode_rows(cf, q, rank, rng)
    nrow = len(rows)
    c0 = [su.from_limbs(cf.buckler_encode(v, emb)[:1])[0] for v in rows]
    assert c0[1] == q - 1 and c0[2] == 0
    # draws[k][i]: the k-th kind of draw for row i; RandEncode needs coefficient `rank`
    draws = list(zip(*[su.encode_rands(q, L, c, rng) for c in c0]))
    if emb == rank:
        draws = draws[-1:]
    dv = _t(rows)
    scr = torch.full((max(1, enc.scratch_bytes(nrow) // 8),), POISON, dtype=torch.int64, device="cuda")
    for rs in draws:
        rand = rs[0] is not None
        want = [cf.buckler_encode(rows[i], emb, rnd=rs[i]) for i in range(nrow)]
        for i in range(nrow):
            assert (want[i][rank + rand:] == 0).all() and (not rand or (want[i][rank] == rs[i]).all())
        dr = _t(np.stack(rs)) if rand else None
        # batch 4 through scratch, then each row alone (in place); one row past the batch stays poison
        for first, batch in [(0, nrow)] + [(i, 1) for i in range(nrow)]:
            dout = torch.full((batch + 1, emb, L), POISON, dtype=torch.int64, device="cuda")
            enc.encode_dev(dout, dv[first:first + batch], batch, d_rand=dr[first:first + batch] if rand else None,
                           d_scratch=scr if batch > 1 else None)
            torch.cuda.synchronize()
            got = _h(dout)
            for b in range(batch):
                i = first + b
                where = (name, rank, emb, su.ENCODE_ROWS[i], _label(rs[i]), "batch", batch)
                assert (got[b, rank + rand:] == 0).all(), where + ("zero fill",)
                assert not rand or (got[b, rank] == rs[i]).all(), where + ("coeff[rank]",)
                assert (got[b] == want[i]).all(), where
            assert (got[batch] == np.uint64(POISON)).all(), (name, rank, emb, batch, "wrote past the batch")
    assert (_h(dv) == rows).all()


def _constraints(F, cons):
    out = []
    for terms in cons:
        c = buckler.ArithmeticConstraint(F)
        for coeff, p, ws in terms:
            c.AddTermWithConst(coeff, p, *ws)
        out.append(c)
    return out


@pytest.mark.parametrize("name", su.ALL)
def test_eval_circuit_edge_circuit(name):
    import torch
    q = su.modulus(name)
    F = ringo.Field(q)
    cf = su.cfield(name)
    L = F.L
    rng = np.random.default_rng(21)
    bcs = su.batch_consts(q, L, rng)
    for what, cons in (("edge circuit", su.circuit_terms(q, L, rng)), ("cancelling", su.circuit_cancel_terms(q, L, rng))):
        gcons = _constraints(F, cons)
        circ = buckler.Circuit(F, gcons)
        for rank in (1, 255, 256, 257):
            w, pw = su.circuit_witnesses(q, L, rank, rng)
            dw, dpw = _t(w), _t(pw)
            for k, bc in enumerate(bcs):
                want = cf.buckler_eval_circuit(cons, bc, w, pw)
                assert what == "edge circuit" or (want == 0).all()
                got = buckler.EvalCircuit(F, bc, gcons, w, pw)
                assert got.IsNTT and (got.Coeffs == want).all(), (name, what, rank, k, "host form")
                dout = torch.full((rank + 1, L), POISON, dtype=torch.int64, device="cuda")
                circ.eval_dev(rank, _t(bc), dw, su.CIRCUIT_NW, dpw, su.CIRCUIT_NPW, dout)
                torch.cuda.synchronize()
                g = _h(dout)
                assert (g[:rank] == want).all(), (name, what, rank, k, "device form")
                assert (g[rank] == np.uint64(POISON)).all(), (name, what, rank, k, "wrote past d_out")
