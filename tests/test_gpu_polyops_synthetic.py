"""GPU parity for the bigpoly evaluators (rg_poly_*: ModSwitchTo, AutTo, QuoRemByVanishing,
Poly.Evaluate, the batched Evaluate) at the inputs where the kernels can be wrong while
test_gpu_polyops.py and test_gpu_poly_evaluate_batch.py pass: moduli without a spare top bit and
the 64-bit single-word ones (tests/golden/synthetic_fields.json), extremal polynomials, and for
ModSwitch the real rounding ties and full-width quotients.  Bit-exact against the C oracle, which
test_oracle_polyops_synthetic.py pins on these moduli and inputs; ModSwitch against
pyref.mod_switch's big-integer restatement.

ModSwitch (poly_ops.hip modswitch_kernel / ms_divmod) is called through rg_poly_modswitch with an
explicit word count w, which the Python mirror never leaves above the minimum.  Per field and per
qBig of synth_util.modswitch_qbigs (1, 2, 3, word boundaries, 2^510, 2^511 - 1, q - 1, q + 1,
2q + 1, q):
  * narrow, at the minimal w and at w = 8 (nqb < w: the reciprocal of qBig is formed from fewer
    words than the kernel divides by): 0, 1, -1, the tie family that puts |p| q mod qBig on both
    rounding thresholds and one step either side for both signs, values beyond qBig;
  * carry, at the minimal w and at w = 8: values on a threshold whose quotient ends in one or two
    words of ones, so the rounding ++Q carries through them;
  * wide, at w = 8: +-(2^511 - 1), -2^511, up to 510 random bits, so the second Barrett division
    (by q, reciprocal mu2) sees a multiword quotient, its correction loop and the carry of ++Q."""
import math

import numpy as np
import pytest

import coracle as co
import pyref
import ringo
from ringo import _lib
from tests import synth_util as su
from tests.test_gpu_poly_evaluate_batch import T, _run

pytestmark = pytest.mark.gpu

RG_ERR_INVALID = -1
POISON = 0x5a5a5a5a5a5a5a5a


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to("cuda")


def _h(t):
    return t.cpu().numpy().view(np.uint64)


# ---- ModSwitch ----------------------------------------------------------------------------------
def _modswitch(F, ps, w, qbig):
    """rg_poly_modswitch on Python ints at word count w -> plain residues (out of Montgomery form)."""
    words = su.signed_words(ps, w)
    qw = su.limbs_of(qbig, w)
    out = np.full((len(ps), F.L), POISON, np.uint64)
    _lib.check(_lib.lib().rg_poly_modswitch(F.h, len(ps), _lib.ptr(words), w, _lib.ptr(qw), _lib.ptr(out)))
    rinv = pow(1 << (64 * F.L), -1, F.q)
    raw = co.from_limbs(out)
    assert max(raw) < F.q
    return [x * rinv % F.q for x in raw]


@pytest.mark.parametrize("name", su.MS)
def test_mod_switch_ties_and_wide_quotients(name):
    q = su.modulus(name)
    F = ringo.Field(q)
    rng = np.random.default_rng(q % 1000003)
    qbigs = su.modswitch_qbigs(q)
    assert len(qbigs) == (12 if name in ("zp880", "s896_top") else 16)
    with_ties = 0
    for qbig in qbigs:
        narrow, wide, nties = su.modswitch_inputs(q, qbig, rng)
        assert nties or math.gcd(q, qbig) != 1
        with_ties += nties > 0
        for what, ps in (("narrow", narrow), ("carry", su.modswitch_carries(q, qbig))):
            want = pyref.mod_switch(ps, qbig, q)
            for w in sorted({su.modswitch_min_words(ps, qbig), 8}) if ps else ():
                got = _modswitch(F, ps, w, qbig)
                bad = [hex(p) for p, g, x in zip(ps, got, want) if g != x]
                assert not bad, (name, hex(qbig), what, w, bad[:4])
        got = _modswitch(F, wide, 8, qbig)
        bad = [hex(p) for p, g, x in zip(wide, got, pyref.mod_switch(wide, qbig, q)) if g != x]
        assert not bad, (name, hex(qbig), "wide", bad[:4])
    assert with_ties >= (12 if name in ("zp880", "s896_top") else 14)


def test_mod_switch_rejects_bad_word_counts_and_moduli():
    F = ringo.Field(su.modulus("s64_lo"))
    lib = _lib.lib()
    out = np.full((2, 1), POISON, np.uint64)

    def call(w, qw):
        p = np.zeros((2, max(w, 1)), np.uint64)
        return lib.rg_poly_modswitch(F.h, 2, _lib.ptr(p), w, _lib.ptr(np.array(qw, np.uint64)), _lib.ptr(out))

    assert call(9, [97] + [0] * 8) == RG_ERR_INVALID          # wider than the kernel's arrays
    assert call(0, [97]) == RG_ERR_INVALID
    assert call(3, [0, 0, 0]) == RG_ERR_INVALID               # qBig = 0
    assert call(2, [5, 1 << 63]) == RG_ERR_INVALID            # qBig negative as a 2-word value
    assert call(8, [0] * 7 + [1 << 63]) == RG_ERR_INVALID
    assert (out == np.uint64(POISON)).all()
    assert call(2, [97, 0]) == 0 and (out == 0).all()         # the handle is live: p = 0 switches to 0


# ---- AutTo --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", su.ALL)
def test_aut_structured_inputs_all_ranks(name):
    """Coefficient domain (a signed scatter: f_neg of a zero coefficient must give 0, of q - 1 raw
    1) and NTT domain (a gather through brv_n, whose logn == 0 case is rank 1), batch 3: ranks 1
    and 2 (a single partly filled workgroup), 256 (3 x 256 lanes: three full workgroups), 512,
    4096; indices on both sides of N and of 2N, negative and beyond 2N."""
    q = su.modulus(name)
    F = ringo.Field(q)
    cf = su.cfield(name)
    L, B = F.L, 3
    lib = _lib.lib()
    rng = np.random.default_rng(11)
    for N in (1, 2, 256, 512, 4096):
        # two batches of 3: alternating 0 / q - 1, zero, all q - 1; then three random polynomials
        host = su.plain_batch(q, L, N, ["alt_0_qm1", "zero", "all_qm1"], 2 * B, rng)
        d = _t(host)
        out = _t(np.full((B + 1, N, L), POISON, np.uint64))
        for idx in su.aut_indices(N):
            for ntt in (False, True):
                for first in (0, B):
                    out.fill_(POISON)
                    _lib.check(lib.rg_poly_aut_dev(F.h, N, idx, int(ntt), out.data_ptr(), d[first].data_ptr(), B, None))
                    got = _h(out)
                    for b in range(B):
                        assert (got[b] == cf.aut(host[first + b], idx, ntt)).all(), (name, N, idx, ntt, first + b)
                    assert (got[B] == np.uint64(POISON)).all(), (name, N, idx, ntt, "wrote past d_out")
        assert lib.rg_poly_aut_dev(F.h, N, 1, 0, d.data_ptr(), d.data_ptr(), B, None) == RG_ERR_INVALID
        assert (_h(d) == host).all()


# ---- QuoRemByVanishing --------------------------------------------------------------------------
@pytest.mark.parametrize("name", su.ALL)
def test_quorem_structured_inputs(name):
    """M = 1 (one lane per polynomial, an (N - 1)-long chain of f_add), M = N - 1, N and N + 1
    (the trivial kernel from M = N), a non-divisor, a non-power-of-two rank; on all q - 1 every
    suffix sum sits on f_add's reduction edge.  Then once more with rem aliasing p."""
    import torch
    q = su.modulus(name)
    F = ringo.Field(q)
    cf = su.cfield(name)
    L, B = F.L, 3
    lib = _lib.lib()
    rng = np.random.default_rng(12)
    for rank, M in ((256, 1), (256, 255), (256, 256), (256, 257), (256, 100), (4096, 1), (1000, 7)):
        host = su.plain_batch(q, L, rank, ["all_qm1", "alt_0_qm1"], B, rng)
        want = [cf.quorem_vanishing(host[b], M) for b in range(B)]
        d = _t(host)
        quo = _t(np.full((B + 1, rank, L), POISON, np.uint64))
        rem = quo.clone()
        _lib.check(lib.rg_poly_quorem_vanishing_dev(F.h, rank, M, quo.data_ptr(), rem.data_ptr(), d.data_ptr(), B, None))
        gq, gr = _h(quo), _h(rem)
        for b in range(B):
            assert (gq[b] == want[b][0]).all() and (gr[b] == want[b][1]).all(), (name, rank, M, b)
        assert (gq[B] == np.uint64(POISON)).all() and (gr[B] == np.uint64(POISON)).all(), (name, rank, M)
        assert (_h(d) == host).all()
        quo.fill_(POISON)
        _lib.check(lib.rg_poly_quorem_vanishing_dev(F.h, rank, M, quo.data_ptr(), d.data_ptr(), d.data_ptr(), B, None))
        torch.cuda.synchronize()
        assert torch.equal(quo, _t(gq)) and (_h(d) == gr[:B]).all(), (name, rank, M, "rem aliasing p")


# ---- Poly.Evaluate, the single Horner tree --------------------------------------------------------
@pytest.mark.parametrize("name", su.ALL)
def test_evaluate_edge_points(name):
    """One chunk, a full chunk, a chunk and one coefficient, a full second level, a third level of
    one value; at 0 (only p_0 survives), raw 1 and q - 1, R mod q (x = 1: the plain sum of the
    coefficients, n (q - 1) on the all-(q - 1) polynomial) and a random point."""
    q = su.modulus(name)
    F = ringo.Field(q)
    cf = su.cfield(name)
    rng = np.random.default_rng(13)
    pts = su.eval_points(q, F.L, rng)
    for n in (1, 64, 65, 4096, 4097):
        for k, coeffs in enumerate(su.plain_batch(q, F.L, n, ["all_qm1"], 2, rng)):
            p = ringo.Poly(F, n, False, coeffs)
            for i, x in enumerate(pts):
                assert (p.Evaluate(x) == cf.evaluate(coeffs, x)).all(), (name, n, "all_qm1" if k == 0 else "random", i)


# ---- rg_poly_evaluate_batch ----------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 257, T + 1])
@pytest.mark.parametrize("name", [n for n in su.ALL if n in su.SYNTH] + ["zp110"])
def test_evaluate_batch_synthetic_fields(name, n):
    """test_gpu_poly_evaluate_batch.py's case (the all-(q - 1) polynomial, the points 0, 1, q - 1,
    gaps that must not be read, the slot past d_out) on the moduli it leaves out: a partial lane
    row either side of 256 and the first two-tile size."""
    _run(name, n, {name: su.modulus(name)})
