"""GPU parity on circuits wider than a workgroup: verify_decide_kernel (buckler_verify.hip) gives each of
its 256 lanes a share of the constraints, the linear-check pairs and the pwEvals copy, and every circuit
of test_gpu_buckler_verify*.py fits in lanes 0..4.  Here the circuits of tests/buckler_wide_util.py
(pinned on the CPU by test_buckler_wide_ref.py) make every stride loop take a second and a third trip,
put pairs on the lanes that first compute a power of their own, leave checkers empty and fill every
lane's accumulator, at rank 128 throughout.  The verdict word, all eight sides and pwEvals, into buffers
pre-filled with -1, are compared bit for bit with tests/buckler_verify_ref.py through
VerifyPlan.checks_dev and checks_multi_dev.  The prover's kernels of the same programs
(LinCheckPlan.lin_check_dev, Circuit.eval_dev) are compared with R.linCheck and the C oracle."""
import functools

import numpy as np
import pytest

import ringo
from ringo import buckler
from tests import buckler_lin_ref as R
from tests import buckler_verify_ref as V
from tests import buckler_wide_util as W
from tests import synth_util as su

pytestmark = pytest.mark.gpu

RANK = W.RANK
JR = 4 * RANK + 3  # a multi-bit shift exponent
# synthetic moduli with no spare top bit and a supported limb count: where an unreduced sum would overflow
NOSPARE = sorted(k for k, v in su.SYNTH.items() if v["bits"] == 64 * v["limbs"] and v["limbs"] in (1, 2, 4, 7, 14))
WIDE = W.WIDE_FIELDS + NOSPARE[:1]
ALL_BITS = V.ARITH | V.LIN_REM | V.LIN | V.SUM_REM | V.SUM


@functools.lru_cache(maxsize=None)
def _ctx(key):
    q = su.modulus(key)
    return ringo.Field(q), R.Ref(q)


def _dev(a, dtype=np.uint64):
    import torch
    a = np.ascontiguousarray(a, dtype)
    return torch.from_numpy(a.view(np.int64) if dtype == np.uint64 else a).cuda()


def _filled(*shape):
    import torch
    return torch.full(shape, -1, dtype=torch.int64, device="cuda")


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def _scratch(nbytes):
    import torch
    return torch.empty(max(1, nbytes // 8), dtype=torch.int64, device="cuda")


def _device_checkers(F, rank, spec):
    out = []
    for s in spec:
        if s[0] == "ntt":
            out.append(buckler.NewNTTChecker(F, rank))
        elif s[0] == "aut":
            out.append(buckler.NewAutChecker(F, rank, s[1], s[2]))
        elif s[0] == "proj":
            out.append(buckler.ProjChecker(F, rank).SetXOF(s[1]))
        else:
            out.append(buckler.ProjRecomposeChecker(F, rank, s[1]))
    return out


def _constraints(F, ref, cons):
    """The restatement's term lists as the mirror's ArithmeticConstraints."""
    out = []
    for c in cons:
        ac = buckler.ArithmeticConstraint(F)
        for coeff, pw, ws in c:
            ac.AddTermWithConst(ref.arr([coeff])[0], pw, *ws)
        out.append(ac)
    return out


def _plan(F, ref, wc, jr, emb=RANK):
    """(VerifyPlan, device checkers) of a W.WideCircuit or W.WideLinProof."""
    lin, arith, sm = wc.cons() if hasattr(wc, "cons") else (wc.lin, None, None)
    chks, lp = [], None
    if lin is not None:
        chks = _device_checkers(F, RANK, wc.spec)
        lp = buckler.LinCheckPlan(F, RANK, emb, chks, lin)
    n_pw = getattr(wc, "nPw", 0)
    plan = buckler.VerifyPlan(F, RANK, jr, wc.wCnt, n_pw, lp, _constraints(F, ref, arith) if arith is not None else None,
                              _constraints(F, ref, sm) if sm is not None else None)
    return plan, chks


def _run(plan, ref, evals, pw, chal, mask_sums):
    """One rg_buckler_verify_checks_dev into buffers of -1 -> (verdict, sides, pwEvals) as host arrays."""
    L = plan.field.L
    d_pw = _dev(np.stack([ref.arr(v) for v in pw])) if plan.nPw else None
    d_verdict, d_sides = _filled(1), _filled(8, L)
    d_pwe = _filled(plan.nPw, L) if plan.nPw else None
    plan.checks_dev(_dev(ref.arr(evals)), d_pw, _dev(ref.arr(chal)), _dev(ref.arr(mask_sums)), d_verdict, d_sides,
                    d_pwe, _scratch(plan.scratch_bytes()))
    return int(_host(d_verdict)[0]), _host(d_sides), (_host(d_pwe) if plan.nPw else np.zeros((0, L), np.uint64))


def _same(ref, got, want, what=""):
    """(verdict, sides, pwEvals) from the device against the restatement's."""
    assert got[0] == want[0], (what, got[0], want[0])
    assert (got[1] == ref.arr(want[1])).all(), (what, "sides")
    assert got[2].shape[0] == len(want[2]) and (len(want[2]) == 0 or (got[2] == ref.arr(want[2])).all()), (what, "pw")


@functools.lru_cache(maxsize=None)
def _wide(key, proof_seed=0):
    """The wide circuit with one proof's inputs, and the verifier's own evaluations for them (read-only)."""
    _, ref = _ctx(key)
    wc = W.wide_circuit(ref, proof_seed)
    return wc, wc.own()


def _check(ref, plan, wc, own, jr, evals, ms, bits, what):
    """One device run against V.decide; the restatement's verdict is `bits`."""
    verdict, sides = wc.decide(jr, own, evals, ms)
    assert verdict == bits, (what, verdict, bits)
    got = _run(plan, ref, evals, wc.pw, wc.chal(), ms)
    _same(ref, got, (verdict, sides, own[2]), what)
    return got


# ---- the forged wide circuit ----------------------------------------------------------------------------
@pytest.mark.parametrize("key", WIDE)
def test_wide_circuit_accepted_and_unforged(key):
    """300 + 270 constraints, 600 pairs over six checkers (two empty), n_pw L words past 256: the forged
    proof is accepted at shift exponent 0 and at a multi-bit one; random evals set every bit and the
    sides still match."""
    F, ref = _ctx(key)
    wc, own = _wide(key)
    W.assert_wide_shape(wc)
    for jr in (RANK - 1, JR):
        plan, _ = _plan(F, ref, wc, jr)
        assert plan.n_evals == W.W_CNT + 9
        evals, ms, _ = wc.forge(jr, own)
        _check(ref, plan, wc, own, jr, evals, ms, 0, ("forged", jr))
    n = plan.n_evals
    rnd = W.rand_ints(ref.q, n + 2, np.random.default_rng(5))
    _check(ref, plan, wc, own, JR, rnd[:n], rnd[n:], ALL_BITS, "unforged")


@pytest.mark.parametrize("key", WIDE)
def test_wide_circuit_rejections(key):
    """Every one-change rejection of the forged proof gives its bits, sides included."""
    F, ref = _ctx(key)
    wc, own = _wide(key)
    plan, _ = _plan(F, ref, wc, JR)
    _, _, rej = wc.forge(JR, own)
    assert len(rej) == 10 and "shared_witness" in rej
    for name, (evals, ms, bits) in rej.items():
        _check(ref, plan, wc, own, JR, evals, ms, bits, name)


# ---- trip boundaries --------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", W.SPLITS, ids=lambda s: f"{s[0]}+{s[1]}")
@pytest.mark.parametrize("key", W.BOUNDARY_FIELDS)
def test_trip_boundaries(key, split):
    """nc0 + nc1 = 256 and 257 (all in one list, one constraint in the first list, a sum list that is
    there and empty) with 64, 65, 256 and 257 pairs: lane 64 with and without a pair beside its power,
    lane 0 with and without pair 256, a checker's first pair on each, an empty first and last checker."""
    F, ref = _ctx(key)
    assert sorted(sum(p) for p in W.BOUNDARY_PAIRS) == [64, 65, 256, 257]
    for npairs in W.BOUNDARY_PAIRS:
        wc = W.boundary_circuit(ref, split, npairs)
        lanes = W.lanes_of_pairs(npairs)
        assert lanes["empty"] and lanes["lane64"] == (lanes["n"] > 64) and lanes["second_trip"] == (lanes["n"] == 257)
        assert lanes["n"] == 64 or 64 in lanes["starts"]
        assert len(wc.arith) == split[0] and (wc.sum is None if split[1] is None else len(wc.sum) == split[1])
        assert len(wc.arith) + len(wc.sum or []) in (W.LANES, W.LANES + 1)
        own = wc.own()
        plan, _ = _plan(F, ref, wc, JR)
        evals, ms, rej = wc.forge(JR, own)
        _check(ref, plan, wc, own, JR, evals, ms, 0, (npairs, "forged"))
        for name, (e, m, bits) in rej.items():
            _check(ref, plan, wc, own, JR, e, m, bits, (npairs, name))


# ---- every lane's accumulator full -----------------------------------------------------------------------
@pytest.mark.parametrize("key", ["p63"] + NOSPARE)
def test_saturated_tree(key):
    """256 arithmetic and 511 sum constraints, each the constant q - 1: every lane enters the fold with
    q - 1 (or 2 (q - 1)), so every addition of every level wraps; on a modulus without a spare bit the
    unreduced sum does not fit the limbs."""
    F, ref = _ctx(key)
    q = ref.q
    wc = W.saturated_circuit(ref)
    assert (len(wc.arith), len(wc.sum)) == (W.LANES, 2 * W.LANES - 1) and wc.lin is None
    assert all(c == [(q - 1, None, [])] for c in wc.arith + wc.sum)
    own = wc.own()
    plan, _ = _plan(F, ref, wc, JR)
    evals, ms, rej = wc.forge(JR, own)
    _check(ref, plan, wc, own, JR, evals, ms, 0, "forged")
    for name, (e, m, bits) in rej.items():
        _check(ref, plan, wc, own, JR, e, m, bits, name)
    _check(ref, plan, wc, own, JR, [q - 1] * plan.n_evals, [q - 1] * 2, V.ARITH | V.SUM_REM | V.SUM, "all q - 1")


# ---- an honest prover's 257 pairs ------------------------------------------------------------------------
@pytest.mark.parametrize("key", W.HONEST_FIELDS)
def test_honest_wide_linear_check(key):
    """The proof R.linCheck makes of 257 honest pairs (two checkers empty, pair 256 alone on the last):
    the kernel's term_k bc^(n_pairs - k) over all lanes is the prover's Horner chain."""
    F, ref = _ctx(key)
    hp = W.honest_lin_proof(ref)
    lanes = W.lanes_of_pairs([len(p) for p in hp.lin])
    assert lanes["n"] == 257 and lanes["second_trip"] and lanes["lane64"] and lanes["empty"] == [1, 3]
    own = V.own_evals(ref, RANK, hp.x, hp.lc, hp.checkers, [])

    def check(plan, jr, evals, bits, what):
        verdict, sides = V.decide(ref, RANK, jr, hp.wCnt, hp.chal(), hp.mask_sums(), evals, own, hp.lin, None, None)
        assert verdict == bits, (what, verdict, bits)
        _same(ref, _run(plan, ref, evals, [], hp.chal(), hp.mask_sums()), (verdict, sides, []), what)

    for jr in (RANK - 1, RANK, JR):
        plan, _ = _plan(F, ref, hp, jr)
        assert plan.n_evals == hp.wCnt + 4
        check(plan, jr, hp.evals(jr), 0, ("honest", jr))
    for name, (evals, bits) in hp.perturbations(JR).items():
        check(plan, JR, evals, bits, name)


# ---- the batch entry -------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["p63", "zp880"])
def test_batch_of_wide_proofs(key):
    """Three proofs of the wide circuit in one call, a workgroup each: an accepted one, a rejection and
    random evals, each with its own challenges, public witnesses and XOF bytes.  Every word equals the
    restatement's for that proof and the single entry's."""
    F, ref = _ctx(key)
    L = F.L
    proofs = [_wide(key, s) for s in range(3)]
    wc0 = proofs[0][0]
    W.assert_wide_shape(wc0)
    plan, chks = _plan(F, ref, wc0, JR)
    assert plan.n_evals * L > W.LANES and plan.nPw * L > W.LANES  # the per-proof strides pass a workgroup's lanes
    items = []
    for slot, (wc, own) in enumerate(proofs):
        assert wc.cons() == wc0.cons()
        evals, ms, rej = wc.forge(JR, own, seed=slot)
        bits = 0
        if slot == 1:
            evals, ms, bits = rej["shared_witness"]
        elif slot == 2:
            rnd = W.rand_ints(ref.q, plan.n_evals + 2, np.random.default_rng(7))
            evals, ms, bits = rnd[:-2], rnd[-2:], ALL_BITS
        verdict, sides = wc.decide(JR, own, evals, ms)
        assert verdict == bits
        items.append((wc, evals, ms, (verdict, sides, own[2])))
    assert len({tuple(it[0].chal()) for it in items}) == 3 and len({it[0].xof for it in items}) == 3  # each its own
    assert items[0][0].pw != items[1][0].pw != items[2][0].pw
    n = len(items)
    d_verdict, d_sides, d_pwe = _filled(n), _filled(n, 8, L), _filled(n, plan.nPw, L)
    xof = np.frombuffer(b"".join(wc.xof for wc, _, _, _ in items), np.uint8).copy()
    plan.checks_multi_dev(n, _dev(np.stack([ref.arr(e) for _, e, _, _ in items])),
                          _dev(np.stack([np.stack([ref.arr(v) for v in wc.pw]) for wc, _, _, _ in items])),
                          _dev(xof, np.uint8), _dev(np.stack([ref.arr(wc.chal()) for wc, _, _, _ in items])),
                          _dev(np.stack([ref.arr(m) for _, _, m, _ in items])), d_verdict, d_sides, d_pwe,
                          _scratch(plan.scratch_bytes_multi(n)))
    batch = (_host(d_verdict), _host(d_sides), _host(d_pwe))
    for i, (wc, evals, ms, want) in enumerate(items):
        _same(ref, (int(batch[0][i]), batch[1][i], batch[2][i]), want, ("batch", i))
        chks[2].SetXOF(wc.xof)  # the single entry reads the checker's own matrix
        single = _run(plan, ref, evals, wc.pw, wc.chal(), ms)
        _same(ref, single, want, ("single", i))
        assert single[0] == int(batch[0][i]) and (single[1] == batch[1][i]).all() and (single[2] == batch[2][i]).all()


# ---- the prover's kernels on the same programs -----------------------------------------------------------
@pytest.mark.parametrize("key", W.HONEST_FIELDS)
def test_lin_check_dev_257_pairs(key):
    """lin_kernel on 257 pairs with two empty checkers: quo, remLo, remHi and remPoly[0] (the mask sum)
    equal R.linCheck."""
    F, ref = _ctx(key)
    L = F.L
    hp = W.honest_lin_proof(ref)
    assert [len(p) for p in hp.lin] == W.HONEST_PAIRS and W.HONEST_PAIRS[1] == W.HONEST_PAIRS[3] == 0
    emb, circ = hp.emb, hp.circ
    plan = buckler.LinCheckPlan(F, RANK, emb, _device_checkers(F, RANK, hp.spec), hp.lin)
    dquo, dlo, dhi = _filled(RANK, L), _filled(RANK - 1, L), _filled(JR, L)
    scr = _scratch(plan.scratch_bytes())
    plan.lin_check_dev(_dev(ref.arr([hp.bcL])[0]), _dev(ref.arr([hp.lc])[0]), _dev(ref.arr(hp.linMask)),
                       _dev(np.stack([ref.arr(p) for p in circ["wEcdNTT"]])), hp.wCnt, JR, dquo, dlo, dhi, scr)
    want_hi = [0] * (JR - (RANK - 1)) + list(hp.linLo)  # prover.go:450-456
    for got, want in ((dquo, hp.linQuo), (dlo, hp.linLo), (dhi, want_hi)):
        assert (_host(got) == ref.arr(want)).all()
    o = plan.rem_offset_words()
    assert (_host(scr)[o:o + L] == ref.arr([hp.linMaskSum])[0]).all() and hp.rem[0] == hp.linMaskSum


@pytest.mark.parametrize("key", WIDE)
def test_eval_circuit_dev_300_constraints(key):
    """circuit_kernel on the wide circuit's arithmetic list (300 constraints over 600 witnesses and n_pw
    public witnesses) against the C oracle's buckler_eval_circuit."""
    F, ref = _ctx(key)
    L = F.L
    wc, _ = _wide(key)
    assert len(wc.arith) == W.NC0 > W.LANES
    rng = np.random.default_rng(11)
    w = su.rand_residues(ref.q, L, wc.wCnt * RANK, rng).reshape(wc.wCnt, RANK, L)
    pw = su.rand_residues(ref.q, L, wc.nPw * RANK, rng).reshape(wc.nPw, RANK, L)
    w[0], w[1] = su.limbs_of(ref.q - 1, L), 0
    bc = su.rand_residues(ref.q, L, 1, rng)[0]
    cons = [[(ref.arr([coeff])[0], p, ws) for coeff, p, ws in c] for c in wc.arith]
    want = ref.cf.buckler_eval_circuit(cons, bc, w, pw)
    circ = buckler.Circuit(F, _constraints(F, ref, wc.arith))
    assert circ.n_w <= wc.wCnt and circ.n_pw == wc.nPw
    d_out = _filled(RANK + 1, L)
    circ.eval_dev(RANK, _dev(bc), _dev(w), wc.wCnt, _dev(pw), wc.nPw, d_out)
    got = _host(d_out)
    assert (got[:RANK] == want).all() and (got[RANK] == np.uint64(2 ** 64 - 1)).all()
