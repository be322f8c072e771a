"""GPU parity: the Buckler verifier's checks on the device (rg_buckler_verifier_*,
rg_buckler_verify_checks*; buckler/verifier.go:178-315), bit for bit against tests/buckler_verify_ref.py
(pinned on the CPU by test_buckler_verify_ref.py): the verdict word, all eight sides and pwEvals,
into buffers pre-filled with -1, through the `_dev` entry, the host form and the Python mirror."""
import functools

import numpy as np
import pytest

import ringo
from ringo import _lib, bigpoly, buckler
from ringo.bigpoly import RingoPanic
from tests import buckler_lin_ref as R
from tests import buckler_verify_ref as V
from tests import synth_util as su
from tests.buckler_verify_util import HonestProof, perturbations

pytestmark = pytest.mark.gpu

GOLD = ["p63", "mult_zp", "jindo_zp", "zp440", "zp880"]  # 1, 2, 4, 7 and 14 limbs
# synthetic moduli with no spare top bit and a supported limb count: where an unreduced sum would overflow
NOSPARE = sorted(k for k, v in su.SYNTH.items() if v["bits"] == 64 * v["limbs"] and v["limbs"] in (1, 2, 4, 7, 14))
# 128: the projection checker's minimum; 8192: two tiles of the batched evaluate's 4096
SHAPES = [(k, r) for k in GOLD for r in (128, 256)] + [(k, 128) for k in NOSPARE] + [("p63", 8192), ("jindo_zp", 8192)]
ALL = (True, True, True)


@functools.lru_cache(maxsize=None)
def _ctx(key):
    q = su.modulus(key)
    return ringo.Field(q), R.Ref(q)


@functools.lru_cache(maxsize=None)
def _proof(key, rank, two_pairs=False):
    """The honest proof and the evaluations of the verifier's own vectors, computed once and shared
    (read-only)."""
    _, ref = _ctx(key)
    hp = HonestProof(ref, rank, seed=rank + len(key), two_pairs=two_pairs)
    return hp, V.own_evals(ref, rank, hp.x, hp.lc, hp.checkers, hp.pw)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


def _filled(*shape):
    import torch
    return torch.full(shape, -1, dtype=torch.int64, device="cuda")


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


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


def _plan(key, hp, jindo_rank, has=ALL, n_pw=3, emb=None):
    F, ref = _ctx(key)
    lin = None
    if has[0]:
        lin = buckler.LinCheckPlan(F, hp.rank, emb or hp.rank, _device_checkers(F, hp.rank, hp.spec), hp.lin)
    return buckler.VerifyPlan(F, hp.rank, jindo_rank, hp.wCnt, n_pw, lin,
                              _constraints(F, ref, hp.arith) if has[1] else None,
                              _constraints(F, ref, hp.sum) if has[2] else None)


def _run(plan, ref, evals, pw, chal, mask_sums, stream=None):
    """One rg_buckler_verify_checks_dev into buffers of -1 -> (verdict, sides, pwEvals) as host arrays."""
    import torch
    L = plan.field.L
    d_pw = _dev(np.stack([ref.arr(v) for v in pw])) if plan.nPw else None
    d_verdict, d_sides = _filled(1), _filled(8, L)
    d_pwe = _filled(plan.nPw, L) if plan.nPw else None
    scr = torch.empty(max(1, plan.scratch_bytes() // 8), dtype=torch.int64, device="cuda")
    plan.checks_dev(_dev(ref.arr(evals)), d_pw, _dev(ref.arr(chal)), _dev(ref.arr(mask_sums)), d_verdict, d_sides,
                    d_pwe, scr, stream=stream)
    return int(_host(d_verdict)[0]), _host(d_sides), (_host(d_pwe) if plan.nPw else np.zeros((0, L), np.uint64))


def _same(ref, got, want, what=""):
    """(verdict, sides, pwEvals) from the device against the restatement's."""
    assert got[0] == want[0], (what, got[0], want[0])
    assert (got[1] == ref.arr(want[1])).all(), (what, "sides")
    assert got[2].shape[0] == len(want[2]) and (len(want[2]) == 0 or (got[2] == ref.arr(want[2])).all()), (what, "pw")


def _want(ref, hp, jindo_rank, own, evals, mask_sums, chal, cons):
    verdict, sides = V.decide(ref, hp.rank, jindo_rank, hp.wCnt, chal, mask_sums, evals, own, *cons)
    return verdict, sides, own[2]


@pytest.mark.parametrize("key,rank", SHAPES)
def test_accept_and_reject(key, rank):
    """The honest proof at jindo_rank = rank - 1, rank and 4 rank + 3 (shift exponent 0, 1 and a
    multi-bit one) gives verdict 0, and every one-change rejection the restatement's bits: exactly
    the ones tests/buckler_verify_util.perturbations lists."""
    F, ref = _ctx(key)
    hp, own = _proof(key, rank)
    cons = hp.cons()
    for jr in (rank - 1, rank, 4 * rank + 3):
        plan = _plan(key, hp, jr)
        assert plan.n_evals == hp.wCnt + 9
        evals = hp.evals(jr)
        want = _want(ref, hp, jr, own, evals, hp.mask_sums(), hp.chal(), cons)
        assert want[0] == 0
        _same(ref, _run(plan, ref, evals, hp.pw, hp.chal(), hp.mask_sums()), want, ("honest", jr))
    names = None if rank < 8192 else ("lin_remlo", "sum_quo", "shared_witness", "pw0", "eval_point")
    for jr in ((rank - 1, 4 * rank + 3) if rank == 128 else (4 * rank + 3,)):
        plan = _plan(key, hp, jr)
        for name, (evals, ms, pw, ch, bits) in perturbations(hp, jr).items():
            if names and name not in names:
                continue
            o = own
            if name.startswith("pw"):
                o = (own[0], own[1], V.own_evals(ref, rank, ch[0], ch[3], None, pw)[2])
            elif name == "eval_point":
                o = V.own_evals(ref, rank, ch[0], ch[3], hp.checkers, pw)
            want = _want(ref, hp, jr, o, evals, ms, ch, cons)
            assert want[0] == bits, (name, want[0], bits)
            _same(ref, _run(plan, ref, evals, pw, ch, ms), want, (name, jr))


@pytest.mark.parametrize("key", GOLD)
def test_host_form_and_mirror(key):
    """rg_buckler_verify_checks and buckler.VerifyChecks: the honest proof and one rejection."""
    F, ref = _ctx(key)
    rank, jr = 128, 4 * 128 + 3
    hp, own = _proof(key, rank)
    plan = _plan(key, hp, jr)
    pwa = np.stack([ref.arr(v) for v in hp.pw])
    for name in ("honest", "lin_remlo"):
        evals, ms, pw, ch, _ = perturbations(hp, jr)[name] if name != "honest" else (
            hp.evals(jr), hp.mask_sums(), hp.pw, hp.chal(), 0)
        want = _want(ref, hp, jr, own, evals, ms, ch, hp.cons())
        _same(ref, plan.checks(ref.arr(evals), pwa, ref.arr(ch), ref.arr(ms)), want, name)
        got = buckler.VerifyChecks(F, rank, jr, hp.wCnt, ref.arr(ch), ref.arr(ms), ref.arr(evals), pwa,
                                   _device_checkers(F, rank, hp.spec), hp.lin, _constraints(F, ref, hp.arith),
                                   _constraints(F, ref, hp.sum))
        _same(ref, got, want, name)
    assert (buckler.VERIFY_ARITH, buckler.VERIFY_LIN_REM, buckler.VERIFY_LIN, buckler.VERIFY_SUM_REM,
            buckler.VERIFY_SUM) == (V.ARITH, V.LIN_REM, V.LIN, V.SUM_REM, V.SUM)


HANDLES = [("lin", (True, False, False), 3), ("arith", (False, True, False), 3), ("sum", (False, False, True), 3),
           ("lin_no_pw", (True, False, False), 0), ("arith_sum", (False, True, True), 2)]


@pytest.mark.parametrize("key", ["p63", "jindo_zp", "zp880"])
@pytest.mark.parametrize("name,has,n_pw", HANDLES)
def test_handles_with_fewer_checks(key, name, has, n_pw):
    """Each check alone, in its own pf.Evals layout: the absent checks' sides are zero and their bits
    stay clear even when every evaluation is wrong.  lin_no_pw: n_pw = 0 and d_pw = NULL."""
    F, ref = _ctx(key)
    rank, jr = 128, 128
    hp, own = _proof(key, rank)
    plan = _plan(key, hp, jr, has, n_pw)
    lay = V.layout(hp.wCnt, *has)
    assert plan.n_evals == lay["n"]
    pw = hp.pw[:n_pw]
    o = (own[0] if has[0] else None, own[1] if has[0] else [], own[2][:n_pw])
    evals = hp.evals(jr, *has)
    want = _want(ref, hp, jr, o, evals, hp.mask_sums(), hp.chal(), hp.cons(*has))
    assert want[0] == 0
    _same(ref, _run(plan, ref, evals, pw, hp.chal(), hp.mask_sums()), want, name)
    bad = [(e + 1) % ref.q for e in evals]
    want = _want(ref, hp, jr, o, bad, hp.mask_sums(), hp.chal(), hp.cons(*has))
    present = (V.LIN_REM | V.LIN if has[0] else 0) | (V.ARITH if has[1] else 0) | (V.SUM_REM | V.SUM if has[2] else 0)
    assert want[0] & ~present == 0 and want[0] != 0
    _same(ref, _run(plan, ref, bad, pw, hp.chal(), hp.mask_sums()), want, name + " bad")


@pytest.mark.parametrize("key", ["p63", "jindo_zp"])
def test_two_pairs_on_one_checker(key):
    """Five pairs over four checkers: the chain's powers of batchConst run to 5."""
    F, ref = _ctx(key)
    rank, jr = 128, 4 * 128 + 3
    hp, own = _proof(key, rank, True)
    assert [len(p) for p in hp.lin] == [2, 1, 1, 1]
    plan = _plan(key, hp, jr, emb=4 * rank)  # a linear check shared with the prover: its embedding rank is not read
    for name in ("honest", "shared_witness", "lin_quo"):
        evals, ms, pw, ch, bits = perturbations(hp, jr)[name] if name != "honest" else (
            hp.evals(jr), hp.mask_sums(), hp.pw, hp.chal(), 0)
        want = _want(ref, hp, jr, own, evals, ms, ch, hp.cons())
        assert want[0] == bits
        _same(ref, _run(plan, ref, evals, pw, ch, ms), want, name)


@pytest.mark.parametrize("key", GOLD + NOSPARE[:1])
def test_edge_inputs(key):
    """evalPoint = 0, 1 and q - 1 (as Montgomery elements), batchConst = 0 and all-zero evals: the
    verdict is whatever the restatement says, sides and pwEvals included."""
    F, ref = _ctx(key)
    rank, jr = 128, 4 * 128 + 3
    hp, _ = _proof(key, rank)
    plan = _plan(key, hp, jr)
    one = ref.set_uint64(1)
    cases = {f"x={n}": ([x] + hp.chal()[1:], hp.evals(jr)) for n, x in (("0", 0), ("1", one), ("-1", ref.q - one))}
    cases["bc=0"] = ([hp.x, 0, 0, hp.lc, 0], hp.evals(jr))
    cases["evals=0"] = (hp.chal(), [0] * plan.n_evals)
    cases["all=0"] = ([0] * 5, [0] * plan.n_evals)
    for name, (ch, evals) in cases.items():
        for ms in (hp.mask_sums(), [0, 0]):
            want = V.verify(ref, rank, jr, hp.wCnt, ch, ms, evals, hp.pw, hp.checkers, *hp.cons())
            _same(ref, _run(plan, ref, evals, hp.pw, ch, ms), want, name)
    # all-zero evals and mask sums: the lin and sum identities read 0 = 0; the arithmetic circuit
    # keeps its constant term k2 * bc, so it fails unless bc = 0
    v0 = V.verify(ref, rank, jr, hp.wCnt, hp.chal(), [0, 0], [0] * plan.n_evals, hp.pw, hp.checkers, *hp.cons())[0]
    assert v0 == V.ARITH
    assert V.verify(ref, rank, jr, hp.wCnt, [0] * 5, [0, 0], [0] * plan.n_evals, hp.pw, hp.checkers, *hp.cons())[0] == 0


def test_two_streams_share_one_verifier():
    """Two calls in flight on two streams with one handle (own scratch and outputs each)."""
    import torch
    key, rank, jr = "jindo_zp", 128, 128
    F, ref = _ctx(key)
    hp, own = _proof(key, rank)
    plan = _plan(key, hp, jr)
    good = hp.evals(jr)
    bad, ms, pw, ch, bits = perturbations(hp, jr)["sum_remlo"]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = [_run(plan, ref, e, hp.pw, hp.chal(), hp.mask_sums(), stream=s) for s, e in zip(streams, (good, bad))]
    for g, e in zip(got, (good, bad)):
        _same(ref, g, _want(ref, hp, jr, own, e, hp.mask_sums(), hp.chal(), hp.cons()))
    assert got[0][0] == 0 and got[1][0] == bits


def test_prover_and_verifier_both_on_the_device():
    """The proof from the device prover entries (sumcheck_mask_dev, LinCheckPlan.lin_check_dev,
    Circuit.eval_dev, check_finish_dev, evaluate_batch_dev) straight into the device verifier: no
    value crosses the host between them except the challenges."""
    import torch
    key, rank = "jindo_zp", 128
    jr = 4 * rank + 3
    F, ref = _ctx(key)
    L = F.L
    hp, own = _proof(key, rank)
    emb = hp.emb
    embT = ringo.NewCyclicTransformer(F, emb)
    el = lambda v: _dev(ref.arr([v])[0])  # noqa: E731
    d_x, d_bcA, d_bcL, d_lc, d_bcS = (el(v) for v in hp.chal())
    d_w = _dev(hp.wEcdNTT_arr)
    d_pwNTT = _dev(hp.pwEcdNTT_arr)
    chks = _device_checkers(F, rank, hp.spec)
    scr = lambda n: torch.empty(max(1, n // 8), dtype=torch.int64, device="cuda")  # noqa: E731
    # linCheck
    d_lmask, d_lsum = _filled(emb, L), _filled(L)
    buckler.sumcheck_mask_dev(F, rank, 2 * rank, emb, _dev(ref.arr(hp.linRand)), d_lmask, d_lsum)
    lin = buckler.LinCheckPlan(F, rank, emb, chks, hp.lin)
    d_lquo, d_llo, d_lhi = _filled(rank, L), _filled(rank - 1, L), _filled(jr, L)
    lin.lin_check_dev(d_bcL, d_lc, d_lmask, d_w, hp.wCnt, jr, d_lquo, d_llo, d_lhi, scr(lin.scratch_bytes()))
    # arithCheck
    fscr = scr(buckler.check_finish_scratch_bytes(embT))
    arith, sm = buckler.Circuit(F, _constraints(F, ref, hp.arith)), buckler.Circuit(F, _constraints(F, ref, hp.sum))
    d_ev = _filled(emb, L)
    arith.eval_dev(emb, d_bcA, d_w, hp.wCnt, d_pwNTT, 3, d_ev)
    n_aquo = hp.arithMaxRank - rank
    d_aquo = _filled(n_aquo, L)
    buckler.check_finish_dev(embT, rank, d_ev, None, None, n_aquo, 0, d_aquo, None, None, fscr)
    # sumCheck
    d_smask, d_ssum = _filled(emb, L), _filled(L)
    buckler.sumcheck_mask_dev(F, rank, hp.sumMaxRank, emb, _dev(ref.arr(hp.sumRand)), d_smask, d_ssum)
    d_ev2 = _filled(emb, L)
    sm.eval_dev(emb, d_bcS, d_w, hp.wCnt, d_pwNTT, 3, d_ev2)
    n_squo = hp.sumMaxRank - rank
    d_squo, d_slo, d_shi = _filled(n_squo, L), _filled(rank - 1, L), _filled(jr, L)
    buckler.check_finish_dev(embT, rank, d_ev2, d_bcS, d_smask, n_squo, jr, d_squo, d_slo, d_shi, fscr)
    # pf.Evals: every committed vector at evalPoint, in the roundComIdx order
    committed = [_dev(ref.arr(p)) for p in hp.wEcd] + [d_lmask, d_smask, d_aquo, d_lquo, d_llo, d_lhi, d_squo, d_slo,
                                                       d_shi]
    stride = max(emb, jr)
    d_polys = torch.zeros((len(committed), stride, L), dtype=torch.int64, device="cuda")
    for i, p in enumerate(committed):
        d_polys[i, :p.shape[0]] = p
    d_evals = _filled(len(committed), L)
    bigpoly.evaluate_batch_dev(F, d_polys, stride, stride, len(committed), d_x, d_evals,
                               scr(bigpoly.evaluate_batch_scratch_bytes(F, stride, len(committed))))
    # Verify
    plan = buckler.VerifyPlan(F, rank, jr, hp.wCnt, 3, lin, arith, sm)
    assert plan.n_evals == len(committed)
    d_verdict, d_sides, d_pwe = _filled(1), _filled(8, L), _filled(3, L)
    plan.checks_dev(d_evals, _dev(np.stack([ref.arr(v) for v in hp.pw])), torch.stack([d_x, d_bcA, d_bcL, d_lc, d_bcS]),
                    torch.stack([d_lsum, d_ssum]), d_verdict, d_sides, d_pwe, scr(plan.scratch_bytes()))
    assert int(_host(d_verdict)[0]) == 0
    assert (_host(d_evals) == ref.arr(hp.evals(jr))).all()
    want = _want(ref, hp, jr, own, hp.evals(jr), hp.mask_sums(), hp.chal(), hp.cons())
    _same(ref, (0, _host(d_sides), _host(d_pwe)), want)


def test_argument_errors_with_live_plans():
    """The refusals of rg_buckler_verifier_create and rg_buckler_verify_checks_dev that need an NTT
    plan or an uploaded circuit to reach (the others: test_capi_buckler_verify.py).  The addresses are
    made-up numbers: a call that read them would crash, not fail."""
    import ctypes
    F, ref = _ctx("p63")
    lib = _lib.lib()
    rank = 128
    hp, _ = _proof("p63", rank)
    enc = ringo.NewCyclicTransformer(F, rank)
    lin = buckler.LinCheckPlan(F, rank, rank, _device_checkers(F, rank, hp.spec), hp.lin)
    arith = buckler.Circuit(F, _constraints(F, ref, hp.arith))
    sm = buckler.Circuit(F, _constraints(F, ref, hp.sum))

    def create(plan, jr, w_cnt, n_pw, l, a, s):
        h = ctypes.c_void_p()
        st = lib.rg_buckler_verifier_create(plan.h if plan else None, jr, w_cnt, n_pw, l.h if l else None,
                                            a.h if a else None, s.h if s else None, ctypes.byref(h))
        if st == 0:
            lib.rg_buckler_verifier_destroy(h)
        return st, lib.rg_last_error().decode()

    assert create(enc, rank, hp.wCnt, 3, lin, arith, sm)[0] == 0
    st, why = create(ringo.NewCyclotomicTransformer(F, rank), rank, hp.wCnt, 3, lin, arith, sm)
    assert st == -1 and "cyclic" in why
    st, why = create(enc, rank, hp.wCnt, 3, None, None, None)
    assert st == -1 and "all NULL" in why
    st, why = create(enc, rank - 2, hp.wCnt, 3, lin, arith, sm)
    assert st == -1 and "jindo_rank" in why
    assert create(enc, rank - 1, hp.wCnt, 3, lin, arith, sm)[0] == 0
    st, why = create(ringo.NewCyclicTransformer(F, 2 * rank), 2 * rank, hp.wCnt, 3, lin, None, None)
    assert st == -1 and "another rank or field" in why
    F2, ref2 = _ctx("s63_top")
    st, why = create(ringo.NewCyclicTransformer(F2, rank), rank, hp.wCnt, 3, lin, None, None)
    assert st == -1 and "another rank or field" in why
    st, why = create(ringo.NewCyclicTransformer(F2, rank), rank, hp.wCnt, 3, None, arith, None)
    assert st == -1 and "another field" in why
    st, why = create(enc, rank, 7, 3, lin, None, None)  # the pairs run to witness 7
    assert st == -1 and "pair index" in why
    for a, s in ((arith, None), (None, sm)):
        st, why = create(enc, rank, 9, 3, None, a, s)  # both circuits read witnesses from 9 up
        assert st == -1 and "witness index" in why
    st, why = create(enc, rank, hp.wCnt, 0, None, arith, None)
    assert st == -1 and "public-witness index" in why
    st, why = create(enc, rank, hp.wCnt, 1, None, None, sm)  # the sum check reads pw1
    assert st == -1 and "public-witness index" in why
    with pytest.raises(RingoPanic):
        buckler.VerifyPlan(F, rank, rank, hp.wCnt, 3, None, None, None)
    # the call itself
    plan = buckler.VerifyPlan(F, rank, rank, hp.wCnt, 3, lin, arith, sm)
    A = [0x10000 * (i + 1) for i in range(9)]
    call = lib.rg_buckler_verify_checks_dev
    ok = [A[0], A[1], A[2], A[3], A[4], A[5], A[6], A[7]]
    for i, why in ((0, "NULL evals"), (1, "d_pw"), (2, "NULL evals"), (3, "mask sums"), (4, "NULL evals"),
                   (7, "scratch")):
        args = list(ok)
        args[i] = None
        assert call(plan.h, *args, None) == -1 and why in lib.rg_last_error().decode(), i
    for i, j in ((0, 4), (1, 7), (5, 6), (2, 3)):
        args = list(ok)
        args[j] = args[i]
        assert call(plan.h, *args, None) == -1 and "alias" in lib.rg_last_error().decode(), (i, j)
    no_pw = buckler.VerifyPlan(F, rank, rank, hp.wCnt, 0, lin, None, None)
    assert call(no_pw.h, *ok, None) == -1 and "d_pw" in lib.rg_last_error().decode()
    unset = buckler.LinCheckPlan(F, rank, rank, [buckler.ProjChecker(F, rank)], [[(0, 1)]])
    p2 = buckler.VerifyPlan(F, rank, rank, hp.wCnt, 0, unset, None, None)
    assert call(p2.h, A[0], None, A[2], A[3], A[4], None, None, A[7], None) == -1
    assert "never set" in lib.rg_last_error().decode()
