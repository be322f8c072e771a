"""GPU parity: the Buckler verifier's batch entry (rg_buckler_verify_checks_multi*; n_proofs proofs of
one rg_bverifier decided by one call), bit for bit against tests/buckler_verify_ref.py per proof: the
verdict words, all 8 n sides and all pwEvals, into buffers pre-filled with -1 so that every word must
be written.  The proofs are tests/buckler_verify_multi_util.proofs: one circuit, every per-proof input
different (pinned on the CPU by test_buckler_verify_multi_ref.py)."""
import functools

import numpy as np
import pytest

import ringo
from ringo import _lib, buckler
from ringo.bigpoly import RingoPanic
from tests import buckler_lin_ref as R
from tests import buckler_verify_ref as V
from tests import synth_util as su
from tests.buckler_verify_multi_util import PROJ, proofs, swapped_xof
from tests.buckler_verify_util import perturbations

pytestmark = pytest.mark.gpu

NOSPARE = sorted(k for k, v in su.SYNTH.items() if v["bits"] == 64 * v["limbs"] and v["limbs"] in (1, 2, 4, 7, 14))
FIELDS = ["p63", "jindo_zp", "zp880", NOSPARE[0]]  # 1, 4 and 14 limbs, and a modulus with no spare top bit
ALL = (True, True, True)
MIXED = ("lin_remlo", "pw0", "eval_point", "sum_mask_sum")


@functools.lru_cache(maxsize=None)
def _ctx(key):
    q = su.modulus(key)
    return ringo.Field(q), R.Ref(q)


@functools.lru_cache(maxsize=None)
def _pool(key, rank):
    """The proofs of one circuit and each proof's own evaluations, computed once and shared (read-only)."""
    _, ref = _ctx(key)
    pool = proofs(ref, rank, 6 if rank <= 256 else 2)
    return pool, [hp.own() for hp in pool]


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


def _constraints(F, ref, cons):
    out = []
    for c in cons:
        ac = buckler.ArithmeticConstraint(F)
        for coeff, pw, ws in c:
            ac.AddTermWithConst(ref.arr([coeff])[0], pw, *ws)
        out.append(ac)
    return out


def _plan(key, hp, jindo_rank, has=ALL, n_pw=3, proj=True):
    """(plan, device checkers): the circuit's handle.  The projection checker's own matrix is left
    unset: the batch entry takes each proof's from d_xof.  proj=False: the linear check without its
    projection checker (and without that checker's pairs)."""
    F, ref = _ctx(key)
    lin, chks = None, []
    if has[0]:
        keep = [i for i, s in enumerate(hp.spec) if proj or s[0] != "proj"]
        for i in keep:
            s = hp.spec[i]
            chks.append(buckler.NewNTTChecker(F, hp.rank) if s[0] == "ntt" else
                        buckler.NewAutChecker(F, hp.rank, s[1], s[2]) if s[0] == "aut" else
                        buckler.ProjChecker(F, hp.rank) if s[0] == "proj" else
                        buckler.ProjRecomposeChecker(F, hp.rank, s[1]))
        lin = buckler.LinCheckPlan(F, hp.rank, hp.rank, chks, [hp.lin[i] for i in keep])
    plan = buckler.VerifyPlan(F, hp.rank, jindo_rank, hp.wCnt, n_pw, lin,
                              _constraints(F, ref, hp.arith) if has[1] else None,
                              _constraints(F, ref, hp.sum) if has[2] else None)
    return plan, chks


def _item(hp, own, jr, name=None, xof_of=None, has=ALL, n_pw=3, proj=True):
    """One proof of a batch as the call takes it, with the restatement's answer: dict(evals, ms, pw,
    ch, xof, want = (verdict, sides, pwEvals)).  name: one of buckler_verify_util.perturbations;
    xof_of: the proof whose XOF bytes stand in for this proof's."""
    ref, rank = hp.ref, hp.rank
    evals, ms, pw, ch, xof, o = hp.evals(jr, *has), hp.mask_sums(), hp.pw, hp.chal(), hp.xof, own
    if name is not None:
        evals, ms, pw, ch, _ = perturbations(hp, jr)[name]
        if name.startswith("pw"):
            o = (own[0], own[1], V.own_evals(ref, rank, ch[0], ch[3], None, pw)[2])
        elif name == "eval_point":
            o = hp.own(None, pw, ch)
    if xof_of is not None:
        chk, xof = swapped_xof(hp, xof_of)
        o = hp.own(chk)
    lin_cons, arith_cons, sum_cons = hp.cons(*has)
    tr = list(o[1])
    if has[0] and not proj:
        del tr[PROJ]
        lin_cons = [c for i, c in enumerate(lin_cons) if i != PROJ]
    o = (o[0] if has[0] else None, tr if has[0] else [], o[2][:n_pw])
    verdict, sides = V.decide(ref, rank, jr, hp.wCnt, ch, ms, evals, o, lin_cons, arith_cons, sum_cons)
    return dict(evals=evals, ms=ms, pw=pw[:n_pw], ch=ch, xof=xof, want=(verdict, sides, o[2]), own=o,
                cons=(lin_cons, arith_cons, sum_cons))


def _arrays(plan, ref, items):
    ev = np.stack([ref.arr(it["evals"]) for it in items])
    ch = np.stack([ref.arr(it["ch"]) for it in items])
    ms = np.stack([ref.arr(it["ms"]) for it in items])
    pw = np.stack([np.stack([ref.arr(v) for v in it["pw"]]) for it in items]) if plan.nPw else None
    xof = b"".join(it["xof"] for it in items)
    return ev, pw, xof, ch, ms


def _run(plan, ref, items, xof=True, stream=None):
    """One rg_buckler_verify_checks_multi_dev into buffers of -1 -> (verdicts [n], sides [n][8][L],
    pwEvals [n][n_pw][L]) as host arrays."""
    import torch
    L, n = plan.field.L, len(items)
    ev, pw, xb, ch, ms = _arrays(plan, ref, items)
    d_xof = _dev(np.frombuffer(xb, np.uint8).copy(), np.uint8) if xof else None
    d_verdict, d_sides = _filled(n), _filled(n, 8, L)
    d_pwe = _filled(n, plan.nPw, L) if plan.nPw else None
    scr = torch.empty(max(1, plan.scratch_bytes_multi(n) // 8), dtype=torch.int64, device="cuda")
    plan.checks_multi_dev(n, _dev(ev), _dev(pw) if plan.nPw else None, d_xof, _dev(ch), _dev(ms), d_verdict, d_sides,
                          d_pwe, scr, stream=stream)
    return _host(d_verdict), _host(d_sides), (_host(d_pwe) if plan.nPw else np.zeros((n, 0, L), np.uint64))


def _same(ref, got, items, what=""):
    """Every proof's verdict word, eight sides and pwEvals against the restatement's."""
    for i, it in enumerate(items):
        verdict, sides, pwe = it["want"]
        assert int(got[0][i]) == verdict, (what, i, int(got[0][i]), verdict)
        assert (got[1][i] == ref.arr(sides)).all(), (what, i, "sides")
        assert got[2][i].shape[0] == len(pwe) and (len(pwe) == 0 or (got[2][i] == ref.arr(pwe)).all()), (what, i, "pw")


@pytest.mark.parametrize("rank", [128, 256])
@pytest.mark.parametrize("key", FIELDS)
def test_batches_of_honest_proofs(key, rank):
    """1, 2, 3 and 5 proofs at jindo_rank = rank - 1 and 4 rank + 3 (shift exponent 0 and a multi-bit
    one): every proof is accepted and every word is the restatement's for that proof."""
    F, ref = _ctx(key)
    pool, owns = _pool(key, rank)
    for jr in (rank - 1, 4 * rank + 3):
        plan, _ = _plan(key, pool[0], jr)
        assert plan.n_evals == pool[0].wCnt + 9
        items = [_item(hp, o, jr) for hp, o in zip(pool[:5], owns)]
        assert all(it["want"][0] == 0 for it in items)
        for n in (1, 2, 3, 5):
            _same(ref, _run(plan, ref, items[:n]), items[:n], ("honest", jr, n))


@pytest.mark.parametrize("key", ["p63", "jindo_zp"])
def test_two_tiles_per_polynomial(key):
    """Rank 8192: the evaluate runs two tiles per polynomial, each with its proof's tables."""
    F, ref = _ctx(key)
    rank, jr = 8192, 4 * 8192 + 3
    pool, owns = _pool(key, rank)
    plan, _ = _plan(key, pool[0], jr)
    items = [_item(pool[0], owns[0], jr), _item(pool[1], owns[1], jr, "lin_remlo")]
    assert [it["want"][0] for it in items] == [0, V.LIN_REM | V.LIN]
    _same(ref, _run(plan, ref, items), items, "rank 8192")


def _mixed(pool, owns, jr):
    items = [_item(pool[0], owns[0], jr)]
    items += [_item(hp, o, jr, name) for hp, o, name in zip(pool[1:5], owns[1:5], MIXED)]
    items.append(_item(pool[5], owns[5], jr, xof_of=pool[0]))
    return items


@pytest.mark.parametrize("key", FIELDS)
def test_mixed_batch_and_its_permutation(key):
    """The honest proof, four one-change rejections and a proof presented with another proof's XOF
    bytes in one batch: the verdict vector is the reference's per proof (the bits pinned on the CPU),
    and the same batch in another order gives the same outputs permuted."""
    F, ref = _ctx(key)
    rank = 128
    pool, owns = _pool(key, rank)
    for jr in (rank - 1, 4 * rank + 3):
        plan, _ = _plan(key, pool[0], jr)
        items = _mixed(pool, owns, jr)
        bits = [0] + [perturbations(pool[0], jr)[name][4] for name in MIXED] + [V.LIN]
        assert [it["want"][0] for it in items] == bits
        got = _run(plan, ref, items)
        _same(ref, got, items, ("mixed", jr))
        assert [int(x) for x in got[0]] == bits
        order = [3, 5, 0, 4, 2, 1]
        again = _run(plan, ref, [items[i] for i in order])
        for k in range(3):
            assert (again[k] == got[k][order]).all(), ("permuted", jr, k)


@pytest.mark.parametrize("key", FIELDS)
def test_equals_the_single_proof_entry(key):
    """n_proofs = 1, with the checker's matrix set to the same XOF bytes, equals
    rg_buckler_verify_checks_dev word for word; each proof of a batch equals its own single call."""
    import torch
    F, ref = _ctx(key)
    rank, jr = 128, 4 * 128 + 3
    L = F.L
    pool, owns = _pool(key, rank)
    plan, chks = _plan(key, pool[0], jr)
    items = _mixed(pool, owns, jr)[:4]
    batch = _run(plan, ref, items)
    for i, it in enumerate(items):
        chks[PROJ].SetXOF(it["xof"])
        ev, pw, _, ch, ms = _arrays(plan, ref, [it])
        d_verdict, d_sides, d_pwe = _filled(1), _filled(8, L), _filled(3, L)
        scr = torch.empty(plan.scratch_bytes() // 8, dtype=torch.int64, device="cuda")
        plan.checks_dev(_dev(ev[0]), _dev(pw[0]), _dev(ch[0]), _dev(ms[0]), d_verdict, d_sides, d_pwe, scr)
        single = (_host(d_verdict), _host(d_sides), _host(d_pwe))
        one = _run(plan, ref, [it])  # the checker's own matrix is set by now: the batch entry does not read it
        for k in range(3):
            assert (one[k][0] == single[k].reshape(one[k][0].shape)).all(), ("n = 1", i, k)
            assert (batch[k][i] == one[k][0]).all(), ("batch", i, k)


HANDLES = [("lin", (True, False, False), 3, True), ("arith", (False, True, False), 3, True),
           ("sum", (False, False, True), 3, True), ("lin_no_pw", (True, False, False), 0, True),
           ("arith_sum", (False, True, True), 2, True), ("lin_no_proj", (True, False, False), 3, False)]


@pytest.mark.parametrize("key", ["p63", "jindo_zp", "zp880"])
@pytest.mark.parametrize("name,has,n_pw,proj", HANDLES)
def test_handles_with_fewer_checks(key, name, has, n_pw, proj):
    """Each check alone, in its own pf.Evals layout, three proofs a call.  d_xof goes with a projection
    checker in the linear check: it is required with one, and refused without one."""
    F, ref = _ctx(key)
    rank, jr = 128, 128
    pool, owns = _pool(key, rank)
    plan, _ = _plan(key, pool[0], jr, has, n_pw, proj)
    assert plan.n_evals == V.layout(pool[0].wCnt, *has)["n"]
    needs_xof = has[0] and proj
    items = [_item(hp, o, jr, None, None, has, n_pw, proj) for hp, o in zip(pool[:3], owns)]
    if name != "lin_no_proj":  # without its projection pair the proof's quotient is not the circuit's
        assert all(it["want"][0] == 0 for it in items)
    _same(ref, _run(plan, ref, items, xof=needs_xof), items, name)
    with pytest.raises(RingoPanic):
        _run(plan, ref, items, xof=not needs_xof)
    assert "d_xof" in _lib.lib().rg_last_error().decode()
    present = (V.LIN_REM | V.LIN if has[0] else 0) | (V.ARITH if has[1] else 0) | (V.SUM_REM | V.SUM if has[2] else 0)
    bad = [dict(it) for it in items]
    for it, hp in zip(bad, pool):  # every evaluation wrong: the absent checks' bits stay clear
        it["evals"] = [(e + 1) % ref.q for e in it["evals"]]
        verdict, sides = V.decide(ref, rank, jr, hp.wCnt, it["ch"], it["ms"], it["evals"], it["own"], *it["cons"])
        assert verdict & ~present == 0 and verdict != 0
        it["want"] = (verdict, sides, it["own"][2])
    _same(ref, _run(plan, ref, bad, xof=needs_xof), bad, name + " bad")


@pytest.mark.parametrize("key", ["p63", "jindo_zp", "zp880"])
def test_host_form_and_mirror(key):
    """rg_buckler_verify_checks_multi through the raw entry and VerifyPlan.checks_multi."""
    F, ref = _ctx(key)
    rank, jr = 128, 4 * 128 + 3
    L = F.L
    pool, owns = _pool(key, rank)
    plan, _ = _plan(key, pool[0], jr)
    items = _mixed(pool, owns, jr)[:3]
    ev, pw, xof, ch, ms = _arrays(plan, ref, items)
    _same(ref, plan.checks_multi(ev, pw, xof, ch, ms), items, "mirror")
    verdict = np.full(3, 2 ** 64 - 1, np.uint64)
    sides, pwe = np.full((3, 8, L), 2 ** 64 - 1, np.uint64), np.full((3, 3, L), 2 ** 64 - 1, np.uint64)
    p = _lib.ptr
    c = np.ascontiguousarray
    st = _lib.lib().rg_buckler_verify_checks_multi(plan.h, 3, p(c(ev)), p(c(pw)), xof, p(c(ch)), p(c(ms)), p(verdict),
                                                  p(sides), p(pwe))
    assert st == 0
    _same(ref, (verdict, sides, pwe), items, "host form")
    assert plan.checks_multi(np.zeros((0, plan.n_evals, L), np.uint64), np.zeros((0, 3, rank, L), np.uint64), b"",
                             np.zeros((0, 5, L), np.uint64), np.zeros((0, 2, L), np.uint64))[0] == []


def test_two_streams_share_one_verifier():
    """Two batch calls in flight on two streams with one handle (own scratch and outputs each)."""
    import torch
    key, rank, jr = "jindo_zp", 128, 128
    F, ref = _ctx(key)
    pool, owns = _pool(key, rank)
    plan, _ = _plan(key, pool[0], jr)
    items = _mixed(pool, owns, jr)
    halves = [items[:3], items[3:]]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = [_run(plan, ref, h, stream=s) for s, h in zip(streams, halves)]
    for g, h in zip(got, halves):
        _same(ref, g, h, "two streams")


def test_argument_errors_with_live_plans():
    """The refusals of the batch entry, which need a live handle to get past the NULL-handle test
    (that one: test_capi_buckler_verify_multi.py).  The addresses are made-up numbers: a call that read
    them would crash, not fail."""
    key, rank = "p63", 128
    F, ref = _ctx(key)
    lib = _lib.lib()
    pool, _ = _pool(key, rank)
    plan, _ = _plan(key, pool[0], rank)
    A = [0x10000 * (i + 1) for i in range(10)]
    call = lib.rg_buckler_verify_checks_multi_dev
    why = lambda: lib.rg_last_error().decode()  # noqa: E731
    ok = list(A[:9])  # evals, pw, xof, chal, mask sums, verdict, sides, pw evals, scratch
    for i, text in ((0, "NULL evals"), (1, "d_pw"), (2, "d_xof"), (3, "NULL evals"), (4, "mask sums"),
                    (5, "NULL evals"), (8, "scratch")):
        args = list(ok)
        args[i] = None
        assert call(plan.h, 2, *args, None) == -1 and text in why(), i
    for i, j in ((0, 5), (1, 8), (6, 7), (3, 4), (2, 8), (2, 0)):
        args = list(ok)
        args[j] = args[i]
        assert call(plan.h, 2, *args, None) == -1 and "alias" in why(), (i, j)
    src = open(_lib.HEADER).read()
    assert "#define RG_BK_MULTI_MAX_PROOFS 65535" in src
    assert call(plan.h, 65536, *ok, None) == -1 and "over the limit" in why()
    assert lib.rg_buckler_verify_checks_multi_scratch_bytes(plan.h, 65536) == 0
    assert call(plan.h, 0, *ok, None) == 0  # n_proofs = 0 does nothing: the made-up addresses are not read
    assert call(plan.h, 0, None, None, None, None, None, None, None, None, None, None) == 0
    assert lib.rg_buckler_verify_checks_multi_scratch_bytes(plan.h, 0) == 0
    assert plan.scratch_bytes_multi(1) > plan.scratch_bytes()  # the packed matrix and nothing less
    no_pw, _ = _plan(key, pool[0], rank, (True, False, False), 0)
    assert call(no_pw.h, 2, *ok, None) == -1 and "d_pw" in why()
    no_proj, _ = _plan(key, pool[0], rank, (True, False, False), 3, False)
    assert call(no_proj.h, 2, *ok, None) == -1 and "d_xof" in why()
    arith, _ = _plan(key, pool[0], rank, (False, True, False), 3)
    assert call(arith.h, 2, *ok, None) == -1 and "d_xof" in why()
