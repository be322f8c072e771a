"""GPU parity: the Buckler linear check and sum check on the device (rg_buckler_checker_*,
rg_buckler_powers*, rg_buckler_sumcheck_mask*, rg_buckler_check_finish*, rg_buckler_lin_check*;
buckler/linear.go, buckler/prover.go:381-485), bit-exact against tests/buckler_lin_ref.py (pinned on
the CPU by test_buckler_lin_ref.py), through the `_dev` entry points and the Python mirror."""
import ctypes
import functools

import numpy as np
import pytest

import ringo
from ringo import _lib, buckler
from ringo.bigpoly import RingoPanic
from tests import buckler_lin_ref as R
from tests import synth_util as su
from tests.buckler_lin_util import RECOMPOSE_BOUND, completeness_circuit, rand_ints, xof_bytes

pytestmark = pytest.mark.gpu

GOLD = ["p63", "mult_zp", "jindo_zp", "zp440", "zp880"]
# synthetic moduli with no spare top bit and a supported limb count: where an unreduced sum would overflow
NOSPARE = sorted(k for k, v in su.SYNTH.items() if v["bits"] == 64 * v["limbs"] and v["limbs"] in (1, 2, 4, 7, 14))


@functools.lru_cache(maxsize=None)
def _ctx(key):
    q = su.modulus(key)
    return ringo.Field(q), R.Ref(q)


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


def _scratch(nbytes):
    import torch
    return torch.empty(max(1, nbytes // 8), dtype=torch.int64, device="cuda")


def _inputs(ref, rank, rng):
    """[3][rank]: random, all q - 1, all zero."""
    return [rand_ints(ref.q, rank, rng), [ref.q - 1] * rank, [0] * rank]


def _check_both(F, ref, dchk, rchk, rank, rng, directions=("transform", "transpose")):
    """Batch 3 (random, q - 1, zero) and batch 1 (the random vector) through both `_dev` entry
    points into buffers pre-filled with -1, against the restatement."""
    vs = _inputs(ref, rank, rng)
    dv = _dev(np.stack([ref.arr(v) for v in vs]))
    for d in directions:
        want = np.stack([ref.arr(getattr(rchk, d)(v)) for v in vs])
        for batch in (3, 1):
            out = _filled(batch, rank, F.L)
            if d == "transform":
                dchk.transform_dev(out, dv, batch, d_scratch=_scratch(dchk.scratch_bytes(batch)))
            else:
                dchk.transpose_dev(out, dv, batch)
            assert (_host(out) == want[:batch]).all(), (d, batch)


@pytest.mark.parametrize("key", GOLD)
@pytest.mark.parametrize("rank", [8, 128, 256, 1 << 12])
def test_ntt_and_aut_checkers(key, rank):
    F, ref = _ctx(key)
    rng = np.random.default_rng(rank)
    _check_both(F, ref, buckler.NewNTTChecker(F, rank), R.NTTChecker(ref, rank), rank, rng)
    for idx, is_ntt in ((5, False), (2 * rank - 3, True), (3, True), (2 * rank - 1, False)):
        _check_both(F, ref, buckler.NewAutChecker(F, rank, idx, is_ntt), R.AutChecker(ref, rank, idx, is_ntt), rank,
                    rng)


PROJ_CASES = [(128, "random"), (128, "zeros"), (128, "ones"), (128, "rows_0_127"), (256, "random"), (256, "zeros"),
              (256, "rows_0_127"), (200, "random"), (1 << 12, "random"), (1 << 12, "zeros")]


@pytest.mark.parametrize("key", GOLD)
@pytest.mark.parametrize("rank,pattern", PROJ_CASES)
def test_proj_checker(key, rank, pattern):
    """rank 128: one column chunk and no zero tail; 256: two chunks; 200: a partial last chunk;
    2^12: 32 chunks.  `zeros` makes every entry true (rank addends of q - 1 per row), `ones` none,
    `rows_0_127` pins the bit order."""
    F, ref = _ctx(key)
    rng = np.random.default_rng(rank + len(pattern))
    xof = xof_bytes(pattern, rank, rng)
    dchk = buckler.ProjChecker(F, rank).SetXOF(xof)
    _check_both(F, ref, dchk, R.ProjChecker(ref, rank).set_xof(xof), rank, rng)


def test_proj_checker_reset_and_device_bytes():
    """A checker may be re-set, from device-resident XOF bytes; the host forms agree."""
    import torch
    F, ref = _ctx("jindo_zp")
    rank = 256
    rng = np.random.default_rng(5)
    dchk = buckler.ProjChecker(F, rank).SetXOF(xof_bytes("ones", rank, rng))
    xof = xof_bytes("random", rank, rng)
    dchk.set_xof_dev(torch.frombuffer(bytearray(xof), dtype=torch.uint8).cuda())
    rchk = R.ProjChecker(ref, rank).set_xof(xof)
    _check_both(F, ref, dchk, rchk, rank, rng)
    v = rand_ints(ref.q, rank, rng)
    out = np.full((rank, F.L), 0xFF, np.uint64)
    assert (dchk.TransformTo(out, ref.arr(v)) == ref.arr(rchk.transform(v))).all()
    assert (dchk.TransposeTo(out, ref.arr(v)) == ref.arr(rchk.transpose(v))).all()


@pytest.mark.parametrize("key", GOLD)
@pytest.mark.parametrize("rank,nb", [(128, 1), (128, 3), (128, 7), (128, 129), (256, 3), (200, 7), (1 << 12, 3)])
def test_recompose_checker(key, rank, nb):
    """nb = 3 at rank 128 leaves a two-element zero tail, nb = 129 > rank gives all zeros."""
    F, ref = _ctx(key)
    rng = np.random.default_rng(rank + nb)
    base = rand_ints(ref.q, nb, rng)
    h = _lib.vp()
    barr = np.ascontiguousarray(F.mont(base))
    assert _lib.lib().rg_buckler_checker_create_recompose(F.h, rank, _lib.ptr(barr), nb, ctypes.byref(h)) == 0
    rnd = buckler.LinearChecker(F, rank, h)
    _check_both(F, ref, rnd, R.RecomposeChecker(ref, rank, base), rank, rng)
    if nb == 3:  # the mirror's constructor: decomposeBase(8) = [4, 2, 1]
        dchk = buckler.ProjRecomposeChecker(F, rank, RECOMPOSE_BOUND)
        assert dchk.dcmpBase == [4, 2, 1]
        _check_both(F, ref, dchk, R.RecomposeChecker(ref, rank, R.decomposeBase(RECOMPOSE_BOUND)), rank, rng)


@pytest.mark.parametrize("key", NOSPARE)
def test_transforms_on_moduli_without_spare_bit(key):
    """The projection and recompose transforms sum up to `rank` elements: on a modulus that
    fills its top limb a sum of two residues overflows the limbs, so an accumulator that is not
    reduced (or not widened) per step shows here."""
    F, ref = _ctx(key)
    rng = np.random.default_rng(len(key))
    for rank, pattern in ((128, "random"), (1 << 12, "zeros")):
        xof = xof_bytes(pattern, rank, rng)
        _check_both(F, ref, buckler.ProjChecker(F, rank).SetXOF(xof), R.ProjChecker(ref, rank).set_xof(xof), rank,
                    rng, directions=("transform",))
    base = [ref.q - 1] * 7
    h = _lib.vp()
    barr = np.ascontiguousarray(F.mont(base))
    assert _lib.lib().rg_buckler_checker_create_recompose(F.h, 128, _lib.ptr(barr), 7, ctypes.byref(h)) == 0
    _check_both(F, ref, buckler.LinearChecker(F, 128, h), R.RecomposeChecker(ref, 128, base), 128, rng,
                directions=("transform",))


@pytest.mark.parametrize("key", GOLD)
def test_powers(key):
    """n crosses a lane's block of exponents (16), a workgroup (4096 exponents) and both by one."""
    F, ref = _ctx(key)
    rng = np.random.default_rng(3)
    for c in (0, ref.set_uint64(1), ref.q - 1, rand_ints(ref.q, 1, rng)[0]):
        want = ref.arr(R.powers(ref, c, (1 << 12) + 1))
        dc = _dev(ref.arr([c])[0])
        for n in (1, 2, 255, 256, 257, (1 << 12) + 1):
            out = _filled(n + 1, F.L)
            buckler.powers_dev(F, dc, n, out)
            got = _host(out)
            assert (got[:n] == want[:n]).all(), (c, n)
            assert (got[n] == np.uint64(2 ** 64 - 1)).all(), (c, n)  # nothing past n
    assert (buckler.Powers(F, ref.arr([c])[0], 257) == want[:257]).all()


@pytest.mark.parametrize("key", GOLD)
@pytest.mark.parametrize("rank,mask_rank,emb", [(128, 128, 256), (128, 256, 256), (128, 300, 512), (128, 512, 512)])
def test_sum_check_mask(key, rank, mask_rank, emb):
    F, ref = _ctx(key)
    rng = np.random.default_rng(mask_rank)
    r = rand_ints(ref.q, mask_rank, rng)
    r[0], r[-1] = ref.q - 1, 0
    want, want_sum = R.sumCheckMask(ref, rank, mask_rank, emb, r)
    dmask, dsum = _filled(emb, F.L), _filled(F.L)
    buckler.sumcheck_mask_dev(F, rank, mask_rank, emb, _dev(ref.arr(r)), dmask, dsum)
    assert (_host(dmask) == ref.arr(want)).all()
    assert (_host(dsum) == ref.arr([want_sum])[0]).all()
    mask, msum = buckler.SumCheckMask(F, rank, mask_rank, emb, ref.arr(r))
    assert not mask.IsNTT and (mask.Coeffs == ref.arr(want)).all() and (msum == ref.arr([want_sum])[0]).all()


@pytest.mark.parametrize("key", GOLD)
def test_check_finish(key):
    """The tail alone: with and without scale and mask, jindo_rank = rank - 1 (no zero prefix) and
    4 rank, n_quo = 0 and emb, and the remainder discarded (arithCheck)."""
    F, ref = _ctx(key)
    rank, emb = 128, 512
    rng = np.random.default_rng(9)
    T = ringo.NewCyclicTransformer(F, emb)
    ev, mask = rand_ints(ref.q, emb, rng), rand_ints(ref.q, emb, rng)
    scale = rand_ints(ref.q, 1, rng)[0]
    dmask, dscale = _dev(ref.arr(mask)), _dev(ref.arr([scale])[0])
    scr = _scratch(buckler.check_finish_scratch_bytes(T))
    for use_scale, use_mask, jr, n_quo, rem in [(True, True, rank - 1, emb, True), (False, False, 4 * rank, 0, True),
                                                (True, False, 4 * rank, emb, True), (False, True, rank - 1, rank, True),
                                                (False, False, 0, emb - rank, False)]:
        quo, lo, hi, _ = R.checkTail(ref, ev, rank, scale if use_scale else None, mask if use_mask else None, n_quo,
                                     jr if rem else rank - 1)
        dev_ = _dev(ref.arr(ev))
        dquo, dlo, dhi = _filled(n_quo + 1, F.L), _filled(rank, F.L), _filled(jr + 1, F.L)
        buckler.check_finish_dev(T, rank, dev_, dscale if use_scale else None, dmask if use_mask else None, n_quo, jr,
                                 dquo, dlo if rem else None, dhi if rem else None, scr)
        got = _host(dquo)
        if n_quo:
            assert (got[:n_quo] == ref.arr(quo)).all()
        assert (got[n_quo] == np.uint64(2 ** 64 - 1)).all()
        if rem:
            glo, ghi = _host(dlo), _host(dhi)
            assert (glo[:rank - 1] == ref.arr(lo)).all() and (glo[rank - 1] == np.uint64(2 ** 64 - 1)).all()
            assert (ghi[:jr] == ref.arr(hi)).all() and (ghi[jr] == np.uint64(2 ** 64 - 1)).all()
        else:
            assert (_host(dlo) == np.uint64(2 ** 64 - 1)).all()


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


@functools.lru_cache(maxsize=None)
def _lin_case(key, rank, emb, jindo_rank):
    """The completeness circuit and the restatement's answer, computed once and shared (read-only)."""
    F, ref = _ctx(key)
    circ = completeness_circuit(ref, rank, emb, seed=rank, two_pairs=True)
    mask, mask_sum = R.sumCheckMask(ref, rank, 2 * rank, emb, circ["rand"])
    quo, lo, hi, rem = R.linCheck(ref, rank, emb, jindo_rank, circ["bc"], circ["lc"], mask, circ["checkers"],
                                  circ["constraints"], circ["wEcdNTT"])
    assert rem[0] == mask_sum
    want = tuple(ref.arr(x) for x in (quo, lo, hi))
    return circ, mask, mask_sum, want


@pytest.mark.parametrize("key", GOLD)
@pytest.mark.parametrize("rank,emb", [(128, 512), (1 << 10, 1 << 12)])
def test_lin_check_end_to_end(key, rank, emb):
    """All four checker kinds, two pairs on the NTT checker, wOut = M wIn: quo, remLo and remHi
    equal the restatement and rem[0], read from the device, is linCheckMaskSum."""
    F, ref = _ctx(key)
    jindo_rank = 8 * rank
    circ, mask, mask_sum, want = _lin_case(key, rank, emb, jindo_rank)
    chks = _device_checkers(F, rank, circ["spec"])
    plan = buckler.LinCheckPlan(F, rank, emb, chks, circ["constraints"])
    n_w = len(circ["w"])
    dw = _dev(np.stack([ref.arr(p) for p in circ["wEcdNTT"]]))
    dbc, dlc = _dev(ref.arr([circ["bc"]])[0]), _dev(ref.arr([circ["lc"]])[0])
    # the mask from the device as well
    dmask, dsum = _filled(emb, F.L), _filled(F.L)
    buckler.sumcheck_mask_dev(F, rank, 2 * rank, emb, _dev(ref.arr(circ["rand"])), dmask, dsum)
    dquo, dlo, dhi = _filled(rank, F.L), _filled(rank - 1, F.L), _filled(jindo_rank, F.L)
    scr = _scratch(plan.scratch_bytes())
    plan.lin_check_dev(dbc, dlc, dmask, dw, n_w, jindo_rank, dquo, dlo, dhi, scr)
    for got, w in zip((dquo, dlo, dhi), want):
        assert (_host(got) == w).all()
    o = plan.rem_offset_words()
    rem0 = _host(scr)[o:o + F.L]
    assert (rem0 == _host(dsum)).all() and (rem0 == ref.arr([mask_sum])[0]).all()
    if rank == 128:  # the host form through the mirror
        quo, lo, hi = buckler.LinCheck(F, rank, emb, jindo_rank, ref.arr([circ["bc"]])[0], ref.arr([circ["lc"]])[0],
                                       ref.arr(mask), chks, circ["constraints"],
                                       np.stack([ref.arr(p) for p in circ["wEcdNTT"]]))
        assert (quo == want[0]).all() and (lo == want[1]).all() and (hi == want[2]).all()


def test_lin_check_two_streams_share_one_plan():
    """Two lin_check_dev calls in flight on two streams with one rg_lincheck (own scratch and
    outputs each): both results are correct."""
    import torch
    key, rank, emb = "jindo_zp", 128, 512
    F, ref = _ctx(key)
    jindo_rank = 8 * rank
    circ, mask, mask_sum, want = _lin_case(key, rank, emb, jindo_rank)
    plan = buckler.LinCheckPlan(F, rank, emb, _device_checkers(F, rank, circ["spec"]), circ["constraints"])
    dw = _dev(np.stack([ref.arr(p) for p in circ["wEcdNTT"]]))
    dbc, dlc, dmask = _dev(ref.arr([circ["bc"]])[0]), _dev(ref.arr([circ["lc"]])[0]), _dev(ref.arr(mask))
    outs = [(_filled(rank, F.L), _filled(rank - 1, F.L), _filled(jindo_rank, F.L), _scratch(plan.scratch_bytes()))
            for _ in range(2)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s, (dq, dl, dh, scr) in zip(streams, outs):
        plan.lin_check_dev(dbc, dlc, dmask, dw, len(circ["w"]), jindo_rank, dq, dl, dh, scr, stream=s)
    for s in streams:
        s.synchronize()
    for dq, dl, dh, _ in outs:
        for got, w in zip((dq, dl, dh), want):
            assert (_host(got) == w).all()


def test_argument_errors_with_live_plans():
    """The RG_ERR_INVALID cases that need an NTT plan to reach (the others: test_capi_buckler_lin.py)."""
    F, ref = _ctx("p63")
    rank, emb = 128, 512
    L = _lib.lib()
    A, B, C, D = 0x10000, 0x20000, 0x30000, 0x40000  # never read: every call below is refused first
    T = ringo.NewCyclicTransformer(F, emb)
    assert L.rg_buckler_check_finish_dev(T.h, rank, A, None, None, rank, rank - 2, B, C, D, 0x50000, None) == -1
    assert L.rg_buckler_check_finish_dev(T.h, rank, A, None, None, rank, 4 * rank, B, C, None, 0x50000, None) == -1
    assert L.rg_buckler_check_finish_dev(T.h, rank, A, None, None, emb + 1, 4 * rank, B, C, D, 0x50000, None) == -1
    assert L.rg_buckler_check_finish_dev(T.h, rank, A, None, None, rank, 4 * rank, A, C, D, 0x50000, None) == -1
    neg = ringo.NewCyclotomicTransformer(F, emb)  # the evaluator is cyclic
    assert L.rg_buckler_check_finish_dev(neg.h, rank, A, None, None, rank, 4 * rank, B, C, D, 0x50000, None) == -1
    ntt = buckler.NewNTTChecker(F, rank)
    assert L.rg_buckler_checker_transform_dev(ntt.h, A, A, 1, None, None) == -1  # aliased in/out
    assert L.rg_buckler_checker_transpose_dev(ntt.h, A, A, 1, None) == -1
    rec = buckler.ProjRecomposeChecker(F, rank, 10)
    assert L.rg_buckler_checker_transform_dev(rec.h, A, A, 1, None, None) == -1
    plan = buckler.LinCheckPlan(F, rank, emb, [ntt, rec], [[(0, 1)], [(2, 3)]])
    args = (A, A, B, C)
    assert L.rg_buckler_lin_check_dev(plan.h, *args, 3, 4 * rank, D, 0x50000, 0x60000, 0x70000, None) == -1  # index 3 >= n_w
    assert L.rg_buckler_lin_check_dev(plan.h, *args, 4, rank - 2, D, 0x50000, 0x60000, 0x70000, None) == -1
    assert L.rg_buckler_lin_check_dev(plan.h, *args, 4, 4 * rank, D, 0x50000, 0x60000, None, None) == -1
    with pytest.raises(RingoPanic):  # a checker of another rank
        buckler.LinCheckPlan(F, rank, emb, [buckler.NewNTTChecker(F, 2 * rank)], [[(0, 1)]])
    with pytest.raises(RingoPanic):  # a projection checker that was never set
        p = buckler.LinCheckPlan(F, rank, emb, [buckler.ProjChecker(F, rank)], [[(0, 1)]])
        p.lin_check_dev(A, A, B, C, 2, 4 * rank, D, 0x50000, 0x60000, 0x70000)


def _oracle_cons(cons):
    return [[(c.coeffs[i], c.coeffsPublicWitness[i] if c.hasCoeffPublicWitness[i] else None, c.witness[i])
             for i in range(len(c.coeffs))] for c in cons]


def _circuit(F, ref, rng):
    """Constraints in the style of test_gpu_buckler.py's _circuit: products, a public-witness
    coefficient, a constant term, an empty constraint."""
    k = ref.arr(rand_ints(ref.q, 2, rng))
    c0 = buckler.ArithmeticConstraint(F)
    c0.AddTerm(None, 0, 1)
    c0.SubTerm(None, 2)
    c1 = buckler.ArithmeticConstraint(F)
    c1.AddTermWithConst(k[0], 1, 3, 0)
    c1.AddTerm(0, 2, 2)
    c1.AddTermWithConst(k[1], None)
    c2 = buckler.ArithmeticConstraint(F)
    c3 = buckler.ArithmeticConstraint(F)
    c3.AddTerm(None, 3)
    return [c0, c1, c2, c3]


@pytest.mark.parametrize("key", GOLD)
def test_sum_check_and_arith_check(key):
    """SumCheck / ArithCheck through the mirror: the oracle's evalCircuit plus the restated tail."""
    F, ref = _ctx(key)
    rank, emb, jindo_rank = 128, 512, 1024
    rng = np.random.default_rng(17)
    cons = _circuit(F, ref, rng)
    max_rank = max(c.maxRank(rank) for c in cons)  # 3 rank + 1 <= emb
    assert rank < max_rank <= emb
    w = np.stack([ref.arr(rand_ints(ref.q, emb, rng)) for _ in range(4)])
    pw = np.stack([ref.arr(rand_ints(ref.q, emb, rng)) for _ in range(2)])
    bc = rand_ints(ref.q, 1, rng)[0]
    bca = ref.arr([bc])[0]
    ev = ref.ints(ref.cf.buckler_eval_circuit(_oracle_cons(cons), bca, w, pw))
    mask, _ = R.sumCheckMask(ref, rank, max_rank, emb, rand_ints(ref.q, max_rank, rng))
    want = R.sumCheck(ref, rank, jindo_rank, max_rank, bc, mask, ev)
    wp = [ringo.Poly(F, emb, True, x) for x in w]
    pp = [ringo.Poly(F, emb, True, x) for x in pw]
    got = buckler.SumCheck(F, rank, emb, jindo_rank, max_rank, bca, ref.arr(mask), cons, wp, pp)
    for g, x in zip(got, want):
        assert (g == ref.arr(x)).all()
    assert got[0].shape[0] == max_rank - rank and got[1].shape[0] == rank - 1 and got[2].shape[0] == jindo_rank
    quo, lo, hi = buckler.ArithCheck(F, rank, emb, max_rank, bca, cons, wp, pp)
    assert lo is None and hi is None
    assert (quo == ref.arr(R.arithCheck(ref, rank, max_rank, ev))).all()
