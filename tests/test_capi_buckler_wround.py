"""CPU: the refusals of the prover's two witness rounds (include/ringo.h: rg_buckler_dcmp_round_create,
rg_buckler_prove_dcmp_round*, rg_buckler_encode_round_create, rg_buckler_prove_encode_round*).  Creating
an rg_bdcmp touches no device, and neither does creating the rg_dcmp handles it borrows, so every refusal
of the decomposition round runs here with live handles; each returns its status with a reason in
rg_last_error before the device is touched.  Creating an rg_bencode touches no device either, but the NTT
plan it borrows uploads its tables when it is made: here are the refusals that need no plan, and the rest
run with a live plan in test_gpu_buckler_wround_encode.py.  The device addresses below are made-up
numbers: a call that read them would crash, not fail."""
import ctypes
import re

import numpy as np
import pytest

import ringo
from ringo import _lib, buckler
from ringo.bigpoly import RingoPanic

INVALID, UNSUPPORTED = -1, -3
A, B, C, D, E = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000  # distinct fake device addresses


def _why():
    return _lib.lib().rg_last_error().decode()


@pytest.fixture(scope="module")
def F(fields):
    return ringo.Field(fields["p63"])


@pytest.fixture(scope="module")
def F2(fields):
    return ringo.Field(fields["mult_zp"])


def _u64(xs):
    return (ctypes.c_uint64 * max(1, len(xs)))(*xs)


def _handles(dcs):
    return (ctypes.c_void_p * max(1, len(dcs)))(*[d.h.value if d is not None else None for d in dcs])


def _dcmp_create(f, rank, n_w, inf=(), two=(), null=(), out=True):
    """inf: (src, Decomposer, [rows]); two: (src, Decomposer, dst); null: names of arrays passed as NULL."""
    arrays = dict(inf_src=_u64([c[0] for c in inf]), inf_dcmp=_handles([c[1] for c in inf]),
                  inf_rows=_u64([r for c in inf for r in c[2]]), two_cons=_u64([i for c in two for i in (c[0], c[2])]),
                  two_dcmp=_handles([c[1] for c in two]))
    for name in null:
        arrays[name] = None
    h = ctypes.c_void_p(1)
    st = _lib.lib().rg_buckler_dcmp_round_create(f, rank, n_w, len(inf), arrays["inf_src"], arrays["inf_dcmp"],
                                                 arrays["inf_rows"], len(two), arrays["two_cons"], arrays["two_dcmp"],
                                                 ctypes.byref(h) if out else None)
    return st, h


def _enc_create(plan, emb, n_w, sel, n_sel=None, null_sel=False, out=True):
    h = ctypes.c_void_p(1)
    st = _lib.lib().rg_buckler_encode_round_create(plan, emb, n_w, len(sel) if n_sel is None else n_sel,
                                                   None if null_sel else _u64(sel), ctypes.byref(h) if out else None)
    return st, h


# ---- the decomposition round -----------------------------------------------------------------------
def test_dcmp_handle_is_created_and_destroyed_with_no_device(F):
    L = _lib.lib()
    dc3, dc1 = buckler.Decomposer(F, [4, 2, 1]), buckler.Decomposer(F, [1])
    scr = L.rg_buckler_prove_dcmp_round_scratch_bytes
    # n_proofs * n_two * ceil(rank / 1024) * L * 8
    for rank, chunks in ((200, 1), (1024, 1), (1025, 2), (2500, 3), (1 << 15, 32)):
        st, h = _dcmp_create(F.h, rank, 8, inf=[(0, dc3, [1, 2, 3])], two=[(0, dc1, 4), (5, dc3, 6)])
        assert st == 0 and h.value
        assert scr(h, 1) == 2 * chunks * 8 and scr(h, 64) == 64 * 2 * chunks * 8
        L.rg_buckler_dcmp_round_destroy(h)
    st, h = _dcmp_create(F.h, 2500, 8, inf=[(0, dc3, [1, 2, 3])])  # no two-norm constraint: no scratch
    assert st == 0 and scr(h, 5) == 0
    L.rg_buckler_dcmp_round_destroy(h)
    L.rg_buckler_dcmp_round_destroy(None)  # as free(NULL)


def test_dcmp_create_refusals(F, F2):
    dc1, dc3 = buckler.Decomposer(F, [1]), buckler.Decomposer(F, [4, 2, 1])
    other = buckler.Decomposer(F2, [4, 2, 1])
    ok = dict(f=F.h, rank=200, n_w=8, inf=[(0, dc3, [1, 2, 3])], two=[(0, dc3, 4)])

    def refused(why, **kw):
        st, h = _dcmp_create(**{**ok, **kw})
        assert st == INVALID and h.value is None, kw
        assert _why().startswith("buckler dcmp round:") and why in _why(), (kw, _why())

    refused("NULL field", f=None)
    refused("rank", rank=0)
    refused("rank", rank=(1 << 30) + 1)
    refused("n_w", n_w=0)
    refused("n_inf + n_two = 0", inf=[], two=[])
    refused("is over 32", inf=[(0, dc1, [i + 1]) for i in range(33)], two=[], n_w=100)
    refused("is over 32", inf=[], two=[(0, dc1, i + 1) for i in range(33)], n_w=100)
    for name in ("inf_src", "inf_dcmp", "inf_rows"):
        refused("NULL infinity-norm", null=[name])
    for name in ("two_cons", "two_dcmp"):
        refused("NULL two-norm", null=[name])
    refused("NULL decomposition", inf=[(0, None, [])])
    refused("NULL decomposition", two=[(0, None, 4)])
    # an index >= n_w: a src, a digit row, a dst
    refused(">= n_w", inf=[(8, dc3, [1, 2, 3])])
    refused(">= n_w", inf=[(0, dc3, [1, 2, 8])])
    refused(">= n_w", inf=[(0, dc3, [1 << 40, 2, 3])])
    refused(">= n_w", two=[(8, dc3, 4)])
    refused(">= n_w", two=[(0, dc3, 8)])
    refused("another field", inf=[(0, other, [1, 2, 3])])
    refused("another field", two=[(0, other, 4)])
    refused("another field", f=F2.h)
    refused("nb > rank", rank=2)  # the two-norm digits do not fit the row
    refused("nb > rank", rank=2, inf=[])
    # an output row that is any constraint's src
    refused("src", inf=[(0, dc3, [1, 0, 3])])
    refused("src", two=[(0, dc3, 0)])
    refused("src", two=[(5, dc3, 0)])  # dst is the infinity-norm constraint's src
    refused("src", inf=[(0, dc3, [1, 2, 5])], two=[(5, dc3, 4)])  # a digit row is the two-norm constraint's src
    # an output row that is another output row
    refused("twice", inf=[(0, dc3, [1, 2, 1])])
    refused("twice", two=[(0, dc3, 3)])  # dst is a digit row
    refused("twice", inf=[(0, dc3, [1, 2, 3]), (5, dc1, [2])], two=[])
    refused("twice", inf=[], two=[(0, dc3, 4), (5, dc1, 4)])
    st, _ = _dcmp_create(**ok, out=False)
    assert st == INVALID and "NULL out" in _why()
    # accepted: a shared src, non-consecutive rows in any order, nb = rank, 32 + 32 constraints, one kind alone
    L = _lib.lib()
    for kw in (dict(inf=[(0, dc3, [7, 2, 5]), (0, dc1, [3])]), dict(rank=3), dict(inf=[]), dict(two=[]),
               dict(inf=[(0, dc1, [i + 1]) for i in range(32)], two=[(0, dc1, 40 + i) for i in range(32)], n_w=100)):
        st, h = _dcmp_create(**{**ok, **kw})
        assert st == 0 and h.value, (kw, _why())
        L.rg_buckler_dcmp_round_destroy(h)
    # rank below nb is fine for an infinity-norm constraint alone: a digit row per base element
    st, h = _dcmp_create(F.h, 1, 8, inf=[(0, dc3, [1, 2, 3])])
    assert st == 0
    L.rg_buckler_dcmp_round_destroy(h)
    G = ringo.Field((1 << 130) + 5 | 1, limbs=3)  # a limb count with no kernel: refused before the handles are read
    st, h = _dcmp_create(G.h, 200, 8, inf=[(0, dc3, [1, 2, 3])])
    assert st == UNSUPPORTED and h.value is None and "3 limbs" in _why()


def test_dcmp_round_refusals_with_a_live_handle(F):
    L = _lib.lib()
    dc = buckler.Decomposer(F, [4, 2, 1])
    st, h = _dcmp_create(F.h, 2500, 6, inf=[(0, dc, [1, 2, 3])], two=[(0, dc, 4)])
    st2, h_inf = _dcmp_create(F.h, 2500, 6, inf=[(0, dc, [1, 2, 3])])
    assert st == 0 and st2 == 0
    rnd, host, scr = L.rg_buckler_prove_dcmp_round_dev, L.rg_buckler_prove_dcmp_round, \
        L.rg_buckler_prove_dcmp_round_scratch_bytes
    try:
        for n in (0, 4, 65536, 1 << 40):
            assert scr(None, n) == 0
        assert rnd(None, 4, A, B, C, None) == INVALID and "NULL handle" in _why()
        assert rnd(None, 0, A, B, C, None) == INVALID  # refused even where nothing would run
        assert host(None, 4, None, None) == INVALID and "NULL handle" in _why()
        assert rnd(h, 0, None, None, None, None) == 0  # nothing to do
        assert host(h, 0, None, None) == 0
        assert scr(h, 0) == 0 and scr(h, 65535) == 65535 * 3 * 8
        for n in (65536, 1 << 40):  # over RG_BK_MULTI_MAX_PROOFS: refused, and no scratch
            assert rnd(h, n, A, B, C, None) == INVALID and "n_proofs" in _why()
            assert host(h, n, None, None) == INVALID and "n_proofs" in _why()
            assert scr(h, n) == 0
        assert rnd(h, 2, None, B, C, None) == INVALID and "NULL witness" in _why()
        assert rnd(h, 2, A, B, None, None) == INVALID and "NULL scratch" in _why()
        assert rnd(h, 2, A, None, None, None) == INVALID and "NULL scratch" in _why()
        for w, sq, s in ((A, A, C), (A, B, A), (A, B, B), (A, None, A)):
            assert rnd(h, 2, w, sq, s, None) == INVALID and "alias" in _why(), (w, sq, s)
        # sq belongs to the two-norm constraints
        assert rnd(h_inf, 2, A, B, None, None) == INVALID and "no two-norm" in _why()
        assert rnd(h_inf, 2, A, None, A, None) == INVALID and "alias" in _why()
        one = np.ones(4, np.uint64)
        assert host(h, 1, None, _lib.ptr(one)) == INVALID
        assert host(h, 1, _lib.ptr(one), _lib.ptr(one)) == INVALID and "alias" in _why()
    finally:
        L.rg_buckler_dcmp_round_destroy(h)
        L.rg_buckler_dcmp_round_destroy(h_inf)


# ---- the encode round ----------------------------------------------------------------------------------
# An rg_bencode borrows an NTT plan, and a plan uploads its tables when it is created, so the refusals
# past the NULL plan and the NULL handle run with a live plan in test_gpu_buckler_wround_encode.py
# (test_create_refusals_with_a_live_plan, test_round_refusals_with_a_live_handle).
def test_encode_create_refuses_a_null_plan_and_a_null_out():
    st, h = _enc_create(None, 256, 5, [3, 0])
    assert st == INVALID and h.value is None and "buckler encode round: NULL plan" in _why()
    st, _ = _enc_create(A, 256, 5, [3, 0], out=False)  # out is looked at first: the plan is never read
    assert st == INVALID and "NULL out" in _why()
    _lib.lib().rg_buckler_encode_round_destroy(None)  # as free(NULL)


def test_encode_round_refuses_a_null_handle():
    L = _lib.lib()
    for n in (0, 4, 65536, 1 << 40):
        assert L.rg_buckler_prove_encode_round_scratch_bytes(None, n) == 0
    assert L.rg_buckler_prove_encode_round_dev(None, 4, A, B, C, D, E, None) == INVALID and "NULL handle" in _why()
    assert L.rg_buckler_prove_encode_round_dev(None, 0, A, B, C, D, E, None) == INVALID
    assert L.rg_buckler_prove_encode_round(None, 4, None, None, None, None) == INVALID and "NULL handle" in _why()


# ---- header and mirror ---------------------------------------------------------------------------------
def test_the_header_states_the_calls_and_the_mirror_has_the_entries(F):
    src = open(_lib.HEADER).read()
    names = ("rg_buckler_dcmp_round_create", "rg_buckler_dcmp_round_destroy",
             "rg_buckler_prove_dcmp_round_scratch_bytes", "rg_buckler_prove_dcmp_round_dev",
             "rg_buckler_prove_dcmp_round", "rg_buckler_encode_round_create", "rg_buckler_encode_round_destroy",
             "rg_buckler_prove_encode_round_scratch_bytes", "rg_buckler_prove_encode_round_dev",
             "rg_buckler_prove_encode_round")
    for name in names:
        assert name in _lib._SIGS and re.search(r"\b%s\(" % name, src), name
        assert hasattr(_lib.lib(), name), name
    assert len(_lib._SIGS["rg_buckler_prove_dcmp_round_dev"][1]) == 6
    assert len(_lib._SIGS["rg_buckler_prove_encode_round_dev"][1]) == 8
    flat = " ".join(src.split()).replace(" * ", " ").replace("* ", "")
    assert "n_proofs n_two ceil(rank / 1024) L 8 bytes" in flat  # the scratch formulas
    assert "n_proofs n_sel rank L 8 bytes" in flat
    assert "first-use rule of rg_dcmp" in src
    assert "rg_ntt_fwd_dev(emb_plan, d_wecd, d_wecd, n_proofs * n_w)" in src  # the forward transform is the caller's
    for cls in (buckler.DcmpRoundPlan, buckler.EncodeRoundPlan):
        for name in ("round_dev", "round", "scratch_bytes"):
            assert hasattr(cls, name), (cls, name)
    # a bound in place of a Decomposer: the base is decomposeBase(bound)
    plan = buckler.DcmpRoundPlan(F, 2500, 8, inf=[(0, 8, [1, 2, 3])], two=[(0, buckler.Decomposer(F, 3), 4)])
    assert plan.inf[0][1].dcmpBase == [4, 2, 1] and plan.two[0][1].dcmpBase == [2, 1]
    assert plan.scratch_bytes(3) == 3 * 1 * 3 * 8 and plan.scratch_bytes(65536) == 0
    with pytest.raises(RingoPanic):
        buckler.DcmpRoundPlan(F, 2500, 8, inf=[(0, 8, [1, 2])])  # a digit row per base element
    with pytest.raises(RingoPanic):
        buckler.DcmpRoundPlan(F, 2500, 8, two=[(0, 8, 0)])
