"""CPU: the refusals of the projection round and of the batched masks (include/ringo.h:
rg_buckler_proj_round_create, rg_buckler_prove_proj_round*, rg_buckler_sumcheck_mask_batch*).  Creating
an rg_bproj touches no device, and neither does creating the rg_dcmp handles it borrows, so every
refusal runs here with live handles; each returns its status with a reason in rg_last_error before
the device is touched.  The device addresses below are made-up numbers: a call that read them would
crash, not fail."""
import ctypes
import re

import numpy as np
import pytest

import ringo
from ringo import _lib, buckler
from ringo.bigpoly import RingoPanic

INVALID, UNSUPPORTED = -1, -3
A, B, C, D = 0x10000, 0x20000, 0x30000, 0x40000  # distinct fake device addresses


def _why():
    return _lib.lib().rg_last_error().decode()


@pytest.fixture(scope="module")
def F(fields):
    return ringo.Field(fields["p63"])


@pytest.fixture(scope="module")
def F2(fields):
    return ringo.Field(fields["mult_zp"])


def _create(f, rank, n_w, cons, dcs, n_c=None, null_cons=False, null_dcmp=False, out=True):
    flat = [i for c in cons for i in c]
    arr = (ctypes.c_uint64 * max(1, len(flat)))(*flat)
    hs = (ctypes.c_void_p * max(1, len(dcs)))(*[d.h.value if d is not None else None for d in dcs])
    h = ctypes.c_void_p(1)
    st = _lib.lib().rg_buckler_proj_round_create(f, rank, n_w, len(cons) if n_c is None else n_c,
                                                 None if null_cons else arr, None if null_dcmp else hs,
                                                 ctypes.byref(h) if out else None)
    return st, h


def test_handle_is_created_and_destroyed_with_no_device(F):
    dc = buckler.Decomposer(F, [4, 2, 1])
    st, h = _create(F.h, 384, 5, [(0, 1, 2)], [dc])
    assert st == 0 and h.value
    L = _lib.lib()
    # one partial row of 128 elements per 512 columns, proof and constraint, L = 1
    assert L.rg_buckler_prove_proj_round_scratch_bytes(h, 3) == 3 * 1 * 1 * 128 * 8
    L.rg_buckler_proj_round_destroy(h)
    L.rg_buckler_proj_round_destroy(None)  # as free(NULL)
    st, h = _create(F.h, 1 << 15, 5, [(0, 1, 2), (0, 3, 4)], [dc, dc])
    assert st == 0
    assert L.rg_buckler_prove_proj_round_scratch_bytes(h, 64) == 64 * 2 * 64 * 128 * 8
    assert L.rg_buckler_prove_proj_round_scratch_bytes(h, 1) == 2 * 64 * 128 * 8
    L.rg_buckler_proj_round_destroy(h)
    st, h = _create(F.h, 513, 3, [(0, 1, 2)], [dc])  # a partial chunk opens a second workgroup
    assert st == 0 and L.rg_buckler_prove_proj_round_scratch_bytes(h, 1) == 2 * 128 * 8
    L.rg_buckler_proj_round_destroy(h)


def test_create_refusals(F, F2):
    dc1 = buckler.Decomposer(F, [1])
    dc3 = buckler.Decomposer(F, [4, 2, 1])
    other = buckler.Decomposer(F2, [4, 2, 1])
    ok = dict(f=F.h, rank=384, n_w=6, cons=[(0, 1, 2)], dcs=[dc3])

    def refused(why, **kw):
        st, h = _create(**{**ok, **kw})
        assert st == INVALID and h.value is None, kw
        assert _why().startswith("buckler proj round:") and why in _why(), (kw, _why())

    refused("NULL field", f=None)
    refused("rank", rank=127)
    refused("rank", rank=0)
    refused("rank", rank=(1 << 30) + 1)
    refused("n_w", n_w=0)
    refused("n_c", cons=[], dcs=[])
    refused("n_c", cons=[(0, 2 * i + 1, 2 * i + 2) for i in range(33)], dcs=[dc1] * 33, n_w=100)
    refused("NULL constraints", null_cons=True)
    refused("NULL constraints", null_dcmp=True)
    refused("NULL decomposition", dcs=[None])
    for bad in [(6, 1, 2), (0, 6, 2), (0, 1, 6), (1 << 40, 1, 2)]:
        refused(">= n_w", cons=[bad])
    refused("128 nb > rank", rank=383)
    refused("128 nb > rank", rank=256)
    refused("128 nb > rank", rank=128, cons=[(0, 1, 2), (0, 3, 4)], dcs=[dc1, dc3])  # any constraint
    refused("another field", dcs=[other])
    refused("another field", f=F2.h)
    # an output row equal to another output row or to any constraint's src
    refused("one row", cons=[(0, 1, 1)])
    refused("src", cons=[(0, 0, 2)])
    refused("src", cons=[(0, 1, 0)])
    refused("src", cons=[(0, 1, 2), (1, 3, 4)], dcs=[dc3, dc3])
    refused("src", cons=[(4, 1, 2), (0, 3, 4)], dcs=[dc3, dc3])
    refused("share", cons=[(0, 1, 2), (0, 1, 4)], dcs=[dc3, dc3])
    refused("share", cons=[(0, 1, 2), (0, 3, 2)], dcs=[dc3, dc3])
    refused("share", cons=[(0, 1, 2), (5, 2, 4)], dcs=[dc3, dc3])
    refused("share", cons=[(0, 1, 2), (5, 3, 1)], dcs=[dc3, dc3])
    st, _ = _create(**ok, out=False)
    assert st == INVALID and "NULL out" in _why()
    # accepted: a shared src, 128 nb = rank, 32 constraints
    L = _lib.lib()
    for kw in (dict(cons=[(0, 1, 2), (0, 3, 4)], dcs=[dc3, dc1]), dict(rank=128, dcs=[dc1]),
               dict(cons=[(0, 2 * i + 1, 2 * i + 2) for i in range(32)], dcs=[dc1] * 32, n_w=65)):
        st, h = _create(**{**ok, **kw})
        assert st == 0 and h.value, kw
        L.rg_buckler_proj_round_destroy(h)
    G = ringo.Field((1 << 130) + 5 | 1, limbs=3)  # a limb count with no kernel: refused before the handles are read
    st, h = _create(G.h, 384, 6, [(0, 1, 2)], [dc3])
    assert st == UNSUPPORTED and h.value is None and "3 limbs" in _why()


def test_round_refusals_with_a_live_handle(F):
    L = _lib.lib()
    dc = buckler.Decomposer(F, [4, 2, 1])
    st, h = _create(F.h, 384, 6, [(0, 1, 2)], [dc])
    assert st == 0
    rnd, host, scr = L.rg_buckler_prove_proj_round_dev, L.rg_buckler_prove_proj_round, \
        L.rg_buckler_prove_proj_round_scratch_bytes
    try:
        for n in (0, 4, 65536, 1 << 40):
            assert scr(None, n) == 0
        assert rnd(None, 4, A, B, C, None) == INVALID and "NULL handle" in _why()
        assert rnd(None, 0, A, B, C, None) == INVALID  # refused even where nothing would run
        assert host(None, 4, None, None) == INVALID and "NULL handle" in _why()
        assert rnd(h, 0, None, None, None, None) == 0  # nothing to do
        assert host(h, 0, None, None) == 0
        assert scr(h, 0) == 0 and scr(h, 65535) > 0
        for n in (65536, 1 << 40):  # over RG_BK_MULTI_MAX_PROOFS: refused, and no scratch
            assert rnd(h, n, A, B, C, None) == INVALID and "n_proofs" in _why()
            assert host(h, n, None, None) == INVALID and "n_proofs" in _why()
            assert scr(h, n) == 0
        assert rnd(h, 2, None, B, C, None) == INVALID and "NULL witness" in _why()
        assert rnd(h, 2, A, None, C, None) == INVALID and "NULL XOF" in _why()
        assert rnd(h, 2, A, B, None, None) == INVALID and "NULL scratch" in _why()
        for w, x, s in ((A, A, C), (A, B, A), (A, B, B)):
            assert rnd(h, 2, w, x, s, None) == INVALID and "alias" in _why(), (w, x, s)
        one = np.ones(4, np.uint64)
        assert host(h, 1, None, b"x") == INVALID and host(h, 1, _lib.ptr(one), None) == INVALID
    finally:
        L.rg_buckler_proj_round_destroy(h)


def test_mask_batch_refusals(F):
    L = _lib.lib()
    dev, host = L.rg_buckler_sumcheck_mask_batch_dev, L.rg_buckler_sumcheck_mask_batch

    def refused(why, *a):
        assert dev(*a, None) == INVALID and _why().startswith("buckler mask batch:") and why in _why(), (a, _why())

    refused("NULL field", None, 128, 256, 512, 2, A, B, C, D)
    # the single entry's constraints: rank >= 1, rank <= mask_rank <= emb_rank <= 2^40
    refused("rank", F.h, 0, 256, 512, 2, A, B, C, D)
    refused("rank", F.h, 128, 127, 512, 2, A, B, C, D)
    refused("rank", F.h, 128, 513, 512, 2, A, B, C, D)
    refused("rank", F.h, 128, 256, (1 << 40) + 1, 2, A, B, C, D)
    refused("n_proofs", F.h, 128, 256, 512, 65536, A, B, C, D)
    refused("n_proofs", F.h, 128, 256, 512, 1 << 40, A, B, C, D)
    refused("NULL buffer", F.h, 128, 256, 512, 2, None, B, C, D)
    refused("NULL buffer", F.h, 128, 256, 512, 2, A, None, C, D)
    refused("NULL buffer", F.h, 128, 256, 512, 2, A, B, C, None)
    for a in ((A, A, C, D), (A, B, A, D), (A, B, C, A), (A, B, B, D), (A, B, C, B), (A, B, C, C), (A, B, None, A),
              (A, B, None, B), (A, A, None, D)):
        refused("alias", F.h, 128, 256, 512, 2, *a)
    assert dev(F.h, 128, 256, 512, 0, None, None, None, None, None) == 0  # nothing to do
    assert dev(F.h, 128, 127, 512, 0, None, None, None, None, None) == INVALID  # the shape is checked even then
    G = ringo.Field((1 << 130) + 5 | 1, limbs=3)
    assert dev(G.h, 128, 256, 512, 2, A, B, C, D, None) == UNSUPPORTED and "3 limbs" in _why()
    one = np.ones(4, np.uint64)
    p = _lib.ptr(one)
    assert host(None, 1, 2, 4, 1, p, p, None, p) == INVALID
    assert host(F.h, 0, 2, 4, 1, p, _lib.ptr(np.ones(4, np.uint64)), None, _lib.ptr(np.ones(1, np.uint64))) == INVALID
    assert host(F.h, 1, 2, 4, 65536, p, _lib.ptr(np.ones(4, np.uint64)), None, _lib.ptr(np.ones(1, np.uint64))) == INVALID
    assert host(F.h, 1, 2, 4, 1, p, p, None, _lib.ptr(np.ones(1, np.uint64))) == INVALID and "alias" in _why()
    assert host(F.h, 1, 2, 4, 0, None, None, None, None) == 0
    assert host(G.h, 1, 2, 4, 1, p, p, None, p) == UNSUPPORTED


def test_the_header_states_the_calls_and_the_mirror_has_the_entries(F):
    src = open(_lib.HEADER).read()
    names = ("rg_buckler_proj_round_create", "rg_buckler_proj_round_destroy",
             "rg_buckler_prove_proj_round_scratch_bytes", "rg_buckler_prove_proj_round_dev",
             "rg_buckler_prove_proj_round", "rg_buckler_sumcheck_mask_batch_dev", "rg_buckler_sumcheck_mask_batch")
    for name in names:
        assert name in _lib._SIGS and re.search(r"\b%s\(" % name, src), name
        assert hasattr(_lib.lib(), name), name
    assert len(_lib._SIGS["rg_buckler_prove_proj_round_dev"][1]) == 6
    assert len(_lib._SIGS["rg_buckler_sumcheck_mask_batch_dev"][1]) == 10
    assert "ceil(rank / 512) * 128 * L * 8" in src  # the scratch formula
    for name in ("round_dev", "round", "scratch_bytes"):
        assert hasattr(buckler.ProjRoundPlan, name), name
    assert callable(buckler.SumCheckMaskBatch) and callable(buckler.sumcheck_mask_batch_dev)
    plan = buckler.ProjRoundPlan(F, 2048, 4, [(0, 1, 2, 5)])  # a bound: the base is decomposeBase(rank * bound)
    assert plan.constraints[0][3].dcmpBase == buckler.decomposeBase(2048 * 5)
    assert plan.scratch_bytes(3) == 3 * 4 * 128 * 8 and plan.scratch_bytes(65536) == 0
    with pytest.raises(RingoPanic):
        buckler.ProjRoundPlan(F, 2048, 4, [(0, 1, 1, 5)])
    with pytest.raises(RingoPanic):
        buckler.SumCheckMaskBatch(F, 128, 600, 512, np.zeros((1, 600, 1), np.uint64))
