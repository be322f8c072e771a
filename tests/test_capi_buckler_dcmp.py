"""CPU: argument checks of the Buckler norm-decomposition entry points (include/ringo.h,
rg_buckler_dcmp_*).  Each returns RG_ERR_INVALID before it touches the device, and creating a handle
uploads nothing (the base goes to the device with the first kernel), so none of this needs a GPU.
The device addresses below are made-up numbers: a call that read them would crash, not fail."""
import ctypes

import numpy as np
import pytest

import ringo
from ringo import _lib, buckler
from ringo.bigpoly import RingoPanic

INVALID = -1
A, B, C, D = 0x10000, 0x20000, 0x30000, 0x40000  # distinct fake device addresses


def _create(f, base, nb):
    h = ctypes.c_void_p()
    return _lib.lib().rg_buckler_dcmp_create(f, _lib.ptr(base) if base is not None else None, nb, ctypes.byref(h)), h


@pytest.fixture(scope="module")
def F(fields):
    return ringo.Field(fields["p63"])


@pytest.fixture(scope="module")
def F2(fields):
    return ringo.Field(fields["mult_zp"])


def test_null_handles_rejected_no_gpu(F):
    L = _lib.lib()
    one = np.ones(1, np.uint64)
    assert _create(None, one, 1)[0] == INVALID
    assert L.rg_buckler_dcmp_create(F.h, _lib.ptr(one), 1, None) == INVALID
    assert L.rg_buckler_dcmp_inf_dev(None, A, 1, 128, B, None) == INVALID
    assert L.rg_buckler_dcmp_proj_dev(None, A, 128, B, None) == INVALID
    assert L.rg_buckler_dcmp_two_dev(None, A, 1, 128, B, C, D, None) == INVALID
    assert L.rg_buckler_dcmp_two_scratch_bytes(None, 3, 4096) == 0
    assert L.rg_buckler_dcmp_inf(None, _lib.ptr(one), 1, 1, _lib.ptr(one)) == INVALID
    assert L.rg_buckler_dcmp_proj(None, _lib.ptr(one), 128, _lib.ptr(one)) == INVALID
    assert L.rg_buckler_dcmp_two(None, _lib.ptr(one), 1, 1, _lib.ptr(one), None) == INVALID
    L.rg_buckler_dcmp_destroy(None)


def test_create_argument_errors_no_gpu(F, F2):
    one = np.ones(1, np.uint64)
    assert _create(F.h, one, 0)[0] == INVALID   # nb = 0
    assert _create(F.h, None, 1)[0] == INVALID
    assert _create(F.h, np.array([4, 0, 1], np.uint64), 3)[0] == INVALID  # a zero base element
    assert _create(F2.h, np.array([1, 0, 0, 0], np.uint64), 2)[0] == INVALID  # [1, 0] at L = 2: the second is zero
    st, h = _create(F2.h, np.array([0, 1, 1, 0], np.uint64), 2)  # 2^64 and 1: a high limb alone is not zero
    assert st == 0
    _lib.lib().rg_buckler_dcmp_destroy(h)
    st, h = _create(F.h, np.array([F.q, (1 << 64) - 1], np.uint64), 2)  # plain integers: no need to be below q
    assert st == 0
    _lib.lib().rg_buckler_dcmp_destroy(h)
    G = ringo.Field((1 << 130) + 5 | 1, limbs=3)  # a limb count with no kernel
    assert _create(G.h, np.ones(3, np.uint64), 1)[0] == -3


def test_apply_argument_errors_no_gpu(F):
    """A live handle: creation touches no device, so the shape and aliasing checks run here."""
    L = _lib.lib()
    st, h = _create(F.h, np.array([4, 2, 1], np.uint64), 3)  # decomposeBase(8)
    assert st == 0
    try:
        inf, proj, two = L.rg_buckler_dcmp_inf_dev, L.rg_buckler_dcmp_proj_dev, L.rg_buckler_dcmp_two_dev
        assert inf(h, A, 1, 128, A, None) == INVALID       # d_out == d_w
        assert inf(h, None, 1, 128, B, None) == INVALID
        assert inf(h, A, 1, 128, None, None) == INVALID
        assert inf(h, A, 1, 0, B, None) == INVALID
        assert inf(h, A, 1, (1 << 30) + 1, B, None) == INVALID
        assert inf(h, A, 1 << 16, 128, B, None) == INVALID  # batch beyond the grid's y extent
        assert inf(h, A, 0, 128, B, None) == 0              # nothing to do
        assert proj(h, A, 384, A, None) == INVALID          # aliased
        assert proj(h, None, 384, B, None) == INVALID
        assert proj(h, A, 384, None, None) == INVALID
        assert proj(h, A, 127, B, None) == INVALID          # rank < 128
        assert proj(h, A, 383, B, None) == INVALID          # 128 nb = 384 > rank
        assert proj(h, A, 256, B, None) == INVALID
        assert two(h, A, 1, 128, A, None, D, None) == INVALID  # d_out == d_w
        assert two(h, A, 1, 2, B, None, D, None) == INVALID    # nb = 3 > rank
        assert two(h, A, 1, 0, B, None, D, None) == INVALID
        assert two(h, A, 1, 128, B, None, None, None) == INVALID  # no scratch
        assert two(h, A, 1, 128, B, A, D, None) == INVALID     # d_sq aliases d_w
        assert two(h, A, 1, 128, B, B, D, None) == INVALID     # d_sq aliases d_out
        assert two(h, A, 1, 128, B, D, D, None) == INVALID     # d_sq aliases d_scratch
        assert two(h, A, 1, 128, B, C, A, None) == INVALID     # d_scratch aliases d_w
        assert two(h, A, 1, 128, B, C, B, None) == INVALID     # d_scratch aliases d_out
        assert two(h, None, 1, 128, B, C, D, None) == INVALID
        assert two(h, A, 0, 128, B, C, D, None) == 0
        # one partial sum per 1024 coefficients and witness, L = 1
        assert L.rg_buckler_dcmp_two_scratch_bytes(h, 3, 4096) == 3 * 4 * 8
        assert L.rg_buckler_dcmp_two_scratch_bytes(h, 1, 200) == 8
        assert L.rg_buckler_dcmp_two_scratch_bytes(h, 2, 1025) == 2 * 2 * 8
        one = np.ones(4, np.uint64)
        assert L.rg_buckler_dcmp_inf(h, _lib.ptr(one), 1, 4, _lib.ptr(one)) == INVALID  # aliased host buffers
        assert L.rg_buckler_dcmp_proj(h, _lib.ptr(one), 4, _lib.ptr(np.ones(4, np.uint64))) == INVALID
        assert L.rg_buckler_dcmp_two(h, _lib.ptr(one), 1, 2, _lib.ptr(np.ones(4, np.uint64)), None) == INVALID
    finally:
        L.rg_buckler_dcmp_destroy(h)


def test_mirror_panics_no_gpu(F):
    for bad in (0, 1, [], [4, 0, 1], [-1]):  # decomposeBase(0 / 1) panics; an empty or non-positive base
        with pytest.raises(RingoPanic):
            buckler.Decomposer(F, bad)
    dc = buckler.Decomposer(F, 8)
    assert dc.dcmpBase == [4, 2, 1]
    assert buckler.Decomposer(F, [1 << 70, 5, 1]).dcmpBase == [1 << 70, 5, 1]  # saturated in the handle only
    with pytest.raises(RingoPanic):
        dc.DecomposeProj(np.zeros((256, 1), np.uint64))  # 128 nb > rank
    with pytest.raises(RingoPanic):
        dc.DecomposeTwoNorm(np.zeros((2, 1), np.uint64))  # nb > rank
    with pytest.raises(RingoPanic):
        dc.DecomposeInf(np.zeros((8, 2), np.uint64))      # another field's limb count
    assert dc.scratch_bytes(3, 4096) == 96
