"""CPU: argument checks of the Buckler linear-check / sum-check entry points (include/ringo.h,
rg_buckler_checker_*, rg_buckler_powers*, rg_buckler_sumcheck_mask*, rg_buckler_check_finish*,
rg_buckler_lin*).  Each returns RG_ERR_INVALID before it touches the device, so none needs a GPU.
The device addresses below are made-up numbers: a call that read them would crash, not fail.

The checks that need an NTT plan to get past the NULL test (jindo_rank < rank - 1, a pair index
>= n_w, a checker of another rank) run with live plans in test_gpu_buckler_lin.py: a plan uploads
its tables when it is created."""
import ctypes

import numpy as np
import pytest

import ringo
from ringo import _lib, buckler
from ringo.bigpoly import RingoPanic

INVALID = -1
A, B, C, D = 0x10000, 0x20000, 0x30000, 0x40000  # distinct fake device addresses


def _create(fn, *args):
    h = ctypes.c_void_p()
    return getattr(_lib.lib(), fn)(*args, ctypes.byref(h)), h


@pytest.fixture(scope="module")
def F(fields):
    return ringo.Field(fields["p63"])


def test_null_handles_rejected_no_gpu(F):
    L = _lib.lib()
    one = np.ones(1, np.uint64)
    for fn in ("rg_buckler_checker_create_ntt", "rg_buckler_checker_create_proj"):
        assert _create(fn, None, 128)[0] == INVALID
        assert getattr(L, fn)(F.h, 128, None) == INVALID
    assert _create("rg_buckler_checker_create_aut", None, 128, 5, 0)[0] == INVALID
    assert _create("rg_buckler_checker_create_recompose", None, 128, _lib.ptr(one), 1)[0] == INVALID
    assert L.rg_buckler_checker_set_xof_dev(None, A, None) == INVALID
    assert L.rg_buckler_checker_set_xof(None, b"\0" * 32) == INVALID
    assert L.rg_buckler_checker_scratch_bytes(None, 3) == 0
    assert L.rg_buckler_checker_transform_dev(None, A, B, 1, C, None) == INVALID
    assert L.rg_buckler_checker_transpose_dev(None, A, B, 1, None) == INVALID
    assert L.rg_buckler_checker_transform(None, _lib.ptr(one), _lib.ptr(one)) == INVALID
    assert L.rg_buckler_checker_transpose(None, _lib.ptr(one), _lib.ptr(one)) == INVALID
    assert L.rg_buckler_powers_dev(None, A, 4, B, None) == INVALID
    assert L.rg_buckler_powers(None, _lib.ptr(one), 1, _lib.ptr(one)) == INVALID
    assert L.rg_buckler_sumcheck_mask_dev(None, 128, 256, 256, A, B, C, None) == INVALID
    assert L.rg_buckler_sumcheck_mask(None, 128, 256, 256, None, None, None) == INVALID
    assert L.rg_buckler_check_finish_scratch_bytes(None) == 0
    assert L.rg_buckler_check_finish_dev(None, 128, A, None, None, 128, 1024, B, None, None, C, None) == INVALID
    assert L.rg_buckler_check_finish(None, 128, None, None, None, 0, 0, None, None, None) == INVALID
    assert _create("rg_buckler_lincheck_create", None, None, 0, None, None, None)[0] == INVALID
    assert L.rg_buckler_lin_check_scratch_bytes(None) == 0
    assert L.rg_buckler_lin_check_dev(None, A, A, A, A, 1, 1024, B, C, D, A, None) == INVALID
    assert L.rg_buckler_lin_check(None, None, None, None, None, 0, 0, None, None, None) == INVALID
    L.rg_buckler_checker_destroy(None)
    L.rg_buckler_lincheck_destroy(None)


def test_checker_create_argument_errors_no_gpu(F):
    one = np.ones(1, np.uint64)
    for rank in (0, 12, 129):  # an NTT is involved: the rank is a power of two
        assert _create("rg_buckler_checker_create_ntt", F.h, rank)[0] == INVALID
        assert _create("rg_buckler_checker_create_aut", F.h, rank, 5, 0)[0] == INVALID
    for idx in (0, 2, -4, 256):  # "modular inverse does not exist" / "AutTo: idx must be odd"
        assert _create("rg_buckler_checker_create_aut", F.h, 128, idx, 1)[0] == INVALID
    for rank in (0, 64, 127):  # TransformTo writes 128 rows
        assert _create("rg_buckler_checker_create_proj", F.h, rank)[0] == INVALID
    assert _create("rg_buckler_checker_create_recompose", F.h, 128, _lib.ptr(one), 0)[0] == INVALID
    assert _create("rg_buckler_checker_create_recompose", F.h, 128, None, 1)[0] == INVALID
    notred = np.array([F.q], np.uint64)  # base element not reduced
    assert _create("rg_buckler_checker_create_recompose", F.h, 128, _lib.ptr(notred), 1)[0] == INVALID


def test_checker_apply_argument_errors_no_gpu(F):
    """The automorphism and projection checkers hold no device memory at creation, so their
    argument checks can be exercised with no GPU."""
    L = _lib.lib()
    st, aut = _create("rg_buckler_checker_create_aut", F.h, 128, 5, 0)
    assert st == 0
    st, proj = _create("rg_buckler_checker_create_proj", F.h, 128)
    assert st == 0
    try:
        for chk in (aut, proj):
            assert L.rg_buckler_checker_transform_dev(chk, A, A, 1, C, None) == INVALID  # aliased in/out
            assert L.rg_buckler_checker_transpose_dev(chk, A, A, 1, None) == INVALID
            assert L.rg_buckler_checker_transform_dev(chk, None, B, 1, C, None) == INVALID
            assert L.rg_buckler_checker_transpose_dev(chk, A, None, 1, None) == INVALID
        # a projection checker whose matrix was never set
        assert L.rg_buckler_checker_transform_dev(proj, A, B, 1, C, None) == INVALID
        assert L.rg_buckler_checker_transpose_dev(proj, A, B, 1, None) == INVALID
        assert L.rg_buckler_checker_scratch_bytes(proj, 3) == 3 * 128 * 8  # one chunk of 128 rows, L = 1
        assert L.rg_buckler_checker_scratch_bytes(aut, 3) == 0
        # only a projection checker takes XOF bytes
        assert L.rg_buckler_checker_set_xof_dev(aut, A, None) == INVALID
        assert L.rg_buckler_checker_set_xof_dev(proj, None, None) == INVALID
    finally:
        L.rg_buckler_checker_destroy(aut)
        L.rg_buckler_checker_destroy(proj)


def test_powers_and_mask_argument_errors_no_gpu(F):
    L = _lib.lib()
    assert L.rg_buckler_powers_dev(F.h, None, 4, B, None) == INVALID
    assert L.rg_buckler_powers_dev(F.h, A, 4, None, None) == INVALID
    assert L.rg_buckler_powers_dev(F.h, A, 4, A, None) == INVALID  # aliased
    assert L.rg_buckler_powers_dev(F.h, A, 0, None, None) == 0     # nothing to do
    m = L.rg_buckler_sumcheck_mask_dev
    assert m(F.h, 128, 127, 256, A, B, C, None) == INVALID  # mask_rank < rank
    assert m(F.h, 128, 300, 256, A, B, C, None) == INVALID  # mask_rank > emb_rank
    assert m(F.h, 0, 0, 256, A, B, C, None) == INVALID
    assert m(F.h, 128, 256, 256, A, A, C, None) == INVALID  # d_rand aliases d_mask
    assert m(F.h, 128, 256, 256, None, B, C, None) == INVALID
    assert m(F.h, 128, 256, 256, A, None, C, None) == INVALID
    assert m(F.h, 128, 256, 256, A, B, None, None) == INVALID


def test_mirror_panics_no_gpu(F):
    with pytest.raises(RingoPanic, match="power of two"):
        buckler.NewNTTChecker(F, 12)
    with pytest.raises(RingoPanic, match="modular inverse does not exist"):
        buckler.NewAutChecker(F, 128, 6, False)
    with pytest.raises(RingoPanic):
        buckler.NewAutChecker(F, 100, 5, False)
    with pytest.raises(RingoPanic):
        buckler.ProjChecker(F, 64)
    for bound in (0, 1):  # decomposeBase indexes base[dcmpLen-1] of an empty slice
        with pytest.raises(RingoPanic):
            buckler.decomposeBase(bound)
    assert buckler.decomposeBase(8) == [4, 2, 1] and buckler.decomposeBase(10) == [5, 3, 1, 1]
    chk = buckler.NewAutChecker(F, 128, 5, True)
    with pytest.raises(RingoPanic):  # Go indexes past len(v)
        chk.TransformTo(np.zeros((128, 1), np.uint64), np.zeros((64, 1), np.uint64))
