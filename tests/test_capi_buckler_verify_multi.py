"""CPU: argument checks of the entries the verifier's batch call adds (include/ringo.h:
rg_buckler_verify_checks_multi*, rg_poly_evaluate_multi*, rg_buckler_powers_batch*,
rg_buckler_checker_transpose_xof*).  Each returns RG_ERR_INVALID before it touches the device, so none
needs a GPU.  The device addresses below are made-up numbers: a call that read them would crash, not
fail.

A field handle and a projection or automorphism checker are host objects, so the evaluate's, the power
table's and the projection transpose's refusals all run here.  The verifier's own refusals past the
NULL handle (NULL outputs, the d_xof rule, aliased buffers, n_proofs over the limit) need an rg_bverifier,
hence an NTT plan, and a plan uploads its tables when it is created: those run with live plans in
test_gpu_buckler_verify_multi.py::test_argument_errors_with_live_plans."""
import ctypes
import re

import ringo
from ringo import _lib, bigpoly, buckler

INVALID = -1
A = [0x10000 * (i + 1) for i in range(10)]  # distinct fake device addresses
Q = 2 ** 61 - 1


def _why():
    return _lib.lib().rg_last_error().decode()


def test_null_handle_rejected_no_gpu():
    L = _lib.lib()
    assert L.rg_buckler_verify_checks_multi_scratch_bytes(None, 4) == 0
    assert L.rg_buckler_verify_checks_multi_dev(None, 4, *A[:9], None) == INVALID
    assert "NULL handle" in _why()
    assert L.rg_buckler_verify_checks_multi_dev(None, 0, *A[:9], None) == INVALID
    assert L.rg_buckler_verify_checks_multi(None, 4, None, None, None, None, None, None, None, None) == INVALID
    assert "NULL handle" in _why()


def test_the_limit_is_in_the_header_and_the_mirror_has_the_entries():
    src = open(_lib.HEADER).read()
    m = re.search(r"#define RG_BK_MULTI_MAX_PROOFS (\d+)", src)
    assert m and int(m.group(1)) == 65535
    for name in ("checks_multi_dev", "checks_multi", "scratch_bytes_multi"):
        assert hasattr(buckler.VerifyPlan, name), name
    assert hasattr(buckler.ProjChecker, "transpose_xof_dev")
    assert callable(buckler.PowersBatch) and callable(buckler.powers_batch_dev)
    assert callable(bigpoly.EvaluateMulti) and callable(bigpoly.evaluate_multi_dev)
    assert callable(bigpoly.evaluate_multi_scratch_bytes)


def test_evaluate_multi_refusals_no_gpu():
    L = _lib.lib()
    F = ringo.Field(Q)

    def dev(n=8, stride=8, batch=4, x_stride=1, n_points=2, group=2, f=F.h, scratch=A[3]):
        return L.rg_poly_evaluate_multi_dev(f, A[0], n, stride, batch, A[1], x_stride, n_points, group, A[2], scratch,
                                            None)

    for kw in (dict(group=0), dict(n_points=0), dict(x_stride=0)):
        assert dev(**kw) == INVALID and "is 0" in _why(), kw
        assert dev(batch=0, **kw) == INVALID, kw  # refused even where nothing would be launched
    assert dev(stride=7) == INVALID and "stride" in _why()
    assert dev(f=None) == INVALID
    assert dev(scratch=None) == INVALID and "scratch" in _why()
    assert dev(batch=1 << 17, group=1, n_points=1 << 17) == INVALID and "65535" in _why()
    assert dev(batch=0) == 0
    assert L.rg_poly_evaluate_multi(F.h, None, 0, 0, 2, None, 1, 1, 1, None) == INVALID  # NULL x and out
    assert L.rg_poly_evaluate_multi_scratch_bytes(None, 8, 4, 2) == 0
    # a table pair per point in use (257 + 17 elements), a tile sum per polynomial
    assert L.rg_poly_evaluate_multi_scratch_bytes(F.h, 8, 4, 2) == (2 * 274 + 4) * 8
    assert L.rg_poly_evaluate_multi_scratch_bytes(F.h, 8, 4, 9) == (4 * 274 + 4) * 8
    assert L.rg_poly_evaluate_multi_scratch_bytes(F.h, 8, 4, 1) == L.rg_poly_evaluate_batch_scratch_bytes(F.h, 8, 4)


def test_powers_batch_refusals_no_gpu():
    L = _lib.lib()
    F = ringo.Field(Q)
    call = L.rg_buckler_powers_batch_dev
    assert call(None, A[0], 1, 3, 4, A[1], None) == INVALID
    assert call(F.h, A[0], 0, 3, 4, A[1], None) == INVALID  # c_stride = 0
    assert call(F.h, A[0], 1, 65536, 4, A[1], None) == INVALID  # a base per grid row
    assert call(F.h, A[0], 1, 3, 4, A[0], None) == INVALID  # d_out == d_c
    assert call(F.h, None, 1, 3, 4, A[1], None) == INVALID
    assert call(F.h, A[0], 1, 3, 4, None, None) == INVALID
    assert call(F.h, A[0], 1, 0, 4, A[1], None) == 0 and call(F.h, A[0], 1, 3, 0, A[1], None) == 0
    assert L.rg_buckler_powers_batch(F.h, None, 1, 3, 4, None) == INVALID


def test_transpose_xof_refusals_no_gpu():
    L = _lib.lib()
    F = ringo.Field(Q)
    call = L.rg_buckler_checker_transpose_xof_dev
    assert call(None, A[0], A[1], 1, A[2], A[3], None) == INVALID
    assert L.rg_buckler_checker_transpose_xof_scratch_bytes(None, 2) == 0
    aut = buckler.NewAutChecker(F, 128, 5, False)
    assert call(aut.h, A[0], A[1], 1, A[2], A[3], None) == INVALID  # a projection checker only
    assert L.rg_buckler_checker_transpose_xof_scratch_bytes(aut.h, 2) == 0
    proj = buckler.ProjChecker(F, 128)  # never set: accepted by this entry, so the refusals below are the arguments'
    assert L.rg_buckler_checker_transpose_xof_scratch_bytes(proj.h, 2) == 2 * 128 * 16
    for args in ((None, A[1], 1, A[2], A[3]), (A[0], None, 1, A[2], A[3]), (A[0], A[0], 1, A[2], A[3]),
                 (A[0], A[1], 1, None, A[3]), (A[0], A[1], 1, A[2], None), (A[0], A[1], 1, A[2], A[1]),
                 (A[0], A[1], 65536, A[2], A[3])):
        assert call(proj.h, *args, None) == INVALID, args
    assert call(proj.h, A[0], A[1], 0, A[2], A[3], None) == 0
    h = ctypes.c_void_p()
    assert L.rg_buckler_checker_create_proj(F.h, 127, ctypes.byref(h)) == INVALID
