"""CPU: argument checks of the Buckler verifier's entry points (include/ringo.h, rg_buckler_verifier_*,
rg_buckler_verify_checks*).  Each returns RG_ERR_INVALID with its reason in rg_last_error before it
touches the device, so none needs a GPU.  The device addresses below are made-up numbers: a call that
read them would crash, not fail.

Every other refusal of rg_buckler_verifier_create (a negacyclic plan, all three checks NULL, jindo_rank
< rank - 1, a linear check or circuit of another rank or field, an index >= w_cnt or >= n_pw) and of
the call itself (NULL and aliased buffers, a projection matrix never set) needs an NTT plan to get past
the NULL test, and a plan uploads its tables when it is created: those run with live plans in
test_gpu_buckler_verify.py::test_argument_errors_with_live_plans."""
import ctypes
import re

from ringo import _lib, buckler

INVALID = -1
A = [0x10000 * (i + 1) for i in range(8)]  # distinct fake device addresses


def _why():
    return _lib.lib().rg_last_error().decode()


def test_null_handles_rejected_no_gpu():
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.rg_buckler_verifier_create(None, 128, 4, 0, None, None, None, ctypes.byref(h)) == INVALID
    assert "NULL encoder plan" in _why() and not h.value
    assert L.rg_buckler_verifier_create(None, 128, 4, 0, None, None, None, None) == INVALID
    assert "NULL out" in _why()
    assert L.rg_buckler_verifier_n_evals(None) == 0
    assert L.rg_buckler_verify_checks_scratch_bytes(None) == 0
    assert L.rg_buckler_verify_checks_dev(None, *A, None) == INVALID
    assert "NULL handle" in _why()
    assert L.rg_buckler_verify_checks(None, None, None, None, None, None, None, None) == INVALID
    assert "NULL handle" in _why()
    L.rg_buckler_verifier_destroy(None)


def test_verdict_bits_are_the_headers():
    """The header defines the bits as macros (no enumerator is added); the mirror's constants equal them."""
    src = open(_lib.HEADER).read()
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define RG_BK_VERIFY_(\w+) (\d+)", src)}
    assert got == {"ARITH": buckler.VERIFY_ARITH, "LIN_REM": buckler.VERIFY_LIN_REM, "LIN": buckler.VERIFY_LIN,
                   "SUM_REM": buckler.VERIFY_SUM_REM, "SUM": buckler.VERIFY_SUM}
    assert got == {"ARITH": 1, "LIN_REM": 2, "LIN": 4, "SUM_REM": 8, "SUM": 16}
    assert "typedef struct rg_bverifier rg_bverifier;" in src
    assert callable(buckler.VerifyChecks) and hasattr(buckler.VerifyPlan, "checks_dev")
    assert hasattr(buckler.VerifyPlan, "scratch_bytes")
