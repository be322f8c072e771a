"""CPU: the refusals of the prover's batch entry (include/ringo.h: rg_buckler_prover_create,
rg_buckler_prove_checks*) that can be reached without a device, and the mirror's surface.  Each
returns its status with a reason in rg_last_error before the device is touched.  The device
addresses below are made-up numbers: a call that read them would crash, not fail.

An rg_bprover needs two NTT plans, and a plan uploads its tables when it is created, so the refusals
past the NULL plans and the NULL handle (the checks' own rules, aliased buffers, n_proofs over the
limit, the scratch size of a refused n_proofs on a live handle) run with live plans in
test_gpu_buckler_prove_multi.py::test_create_refusals_with_live_plans and
::test_argument_errors_with_live_plans."""
import ctypes
import re

from ringo import _lib, buckler

INVALID = -1
A = [0x10000 * (i + 1) for i in range(16)]  # distinct fake device addresses


def _why():
    return _lib.lib().rg_last_error().decode()


def test_create_refuses_null_plans_and_null_out_no_gpu():
    L = _lib.lib()
    circ = A[0]  # a circuit uploads its program when it is created; the plans are looked at first, so this is never read
    h = ctypes.c_void_p(1)
    assert L.rg_buckler_prover_create(None, None, 512, 2, 0, None, circ, 256, None, 0, ctypes.byref(h)) == INVALID
    assert h.value is None and "NULL encoder or embedding plan" in _why()
    h = ctypes.c_void_p(1)
    assert L.rg_buckler_prover_create(None, None, 512, 2, 0, None, None, 0, None, 0, ctypes.byref(h)) == INVALID
    assert h.value is None and _why().startswith("buckler prover:")
    assert L.rg_buckler_prover_create(None, None, 512, 2, 0, None, circ, 256, None, 0, None) == INVALID
    assert "NULL out" in _why()
    L.rg_buckler_prover_destroy(None)  # as free(NULL)


def test_null_handle_rejected_no_gpu():
    L = _lib.lib()
    for n in (0, 1, 4, 65535, 65536, 1 << 40):
        assert L.rg_buckler_prove_checks_scratch_bytes(None, n) == 0
    assert L.rg_buckler_prove_checks_dev(None, 4, *A[:15], None) == INVALID
    assert "NULL handle" in _why()
    assert L.rg_buckler_prove_checks_dev(None, 0, *A[:15], None) == INVALID  # refused even where nothing would run
    assert L.rg_buckler_prove_checks(None, 4, *([None] * 14)) == INVALID
    assert "NULL handle" in _why()


def test_the_header_states_the_call_and_the_mirror_has_the_entries():
    src = open(_lib.HEADER).read()
    assert re.search(r"#define RG_BK_MULTI_MAX_PROOFS 65535", src)
    for name in ("rg_buckler_prover_create", "rg_buckler_prover_destroy", "rg_buckler_prove_checks_scratch_bytes",
                 "rg_buckler_prove_checks_dev", "rg_buckler_prove_checks"):
        assert name in _lib._SIGS and re.search(r"\b%s\(" % name, src), name
    # 2 + 15 buffers + the stream; the host form has neither scratch nor stream
    assert len(_lib._SIGS["rg_buckler_prove_checks_dev"][1]) == 18
    assert len(_lib._SIGS["rg_buckler_prove_checks"][1]) == 16
    for name in ("scratch_bytes", "checks_dev", "checks", "out_elems"):
        assert hasattr(buckler.ProvePlan, name), name
    assert callable(buckler.ProveChecks)
