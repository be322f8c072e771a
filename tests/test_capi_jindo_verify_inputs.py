"""CPU: what the batch verifier's front end (include/ringo.h rg_jindo_eval_point_multi_dev,
rg_jindo_verify_inputs_multi_dev) decides without a handle: the NULL handle's refusal and its reason,
the scratch sizes of a NULL handle, the header constant against the mirror, the mirror's methods.
The refusals past the NULL handle need an rg_jindo, whose creation uploads the commit key: they run
in test_gpu_jindo_eval_point_multi.py and test_gpu_jindo_verify_inputs_multi.py.  The device addresses
below are made-up numbers: a call that read them would crash, not fail."""
import re

from ringo import _lib, jindo

INVALID = _lib.STATUS["RG_ERR_INVALID"]
A = [0x100000 * (i + 1) for i in range(9)]  # distinct fake device addresses


def _why():
    return _lib.lib().rg_last_error().decode()


def test_null_handle_refused():
    L = _lib.lib()
    for n in (4, 0):  # the handle is looked at first: n_points == 0 does not excuse it
        assert L.rg_jindo_eval_point_multi_dev(None, n, A[0], 1, A[1], A[2], A[3], None) == INVALID
        assert "jindo eval point multi" in _why() and "NULL handle" in _why()
        assert L.rg_jindo_verify_inputs_multi_dev(None, n, 2, A[0], 5, *A[1:9], None) == INVALID
        assert "jindo verify inputs multi" in _why() and "NULL handle" in _why()


def test_scratch_bytes_of_a_null_handle():
    L = _lib.lib()
    for n in (0, 1, 64, 65535, 65536):
        assert L.rg_jindo_eval_point_multi_scratch_bytes(None, n) == 0
        assert L.rg_jindo_verify_inputs_multi_scratch_bytes(None, n) == 0


def test_constant_is_in_the_header_and_the_mirror():
    m = re.search(r"#define RG_JINDO_POINT_MAX_POINTS (\d+)", open(_lib.HEADER).read())
    assert m and int(m.group(1)) == jindo.POINT_MAX_POINTS == 65535


def test_the_mirror_has_the_methods():
    names = ("eval_point_multi_scratch_bytes", "eval_point_multi_dev")
    for name in names + ("verify_inputs_multi_scratch_bytes", "verify_inputs_multi_dev"):
        assert callable(getattr(jindo.Verifier, name)), name
    for name in names:
        assert callable(getattr(jindo.Prover, name)), name
