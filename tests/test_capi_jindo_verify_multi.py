"""CPU: what the Jindo verifier's batch entry (include/ringo.h rg_jindo_verify_multi_dev) decides on
the host: the refusals that need no handle, the two constants against the mirror, and
rg_jindo_verify_unpack, which is host code alone: hand-built records go into rg_jindo_verify_result
field by field.  The refusals past the NULL handle need an rg_jindo, whose creation uploads the
commit key: they run in test_gpu_jindo_verify_multi.py.  The device addresses below are made-up
numbers: a call that read them would crash, not fail."""
import ctypes
import re

import numpy as np
import pytest

from ringo import _lib, jindo

INVALID = _lib.STATUS["RG_ERR_INVALID"]
A = [0x100000 * (i + 1) for i in range(13)]  # distinct fake device addresses
W = jindo.VERIFY_WORDS
ALL = (1 << 64) - 1


def _why():
    return _lib.lib().rg_last_error().decode()


def test_null_handle_refused():
    L = _lib.lib()
    assert L.rg_jindo_verify_multi_scratch_bytes(None, 4, 1) == 0
    assert L.rg_jindo_verify_multi_dev(None, 4, 2, *A[:11], 1.0, 1.0, A[11], A[12], None) == INVALID
    assert "NULL handle" in _why()
    assert L.rg_jindo_verify_multi_dev(None, 0, 1, *A[:11], 1.0, 1.0, A[11], A[12], None) == INVALID


def test_constants_are_in_the_header_and_the_mirror():
    src = open(_lib.HEADER).read()
    m = re.search(r"#define RG_JINDO_VERIFY_MAX_PROOFS (\d+)", src)
    assert m and int(m.group(1)) == jindo.VERIFY_MAX_PROOFS == 65535
    m = re.search(r"#define RG_JINDO_VERIFY_WORDS (\d+)", src)
    assert m and int(m.group(1)) == jindo.VERIFY_WORDS == 54
    # ok, flags, two sums of the result's 10 words, two sides of its 16 limbs
    r = jindo.VerifyResultC()
    assert jindo.VERIFY_WORDS == 2 + len(r.outer_norm_sq) + len(r.inner_norm_sq) + len(r.eval_lhs) + len(r.eval_rhs)


def test_the_mirror_has_the_methods():
    for name in ("verify_multi_dev", "verify_multi_scratch_bytes", "unpack_verify_words", "VerifyMulti"):
        assert callable(getattr(jindo.Verifier, name)), name


def _record(L, mask, ok, seed):
    """(record words, the fields it states): norms with every word set, sides of L words."""
    rng = np.random.default_rng(seed)
    rec = np.zeros(W, np.uint64)
    rec[0], rec[1] = ok, mask
    rec[2:12] = rng.integers(1, ALL, 10, dtype=np.uint64, endpoint=True)
    rec[12:22] = rng.integers(1, ALL, 10, dtype=np.uint64, endpoint=True)
    rec[11], rec[12] = ALL, ALL  # the outer sum's top word and the inner sum's low word
    rec[22:22 + L] = rng.integers(1, ALL, L, dtype=np.uint64, endpoint=True)
    rec[38:38 + L] = rng.integers(1, ALL, L, dtype=np.uint64, endpoint=True)
    return rec


@pytest.mark.parametrize("L", [1, 4, 14])
def test_unpack_round_trips_every_field(L):
    lib = _lib.lib()
    for mask in range(16):
        for ok in (0, 1):  # word 0 is reported as it stands: the device wrote it
            rec = _record(L, mask, ok, seed=100 * L + mask)
            assert (rec[2:22] != 0).all()
            r = jindo.VerifyResultC()
            assert lib.rg_jindo_verify_unpack(rec.ctypes.data, L, ctypes.byref(r)) == 0
            assert r.ok == ok
            assert [r.outer_ok, r.inner_ok, r.consistency_ok, r.eval_ok] == [(mask >> b) & 1 for b in range(4)]
            assert list(r.outer_norm_sq) == [int(x) for x in rec[2:12]]
            assert list(r.inner_norm_sq) == [int(x) for x in rec[12:22]]
            assert list(r.eval_lhs) == [int(x) for x in rec[22:38]] and list(r.eval_lhs)[L:] == [0] * (16 - L)
            assert list(r.eval_rhs) == [int(x) for x in rec[38:54]] and list(r.eval_rhs)[L:] == [0] * (16 - L)


def test_unpack_refusals():
    lib = _lib.lib()
    rec = _record(4, 15, 1, seed=1)
    r = jindo.VerifyResultC()
    assert lib.rg_jindo_verify_unpack(None, 4, ctypes.byref(r)) == INVALID and "NULL" in _why()
    assert lib.rg_jindo_verify_unpack(rec.ctypes.data, 4, None) == INVALID and "NULL" in _why()
    for L in (0, 3, 15, 16, -1):  # common.hpp dispatch_limbs: 1, 2, 4, 7, 14
        assert lib.rg_jindo_verify_unpack(rec.ctypes.data, L, ctypes.byref(r)) == INVALID, L
        assert "limbs" in _why()


def test_unpack_through_the_mirror():
    """Verifier.unpack_verify_words needs no device: the records of two proofs -> two results."""
    class P:  # the one attribute unpack_verify_words reads
        L = 4
    v = jindo.Verifier.__new__(jindo.Verifier)
    v.params = P
    recs = np.stack([_record(4, 0b1011, 0, seed=5), _record(4, 0b1111, 1, seed=6)])
    a, b = v.unpack_verify_words(recs)
    assert (a.ok, a.outer_ok, a.inner_ok, a.consistency_ok, a.eval_ok) == (False, True, True, False, True)
    assert (b.ok, b.outer_ok, b.inner_ok, b.consistency_ok, b.eval_ok) == (True,) * 5
    assert a.outer_norm_sq == sum(int(x) << (64 * i) for i, x in enumerate(recs[0, 2:12]))
    assert b.inner_norm_sq == sum(int(x) << (64 * i) for i, x in enumerate(recs[1, 12:22]))
    assert (a.eval_lhs == recs[0, 22:26]).all() and (b.eval_rhs == recs[1, 38:42]).all()
