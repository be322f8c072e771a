"""CPU: argument checks of the batched Poly.Evaluate and of the Jindo evaluation-point and
challenge entry points (include/ringo.h rg_poly_evaluate_batch*, rg_jindo_eval_point_dev,
rg_jindo_encode_challenges_dev, rg_jindo_challenge_bound).  Each check runs before any device call,
so none of this needs a GPU.  The device addresses below are made-up numbers: a call that read them
would crash, not fail."""
import ctypes
import json
import os

import numpy as np
import pytest

import ringo
from ringo import _lib, bigpoly, jindo
from ringo.bigpoly import RingoPanic

INVALID, UNSUPPORTED = -1, -3
A, B, C, D = 0x10000, 0x20000, 0x30000, 0x40000  # distinct fake device addresses
HERE = os.path.dirname(os.path.abspath(__file__))
PARAMS = json.load(open(os.path.join(HERE, "golden", "jindo_params.json")))


@pytest.fixture(scope="module")
def F(fields):
    return ringo.Field(fields["p63"])


def _err():
    return _lib.lib().rg_last_error().decode()


def test_evaluate_batch_argument_errors_no_gpu(F):
    L = _lib.lib()
    dev, host = L.rg_poly_evaluate_batch_dev, L.rg_poly_evaluate_batch
    one = np.ones(8, np.uint64)
    assert dev(None, A, 4, 4, 1, B, C, D, None) == INVALID
    assert "NULL field" in _err()
    assert host(None, _lib.ptr(one), 4, 4, 1, _lib.ptr(one), _lib.ptr(one)) == INVALID
    assert "NULL field" in _err()
    assert L.rg_poly_evaluate_batch_scratch_bytes(None, 4, 1) == 0
    assert dev(F.h, A, 5, 4, 1, B, C, D, None) == INVALID  # stride < n
    assert "stride 4 < n 5" in _err()
    assert host(F.h, _lib.ptr(one), 5, 4, 1, _lib.ptr(one), _lib.ptr(one)) == INVALID
    assert "stride 4 < n 5" in _err()
    assert dev(F.h, None, 4, 4, 1, B, C, D, None) == INVALID
    assert "NULL buffer" in _err()
    assert dev(F.h, A, 4, 4, 1, None, C, D, None) == INVALID
    assert dev(F.h, A, 4, 4, 1, B, None, D, None) == INVALID
    assert dev(F.h, A, 4, 4, 1, B, C, None, None) == INVALID
    assert "scratch" in _err()
    assert host(F.h, None, 4, 4, 1, _lib.ptr(one), _lib.ptr(one)) == INVALID
    assert dev(F.h, A, 1 << 20, 1 << 41, 1, B, C, D, None) == INVALID
    assert "out of range" in _err()
    assert dev(F.h, A, 4, 4, 0, B, C, D, None) == 0  # batch = 0: nothing to do, as the neighbouring entries
    assert host(F.h, None, 4, 4, 0, None, None) == 0
    G = ringo.Field((1 << 130) + 5 | 1, limbs=3)  # a limb count with no kernel
    assert dev(G.h, A, 4, 4, 1, B, C, D, None) == UNSUPPORTED
    assert "3 limbs" in _err()
    assert host(G.h, _lib.ptr(one), 1, 1, 1, _lib.ptr(one), _lib.ptr(one)) == UNSUPPORTED
    with pytest.raises(RingoPanic):
        bigpoly.evaluate_batch_dev(F, A, 5, 4, 1, B, C, D)


def test_evaluate_batch_scratch_bytes_monotone_no_gpu(F, fields):
    sb = _lib.lib().rg_poly_evaluate_batch_scratch_bytes
    ns = [0, 1, 255, 256, 4095, 4096, 4097, 8195, 1 << 16, (1 << 16) + 1]
    for f in (F, ringo.Field(fields["zp880"])):
        for batch in (1, 3, 512):
            got = [sb(f.h, n, batch) for n in ns]
            assert got == sorted(got) and all(g > 0 for g in got[1:]), (batch, got)
        for n in ns:
            got = [sb(f.h, n, b) for b in (0, 1, 2, 5, 512)]
            assert got == sorted(got), (n, got)
        # one tile sum per 4096 coefficients (kEvalTile) and polynomial
        assert sb(f.h, 4097, 5) - sb(f.h, 4096, 5) == 5 * f.L * 8
        assert bigpoly.evaluate_batch_scratch_bytes(f, 4097, 5) == sb(f.h, 4097, 5)


def test_jindo_point_and_challenge_argument_errors_no_gpu():
    L = _lib.lib()
    assert L.rg_jindo_eval_point_dev(None, A, B, C, None) == INVALID
    assert "NULL handle" in _err()
    assert L.rg_jindo_encode_challenges_dev(None, 0, A, 1, B, None) == INVALID
    assert "NULL handle" in _err()
    for ring in (2, -1):
        assert L.rg_jindo_encode_challenges_dev(None, ring, A, 1, B, None) == INVALID
        assert f"ring {ring}" in _err()


def test_challenge_bound_no_gpu():
    """Parameters.ChallengeBound() (params.go:357-360) of the fixture sets, and the refusal where the
    reference divides by zero: exp > 120."""
    L = _lib.lib()
    b = ctypes.c_uint64()
    for name, P in PARAMS.items():
        ps = jindo.Parameters.from_dict(P, int(P["field_q_hex"], 16)).c_struct()
        assert L.rg_jindo_challenge_bound(ctypes.byref(ps), ctypes.byref(b)) == 0
        assert b.value == min(P["base"], 1 << (120 // P["exp"])) // 2, name
    ps = jindo.Parameters.from_dict(PARAMS["t10_b1"], int(PARAMS["t10_b1"]["field_q_hex"], 16)).c_struct()
    for exp, want in ((120, 1), (61, 1), (60, 2), (64, 1)):
        ps.exp = exp
        assert L.rg_jindo_challenge_bound(ctypes.byref(ps), ctypes.byref(b)) == 0
        assert b.value == want
    for exp in (121, 500):
        ps.exp = exp
        assert L.rg_jindo_challenge_bound(ctypes.byref(ps), ctypes.byref(b)) == INVALID
        assert f"exp = {exp}" in _err()
    ps.exp = 1  # 1 << 120 is 0 in Go's uint64
    assert L.rg_jindo_challenge_bound(ctypes.byref(ps), ctypes.byref(b)) == INVALID
    ps.exp = 0
    assert L.rg_jindo_challenge_bound(ctypes.byref(ps), ctypes.byref(b)) == INVALID
    assert L.rg_jindo_challenge_bound(None, ctypes.byref(b)) == INVALID
    assert L.rg_jindo_challenge_bound(ctypes.byref(ps), None) == INVALID
