"""CPU: the Montgomery twiddle product of the lazy 2^16 NTT passes (ringo-snark_amd/csrc/ntt64.hpp:
mont64, the portable form of the kernels' mont_x, and the gate ntt64_mont_ok) compiled for the
host with g++ from the same header and compared with Python integers.

Product: for q = q1 2^32 + 1, y in [0, 2q) and w in [0, q), t = mont64(y, w, q1) must satisfy
t 2^64 == y w (mod q), t < q + ceil(2 q^2 / 2^64) and 2q - 1 + t < 2^64 (the forward butterfly
adds t to a lazy value without a 65th bit).  Moduli: p63 = 47104^4 + 1 (the headline prime) and
0x47e0f66500000001, the largest prime == 1 (mod 2^32) under the gate, where the headroom is
tightest.  Inputs: an edge set (y in {0, 1, q - 1, q, q + 1, 2q - 2, 2q - 1, low / high word all
ones or zero}, w in {0, 1, 2, q - 2, q - 1, word patterns}) and seeded random pairs.

Gate: true for those two moduli; false for 0x47e0f67200000001 (the first such prime above the
gate), for s63_top, and for a modulus that is not 1 mod 2^32.  The gate's constant is checked
against the inequality it stands for, 3q + ceil(2 q^2 / 2^64) + 2^33 < 2^64."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from tests import synth_util as su

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "ringo-snark_amd", "csrc")

P63 = 47104 ** 4 + 1
Q_TIGHT = 0x47E0F66500000001  # largest prime == 1 (mod 2^32) that passes the gate
Q_ABOVE = 0x47E0F67200000001  # first such prime above it
M64 = (1 << 64) - 1

HARNESS = r"""
#include "ntt64.hpp"
extern "C" void mont_run(uint64_t q, const uint64_t* y, const uint64_t* w, long n, uint64_t* out) {
  const uint32_t q1 = (uint32_t)(q >> 32);
  for (long i = 0; i < n; ++i) out[i] = rg::mont64(y[i], w[i], q1);
}
extern "C" int mont_ok(uint64_t q) { return rg::ntt64_mont_ok(q) ? 1 : 0; }
extern "C" uint32_t mont_max_q1() { return rg::kMontMaxQ1; }
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("mont64")
    src, so = d / "mont64.cpp", d / "libmont64.so"
    src.write_text(HARNESS)
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, str(src), "-o", str(so)], check=True)
    L = ctypes.CDLL(str(so))
    L.mont_run.argtypes = [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
    L.mont_run.restype = None
    L.mont_ok.argtypes = [ctypes.c_uint64]
    L.mont_max_q1.restype = ctypes.c_uint32
    return L


def _ceil_2q2(q):
    return -((-2 * q * q) >> 64)


def _headroom_ok(q):
    return 3 * q + _ceil_2q2(q) + (1 << 33) < (1 << 64)


def _edges(q):
    q1 = q >> 32
    top = (2 * q - 1) >> 32
    ys = {0, 1, 2, q - 1, q, q + 1, 2 * q - 2, 2 * q - 1,
          0xFFFFFFFF, 1 << 32, (1 << 32) - 2, top << 32, (top << 32) | 1, ((top - 1) << 32) | 0xFFFFFFFF,
          (q1 << 32) | 0xFFFFFFFF, (1 << 63) - 1 if (1 << 63) - 1 < 2 * q else q - 2, 1 << 62, q // 2, q // 2 + 1}
    ws = {0, 1, 2, q - 2, q - 1, 0xFFFFFFFF, 1 << 32, (1 << 32) + 1, q1 << 32, ((q1 - 1) << 32) | 0xFFFFFFFF,
          (1 << 64) % q, (1 << 128) % q, q // 2, q // 2 + 1}
    ys = sorted(v for v in ys if 0 <= v < 2 * q)
    ws = sorted(v for v in ws if 0 <= v < q)
    return [(y, w) for y in ys for w in ws]


@pytest.mark.parametrize("q", [P63, Q_TIGHT], ids=["p63", "tight"])
def test_mont64_matches_integers(lib, q):
    assert lib.mont_ok(q) == 1
    rng = random.Random(64)
    pairs = _edges(q)
    pairs += [(rng.randrange(2 * q), rng.randrange(q)) for _ in range(200000)]
    # the top sliver of both ranges, where the bound on t is approached
    pairs += [(2 * q - 1 - rng.randrange(1 << 20), q - 1 - rng.randrange(1 << 20)) for _ in range(20000)]
    y = np.array([p[0] for p in pairs], dtype=np.uint64)
    w = np.array([p[1] for p in pairs], dtype=np.uint64)
    out = np.zeros(len(pairs), dtype=np.uint64)
    lib.mont_run(q, y.ctypes.data, w.ctypes.data, len(pairs), out.ctypes.data)
    bound = q + _ceil_2q2(q)
    rinv = pow(1 << 64, -1, q)
    tmax = 0
    for (yv, wv), t in zip(pairs, out.tolist()):
        assert t % q == yv * wv * rinv % q, (hex(yv), hex(wv), hex(t))
        assert t < bound, (hex(yv), hex(wv), hex(t))
        assert 2 * q - 1 + t < (1 << 64), (hex(yv), hex(wv), hex(t))
        tmax = max(tmax, t)
    print(f"q = {q:#x}: max t / q = {tmax / q:.5f} (bound {bound / q:.5f})")


def test_mont64_gate(lib):
    assert lib.mont_ok(P63) == 1
    assert lib.mont_ok(Q_TIGHT) == 1
    assert lib.mont_ok(Q_ABOVE) == 0
    s63 = su.modulus("s63_top")
    assert s63 & 0xFFFFFFFF == 1 and lib.mont_ok(s63) == 0
    s62 = su.modulus("s62_lo")
    assert s62 & 0xFFFFFFFF != 1 and s62 >> 32 <= lib.mont_max_q1() and lib.mont_ok(s62) == 0
    # the constant is the inequality's threshold: the headroom bound is monotone in q1
    m = lib.mont_max_q1()
    assert _headroom_ok((m << 32) + 1) and not _headroom_ok(((m + 1) << 32) + 1)
    assert _headroom_ok(Q_TIGHT) and not _headroom_ok(Q_ABOVE)
