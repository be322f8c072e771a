"""CPU: the arithmetic core of the norm decomposition (ringo-snark_amd/csrc/dcmp.hpp, used by the
kernels of buckler_dcmp.hip on the device) compiled for the host with g++ from the same source and
compared with the loop-by-loop restatement of decomposeBig (tests/buckler_dcmp_ref.py) at every
limb count the library supports: 1, 2, 4, 7, 14.  The moduli include the synthetic ones that fill
their top limb, where q - x and the compare with q >> 1 have no spare bit; the bases include
elements that cross a limb and one close to q / 2.  The GPU parity tests pin the device build."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import buckler_dcmp_ref as D
from tests import synth_util as su

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "ringo-snark_amd", "csrc")

HARNESS = r"""
#include "dcmp.hpp"
template <int L>
static void run(const uint64_t* q, uint64_t qinv, const uint64_t* base, long nb, const uint64_t* w, long n,
                int8_t* digits, uint64_t* resid) {
  rg::FieldParams<L> F;
  for (int l = 0; l < L; ++l) F.q[l] = q[l];
  F.qinv = qinv;
  for (long i = 0; i < n; ++i) {
    rg::Dcmp<L> d;
    rg::dcmp_init<L>(d, w + i * L, F);
    for (long j = 0; j < nb; ++j) digits[i * nb + j] = rg::dcmp_step<L>(d, base + j * L) ? (d.s ? -1 : 1) : 0;
    for (int l = 0; l < L; ++l) resid[i * (L + 1) + l] = d.m[l];
    resid[i * (L + 1) + L] = d.s;
  }
}
extern "C" int dcmp_run(int L, const uint64_t* q, uint64_t qinv, const uint64_t* base, long nb, const uint64_t* w,
                        long n, int8_t* digits, uint64_t* resid) {
  switch (L) {
    case 1: run<1>(q, qinv, base, nb, w, n, digits, resid); return 0;
    case 2: run<2>(q, qinv, base, nb, w, n, digits, resid); return 0;
    case 4: run<4>(q, qinv, base, nb, w, n, digits, resid); return 0;
    case 7: run<7>(q, qinv, base, nb, w, n, digits, resid); return 0;
    case 14: run<14>(q, qinv, base, nb, w, n, digits, resid); return 0;
  }
  return 1;
}
extern "C" void dcmp_unit_run(int s, const uint64_t* one, const uint64_t* neg, uint64_t* out) {
  rg::Dcmp<2> d;
  d.m[0] = d.m[1] = 0;
  d.s = s != 0;
  rg::dcmp_unit<2>(out, d, one, neg);
}
"""

# every supported limb count, with and without a spare top bit
FIELDS = ["p63", "s64_lo", "s64_gold", "mult_zp", "zp110", "jindo_zp", "s256_top", "s256_lo", "zp440", "s448_top",
          "zp880", "s896_top"]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("dcmp")
    src, so = d / "dcmp.cpp", d / "libdcmp.so"
    src.write_text(HARNESS)
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, str(src), "-o", str(so)], check=True)
    L = ctypes.CDLL(str(so))
    L.dcmp_run.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_long,
                           ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p]
    L.dcmp_unit_run.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return L


def _limbs(vals, L):
    return np.array([[(v >> (64 * i)) & su.M64 for i in range(L)] for v in vals], dtype=np.uint64).reshape(-1, L)


def plain_values(q, base, rng, n_rand=64):
    """Plain coefficient values on every edge: 0, 1, q - 1, q >> 1 and its successor, +-b_j and
    +-(b_j - 1) for every j, +-sum(base) and one beyond, random values within the bound and over
    the whole field."""
    S = sum(base)
    vals = [0, 1, q - 1, q >> 1, (q >> 1) + 1, S, -S, S + 1, -S - 1]
    for b in base:
        vals += [b, -b, b - 1, 1 - b]
    nbytes = (q.bit_length() + 7) // 8 + 8
    for _ in range(n_rand):
        vals.append(int.from_bytes(rng.bytes(nbytes), "little") % q)
        vals.append(int.from_bytes(rng.bytes(nbytes), "little") % (2 * S + 1) - S)
    return [v % q for v in vals]


def bases_for(q, L):
    bounds = [2, 3, 8, 1000, (1 << 20) - 1]
    if L >= 2:
        bounds += [1 << 64, (1 << 64) + 1, (1 << 65) - 1]
    bases = [[1]] + [D.decomposeBase(b) for b in bounds]
    if q.bit_length() <= 256:
        bases.append(D.decomposeBase(q - 1))  # nb = the bit length of q, b_0 = q / 2
    bases.append([(1 << (64 * L)) - 1, (q >> 1) + 1, q >> 1, 5, 1])  # a saturated element, then the edge of reach
    return bases


@pytest.mark.parametrize("name", FIELDS)
def test_dcmp_core_matches_restatement(lib, name):
    q = su.modulus(name)
    L = (q.bit_length() + 63) // 64
    R = 1 << (64 * L)
    qinv = (-pow(q, -1, 1 << 64)) % (1 << 64)
    rng = np.random.default_rng(L)
    ql = _limbs([q], L)
    for base in bases_for(q, L):
        vals = plain_values(q, base, rng)
        w = _limbs([v * R % q for v in vals], L)
        bl = _limbs(base, L)
        digits = np.full((len(vals), len(base)), 9, np.int8)
        resid = np.zeros((len(vals), L + 1), np.uint64)
        assert lib.dcmp_run(L, ql.ctypes.data, qinv, bl.ctypes.data, len(base), w.ctypes.data, len(vals),
                            digits.ctypes.data, resid.ctypes.data) == 0
        for i, v in enumerate(vals):
            assert digits[i].tolist() == D.decomposeBig(v, base, q), (name, base[:3], v)
            r = D.residual(v, base, q)
            m = sum(int(resid[i, l]) << (64 * l) for l in range(L))
            assert m == abs(r), (name, v)
            if r:
                assert int(resid[i, L]) == (r < 0)


def test_dcmp_unit_selects_by_sign(lib):
    one = np.array([3, 4], np.uint64)
    neg = np.array([5, 6], np.uint64)
    out = np.zeros(2, np.uint64)
    lib.dcmp_unit_run(0, one.ctypes.data, neg.ctypes.data, out.ctypes.data)
    assert out.tolist() == [3, 4]
    lib.dcmp_unit_run(1, one.ctypes.data, neg.ctypes.data, out.ctypes.data)
    assert out.tolist() == [5, 6]
