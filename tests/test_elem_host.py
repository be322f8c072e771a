"""CPU: the element helpers every device unit shares (el_copy, el_zero, el_neq of
ringo-snark_amd/csrc/field.hpp) compiled for the host with g++ from the same source, at every limb
count the library supports: 1, 2, 4, 7, 14.  Each helper works in the middle of a longer array, so a
word written or read outside its L words shows; el_neq sees equal inputs, a difference in the lowest
word only and a difference in the highest word only.  The GPU parity tests pin the device build."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "ringo-snark_amd", "csrc")

HARNESS = r"""
#include "field.hpp"
template <int L>
static int run(int op, uint64_t* d, const uint64_t* s) {
  switch (op) {
    case 0: rg::el_copy<L>(d, s); return 0;
    case 1: rg::el_zero<L>(d); return 0;
    default: return rg::el_neq<L>(d, s) ? 1 : 0;
  }
}
extern "C" int elem_run(int L, int op, uint64_t* d, const uint64_t* s) {
  switch (L) {
    case 1: return run<1>(op, d, s);
    case 2: return run<2>(op, d, s);
    case 4: return run<4>(op, d, s);
    case 7: return run<7>(op, d, s);
    case 14: return run<14>(op, d, s);
  }
  return -1;
}
"""

LIMBS = [1, 2, 4, 7, 14]
COPY, ZERO, NEQ = 0, 1, 2
GUARD = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("elem")
    src, so = d / "elem.cpp", d / "libelem.so"
    src.write_text(HARNESS)
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, str(src), "-o", str(so)], check=True)
    L = ctypes.CDLL(str(so))
    L.elem_run.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return L


def _words(L, seed):
    """L + 2 nonzero words: the element with one guard word on each side."""
    return np.random.default_rng(seed).integers(1, 2 ** 63, size=L + 2, dtype=np.int64).astype(np.uint64)


def _at(a, i=1):
    return a.ctypes.data + 8 * i


@pytest.mark.parametrize("L", LIMBS)
def test_el_copy_moves_exactly_the_element(lib, L):
    src = _words(L, L)
    dst = np.full(L + 2, GUARD, np.uint64)
    keep = src.copy()
    assert lib.elem_run(L, COPY, _at(dst), _at(src)) == 0
    assert dst[1:L + 1].tolist() == keep[1:L + 1].tolist()
    assert int(dst[0]) == GUARD and int(dst[L + 1]) == GUARD
    assert src.tolist() == keep.tolist()


@pytest.mark.parametrize("L", LIMBS)
def test_el_zero_clears_exactly_the_element(lib, L):
    dst = _words(L, 100 + L)
    keep = dst.copy()
    assert lib.elem_run(L, ZERO, _at(dst), None) == 0
    assert dst[1:L + 1].tolist() == [0] * L
    assert int(dst[0]) == int(keep[0]) and int(dst[L + 1]) == int(keep[L + 1])


@pytest.mark.parametrize("L", LIMBS)
def test_el_neq_sees_every_word_and_no_other(lib, L):
    a = _words(L, 200 + L)
    b = a.copy()
    assert lib.elem_run(L, NEQ, _at(a), _at(b)) == 0  # equal
    b[0] ^= np.uint64(1)  # the guards differ, the element does not
    b[L + 1] ^= np.uint64(1)
    assert lib.elem_run(L, NEQ, _at(a), _at(b)) == 0
    lo = a.copy()
    lo[1] ^= np.uint64(1)  # the lowest word only, in its lowest bit
    assert lib.elem_run(L, NEQ, _at(a), _at(lo)) == 1
    assert lib.elem_run(L, NEQ, _at(lo), _at(a)) == 1
    hi = a.copy()
    hi[L] ^= np.uint64(1 << 63)  # the highest word only, in its highest bit
    assert lib.elem_run(L, NEQ, _at(a), _at(hi)) == 1
    assert lib.elem_run(L, NEQ, _at(hi), _at(a)) == 1
