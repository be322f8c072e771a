"""CPU: the NTT plan's route decision (ringo-snark_amd/csrc/ntt_route.hpp: ntt_route, the pass
limits and ntt64_mont_ok) compiled for the host with g++ from the same header, against a Python
restatement of the rules.

Grid: every field of tests/golden/fields.json and tests/golden/synthetic_fields.json, every logN
from 0 to 26, both directions, rank_inv == N^-1 or not (`halving`), and the NttKernel switch unset,
"r", "r8" and "stage".  Compared: the route, the Shoup and Montgomery flags and the pass list.

The rules (the header restates them in C++; this file was written from the rules, not from it):
  radix 4, 4, 3, 2, 2 for L = 1, 2, 4, 7, 14; pmax = radix + 8; smallest tiled pass 6.
  L = 1:  shoup = q < 2^63.  lazy64 iff shoup, logN = 16, q mod 2^32 == 1 and the switch does not
          start with r; its Montgomery variant iff q mod 2^32 == 1 and 0 < q >> 32 <= 0x47e0f66a.
          Else tiled iff 6 <= logN <= 2 pmax, else stages.
  L = 2:  tiled iff 6 <= logN <= 2 pmax, else stages.
  L = 4:  fast256 iff logN in {15, 16}, q[0] == 1, q[3] < 2^63 and the switch does not start with
          r; else tiled iff 6 <= logN <= 2 pmax, else stages.
  L = 7, 14: wide iff 1 <= logN <= 16, top bit of q clear, not (inverse and not halving) and the
          switch does not start with s; else stages.
  Passes (G0, P), forward order: tiled / lazy64 / fast256: one pass of logN when logN <= pmax,
  else pa = max(logN // 2, 6) then logN - pa; wide: one pass when logN <= 8, else logN // 2 then
  the rest; stages: none."""
import ctypes
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "ringo-snark_amd", "csrc")

HARNESS = r"""
#include "ntt_route.hpp"
// out: route, shoup, mont, npasses, G0_0, P_0, G0_1, P_1
extern "C" void route_run(int L, const uint64_t* q, int logN, int inv, int halving, const char* sw, int* out) {
  const rg::NttRouting r = rg::ntt_route(L, q, logN, inv != 0, halving != 0, sw);
  out[0] = (int)r.route;
  out[1] = r.shoup;
  out[2] = r.mont;
  out[3] = r.npasses;
  for (int i = 0; i < 2; ++i) {
    out[4 + 2 * i] = r.passes[i].G0;
    out[5 + 2 * i] = r.passes[i].P;
  }
}
extern "C" int route_id(int i) {
  const rg::NttRoute ids[5] = {rg::NttRoute::Stages, rg::NttRoute::Tiled, rg::NttRoute::Lazy64,
                               rg::NttRoute::Fast256, rg::NttRoute::Wide};
  return (int)ids[i];
}
extern "C" int radix(int L) { return rg::ntt_radix(L); }
extern "C" int pmax(int L) { return rg::ntt_pmax(L); }
extern "C" int pmax_template(int L) {
  return L == 1 ? rg::pmax_of<1>() : L == 2 ? rg::pmax_of<2>() : L == 4 ? rg::pmax_of<4>()
       : L == 7 ? rg::pmax_of<7>() : rg::pmax_of<14>();
}
extern "C" int min_tiled() { return rg::kMinTiledP; }
"""

NAMES = ["stages", "tiled", "lazy64", "fast256", "wide"]
RADIX = {1: 4, 2: 4, 4: 3, 7: 2, 14: 2}
MIN_TILED = 6
MONT_MAX_Q1 = 0x47E0F66A
SWITCHES = [None, "r", "r8", "stage"]
LOGNS = range(0, 27)


def _fields():
    out = {}
    for name in ("fields.json", "synthetic_fields.json"):
        for k, v in json.load(open(os.path.join(HERE, "golden", name))).items():
            out[k] = (int(v["limbs"]), int(v["q_hex"], 16))
    return out


FIELDS = _fields()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("ntt_route")
    src, so = d / "route.cpp", d / "libroute.so"
    src.write_text(HARNESS)
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, str(src), "-o", str(so)], check=True)
    L = ctypes.CDLL(str(so))
    L.route_run.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p,
                            ctypes.c_void_p]
    L.route_run.restype = None
    return L


def got(lib, L, q, logN, inv=False, halving=True, sw=None):
    """(route name, shoup, mont, [(G0, P), ...]) from the header."""
    words = (ctypes.c_uint64 * L)(*[(q >> (64 * i)) & ((1 << 64) - 1) for i in range(L)])
    out = (ctypes.c_int * 8)()
    lib.route_run(L, words, logN, int(inv), int(halving), sw.encode() if sw is not None else None, out)
    ids = [lib.route_id(i) for i in range(5)]
    return NAMES[ids.index(out[0])], bool(out[1]), bool(out[2]), [(out[4 + 2 * i], out[5 + 2 * i]) for i in range(out[3])]


def mont_ok(q):
    return q & 0xFFFFFFFF == 1 and 0 < (q >> 32) <= MONT_MAX_Q1


def want(L, q, logN, inv, halving, sw):
    """The rules of the module docstring."""
    pmax = RADIX[L] + 8
    starts = (lambda c: sw is not None and sw[:1] == c)
    if L in (7, 14):
        top_clear = (q >> (64 * L - 1)) == 0
        if 1 <= logN <= 16 and top_clear and not (inv and not halving) and not starts("s"):
            passes = [(0, logN)] if logN <= 8 else [(0, logN // 2), (logN // 2, logN - logN // 2)]
            return "wide", False, False, passes
        return "stages", False, False, []
    shoup = L == 1 and q < (1 << 63)
    mont = False
    if L == 1 and shoup and logN == 16 and q % (1 << 32) == 1 and not starts("r"):
        route, mont = "lazy64", mont_ok(q)
    elif (L == 4 and logN in (15, 16) and q % (1 << 64) == 1 and (q >> 192) < (1 << 63) and not starts("r")):
        route = "fast256"
    elif MIN_TILED <= logN <= 2 * pmax:
        route = "tiled"
    else:
        return "stages", shoup, False, []
    if logN <= pmax:
        return route, shoup, mont, [(0, logN)]
    pa = max(logN // 2, MIN_TILED)
    return route, shoup, mont, [(0, pa), (pa, logN - pa)]


def test_constants_are_the_rules(lib):
    for L, r in RADIX.items():
        assert lib.radix(L) == r and lib.pmax(L) == r + 8 and lib.pmax_template(L) == r + 8
    assert lib.min_tiled() == MIN_TILED


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_route_matches_the_rules_on_the_whole_grid(lib, name):
    L, q = FIELDS[name]
    pmax = RADIX[L] + 8
    for logN in LOGNS:
        for inv in (False, True):
            for halving in (True, False):
                for sw in SWITCHES:
                    g = got(lib, L, q, logN, inv, halving, sw)
                    assert g == want(L, q, logN, inv, halving, sw), (name, logN, inv, halving, sw)
                    route, _, _, passes = g
                    if route in ("tiled", "lazy64", "fast256"):
                        assert sum(p for _, p in passes) == logN
                        assert passes[0][0] == 0
                        if len(passes) == 1:
                            assert passes[0][1] == logN
                        else:
                            assert len(passes) == 2 and all(MIN_TILED <= p <= pmax for _, p in passes)
                            assert passes[1][0] == passes[0][1]


def _pick(pred):
    """The fixture fields with a property, by property and not by name."""
    out = [(L, q) for L, q in FIELDS.values() if pred(L, q)]
    assert out, "no fixture field has this property"
    return out


def _single(lo1, below63, mont=None):
    return _pick(lambda L, q: L == 1 and (q % (1 << 32) == 1) == lo1 and (q < (1 << 63)) == below63
                 and (mont is None or mont_ok(q) == mont))


def Q255(L, q):
    return L == 4 and q % (1 << 64) == 1 and q < (1 << 255)


def WIDE_SPARE(L, q):
    return L in (7, 14) and (q >> (64 * L - 1)) == 0


def test_pinned_single_word_routes(lib):
    for L, q in _single(True, True, mont=True):
        assert got(lib, L, q, 16) == ("lazy64", True, True, [(0, 8), (8, 8)])
    for L, q in _single(True, True, mont=False):
        assert got(lib, L, q, 16) == ("lazy64", True, False, [(0, 8), (8, 8)])
    for L, q in _single(False, True):
        assert got(lib, L, q, 16) == ("tiled", True, False, [(0, 8), (8, 8)])
    above = _pick(lambda L, q: L == 1 and q >= (1 << 63))
    for L, q in above:
        route, shoup, mont, _ = got(lib, L, q, 16)
        assert (route, shoup, mont) == ("tiled", False, False)
    every = _single(True, True, mont=True) + _single(True, True, mont=False) + _single(False, True) + above
    for L, q in every:
        for logN in (5, 25):
            assert got(lib, L, q, logN)[0] == "stages"
            assert got(lib, L, q, logN)[3] == []


def test_pinned_four_limb_routes(lib):
    for L, q in _pick(Q255):
        assert got(lib, L, q, 15) == ("fast256", False, False, [(0, 7), (7, 8)])
        assert got(lib, L, q, 16) == ("fast256", False, False, [(0, 8), (8, 8)])
        assert got(lib, L, q, 14)[0] == "tiled"
        assert got(lib, L, q, 16, sw="r")[0] == "tiled"
        assert got(lib, L, q, 16, inv=True, halving=False) == got(lib, L, q, 16)
    for L, q in _pick(lambda L, q: L == 4 and q % (1 << 64) != 1):
        assert got(lib, L, q, 16)[0] == "tiled"


def test_pinned_wide_routes(lib):
    for L, q in _pick(WIDE_SPARE):
        assert got(lib, L, q, 10) == ("wide", False, False, [(0, 5), (5, 5)])
        assert got(lib, L, q, 10, inv=True, halving=True) == ("wide", False, False, [(0, 5), (5, 5)])
        assert got(lib, L, q, 10, inv=True, halving=False) == ("stages", False, False, [])
        assert got(lib, L, q, 10, inv=False, halving=False)[0] == "wide"  # the route is per direction
        assert got(lib, L, q, 17)[0] == "stages"
        assert got(lib, L, q, 10, sw="stage")[0] == "stages"
    for L, q in _pick(lambda L, q: L in (7, 14) and (q >> (64 * L - 1)) == 1):
        for logN in LOGNS:
            for inv in (False, True):
                assert got(lib, L, q, logN, inv) == ("stages", False, False, [])
