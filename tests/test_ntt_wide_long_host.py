"""CPU: the long wide route (ringo-snark_amd/csrc/ntt_route.hpp ntt_wide_long, ntt_wide_split) and the
index algebra of the wide pass tiles (ntt_wide_tile.hpp: wide_cpt, wide_grid, wide_elem, wide_load_c /
wide_load_x, wide_bfly_x0, wide_tw_idx -- the functions ntt_wide_pass itself calls), compiled for the
host with g++ from the same headers.

The rules (restated here, not read from the header):
  L = 7, 14 only.  No long route when the top bit of q is set, for an inverse whose rank_inv is not
  N^-1 (`halving` false), or when the switch starts with s.  Otherwise
    switch "w3" and 3 <= logN <= 24: three passes;
    else 17 <= logN <= 24: ceil(logN / 8) passes (three at every such logN);
    else none.
  n passes split logN as evenly as possible, larger first: pass k has logN // n stages, one more for
  k < logN % n, and starts where the one before it ends; forward order.
  ntt_route() itself is untouched: above 2^16 it still says stages (tests/test_ntt_route_host.py).

A tile: cpt = min(256 >> P, 2^logS) sub-transforms (256 >> P at logS = 0), a launch has
ceil(batch 2^(logN - P) / cpt) workgroups and is refused (-1) above 2^31 - 1.

The replay runs the kernel's loops on the host with Python integers over GF(65537): per pass, per
workgroup, the tile load in the kernel's order through wide_elem, the P stages with wide_bfly_x0 and
wide_tw_idx, the store; forward passes in order, inverse passes and stages reversed with every
butterfly output halved.  The result must equal oracle/pyref.py's transforms.  With the forced split
the middle pass (G0 > 0 and logS > 0) runs at logN = 3, 7, 9, 12; batch 3 leaves the last row tile
partly past the batch."""
import ctypes
import json
import os
import subprocess

import pytest

import pyref

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "ringo-snark_amd", "csrc")

HARNESS = r"""
#include "ntt_route.hpp"
#include "ntt_wide_tile.hpp"
// out: npasses, then (G0, P) of three passes
extern "C" void long_run(int L, const uint64_t* q, int logN, int inv, int halving, const char* sw, int* out) {
  const rg::WidePasses w = rg::ntt_wide_long(L, q, logN, inv != 0, halving != 0, sw);
  out[0] = w.npasses;
  for (int i = 0; i < 3; ++i) {
    out[1 + 2 * i] = w.passes[i].G0;
    out[2 + 2 * i] = w.passes[i].P;
  }
}
extern "C" int route_of(int L, const uint64_t* q, int logN, int inv, int halving, const char* sw) {
  return (int)rg::ntt_route(L, q, logN, inv != 0, halving != 0, sw).route;
}
extern "C" int route_stages() { return (int)rg::NttRoute::Stages; }
extern "C" int cpt(int P, int logS) { return rg::wide_cpt(P, logS); }
extern "C" long long grid(unsigned long long batch, int logN, int P, int cpt) { return rg::wide_grid(batch, logN, P, cpt); }
extern "C" long long elem(long long s, long long nsub, int logN, int G0, int P, int logS, int x) {
  return rg::wide_elem(s, nsub, logN, G0, P, logS, x);
}
extern "C" int load_c(int P, int logS, int cpt, int e) { return rg::wide_load_c(P, logS, cpt, e); }
extern "C" int load_x(int P, int logS, int cpt, int e) { return rg::wide_load_x(P, logS, cpt, e); }
extern "C" int bfly_x0(int P, int g, int p) { return rg::wide_bfly_x0(P, g, p); }
extern "C" long long tw_idx(long long s, int logN, int G0, int P, int logS, int g, int x0) {
  return rg::wide_tw_idx(s, logN, G0, P, logS, g, x0);
}
"""

SWITCHES = [None, "s", "w3"]
LOGNS = range(0, 27)
MAX_GRID = (1 << 31) - 1


def _fields():
    out = {}
    for name in ("fields.json", "synthetic_fields.json"):
        for k, v in json.load(open(os.path.join(HERE, "golden", name))).items():
            if int(v["limbs"]) in (7, 14):
                out[k] = (int(v["limbs"]), int(v["q_hex"], 16))
    return out


FIELDS = _fields()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("ntt_wide_long")
    src, so = d / "wide_long.cpp", d / "libwidelong.so"
    src.write_text(HARNESS)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", CSRC, str(src), "-o", str(so)],
                   check=True)
    L = ctypes.CDLL(str(so))
    i, ll = ctypes.c_int, ctypes.c_longlong
    L.long_run.argtypes = [i, ctypes.c_void_p, i, i, i, ctypes.c_char_p, ctypes.c_void_p]
    L.long_run.restype = None
    L.route_of.argtypes = [i, ctypes.c_void_p, i, i, i, ctypes.c_char_p]
    L.grid.argtypes, L.grid.restype = [ctypes.c_ulonglong, i, i, i], ll
    L.elem.argtypes, L.elem.restype = [ll, ll, i, i, i, i, i], ll
    L.tw_idx.argtypes, L.tw_idx.restype = [ll, i, i, i, i, i, i], ll
    return L


def _words(L, q):
    return (ctypes.c_uint64 * L)(*[(q >> (64 * i)) & ((1 << 64) - 1) for i in range(L)])


def got(lib, L, q, logN, inv=False, halving=True, sw=None):
    """[(G0, P), ...] of the long route, [] for none."""
    out = (ctypes.c_int * 7)()
    lib.long_run(L, _words(L, q), logN, int(inv), int(halving), sw.encode() if sw is not None else None, out)
    return [(out[1 + 2 * i], out[2 + 2 * i]) for i in range(out[0])]


def split(logN, n):
    passes, g0 = [], 0
    for k in range(n):
        P = logN // n + (1 if k < logN % n else 0)
        passes.append((g0, P))
        g0 += P
    return passes


def want(L, q, logN, inv, halving, sw):
    """The rules of the module docstring."""
    if L not in (7, 14) or (q >> (64 * L - 1)) or (inv and not halving) or (sw is not None and sw[:1] == "s"):
        return []
    if sw == "w3" and 3 <= logN <= 24:
        return split(logN, 3)
    if 17 <= logN <= 24:
        return split(logN, -(-logN // 8))
    return []


def test_split_examples():
    assert [p for _, p in split(17, 3)] == [6, 6, 5]
    assert [p for _, p in split(18, 3)] == [6, 6, 6]
    assert [p for _, p in split(20, 3)] == [7, 7, 6]
    assert [p for _, p in split(24, 3)] == [8, 8, 8]
    assert split(17, 3) == [(0, 6), (6, 6), (12, 5)]


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_long_route_matches_the_rules_on_the_whole_grid(lib, name):
    L, q = FIELDS[name]
    spare = (q >> (64 * L - 1)) == 0
    taken = 0
    for logN in LOGNS:
        for inv in (False, True):
            for halving in (True, False):
                for sw in SWITCHES:
                    passes = got(lib, L, q, logN, inv, halving, sw)
                    assert passes == want(L, q, logN, inv, halving, sw), (name, logN, inv, halving, sw)
                    if not spare:
                        assert passes == []
                    if passes:
                        taken += 1
                        assert len(passes) <= 3 and sum(p for _, p in passes) == logN
                        assert all(1 <= p <= 8 for _, p in passes)
                        g0 = 0
                        for G0, P in passes:  # contiguous from G0 = 0
                            assert G0 == g0
                            g0 += P
                        assert sorted((p for _, p in passes), reverse=True) == [p for _, p in passes]
                        assert max(p for _, p in passes) - min(p for _, p in passes) <= 1
                    # ntt_route() keeps its answer above 2^16: stages
                    if logN > 16:
                        enc = sw.encode() if sw is not None else None
                        assert lib.route_of(L, _words(L, q), logN, int(inv), int(halving), enc) == lib.route_stages()
    assert (taken > 0) == spare


def test_pinned_long_routes(lib):
    spare = [(L, q) for L, q in FIELDS.values() if (q >> (64 * L - 1)) == 0]
    assert {L for L, _ in spare} == {7, 14}
    for L, q in spare:
        assert got(lib, L, q, 17) == [(0, 6), (6, 6), (12, 5)]
        assert got(lib, L, q, 17, inv=True) == [(0, 6), (6, 6), (12, 5)]  # forward order; the runner reverses
        assert got(lib, L, q, 17, inv=True, halving=False) == []
        assert got(lib, L, q, 17, inv=False, halving=False) == [(0, 6), (6, 6), (12, 5)]
        assert got(lib, L, q, 24) == [(0, 8), (8, 8), (16, 8)]
        assert got(lib, L, q, 16) == [] and got(lib, L, q, 25) == []
        assert got(lib, L, q, 17, sw="stage") == []
        assert got(lib, L, q, 3, sw="w3") == [(0, 1), (1, 1), (2, 1)]
        assert got(lib, L, q, 7, sw="w3") == [(0, 3), (3, 2), (5, 2)]
        assert got(lib, L, q, 2, sw="w3") == [] and got(lib, L, q, 25, sw="w3") == []
    q = FIELDS["zp440"][1]
    for L in (1, 2, 4):  # no other limb count has a long route
        assert got(lib, L, q, 17) == [] and got(lib, L, q, 9, sw="w3") == []


def test_tile_shape(lib):
    for P in range(1, 9):
        for logS in range(0, 24):
            want_cpt = (256 >> P) if logS == 0 else min(256 >> P, 1 << logS)
            assert lib.cpt(P, logS) == want_cpt
            assert want_cpt << P <= 256
            if logS:
                assert (1 << logS) % want_cpt == 0  # a tile stays inside one stride


def test_grid_limit(lib):
    """wide_grid: ceil(batch 2^(logN - P) / cpt), -1 above 2^31 - 1 workgroups (the launch takes an
    unsigned).  At 2^24 a pass of 8 stages has 2^16 one-tile workgroups per polynomial, so batch
    32767 is the last that fits: 30 TB of zp440 polynomials, beyond any device, hence a host test."""
    def ref(batch, logN, P, cpt):
        g = -(-(batch << (logN - P)) // cpt)
        return g if g <= MAX_GRID else -1

    assert lib.grid(32767, 24, 8, 1) == 32767 << 16
    assert lib.grid(32768, 24, 8, 1) == -1
    assert lib.grid(MAX_GRID, 8, 8, 1) == MAX_GRID and lib.grid(MAX_GRID + 1, 8, 8, 1) == -1
    for logN in (3, 9, 16, 17, 20, 24):
        for passes in (split(logN, 3), split(logN, 2) if logN <= 16 else []):
            for G0, P in passes:
                cpt = lib.cpt(P, logN - G0 - P)
                edge = (MAX_GRID * cpt) >> (logN - P)
                for batch in (1, 3, 16, edge - 1, edge, edge + 1, 2 * edge, 1 << 40, 1 << 62, (1 << 63) + 5, (1 << 64) - 1):
                    assert lib.grid(batch, logN, P, cpt) == ref(batch, logN, P, cpt), (batch, logN, P, cpt)


# ---- the replay ---------------------------------------------------------------------------------------
Q = 65537  # 2^16 + 1: 2N | q - 1 up to N = 2^15


def _run_pass(lib, F, data, table, batch, logN, G0, P, inv):
    """One ntt_wide_pass launch over `data` (batch 2^logN Montgomery values), in the kernel's loops."""
    logS = logN - G0 - P
    NP, cpt = 1 << P, lib.cpt(P, logS)
    nsub = batch << (logN - P)
    grid = lib.grid(batch, logN, P, cpt)
    assert grid == -(-nsub // cpt)
    half = (F.q + 1) // 2
    seen = set()
    for block in range(grid):
        s0 = block * cpt
        lds, where = [None] * (cpt * NP), [None] * (cpt * NP)
        for e in range(cpt * NP):
            c, x = lib.load_c(P, logS, cpt, e), lib.load_x(P, logS, cpt, e)
            g = lib.elem(s0 + c, nsub, logN, G0, P, logS, x)
            assert where[c * NP + x] is None  # the load order is a bijection onto the tile
            where[c * NP + x] = g
            if g >= 0:
                assert 0 <= g < len(data) and g not in seen
                seen.add(g)
                lds[c * NP + x] = data[g]
            else:
                assert s0 + c >= nsub
        for st in range(P):
            g = P - 1 - st if inv else st
            for bf in range(cpt * (NP >> 1)):
                c, p = bf >> (P - 1), bf & ((NP >> 1) - 1)
                x0 = lib.bfly_x0(P, g, p)
                x1 = x0 | (1 << (P - 1 - g))
                assert 0 <= x0 < x1 < NP
                ti = lib.tw_idx(s0 + c, logN, G0, P, logS, g, x0)
                assert (1 << (G0 + g)) <= ti < (2 << (G0 + g)) <= len(table)
                u, v = lds[c * NP + x0], lds[c * NP + x1]
                if u is None:  # a sub-transform past the batch: the kernel's lanes work on nothing stored
                    assert v is None
                    continue
                w = table[ti]
                if not inv:
                    t = F.mul(v, w)
                    lds[c * NP + x0], lds[c * NP + x1] = F.add(u, t), F.sub(u, t)
                else:  # every stage halved: log N halvings are N^-1; the table holds twInv / 2
                    lds[c * NP + x0], lds[c * NP + x1] = F.add(u, v) * half % F.q, F.mul(F.sub(u, v), w)
        for i, g in enumerate(where):
            if g >= 0:
                data[g] = lds[i]
    assert len(seen) == len(data)  # every element in exactly one tile


def _replay(lib, F, a, passes, table, batch, logN, inv):
    data = list(a)
    for G0, P in (reversed(passes) if inv else passes):
        _run_pass(lib, F, data, table, batch, logN, G0, P, inv)
    return data


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("logN", [3, 7, 9, 12])
def test_replay_of_the_forced_split_equals_the_reference(lib, logN, batch):
    import random
    F = pyref.Field(Q, 1)
    N = 1 << logN
    L, q = FIELDS["zp440"]
    passes = got(lib, L, q, logN, sw="w3")
    assert len(passes) == 3 and passes[1][0] > 0 and logN - passes[1][0] - passes[1][1] > 0  # a middle pass
    rng = random.Random(100 * logN + batch)
    half = (Q + 1) // 2
    for tables in (pyref.cyclic_tables, pyref.cyclotomic_tables):
        tw, twi, ninv, _ = tables(F, N)
        twi_half = [w * half % Q for w in twi]  # what upload_wide() builds
        a = [rng.randrange(Q) for _ in range(batch * N)]
        a[:N] = [Q - 1] * (N // 2) + [0] * (N // 2)
        fwd = _replay(lib, F, a, passes, tw, batch, logN, False)
        inv = _replay(lib, F, a, passes, twi_half, batch, logN, True)
        for b in range(batch):
            assert fwd[b * N:(b + 1) * N] == pyref.ntt_fwd(F, a[b * N:(b + 1) * N], tw), (tables.__name__, b)
            assert inv[b * N:(b + 1) * N] == pyref.ntt_inv(F, a[b * N:(b + 1) * N], twi, ninv), (tables.__name__, b)
        assert _replay(lib, F, fwd, passes, twi_half, batch, logN, True) == a


def test_replay_of_the_two_pass_plan_still_equals_the_reference(lib):
    """The same functions at the positions the kernel already ran at: COL then ROW, 2^9 = 4 + 5."""
    F = pyref.Field(Q, 1)
    logN, N = 9, 512
    tw, twi, ninv, _ = pyref.cyclotomic_tables(F, N)
    a = [(7 * i * i + 3) % Q for i in range(2 * N)]
    fwd = _replay(lib, F, a, [(0, 4), (4, 5)], tw, 2, logN, False)
    assert fwd[:N] == pyref.ntt_fwd(F, a[:N], tw) and fwd[N:] == pyref.ntt_fwd(F, a[N:], tw)
