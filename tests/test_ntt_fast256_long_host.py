"""CPU: the long Fast256 route (ringo-snark_amd/csrc/ntt_route.hpp ntt_fast256_long) and the twiddle
index algebra of its decomposition (ntt_long_prefix_tw, ntt_long_block_off, ntt_long_block_tw -- the
functions the kernels of ntt256.hpp themselves call), compiled for the host with g++ from the header.

The rule (restated here, not read from the header): the long route is taken exactly when
  L = 4, q[0] == 1 and the top bit of q[3] is clear;
  17 <= logN <= 19;
  not (inverse and rank_inv != N^-1, `halving` false): the fused last stage divides by 2^logN exactly;
  the switch does not start with r (the experiments build's generic route).
ntt_route() itself is untouched: for these plans it still answers tiled in two passes
(tests/test_ntt_route_host.py pins it); ntt.hip finalize() overrides the direction.

The replay runs the decomposition with Python integers over GF(257), scaled down so that the bottom
block is 2^4 points in 2 + 2 stages (COL on 4 columns of 4, ROW on 4 rows of 4) instead of 2^16 in
8 + 8, with M = 1, 2, 3 prefix stages above it: N = 2^5, 2^6, 2^7.  Forward: prefix (one 2^M-point
sub-transform at stride 2^4 per offset), then per block the COL and ROW stages at the 2^4 route's
own index moved by the block's offset.  Inverse: blocks (ROW, COL), then the suffix whose last stage
multiplies the difference by twInv[1] N^-1 and the sum by N^-1.  The blocks are walked as the runner
splits them: two halves, the second carrying its first block's index.  Every result must equal the
plain stage loop of oracle/pyref.py (ntt.go:261-275 / 372-386) element for element."""
import ctypes
import json
import os
import random
import subprocess

import pytest

import pyref

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "ringo-snark_amd", "csrc")

HARNESS = r"""
#include "ntt_route.hpp"
extern "C" int fast_long(int L, const uint64_t* q, int logN, int inv, int halving, const char* sw) {
  return rg::ntt_fast256_long(L, q, logN, inv != 0, halving != 0, sw) ? 1 : 0;
}
extern "C" int route_of(int L, const uint64_t* q, int logN, int inv, int halving, const char* sw) {
  return (int)rg::ntt_route(L, q, logN, inv != 0, halving != 0, sw).route;
}
extern "C" int route_tiled() { return (int)rg::NttRoute::Tiled; }
extern "C" unsigned prefix_tw(int M, int g, unsigned j) { return rg::ntt_long_prefix_tw(M, g, j); }
extern "C" unsigned block_off(int M, unsigned B) { return rg::ntt_long_block_off(M, B); }
extern "C" unsigned block_tw(unsigned idx16, unsigned boff, int gl) { return rg::ntt_long_block_tw(idx16, boff, gl); }
"""

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
    d = tmp_path_factory.mktemp("ntt_fast256_long")
    src, so = d / "fast256_long.cpp", d / "libfast256long.so"
    src.write_text(HARNESS)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", CSRC, str(src), "-o", str(so)],
                   check=True)
    lib = ctypes.CDLL(str(so))
    i, u = ctypes.c_int, ctypes.c_uint
    lib.fast_long.argtypes = [i, ctypes.c_void_p, i, i, i, ctypes.c_char_p]
    lib.route_of.argtypes = [i, ctypes.c_void_p, i, i, i, ctypes.c_char_p]
    lib.prefix_tw.argtypes, lib.prefix_tw.restype = [i, i, u], u
    lib.block_off.argtypes, lib.block_off.restype = [i, u], u
    lib.block_tw.argtypes, lib.block_tw.restype = [u, u, i], u
    return lib


def _words(L, q):
    return (ctypes.c_uint64 * L)(*[(q >> (64 * i)) & ((1 << 64) - 1) for i in range(L)])


def got(lib, name, logN, inv=False, halving=True, sw=None):
    L, q = FIELDS[name]
    return bool(lib.fast_long(L, _words(L, q), logN, int(inv), int(halving), sw.encode() if sw is not None else None))


def want(L, q, logN, inv, halving, sw):
    """The rule of the module docstring."""
    if L != 4 or (q & ((1 << 64) - 1)) != 1 or (q >> 255):
        return False
    if not 17 <= logN <= 19:
        return False
    if inv and not halving:
        return False
    return not (sw is not None and sw[:1] == "r")


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_long_route_matches_the_rule_on_the_whole_grid(lib, name):
    L, q = FIELDS[name]
    taken = 0
    for logN in LOGNS:
        for inv in (False, True):
            for halving in (True, False):
                for sw in SWITCHES:
                    g = got(lib, name, logN, inv, halving, sw)
                    assert g == want(L, q, logN, inv, halving, sw), (name, logN, inv, halving, sw)
                    taken += g
                    if g:  # ntt_route() keeps its answer: tiled
                        enc = sw.encode() if sw is not None else None
                        assert lib.route_of(L, _words(L, q), logN, int(inv), int(halving), enc) == lib.route_tiled()
    assert (taken > 0) == (name in ("jindo_zp", "zp220"))


def test_pinned_cases(lib):
    for name in ("jindo_zp", "zp220"):
        L, q = FIELDS[name]
        assert L == 4 and q & ((1 << 64) - 1) == 1 and q >> 255 == 0
        for logN in (17, 18, 19):
            assert got(lib, name, logN) and got(lib, name, logN, inv=True)
            assert got(lib, name, logN, inv=False, halving=False)  # forward does not scale
            assert not got(lib, name, logN, inv=True, halving=False)
            assert not got(lib, name, logN, sw="r") and not got(lib, name, logN, inv=True, sw="r")
            assert not got(lib, name, logN, sw="r8")
            assert got(lib, name, logN, sw="stage")
        for logN in (15, 16, 20, 24):
            assert not got(lib, name, logN) and not got(lib, name, logN, inv=True)
    assert FIELDS["s256_top"][1] >> 255 == 1 and FIELDS["bfv_zp"][1] & ((1 << 64) - 1) != 1
    for name in ("s256_top", "bfv_zp"):
        for logN in LOGNS:
            for inv in (False, True):
                assert not got(lib, name, logN, inv)
    for name, (L, _) in FIELDS.items():  # no other limb count
        if L != 4:
            assert not got(lib, name, 17) and not got(lib, name, 18, inv=True)


def test_index_functions(lib):
    for M in (1, 2, 3):
        for g in range(M):
            for j in range(1 << M):
                assert lib.prefix_tw(M, g, j) == (1 << g) + (j >> (M - g))
        for B in range(1 << M):
            boff = lib.block_off(M, B)
            assert boff == (1 << M) - 1 + B
            for gl in range(16):
                for i in (0, 1, (1 << gl) - 1):
                    # tw[2^(M+gl) + (B << gl) + i] from the 2^16 route's tw[2^gl + i]
                    assert lib.block_tw((1 << gl) + i, boff, gl) == (1 << (M + gl)) + (B << gl) + i
    assert lib.block_off(0, 0) == 0 and lib.block_tw(12345, 0, 7) == 12345


# ---- the replay ---------------------------------------------------------------------------------------
Q = 257   # 2N | q - 1 up to N = 2^7
LB = 4    # the scaled-down block: 2^4 points, COL = stages [0, 2) on 4 columns, ROW = [2, 4) on 4 rows
LC = 2    # stages per bottom pass


def _edge(lib, F, data, table, batch, M, inv, w1n=None, ninv=None):
    """The prefix (forward) or suffix (inverse) pass: a thread per (polynomial, offset)."""
    NP = 1 << M
    for p in range(batch):
        for o in range(1 << LB):
            at = [(p << (LB + M)) + (j << LB) + o for j in range(NP)]
            e = [data[i] for i in at]
            for sp in range(M):
                g = M - 1 - sp if inv else sp
                half = 1 << (M - 1 - g)
                for jj in range(NP // 2):
                    j0 = ((jj >> (M - 1 - g)) << (M - g)) + (jj & (half - 1))
                    j1 = j0 + half
                    ti = lib.prefix_tw(M, g, j0)
                    assert (1 << g) <= ti < (2 << g)
                    u, v = e[j0], e[j1]
                    if not inv:
                        t = F.mul(v, table[ti])
                        e[j0], e[j1] = F.add(u, t), F.sub(u, t)
                    elif g == 0:  # the fused last stage
                        assert ti == 1
                        e[j0], e[j1] = F.mul(F.add(u, v), ninv), F.mul(F.sub(u, v), w1n)
                    else:
                        e[j0], e[j1] = F.add(u, v), F.mul(F.sub(u, v), table[ti])
            for i, v in zip(at, e):
                data[i] = v


def _block_pass(lib, F, data, table, base, boff, col, inv):
    """One bottom pass over the block at `base`: LC stages, the 2^LB route's index moved by boff."""
    G0 = 0 if col else LB - LC
    for sub in range(1 << (LB - LC)):           # COL: a column (stride 4); ROW: a row
        hi = 0 if col else sub
        at = [base + ((x << (LB - LC)) + sub if col else (sub << LC) + x) for x in range(1 << LC)]
        e = [data[i] for i in at]
        for sp in range(LC):
            k = LC - 1 - sp if inv else sp      # local stage; bit b = LC - 1 - k of x
            b = LC - 1 - k
            for x0 in range(1 << LC):
                if x0 & (1 << b):
                    continue
                x1 = x0 | (1 << b)
                idx16 = (1 << (G0 + k)) + (hi << k) + (x0 >> (b + 1))
                ti = lib.block_tw(idx16, boff, G0 + k)
                u, v = e[x0], e[x1]
                if not inv:
                    t = F.mul(v, table[ti])
                    e[x0], e[x1] = F.add(u, t), F.sub(u, t)
                else:
                    e[x0], e[x1] = F.add(u, v), F.mul(F.sub(u, v), table[ti])
        for i, v in zip(at, e):
            data[i] = v


def _blocks(lib, F, data, table, first, count, blk0, M, inv):
    """run_blocks: `count` blocks from block `first` of the buffer; blk0 is the launch's first block."""
    for col in ((False, True) if inv else (True, False)):
        for i in range(count):
            B = (blk0 + i) & ((1 << M) - 1)
            _block_pass(lib, F, data, table, (first + i) << LB, lib.block_off(M, B), col, inv)


def _replay(lib, F, a, tw, twi, ninv, batch, M, inv):
    data = list(a)
    nb = batch << M
    h = (nb + 1) // 2  # the runner's two halves (there from 8 blocks up; here always, to walk blk0)
    if not inv:
        _edge(lib, F, data, tw, batch, M, False)
        _blocks(lib, F, data, tw, 0, h, 0, M, False)
        _blocks(lib, F, data, tw, h, nb - h, h, M, False)
    else:
        _blocks(lib, F, data, twi, 0, h, 0, M, True)
        _blocks(lib, F, data, twi, h, nb - h, h, M, True)
        _edge(lib, F, data, twi, batch, M, True, w1n=F.mul(twi[1], ninv), ninv=ninv)
    return data


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("M", [1, 2, 3])
def test_replay_of_the_decomposition_equals_the_reference(lib, M, batch):
    F = pyref.Field(Q, 1)
    N = 1 << (LB + M)
    rng = random.Random(10 * M + batch)
    for tables in (pyref.cyclic_tables, pyref.cyclotomic_tables):
        tw, twi, ninv, _ = tables(F, N)
        a = [rng.randrange(Q) for _ in range(batch * N)]
        a[:N] = [Q - 1] * (N // 2) + [0] * (N // 2)
        fwd = _replay(lib, F, a, tw, twi, ninv, batch, M, False)
        inv = _replay(lib, F, a, tw, twi, ninv, batch, M, True)
        for b in range(batch):
            assert fwd[b * N:(b + 1) * N] == pyref.ntt_fwd(F, a[b * N:(b + 1) * N], tw), (tables.__name__, b)
            assert inv[b * N:(b + 1) * N] == pyref.ntt_inv(F, a[b * N:(b + 1) * N], twi, ninv), (tables.__name__, b)
        assert _replay(lib, F, fwd, tw, twi, ninv, batch, M, True) == a


def test_replay_notices_a_wrong_block_offset(lib):
    """The replay is a check: with every block given block 0's offset the forward result is wrong."""
    F = pyref.Field(Q, 1)
    M, N = 2, 1 << (LB + 2)
    tw, _, _, _ = pyref.cyclotomic_tables(F, N)
    a = [(5 * i * i + 1) % Q for i in range(N)]
    data = list(a)
    _edge(lib, F, data, tw, 1, M, False)
    _blocks(lib, F, data, tw, 0, 1 << M, 0, 0, False)  # M = 0: boff = 0 everywhere
    assert data != pyref.ntt_fwd(F, a, tw)
