"""CPU: the index algebra of the 2^16 lazy pass tiles (ringo-snark_amd/csrc/ntt_tile.hpp: register
patterns, pair order, twiddle index, and the fold of rank_inv into the last inverse round) compiled
for the host with g++ and executed as a model of the tiles, with the portable Montgomery product
(ntt64.hpp mont64) and the kernels' lazy ranges.

The model runs a pass the way the kernels do: per sub-transform of 256 points and per lane slot t it
gathers the thread's registers through the pattern's x-of-register map, runs the round's stages in
the executed order on the pairs ntt_pair_rho0 lists with the table entry ntt_tw_index names, and
scatters them back.  It knows nothing of LDS images or of global addressing: what it checks is that
the patterns, the twiddle indices and the scaled / plain selection compute the reference's
transform.  Both tile shapes run: 8 points per thread (rounds of 3 + 3 + 2 stages, the shipped
kernels) and 16 points per thread (rounds of 4 + 4), COL and ROW, forward and inverse, every tile
of one polynomial, bit for bit against the C oracle for p63 = 47104^4 + 1 and 0x47e0f66500000001
(the tightest modulus under the Montgomery gate), negacyclic and cyclic.

The fold, three ways:
  * symbolically, from the header's own predicates: walking the last round's stages, both inputs of
    every butterfly have been scaled equally often, and after the round every one of the 8 (16)
    registers has been scaled exactly once;
  * numerically: the folded inverse equals the oracle's inverse with rank_inv = N^-1, = 1 and = a
    random residue, and equals the unfolded model (twInv[1] S on every last-stage butterfly and S on
    every x output, the form before the fold) limb for limb;
  * the constants ntt_fold_consts builds equal twInv[i] S computed with Python integers."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "ringo-snark_amd", "csrc")

LOGN = 16
N = 1 << LOGN
MODULI = {"p63": 47104 ** 4 + 1, "mont_tight": 0x47E0F66500000001}

HARNESS = r"""
#include "ntt64.hpp"
using namespace rg;
typedef unsigned __int128 u128;
namespace {
struct Mod {
  uint64_t q, q2;
  uint32_t q1;
  const uint64_t* tw;    // [N], Montgomery form
  const uint64_t* fold;  // [kNttFoldLen]: S, S tw[1 .. 16)
};
uint64_t canon(uint64_t v, uint64_t q) { return v >= q ? v - q : v; }
int g_range_errors = 0;
void in_range(uint64_t v, const Mod& m) { if (v >= m.q2) ++g_range_errors; }
// the kernels' lazy butterflies on [0, 2q)
void fwd_bfly(uint64_t& x, uint64_t& y, uint64_t w, const Mod& m) {
  const uint64_t t = mont64(y, w, m.q1);
  const u128 s = (u128)x + t;
  if (s >> 64) ++g_range_errors;  // the gate's promise: no 65th bit
  const uint64_t d = x >= t ? x - t : x - t + m.q2;
  x = (uint64_t)s >= m.q2 ? (uint64_t)s - m.q2 : (uint64_t)s;
  y = d;
}
void inv_bfly(uint64_t& x, uint64_t& y, uint64_t w, const Mod& m) {
  const u128 s = (u128)x + y;
  const uint64_t d = x >= y ? x - y : x - y + m.q2;
  x = s >= m.q2 ? (uint64_t)(s - m.q2) : (uint64_t)s;
  y = mont64(d, w, m.q1);
}
uint32_t xof(int pts, int pat, uint32_t t, int rho) { return pts == 8 ? ntt8_xof(pat, t, rho) : ntt16_xof(pat, t, rho); }
// scale: 0 none, 1 rank_inv the old way (on the last stage alone), 2 folded over the round
void round_model(uint64_t* p, size_t stride, int pts, int pat, int RK, int LO, bool inv, int scale, int G0, uint32_t hi,
                 const Mod& m) {
  uint64_t e[16];
  // the 16-point tile's round B reads the tile's staged LDS copy, as the kernel does
  const bool staged = pts == 16 && pat == 1;
  uint64_t ltw[kNtt16LtwLen];
  for (uint32_t i = 0; i < kNtt16LtwLen; ++i) ltw[i] = ~0ull;
  if (staged)
    for (uint32_t tid = 0; tid < 240; ++tid) ltw[ntt16_ltw_pos(16u + tid)] = m.tw[ntt16_stage_src(G0 == 0, hi, 16u + tid)];
  for (uint32_t t = 0; t < 256u / pts; ++t) {
    for (int r = 0; r < pts; ++r) e[r] = p[xof(pts, pat, t, r) * stride];
    for (int sp = 0; sp < RK; ++sp) {
      const int bw = ntt_round_bw(inv, RK, sp), b = LO + bw;
      for (int j = 0; j < pts / 2; ++j) {
        const int rho0 = ntt_pair_rho0(RK, bw, j), rho1 = rho0 + (1 << bw);
        const uint32_t idx = ntt_tw_index(G0, b, hi, xof(pts, pat, t, rho0));
        // both registers of a pair differ in bit b of x alone
        if (xof(pts, pat, t, rho1) != xof(pts, pat, t, rho0) + (1u << b)) ++g_range_errors;
        in_range(e[rho0], m);
        in_range(e[rho1], m);
        if (staged) {
          const uint64_t w = ltw[ntt16_ltw_pos((1u << (7 - b)) + (xof(pts, pat, t, rho0) >> (b + 1)))];
          if (w != m.tw[idx]) ++g_range_errors;
          if (!inv) fwd_bfly(e[rho0], e[rho1], w, m);
          else inv_bfly(e[rho0], e[rho1], w, m);
        } else if (!inv) {
          fwd_bfly(e[rho0], e[rho1], m.tw[idx], m);
        } else if (scale == 2) {
          const bool sc = ntt_fold_scaled(rho0, bw);
          if (sc && idx >= kNttFoldLen) ++g_range_errors;
          inv_bfly(e[rho0], e[rho1], sc ? m.fold[idx] : m.tw[idx], m);
          if (ntt_fold_product(rho0, bw, RK)) e[rho0] = mont64(e[rho0], m.fold[0], m.q1);
        } else if (scale == 1 && G0 + 7 - b == 0) {
          inv_bfly(e[rho0], e[rho1], m.fold[1], m);
          e[rho0] = mont64(e[rho0], m.fold[0], m.q1);
        } else {
          inv_bfly(e[rho0], e[rho1], m.tw[idx], m);
        }
      }
    }
    for (int r = 0; r < pts; ++r) p[xof(pts, pat, t, r) * stride] = e[r];
  }
}
// one pass over one polynomial, tile by tile (16 sub-transforms each): COL = global stages [0, 8)
// on the 256 columns, ROW = [8, 16) on the 256 rows
void pass_model(uint64_t* poly, int pts, bool col, bool inv, int scale, bool do_canon, const Mod& m) {
  static const int R8[3][3] = {{0, 3, 5}, {1, 3, 2}, {2, 2, 0}}, R16[2][3] = {{0, 4, 4}, {1, 4, 0}};
  const int nr = pts == 8 ? 3 : 2;
  for (int tile = 0; tile < 16; ++tile)
    for (int s = 0; s < 16; ++s) {
      const uint32_t sub = 16u * tile + s;
      uint64_t* p = poly + (col ? sub : 256u * sub);
      const size_t stride = col ? 256 : 1;
      for (int i = 0; i < nr; ++i) {
        const int* R = pts == 8 ? R8[inv ? nr - 1 - i : i] : R16[inv ? nr - 1 - i : i];
        const bool top = col && inv && R[0] == 0;  // the round that holds global stage 0
        round_model(p, stride, pts, R[0], R[1], R[2], inv, top ? scale : 0, col ? 0 : 8, col ? 0u : sub, m);
      }
      if (do_canon)
        for (int x = 0; x < 256; ++x) p[x * stride] = canon(p[x * stride], m.q);
    }
}
}  // namespace

extern "C" int model_ntt(uint64_t q, const uint64_t* tw, const uint64_t* fold, int pts_col, int pts_row, int inv,
                         int scale, uint64_t* poly) {
  const Mod m = {q, 2 * q, (uint32_t)(q >> 32), tw, fold};
  g_range_errors = 0;
  if (!inv) {
    pass_model(poly, pts_col, true, false, 0, false, m);
    pass_model(poly, pts_row, false, false, 0, true, m);
  } else {
    pass_model(poly, pts_row, false, true, 0, false, m);
    pass_model(poly, pts_col, true, true, scale, true, m);
  }
  return g_range_errors;
}
extern "C" void fold_consts(uint64_t q, const uint64_t* twinv, uint64_t S, uint64_t* out) {
  const uint32_t q1 = (uint32_t)(q >> 32);
  ntt_fold_consts(twinv, S, [&](uint64_t* z, const uint64_t* x, const uint64_t* y) { *z = canon(mont64(*x, *y, q1), q); }, out);
}
extern "C" int lds_pos(int col, int tid, int pat, int v) {
  const uint32_t s = ntt16_s_of(col != 0, tid), t = ntt16_t_of(col != 0, tid);
  return (int)ntt16_lds_pos(col != 0, s, ntt16_xof(pat, t, v));
}
extern "C" int lds_sx(int col, int tid, int pat, int v) {  // 256 s + x: which point the access moves
  return (int)(256u * ntt16_s_of(col != 0, tid) + ntt16_xof(pat, ntt16_t_of(col != 0, tid), v));
}
extern "C" int ltw_read_pos(int col, int tid, int b, int rho0) {
  return (int)ntt16_ltw_pos((1u << (7 - b)) + (ntt16_xof(1, ntt16_t_of(col != 0, tid), rho0) >> (b + 1)));
}
extern "C" int lds_len() { return (int)kNtt16LdsLen; }
extern "C" int ltw_len() { return (int)kNtt16LtwLen; }
extern "C" int ltw_pos(int i) { return (int)ntt16_ltw_pos(i); }
extern "C" int fold_len() { return (int)kNttFoldLen; }
extern "C" int fold_base() { return (int)kNttFoldBase; }
extern "C" int pair_rho0(int rk, int bw, int j) { return ntt_pair_rho0(rk, bw, j); }
extern "C" int round_bw(int inv, int rk, int sp) { return ntt_round_bw(inv != 0, rk, sp); }
extern "C" int fold_scaled(int rho0, int bw) { return ntt_fold_scaled(rho0, bw) ? 1 : 0; }
extern "C" int fold_product(int rho0, int bw, int rk) { return ntt_fold_product(rho0, bw, rk) ? 1 : 0; }
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("ntt_tile16")
    src, so = d / "tile.cpp", d / "libtile.so"
    src.write_text(HARNESS)
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, str(src), "-o", str(so)], check=True)
    L = ctypes.CDLL(str(so))
    L.model_ntt.argtypes = [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                            ctypes.c_int, ctypes.c_void_p]
    L.fold_consts.argtypes = [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    L.fold_consts.restype = None
    return L


@functools.lru_cache(maxsize=None)
def _cfield(name):
    import coracle as co
    return co.CField(MODULI[name])


@functools.lru_cache(maxsize=None)
def _case(name, cyclic):
    """(tables, input, forward, inverse with N^-1) of one polynomial, computed once; read-only."""
    from tests import synth_util as su
    cf = _cfield(name)
    q = MODULI[name]
    tabs = cf.tables(N, cyclic=cyclic)
    rng = np.random.default_rng(16 + cyclic)
    a = su.rand_residues(q, 1, N, rng).reshape(1, N, 1)
    a[0, :4, 0] = [q - 1, 0, 1, q - 1]
    out = tabs + (a, cf.ntt_fwd(a, tabs[0]), cf.ntt_inv(a, tabs[1], tabs[2]))
    for t in out:
        t.setflags(write=False)
    return out


def _fold(lib, q, twi, S):
    out = np.zeros(lib.fold_len(), np.uint64)
    tw = np.ascontiguousarray(twi.reshape(-1))
    lib.fold_consts(q, tw.ctypes.data, int(S), out.ctypes.data)
    return out


def _run(lib, q, tw, fold, pts_col, pts_row, inv, scale, a):
    poly = np.ascontiguousarray(a.reshape(-1)).copy()
    tw = np.ascontiguousarray(tw.reshape(-1))
    bad = lib.model_ntt(q, tw.ctypes.data, fold.ctypes.data, pts_col, pts_row, int(inv), scale, poly.ctypes.data)
    assert bad == 0, "a value left [0, 2q), a sum needed a 65th bit, or a pair is not one bit of x apart"
    return poly.reshape(a.shape)


SHAPES = [(8, 8), (16, 16), (16, 8), (8, 16)]  # points per thread: (COL, ROW); mixed plans are allowed


@pytest.mark.parametrize("cyclic", [False, True], ids=["negacyclic", "cyclic"])
@pytest.mark.parametrize("name", list(MODULI))
def test_tile_model_matches_the_oracle(lib, name, cyclic):
    q = MODULI[name]
    tw, twi, ninv, a, want_fwd, want_inv = _case(name, cyclic)
    S = int(ninv.reshape(-1)[0])
    fold = _fold(lib, q, twi, S)
    for pc, pr in SHAPES:
        got = _run(lib, q, tw, fold, pc, pr, False, 0, a)
        assert (got == want_fwd).all(), (name, cyclic, pc, pr, "forward")
        back = _run(lib, q, twi, fold, pc, pr, True, 2, got)
        assert (back == a).all(), (name, cyclic, pc, pr, "inverse of the forward")
        got_inv = _run(lib, q, twi, fold, pc, pr, True, 2, a)
        assert (got_inv == want_inv).all(), (name, cyclic, pc, pr, "inverse, folded")
        unfolded = _run(lib, q, twi, fold, pc, pr, True, 1, a)
        assert (unfolded == want_inv).all(), (name, cyclic, pc, pr, "inverse, rank_inv on the last stage")


@pytest.mark.parametrize("rk,nreg", [(3, 8), (4, 16)], ids=["8-point", "16-point"])
def test_fold_scales_every_output_exactly_once(lib, rk, nreg):
    """From the header's predicates alone: count how often each register has been scaled."""
    count = [0] * nreg
    for sp in range(rk):
        bw = lib.round_bw(1, rk, sp)
        assert bw == sp  # Gentleman-Sande: the window's bits upwards
        seen = set()
        for j in range(nreg // 2):
            rho0 = lib.pair_rho0(rk, bw, j)
            rho1 = rho0 + (1 << bw)
            assert not {rho0, rho1} & seen and rho1 < nreg
            seen |= {rho0, rho1}
            assert count[rho0] == count[rho1], "a butterfly adds and subtracts values of one scale"
            sc = lib.fold_scaled(rho0, bw)
            assert sc == (count[rho0] == 0), "scaled twiddle exactly where the inputs are still unscaled"
            count[rho1] += sc
            if lib.fold_product(rho0, bw, rk):
                assert (rho0, sp) == (0, rk - 1)
                count[rho0] += 1
        assert len(seen) == nreg
    assert count == [1] * nreg


@pytest.mark.parametrize("col", [1, 0], ids=["COL", "ROW"])
def test_16_point_lds_images_are_conflict_free(lib, col):
    """Every LDS access of the 16-point tile, lane group by lane group: ds_write_b64 is served in
    groups of 16 consecutive lanes on 32 banks of 4 B (the 16 u64 indices distinct mod 16),
    ds_read_b64 in half-waves on 64 banks (32 indices distinct mod 32).  The image holds each of the
    tile's 4096 points exactly once, inside the array, whichever pattern names it."""
    where = {}
    for pat in (0, 1):
        for v in range(16):
            pos = [lib.lds_pos(col, tid, pat, v) for tid in range(256)]
            for tid in range(256):
                sx = lib.lds_sx(col, tid, pat, v)
                assert where.setdefault(sx, pos[tid]) == pos[tid], "both patterns find a point at one place"
            for g in range(0, 256, 16):
                assert len({p % 16 for p in pos[g:g + 16]}) == 16, ("write", pat, v, g)
            for g in range(0, 256, 32):
                assert len({p % 32 for p in pos[g:g + 32]}) == 32, ("read", pat, v, g)
    assert len(where) == 4096 and len(set(where.values())) == 4096
    assert 0 <= min(where.values()) and max(where.values()) < lib.lds_len()
    # the staged twiddles: 240 distinct slots, and round B's reads hit distinct banks or one address
    slots = {lib.ltw_pos(i) for i in range(16, 256)}
    assert len(slots) == 240 and 0 <= min(slots) and max(slots) < lib.ltw_len()
    for b in range(4):
        for rho0 in range(16):
            if rho0 >> b & 1:
                continue
            for g in range(0, 256, 32):
                addrs = {lib.ltw_read_pos(col, tid, b, rho0) for tid in range(g, g + 32)}
                assert addrs <= slots
                assert len({p % 32 for p in addrs}) == len(addrs), ("twiddle read", b, rho0, g)


@pytest.mark.parametrize("name", list(MODULI))
def test_fold_with_any_rank_inv(lib, name):
    """S = N^-1, S = 1 (Montgomery form) and a random S: the fold uses the plan's value."""
    q = MODULI[name]
    cf = _cfield(name)
    tw, twi, ninv, a, _, _ = _case(name, False)
    R = (1 << 64) % q
    rnd = int(np.random.default_rng(7).integers(1, q, dtype=np.uint64))
    for what, S in (("N^-1", int(ninv.reshape(-1)[0])), ("one", R), ("random", rnd)):
        fold = _fold(lib, q, twi, S)
        want = cf.ntt_inv(a, twi, np.array([S], np.uint64))
        for pc, pr in SHAPES[:2]:
            got = _run(lib, q, twi, fold, pc, pr, True, 2, a)
            assert (got == want).all(), (name, what, pc, pr)


@pytest.mark.parametrize("name", list(MODULI))
def test_fold_constants_are_the_products(lib, name):
    q = MODULI[name]
    _, twi, ninv, _, _, _ = _case(name, False)
    rinv = pow(1 << 64, -1, q)
    tv = [int(v) for v in twi.reshape(-1)[:lib.fold_len()]]
    assert lib.fold_len() == 16 and lib.fold_base() == N + 256 * 192
    for S in (int(ninv.reshape(-1)[0]), (1 << 64) % q, 0x123456789ABCDEF % q):
        got = [int(v) for v in _fold(lib, q, twi, S)]
        assert got[0] == S
        for i in range(1, 16):
            assert got[i] == tv[i] * S * rinv % q, (name, i)  # the Montgomery product of the two forms
