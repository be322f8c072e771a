// ntt_tile.hpp -- index algebra of the 2^16 lazy pass tiles (ntt64.hpp ntt16_pass), HIP-free and
// <stdint.h> only, shared by the kernels, by the plan's table upload (ntt.hip) and by the host model
// of tests/test_ntt_tile16_host.py: which point a register holds in each round, which table entry a
// butterfly reads, in which order a round pairs its registers, and which butterflies of the last
// inverse round carry the rank_inv factor.
//
// A tile is 16 sub-transforms of 256 points; x < 256 is the index inside one sub-transform, a pass
// covers the 8 global stages [G0, G0 + 8), local stage k combines bit b = 7 - k of x.  A round runs
// RK consecutive stages on the 2^RK (or, L round, two groups of 2^RK) registers of a thread without
// leaving them; `bw` is the stage's bit inside the round's window [LO, LO + RK), b = LO + bw.
#pragma once
#include <stdint.h>

namespace rg {

// ---- register patterns: x of register rho in lane slot t ----
// 8 points per thread, rounds of 3 + 3 + 2 stages (t < 32):
//   H (pat 0): window [5, 8)   M (pat 1): window [2, 5)   L (pat 2): window [0, 2), rho >> 2 = x bit 2
constexpr uint32_t ntt8_xof(int pat, uint32_t t, int rho) {
  return pat == 0 ? t + 32u * (uint32_t)rho
       : pat == 1 ? (((t >> 2) << 5) | ((uint32_t)rho << 2) | (t & 3u))
                  : 8u * t + (uint32_t)rho;
}
// 16 points per thread, rounds of 4 + 4 stages (t < 16): A (pat 0): window [4, 8), B (pat 1): [0, 4)
constexpr uint32_t ntt16_xof(int pat, uint32_t t, int rho) { return pat == 0 ? t + 16u * (uint32_t)rho : 16u * t + (uint32_t)rho; }

// Round B of the 16-point tile reads its 240 per-lane twiddles, local table entries i = 2^k + j in
// [16, 256) (k = 4 .. 7 the local stage, j = x >> (b + 1) < 2^k), from a copy in LDS that the tile
// stages itself, one word per thread:
//   COL: tw[i];   ROW, row `hi`: tw[2^(8+k) + (hi << k) + j], the row's four contiguous runs
// at ntt16_ltw_pos(i): the pad i >> 5 keeps the 16 lane slots of a ROW half-wave (stride 2^(k-4)
// entries) on distinct banks; COL lanes of a half-wave share two addresses either way.
constexpr uint32_t kNtt16LtwLen = 248;
constexpr uint32_t ntt16_ltw_pos(uint32_t i) { return i - 16u + (i >> 5); }
constexpr uint32_t ntt16_stage_src(bool col, uint32_t hi, uint32_t i) {
  const uint32_t k = i < 32u ? 4u : i < 64u ? 5u : i < 128u ? 6u : 7u;
  return col ? i : (1u << (8u + k)) + (hi << k) + (i - (1u << k));
}
// LDS images of the 16-point tile (u64 index), a lane base plus compile-time offsets per register:
//   COL: 16 x + s + 16 (x >> 4)   A: 16 t + s + 272 y     B: 272 t + s + 16 r
//   ROW: 272 s + x + (x >> 4)     A: 272 s + t + 17 y     B: 272 s + 17 t + r
// ds_write_b64 is served in groups of 16 consecutive lanes on 32 banks of 4 B (16 distinct u64
// indices mod 16), ds_read_b64 in half-waves on 64 banks (32 distinct mod 32):
// tests/test_ntt_tile16_host.py walks every lane group of every access.
constexpr uint32_t kNtt16LdsLen = 16u * 272u;
constexpr uint32_t ntt16_lds_pos(bool col, uint32_t s, uint32_t x) {
  return col ? 16u * x + s + 16u * (x >> 4) : 272u * s + x + (x >> 4);
}
// thread -> (s, t): COL keeps the 16 columns of a row in consecutive lanes (128-B runs of the
// global accesses), ROW the 16 lane slots of one sub-transform (128-B runs of the A pattern)
constexpr uint32_t ntt16_s_of(bool col, uint32_t tid) { return col ? tid & 15u : tid >> 4; }
constexpr uint32_t ntt16_t_of(bool col, uint32_t tid) { return col ? tid >> 4 : tid & 15u; }

// stage order inside a round: forward (Cooley-Tukey) runs the window's bits downwards, inverse
// (Gentleman-Sande) upwards; sp = 0 .. RK - 1 is the executed order
constexpr int ntt_round_bw(bool inv, int rk, int sp) { return inv ? sp : rk - 1 - sp; }

// low register of the j-th butterfly of a stage (its partner is rho0 + 2^bw); j runs over half the
// thread's registers, groups of 2^rk registers one after the other
constexpr int ntt_pair_rho0(int rk, int bw, int j) {
  const int npk = 1 << rk, grp = j / (npk / 2), jj = j % (npk / 2), half = 1 << bw;
  return grp * npk + ((jj >> bw) << (bw + 1)) + (jj & (half - 1));
}

// table entry of the butterfly on bit b of x in sub-transform `hi` (COL: 0, ROW: the row): the
// reference's tw[m + i] order (ntt.go:98-115 forward, :357-466 inverse)
constexpr uint32_t ntt_tw_index(int G0, int b, uint32_t hi, uint32_t x) {
  return (1u << (G0 + 7 - b)) + (hi << (7 - b)) + (x >> (b + 1));
}

// ---- rank_inv folded into the last inverse round (the round that holds global stage 0) ----
// In a Gentleman-Sande network both inputs of a butterfly took the same branch at every earlier
// stage of the round, so the factor S = rank_inv rides on the y-branch twiddle of the first stage at
// which a register takes the y branch: the butterfly (rho0, rho0 + 2^bw) uses S tw when the low bw
// bits of rho0 are zero (its inputs have only taken x branches so far, and are unscaled) and plain
// tw otherwise.  The one output that never takes a y branch, register 0 after the round's last
// stage, is multiplied by S explicitly.  Every output is scaled exactly once.
constexpr bool ntt_fold_scaled(int rho0, int bw) { return (rho0 & ((1 << bw) - 1)) == 0; }
constexpr bool ntt_fold_product(int rho0, int bw, int rk) { return bw == rk - 1 && rho0 == 0; }

// The scaled variants live behind the inverse table of a MONT plan (ntt.hip upload_mont64):
// [kNttFoldBase] = S, [kNttFoldBase + i] = S twInv[i] for 0 < i < 16, Montgomery form.  The last
// round's stages read twInv[1 .. 2^RK) only (G0 = 0, hi = 0, window at the top of x), so the 8-point
// tile uses entries 1 .. 7 and a 16-point tile all of them.
constexpr uint32_t kNttRowCopyBase = 65536u, kNttRowCopyLen = 256u * 192u;
constexpr uint32_t kNttFoldBase = kNttRowCopyBase + kNttRowCopyLen, kNttFoldLen = 16u;
// mul(z, x, y): z = x y in the table's form
template <class Mul>
inline void ntt_fold_consts(const uint64_t* twinv, uint64_t S, Mul mul, uint64_t* out) {
  out[0] = S;
  for (uint32_t i = 1; i < kNttFoldLen; ++i) mul(&out[i], &twinv[i], &S);
}

}  // namespace rg
