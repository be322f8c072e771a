// ntt_route.hpp -- which of the five NTT kernel families serves a plan, and in which passes:
// decided once, when the plan is created (ntt.hip finalize()), by ntt_route() below and, above 2^16,
// by ntt_wide_long() (the wide fields) and ntt_fast256_long() (the 4-limb q = 1 mod 2^64 fields) at
// the end.  HIP-free, <stdint.h> only: tests/test_ntt_route_host.py, tests/test_ntt_wide_long_host.py
// and tests/test_ntt_fast256_long_host.py compile it with g++ and walk every field, rank, direction
// and switch value.  DESIGN.md section 4.0 has the rules as a table.
#pragma once
#include <stdint.h>

namespace rg {

// per-L register radix (points per thread = 2^R) keeps VGPR use near 128
constexpr int ntt_radix(int L) { return L <= 2 ? 4 : (L <= 4 ? 3 : 2); }
constexpr int ntt_pmax(int L) { return ntt_radix(L) + 8; }  // most stages in one LDS-tiled pass
template <int L>
struct RadixOf {
  static constexpr int value = ntt_radix(L);
};
template <int L>
constexpr int pmax_of() {
  return ntt_pmax(L);
}
// smallest P handled by the LDS-tiled pass kernel (smaller transforms use stage kernels)
constexpr int kMinTiledP = 6;

// The Montgomery twiddle product of the lazy passes (ntt64.hpp, MONT) needs
// 3q + ceil(2 q^2 / 2^64) + 2^33 < 2^64, that is q1 = q >> 32 <= 0x47e0f66a (q / 2^64 <= 0.28078);
// the derivation is at mont64 in ntt64.hpp, tests/test_mont64_host.py checks the constant.
constexpr uint32_t kMontMaxQ1 = 0x47e0f66au;
constexpr bool ntt64_mont_ok(uint64_t q) { return (uint32_t)q == 1u && (q >> 32) != 0 && (q >> 32) <= kMontMaxQ1; }

// Lazy64 with the Montgomery product: whether a direction's 16-point pass (ntt64.hpp: ROW forward
// on RP tiles, batch % 16 == 0; COL inverse) runs on the tile of 16 points per thread (rounds of
// 4 + 4 stages, one LDS exchange fewer) or, like every other pass and every Shoup plan, on 8 points
// (3 + 3 + 2).  sw: the NttKernel switch of the experiments build or null; t8 keeps 8 points.
inline bool ntt64_tile16(bool mont, const char* sw) { return mont && !(sw && sw[0] == 't' && sw[1] == '8'); }

enum class NttRoute : int {
  Stages,   // ntt_stage_kernel, one launch per stage: whatever the others leave
  Tiled,    // ntt_pass_kernel / ntt_r2 / ntt_r8, LDS-tiled: L <= 4, kMinTiledP <= logN <= 2 pmax
  Lazy64,   // ntt16_pass (ntt64.hpp): L = 1, q < 2^63, q mod 2^32 == 1, logN = 16
  Fast256,  // ntt256_pass (ntt256.hpp): L = 4, q[0] == 1, q < 2^255, logN = 15, 16 here;
            // 17 <= logN <= 19 by ntt_fast256_long() below
  Wide      // ntt_wide_pass (ntt_wide.hpp): L = 7, 14, spare top bit, 1 <= logN <= 16 here;
            // 17 <= logN <= 24 by ntt_wide_long() below
};

// a pass covers the P global stages [G0, G0 + P)
struct PassDesc {
  int G0, P;
};

struct NttRouting {
  NttRoute route;
  bool shoup;  // L = 1, q < 2^63: (w, w') Shoup pair tables and products (all routes but Lazy64 with mont)
  bool mont;   // Lazy64 only: ntt64_mont_ok(q), single-word Montgomery tables and the MONT kernels
  int npasses;
  PassDesc passes[2];  // forward order; none for Stages
};

// one pass of logN when pa == logN, else pa stages then the rest
inline void ntt_set_passes(NttRouting& r, int logN, int pa) {
  r.npasses = pa < logN ? 2 : 1;
  r.passes[0] = {0, pa};
  if (pa < logN) r.passes[1] = {pa, logN - pa};
}

// L limbs of modulus q, N = 2^logN, one direction; halving: rank_inv == N^-1 (the wide inverse
// halves per stage and so cannot scale by anything else); sw: the NttKernel switch of the
// experiments build (common.hpp) or null: r* leaves Lazy64 and Fast256 to Tiled, s* Wide to Stages.
inline NttRouting ntt_route(int L, const uint64_t* q, int logN, bool inv, bool halving, const char* sw) {
  NttRouting r = {NttRoute::Stages, false, false, 0, {{0, 0}, {0, 0}}};
  const bool generic = sw && sw[0] == 'r', per_stage = sw && sw[0] == 's';
  if (L == 7 || L == 14) {
    if (logN >= 1 && logN <= 16 && (q[L - 1] >> 63) == 0 && !(inv && !halving) && !per_stage) {
      r.route = NttRoute::Wide;
      ntt_set_passes(r, logN, logN <= 8 ? logN : logN / 2);  // COL then ROW
    }
    return r;
  }
  r.shoup = L == 1 && (q[0] >> 63) == 0;
  if (r.shoup && logN == 16 && (uint32_t)q[0] == 1u && !generic) {
    r.route = NttRoute::Lazy64;
    r.mont = ntt64_mont_ok(q[0]);
  } else if (L == 4 && (logN == 15 || logN == 16) && q[0] == 1 && (q[3] >> 63) == 0 && !generic) {
    r.route = NttRoute::Fast256;
  } else if (logN >= kMinTiledP && logN <= 2 * ntt_pmax(L)) {
    r.route = NttRoute::Tiled;
  } else {
    return r;
  }
  const int half = logN / 2 < kMinTiledP ? kMinTiledP : logN / 2;
  ntt_set_passes(r, logN, logN <= ntt_pmax(L) ? logN : half);
  return r;
}

// ---- the long wide route: ntt_wide_pass in up to three passes, 2^17 <= N <= 2^24 ----
// Buckler's evaluator and encoder run at embRank = 4 rank under any infinity-norm constraint with
// bound >= 1 (w w w - w has maxRank 3 rank + 1), so the reference's LogN = 15 benchmark
// transforms at 2^17.  ntt_route() above keeps its answer there (Stages, no passes: its pass list
// holds two); finalize() asks ntt_wide_long() for every L = 7, 14 plan and, where it gives
// passes, runs the direction on ntt_wide_pass over them instead.
constexpr int kWidePassStages = 8;  // most stages of one ntt_wide_pass launch (a 256-point tile)
constexpr int kWideLongMin = 17, kWideLongMax = 24;
constexpr int kWideForcedMin = 3;   // the w3 switch: three passes need three stages

struct WidePasses {
  int npasses;  // 0: no long route for this plan and direction
  PassDesc passes[3];  // forward order, contiguous from G0 = 0
};

// logN stages in n passes, as evenly as possible, larger passes first
inline WidePasses ntt_wide_split(int logN, int n) {
  WidePasses w = {n, {{0, 0}, {0, 0}, {0, 0}}};
  for (int k = 0, g0 = 0; k < n; ++k) {
    const int P = logN / n + (k < logN % n ? 1 : 0);
    w.passes[k] = {g0, P};
    g0 += P;
  }
  return w;
}

// Same arguments as ntt_route().  L = 7, 14 with 17 <= logN <= 24, the top bit of q clear, not
// (inverse and rank_inv != N^-1: the inverse scales by halving every stage) and a switch that
// does not start with s: ceil(logN / 8) passes (always three here: 17 -> 6, 6, 5; 20 -> 7, 7, 6;
// 24 -> 8, 8, 8).  Three passes of <= 8 and not two of 9: the transform is bound by the
// multiplier, a third HBM round trip costs a few percent, a 512-point L = 14 tile doubles the LDS
// per workgroup.  The switch w3 (experiments build) forces three even passes onto any
// 3 <= logN <= 24 under the same conditions, so the middle pass runs at sizes a test can afford.
inline WidePasses ntt_wide_long(int L, const uint64_t* q, int logN, bool inv, bool halving, const char* sw) {
  const WidePasses none = {0, {{0, 0}, {0, 0}, {0, 0}}};
  if (L != 7 && L != 14) return none;
  const bool per_stage = sw && sw[0] == 's', forced = sw && sw[0] == 'w' && sw[1] == '3';
  if ((q[L - 1] >> 63) != 0 || (inv && !halving) || per_stage) return none;
  if (forced && logN >= kWideForcedMin && logN <= kWideLongMax) return ntt_wide_split(logN, 3);
  if (logN < kWideLongMin || logN > kWideLongMax) return none;
  return ntt_wide_split(logN, (logN + kWidePassStages - 1) / kWidePassStages);
}

// ---- the long Fast256 route: ntt256_pass over 2^16-point blocks plus one register pass ----
// The 4-limb q = 1 mod 2^64, q < 2^255 plans (q255, zp220) at N = 2^(16 + M), M = 1, 2, 3: Buckler's
// embedding rank of a LogN = 15 / 16 circuit.  ntt_route() keeps its answer there (Tiled, two
// passes); finalize() asks ntt_fast256_long() for each direction and, where it says yes, runs the
// direction as Fast256 in three passes (ntt_l4_fast.hip): forward a prefix of the first M stages
// with one 2^M-point sub-transform (element stride 2^16) per thread, then the COL and ROW passes
// of the 2^16 route over the batch 2^M contiguous blocks; inverse ROW, COL, then a suffix of the
// last M stages whose final stage is the fused one (w1n, exact division by 2^logN): hence not for
// an inverse whose rank_inv is not N^-1.  A switch that starts with r keeps Tiled, as at 2^16.
constexpr int kFast256LongMin = 17, kFast256LongMax = 19;
constexpr int kFast256BlockLog = 16;  // the bottom passes' block: the 2^16 route's polynomial

inline bool ntt_fast256_long(int L, const uint64_t* q, int logN, bool inv, bool halving, const char* sw) {
  if (L != 4 || q[0] != 1 || (q[3] >> 63) != 0) return false;
  if (logN < kFast256LongMin || logN > kFast256LongMax) return false;
  if (inv && !halving) return false;
  return !(sw && sw[0] == 'r');
}

// The twiddle indices of the decomposition, in the reference's table layout (stage g of the whole
// transform reads tw[2^g + i] for its block i, ntt.go:261-275); the kernels call these.
// Prefix / suffix stage g < M on element j < 2^M of a sub-transform: the butterfly pairs j with
// j + 2^(M-1-g), and element j lies in block j >> (M - g) of the stage.
constexpr uint32_t ntt_long_prefix_tw(int M, int g, uint32_t j) { return (1u << g) + (j >> (M - g)); }
// Bottom passes: stage gl of a 2^16 block is stage M + gl of the transform, and block i of the
// block's own stage is block (B << gl) + i there, B the block's index in its polynomial:
// tw[2^(M+gl) + (B << gl) + i] = tw[idx16 + ((2^M - 1 + B) << gl)] for idx16 = 2^gl + i, the index the
// 2^16 route reads.  ntt_long_block_off() is the per-workgroup constant (0 for M = 0, B = 0).
constexpr uint32_t ntt_long_block_off(int M, uint32_t B) { return (1u << M) - 1u + B; }
constexpr uint32_t ntt_long_block_tw(uint32_t idx16, uint32_t boff, int gl) { return idx16 + (boff << gl); }

}  // namespace rg
