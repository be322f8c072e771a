// ntt_wide_tile.hpp -- index algebra of the wide pass tiles (ntt_wide.hpp ntt_wide_pass), HIP-free
// and <stdint.h> only, shared by the kernel, by its runner (ntt_lwide.hip) and by the host replay
// of tests/test_ntt_wide_long_host.py: how many sub-transforms a workgroup takes, how many
// workgroups a pass needs, which element of the batch a tile point is, in which order a tile is
// loaded, and which table entry a butterfly reads.
//
// A pass covers the P <= 8 global stages [G0, G0 + P) of a 2^logN-point transform; logS =
// logN - G0 - P stages follow it.  It splits every polynomial into 2^(logN - P) sub-transforms of
// 2^P points at stride 2^logS: sub-transform r = (hi, lo), hi = r >> logS < 2^G0 the block the
// earlier passes left it in, lo < 2^logS its offset inside the stride; point x is element
// hi 2^(logN - G0) + x 2^logS + lo.  Sub-transforms are numbered over the batch, s = b 2^(logN - P) + r.
// The first pass of a plan (COL, G0 = 0), its last (ROW, logS = 0) and, on the long route, the one
// between them (G0 > 0 and logS > 0) are the same code at three positions.
#pragma once
#include <stdint.h>

namespace rg {

constexpr int kWideMaxP = 8;          // most stages in one pass: a tile is at most 256 points
constexpr int kWideTilePoints = 256;  // 14 / 28 KiB of LDS at L = 7 / 14: LDS does not cap occupancy below the VGPRs
constexpr long long kWideMaxGrid = 0x7fffffffLL;  // workgroups of one launch

// sub-transforms per workgroup: a 256-point tile, inside one stride (2^logS consecutive lo share
// hi, so a tile's sub-transforms are neighbours in memory and never straddle two polynomials;
// at logS = 0 they are consecutive rows and the last tile may end past the batch)
constexpr int wide_cpt(int P, int logS) {
  int cpt = kWideTilePoints >> P;
  if (cpt < 1) cpt = 1;
  if (logS > 0 && cpt > (1 << logS)) cpt = 1 << logS;
  return cpt;
}

// workgroups of a pass over `batch` polynomials, or -1 when a launch cannot take them
constexpr long long wide_grid(unsigned long long batch, int logN, int P, int cpt) {
  const unsigned long long most = (unsigned long long)kWideMaxGrid * (unsigned long long)cpt;  // sub-transforms
  if (batch > (most >> (logN - P))) return -1;
  const long long nsub = (long long)(batch << (logN - P));
  return (nsub + cpt - 1) / cpt;
}

// global element index of point x of sub-transform s, or -1 past the batch's nsub sub-transforms
constexpr long long wide_elem(long long s, long long nsub, int logN, int G0, int P, int logS, int x) {
  if (s >= nsub) return -1;
  const int subs_log = logN - P;
  const long long b = s >> subs_log, r = s & ((1LL << subs_log) - 1);
  const long long hi = r >> logS, lo = r & ((1LL << logS) - 1);
  return (b << logN) | (hi << (logN - G0)) | ((long long)x << logS) | lo;
}

// tile load / store order: flat point e < cpt 2^P of the tile -> sub-transform c and point x, so
// that consecutive lanes touch consecutive memory (logS = 0, rows: c, x; else columns: x, c)
constexpr int wide_load_c(int P, int logS, int cpt, int e) { return logS == 0 ? e / (1 << P) : e % cpt; }
constexpr int wide_load_x(int P, int logS, int cpt, int e) { return logS == 0 ? e % (1 << P) : e / cpt; }

// local stage g < P (global G0 + g) combines bit P - 1 - g of x: the low point of butterfly
// p < 2^(P - 1); its partner is x0 | 2^(P - 1 - g)
constexpr int wide_bfly_x0(int P, int g, int p) {
  const int bitpos = P - 1 - g;
  return ((p >> bitpos) << (bitpos + 1)) | (p & ((1 << bitpos) - 1));
}

// table entry of that butterfly in sub-transform s: the reference's tw[m + i] (ntt.go:98-115
// forward, :357-466 inverse), m = 2^(G0 + g), i = the block of 2^(logN - G0 - g) elements it is in
constexpr long long wide_tw_idx(long long s, int logN, int G0, int P, int logS, int g, int x0) {
  const int bitpos = P - 1 - g;
  const long long r = s & ((1LL << (logN - P)) - 1);
  const long long hi = (r >> logS) & ((1LL << G0) - 1);
  return (1LL << (G0 + g)) + (hi << g) + (x0 >> (bitpos + 1));
}

}  // namespace rg
