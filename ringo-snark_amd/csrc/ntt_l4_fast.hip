// ntt_l4_fast.hip -- the Fast256 route's runner: the 4-limb degree-2^16 / 2^15 kernels (ntt256.hpp)
// and their three-pass form at 2^17 .. 2^19, for q = 1 mod 2^64, q < 2^255 (the Jindo default prime
// q255, Buckler's zp220).  ntt_route.hpp decides which plans
// come here, and only those own a helper stream; this unit derives Ntt256Args from the modulus and
// splits the batch over the two streams.
#include "ntt256.hpp"
#include "ntt_plan.hpp"

namespace rg {

template <bool INV, bool COL, bool SCALE, bool CANON, int LOGN>
static rg_status launch256(const Ntt256Args& a, size_t polys, hipStream_t st) {
  const unsigned grid = (unsigned)(polys << (LOGN - 10));  // 1024 points (32 KiB) per workgroup
  if (LOGN == 16 && measure_probe() == 5) {  // bench.py's L = 4 compute floor (experiments build)
    if (!COL && polys % 4 == 0)
      hipLaunchKernelGGL((ntt256_pass<INV, COL, SCALE, CANON, true, LOGN, 1>), dim3(grid), dim3(128), 0, st, a);
    else
      hipLaunchKernelGGL((ntt256_pass<INV, COL, SCALE, CANON, false, LOGN, 1>), dim3(grid), dim3(128), 0, st, a);
    return check_launch("ntt256_pass (probe)");
  }
  if (!COL && polys % 4 == 0)
    hipLaunchKernelGGL((ntt256_pass<INV, COL, SCALE, CANON, true, LOGN>), dim3(grid), dim3(128), 0, st, a);
  else
    hipLaunchKernelGGL((ntt256_pass<INV, COL, SCALE, CANON, false, LOGN>), dim3(grid), dim3(128), 0, st, a);
  return check_launch("ntt256_pass");
}

template <int LOGN>
static rg_status run_passes(Ntt256Args a, const NttLaunch& p, size_t polys, hipStream_t st) {
  if (!p.inv) {
    RG_TRY((launch256<false, true, false, false, LOGN>(a, polys, st)));
    a.in = a.out;
    RG_TRY((launch256<false, false, false, true, LOGN>(a, polys, st)));
  } else {
    RG_TRY((launch256<true, false, false, false, LOGN>(a, polys, st)));
    a.in = a.out;
    RG_TRY((launch256<true, true, true, true, LOGN>(a, polys, st)));
  }
  return RG_OK;
}

// first(st) on the caller's stream and second(x->s) on the helper stream, forked from and joined
// back to the caller's stream
template <class F0, class F1>
static rg_status fork_join(Aux* x, hipStream_t st, F0 first, F1 second) {
  std::lock_guard<std::mutex> lk(x->mu);
  RG_HIP(hipEventRecord(x->fork, st));
  RG_HIP(hipStreamWaitEvent(x->s, x->fork, 0));
  rg_status s = first(st);
  if (s == RG_OK) s = second(x->s);
  // joined on every path, so the caller's stream orders whatever was queued on the helper
  const hipError_t j[2] = {hipEventRecord(x->join, x->s), hipStreamWaitEvent(st, x->join, 0)};
  for (hipError_t e : j)
    if (e != hipSuccess && s == RG_OK) {
      set_last_error(std::string("ntt256: joining the helper stream: ") + hipGetErrorString(e));
      s = RG_ERR_DEVICE;
    }
  return s;
}

// The batch as two halves, the first on the caller's stream and the second on the plan's helper
// stream: each pass is ~2.7 rounds of workgroups (3 per SIMD resident), and the halves' passes
// fill each other's last round (configs[3] fwd+inv: 182.5 -> 187.3 K NTT/s; four quarters
// alternating measured 160 K, the headline ntt16_pass split lost 1.5%: profiles/r06r_ntt_split.txt)
template <int LOGN>
static rg_status run_split(Ntt256Args a, const NttLaunch& p, hipStream_t st) {
  Aux* x = p.aux;
  if (!x || p.batch < 8 || measure_probe() == 5) return run_passes<LOGN>(a, p, p.batch, st);
  const size_t N = (size_t)1 << LOGN;
  const size_t h = (p.batch / 2 + 3) & ~(size_t)3;  // the ROW passes' RP tiles take 4 polys
  Ntt256Args b = a;
  a.total_sub = (long long)(h * (N >> 8));
  b.total_sub = (long long)((p.batch - h) * (N >> 8));
  b.in += h * N * 4;
  b.out += h * N * 4;
  return fork_join(
      x, st, [&](hipStream_t s0) { return run_passes<LOGN>(a, p, h, s0); },
      [&](hipStream_t s1) { return run_passes<LOGN>(b, p, p.batch - h, s1); });
}

// ---- N = 2^(16 + M), M = 1, 2, 3: the long route (ntt_route.hpp ntt_fast256_long) ----
template <bool INV, bool COL, bool CANON, int LOGN>
static rg_status launch_long(const Ntt256Args& a, size_t blocks, hipStream_t st) {
  hipLaunchKernelGGL((ntt256_pass<INV, COL, false, CANON, false, LOGN>), dim3((unsigned)(blocks << 6)), dim3(128), 0, st, a);
  return check_launch("ntt256_pass (long)");
}

// the two 8-stage passes over `blocks` 2^16 blocks from a.in (a.blk0 the first one's index)
template <int LOGN>
static rg_status run_blocks(Ntt256Args a, bool inv, size_t blocks, hipStream_t st) {
  if (!inv) {
    RG_TRY((launch_long<false, true, false, LOGN>(a, blocks, st)));
    a.in = a.out;
    RG_TRY((launch_long<false, false, true, LOGN>(a, blocks, st)));
  } else {
    RG_TRY((launch_long<true, false, false, LOGN>(a, blocks, st)));
    a.in = a.out;
    RG_TRY((launch_long<true, true, false, LOGN>(a, blocks, st)));
  }
  return RG_OK;
}

template <bool INV>
static rg_status launch_edge(const Ntt256Args& a, int M, size_t batch, hipStream_t st) {
  const dim3 grid((unsigned)(batch << 8)), wg(256);  // a thread per offset: 2^16 / 256 workgroups per polynomial
  switch (M) {
    case 1: hipLaunchKernelGGL((ntt256_edge_pass<1, INV>), grid, wg, 0, st, a); break;
    case 2: hipLaunchKernelGGL((ntt256_edge_pass<2, INV>), grid, wg, 0, st, a); break;
    case 3: hipLaunchKernelGGL((ntt256_edge_pass<3, INV>), grid, wg, 0, st, a); break;
    default: return RG_ERR_INVALID;
  }
  return check_launch("ntt256_edge_pass");
}

// Forward: the prefix on the caller's stream, then the blocks; inverse: the blocks, then the suffix.
// The blocks as two halves on the two streams from 8 blocks up (one 2^19 polynomial already):
// a half need not end on a polynomial, the second carries its first block's index.
template <int LOGN>
static rg_status run_long(Ntt256Args a, const NttLaunch& p, hipStream_t st) {
  constexpr int M = LOGN - kFast256BlockLog;
  const size_t nb = p.batch << M;
  if (nb > ((size_t)1 << 24)) {  // grids of nb 2^6 and batch 2^8 workgroups
    set_last_error("ntt256: the long route takes at most 2^24 blocks of 2^16 points");
    return RG_ERR_INVALID;
  }
  Ntt256Args e = a;  // the prefix / suffix pass
  e.total_sub = (long long)(p.batch << 16);
  if (!p.inv) {
    RG_TRY(launch_edge<false>(e, M, p.batch, st));
    a.in = a.out;
  }
  rg_status s;
  Aux* x = p.aux;
  if (!x || nb < 8) {
    s = run_blocks<LOGN>(a, p.inv, nb, st);
  } else {
    const size_t h = (nb + 1) / 2;
    Ntt256Args b = a;
    b.in += h << (kFast256BlockLog + 2);
    b.out += h << (kFast256BlockLog + 2);
    b.blk0 = (uint32_t)h;
    s = fork_join(
        x, st, [&](hipStream_t s0) { return run_blocks<LOGN>(a, p.inv, h, s0); },
        [&](hipStream_t s1) { return run_blocks<LOGN>(b, p.inv, nb - h, s1); });
  }
  if (s != RG_OK || !p.inv) return s;
  e.in = e.out;
  return launch_edge<true>(e, M, p.batch, st);
}

// N = 2^16 (passes 8 + 8), N = 2^15 (7 + 8: the Buckler witness rank of the bench) and
// N = 2^17 .. 2^19 (M + 8 + 8: Buckler's embedding rank of a LogN = 15 / 16 circuit)
rg_status ntt256_run(const NttLaunch& p, hipStream_t st) {
  const size_t N = (size_t)1 << p.logN;
  Ntt256Args a{};
  a.tw = p.tw;
  uint32_t c = 0;
  for (int i = 0; i < 4; ++i) {
    a.q[2 * i] = (uint32_t)p.q[i];
    a.q[2 * i + 1] = (uint32_t)(p.q[i] >> 32);
    a.w1n[2 * i] = (uint32_t)p.w1n[i];
    a.w1n[2 * i + 1] = (uint32_t)(p.w1n[i] >> 32);
  }
  for (int i = 0; i < 8; ++i) {
    const uint64_t v = 2ull * a.q[i] + c;
    a.q2[i] = (uint32_t)v;
    c = (uint32_t)(v >> 32);
  }
  a.total_sub = (long long)(p.batch * (N >> 8));
  a.in = p.in;
  a.out = p.out;
  switch (p.logN) {
    case 15: return run_split<15>(a, p, st);
    case 16: return run_split<16>(a, p, st);
    case 17: return run_long<17>(a, p, st);
    case 18: return run_long<18>(a, p, st);
    case 19: return run_long<19>(a, p, st);
    default: return RG_ERR_INVALID;  // ntt_route.hpp sends no other rank here
  }
}

}  // namespace rg
