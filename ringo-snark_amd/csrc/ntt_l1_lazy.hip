// ntt_l1_lazy.hip -- the Lazy64 route's runner: the lazy single-word pass kernels (ntt64.hpp) on
// N = 2^16 as two 8-stage passes, q < 2^63 with q mod 2^32 == 1 (the config-2 jindo-modulus prime
// 47104^4 + 1 and every other p - 1 = b^(2^e) with b even).  ntt_route.hpp decides which plans come
// here and which take the Montgomery variant (p.mont: the MONT instantiations, the Montgomery
// twiddle product on single-word tables; the others keep Shoup's product); this unit derives
// Ntt64Args from the modulus and launches the two passes per chunk.
#include "ntt64.hpp"
#include "ntt_plan.hpp"

namespace rg {

// ROW passes tile the same row of 16 polynomials when the chunk allows it (RP, twiddles
// shared by the whole tile); otherwise 16 consecutive rows of one polynomial.  tile16: the plan's
// choice (NttLaunch::tile16) for the two MONT passes that have a 16-point tile, ROW forward on RP
// tiles and COL inverse: 256 threads and at most 128 VGPRs, so that four workgroups share a CU as
// they do on 8 points
template <bool MONT, bool INV, bool COL, bool SCALE, bool CANON>
static rg_status launch64m(const Ntt64Args& a, size_t polys, bool tile16, hipStream_t st) {
  const long long tiles = a.total_sub / 16;
  const bool rp = !COL && polys % 16 == 0;
  const bool probe = measure_probe() == 4;  // bench.py's compute floor (rg_set_probe, experiments build): no HBM data movement
  if constexpr (MONT && INV == COL) {
    if (tile16 && (COL || rp)) {
      if (probe)
        hipLaunchKernelGGL((ntt16_pass<true, INV, COL, SCALE, CANON, !COL, 4, 16, 4>), dim3((unsigned)tiles), dim3(256), 0, st, a);
      else
        hipLaunchKernelGGL((ntt16_pass<true, INV, COL, SCALE, CANON, !COL, 4, 16>), dim3((unsigned)tiles), dim3(256), 0, st, a);
      return check_launch(probe ? "ntt16_pass (16 points, probe)" : "ntt16_pass (16 points)");
    }
  }
  if (probe) {
    if (rp)
      hipLaunchKernelGGL((ntt16_pass<MONT, INV, COL, SCALE, CANON, true, 1, 8, 4>), dim3((unsigned)tiles), dim3(512), 0, st, a);
    else
      hipLaunchKernelGGL((ntt16_pass<MONT, INV, COL, SCALE, CANON, false, 1, 8, 4>), dim3((unsigned)tiles), dim3(512), 0, st, a);
    return check_launch("ntt16_pass (probe)");
  }
  if (rp)
    hipLaunchKernelGGL((ntt16_pass<MONT, INV, COL, SCALE, CANON, true>), dim3((unsigned)tiles), dim3(512), 0, st, a);
  else
    hipLaunchKernelGGL((ntt16_pass<MONT, INV, COL, SCALE, CANON, false>), dim3((unsigned)tiles), dim3(512), 0, st, a);
  return check_launch("ntt16_pass");
}

template <bool INV, bool COL, bool SCALE, bool CANON>
static rg_status launch64(const Ntt64Args& a, const NttLaunch& p, size_t polys, hipStream_t st) {
  return p.mont ? launch64m<true, INV, COL, SCALE, CANON>(a, polys, p.tile16, st)
                : launch64m<false, INV, COL, SCALE, CANON>(a, polys, false, st);
}

rg_status ntt64_run(const NttLaunch& p, hipStream_t st) {
  const uint64_t q = p.q[0];
  const size_t N = (size_t)1 << p.logN;
  Ntt64Args a{};
  a.tw = p.tw;
  a.q = q;
  a.q2 = 2 * q;
  a.nqhi = 0u - (uint32_t)(q >> 32);
  a.q1 = (uint32_t)(q >> 32);
  a.ninv = p.nsc[0];
  a.ninv_p = p.nsc_sh;
  a.w1n = p.w1n[0];
  a.w1n_p = p.w1n_sh;
  a.logN = p.logN;
  for (size_t b0 = 0; b0 < p.batch; b0 += p.chunk_polys) {
    const size_t nb = std::min(p.chunk_polys, p.batch - b0);
    a.total_sub = (long long)(nb * (N >> 8));
    a.in = p.in + b0 * N;
    a.out = p.out + b0 * N;
    a.rev = 0;
    if (!p.inv) {
      a.G0 = 0;
      RG_TRY((launch64<false, true, false, false>(a, p, nb, st)));
      a.in = a.out;
      a.G0 = 8;
      a.rev = 1;  // reverse tile order: reads what the first pass wrote last first (ntt64.hpp)
      RG_TRY((launch64<false, false, false, true>(a, p, nb, st)));
    } else {
      a.G0 = 8;
      RG_TRY((launch64<true, false, false, false>(a, p, nb, st)));
      a.in = a.out;
      a.G0 = 0;
      a.rev = 1;  // reverse tile order: reads what the first pass wrote last first (ntt64.hpp)
      RG_TRY((launch64<true, true, true, true>(a, p, nb, st)));
    }
  }
  return RG_OK;
}

}  // namespace rg
