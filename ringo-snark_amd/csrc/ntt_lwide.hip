// ntt_lwide.hip -- wide buckler fields (zp440: 7 limbs, zp880: 14 limbs): the Wide route's runner
// (the LDS-tiled pass kernel of ntt_wide.hpp over the plan's passes: one pass for N <= 2^8, COL
// then ROW up to 2^16, three passes on the long route up to 2^24) and the Stages route's per-stage
// kernels of ntt_kernels.hpp.  ntt_route.hpp decides per direction which of the two a plan takes
// and in which passes; this unit derives WideArgs from the modulus.
#include "ntt_kernels.hpp"
#include "ntt_wide.hpp"

namespace rg {

template <int L>
static rg_status wide_run(const NttLaunch& p, hipStream_t st) {
  if (p.route != NttRoute::Wide) return run_stages<L, false>(p, st);
  const int logN = p.logN, np = p.wide.npasses;
  // every pass's grid, before anything is launched: `grid` goes to the launch as an unsigned
  long long grids[3];
  for (int k = 0; k < np; ++k) {
    const PassDesc& ps = p.wide.passes[k];
    grids[k] = wide_grid(p.batch, logN, ps.P, wide_cpt(ps.P, logN - ps.G0 - ps.P));
    if (grids[k] < 0) {
      set_last_error("rg_ntt: batch " + std::to_string(p.batch) + " at rank 2^" + std::to_string(logN) + " needs more than " +
                     std::to_string(kWideMaxGrid) + " workgroups in the pass of " + std::to_string(ps.P) +
                     " stages: split the batch");
      return RG_ERR_INVALID;
    }
  }
  WideArgs a;
  memset(&a, 0, sizeof(a));
  a.tw = p.tw;  // inverse: twInv[i] / 2 (ntt.hip upload_wide)
  for (int l = 0; l < L; ++l) {
    a.q[2 * l] = (uint32_t)p.q[l];
    a.q[2 * l + 1] = (uint32_t)(p.q[l] >> 32);
  }
  a.qinv28 = (uint32_t)p.qinv & 0x0FFFFFFFu;  // -q^-1 mod 2^64, so its low 28 bits are -q^-1 mod 2^28
  for (int k = 0; k < 64 * L / 28; ++k) {  // q in 28-bit digits
    const int bit = 28 * k, l = bit >> 6, sh = bit & 63;
    uint64_t v = p.q[l] >> sh;
    if (sh > 36 && l + 1 < L) v |= p.q[l + 1] << (64 - sh);
    a.q28[k] = (uint32_t)v & 0x0FFFFFFFu;
  }
  a.logN = logN;
  for (int k = 0; k < np; ++k) {
    const int at = p.inv ? np - 1 - k : k;  // the inverse runs the passes backwards
    const PassDesc& ps = p.wide.passes[at];
    a.G0 = ps.G0;
    a.P = ps.P;
    a.logS = logN - a.G0 - a.P;
    a.cpt = wide_cpt(a.P, a.logS);  // one 256-point tile per workgroup, inside one row of columns
    a.nsub = (long long)p.batch << (logN - a.P);
    a.in = k == 0 ? p.in : p.out;
    a.out = p.out;
    const size_t lds = (size_t)a.cpt * ((size_t)1 << a.P) * L * 8;
    if (p.inv)
      hipLaunchKernelGGL((ntt_wide_pass<L, true>), dim3((unsigned)grids[at]), dim3(kWideThreads), lds, st, a);
    else
      hipLaunchKernelGGL((ntt_wide_pass<L, false>), dim3((unsigned)grids[at]), dim3(kWideThreads), lds, st, a);
    RG_TRY(check_launch("ntt_wide_pass"));
  }
  return RG_OK;
}

rg_status ntt_run_L7(const NttLaunch& p, hipStream_t st) { return wide_run<7>(p, st); }
rg_status ntt_run_L14(const NttLaunch& p, hipStream_t st) { return wide_run<14>(p, st); }
}  // namespace rg
