// jindo_sample.hip -- the randomness of Prover.Commit drawn on the device, and the sampled commit
// that schedules the samplers and the commit stages (jindo_commit.hip: digits_stage, prep_launch,
// commit_core; the stream scratch: jindo_setup.hip) as one DAG over three streams.  Section 6 of
// the pipeline overview at the top of jindo_commit.hip.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "ck_crs.hpp"
#include "csprng.hpp"
#include "csprng_host.hpp"
#include "jindo_impl.hpp"

namespace rg {

// ------------------------------------------------------------------------------------------
// 6. sampling: the randomness Prover.Commit draws (prover.go:65-139, encoder.go:149-183) on the
// device, from six sampler domains (csprng.hpp: one AES-256-CTR key per domain, a window of
// the domain's counter space per sampler instance):
//   kDomEncCdt    Encoder.twinCDT      one instance per encode polynomial (256 words)
//   kDomCosac     Encoder.cosac        one instance per group of kCosGroup samples (in order) ...
//   kDomCosacRnd  ... and its RoundedGaussianSampler, the same groups
//   kDomMlweCdt   Prover.mlweSampler   one instance per MLWE polynomial
//   kDomMlweRnd   Prover.roundedSampler one instance per sample
//   kDomUniform   crypto/rand (MustSetRandom), one instance per field element
// Instances are numbered from `first_commit`, the index of the batch's first commit in the
// prover's sequence, so batches and ranks never share keystream.
// ------------------------------------------------------------------------------------------
enum { kDomEncCdt = 0, kDomCosac, kDomCosacRnd, kDomMlweCdt, kDomMlweRnd, kDomUniform, kNumDom };
// COSAC samples per sampler-instance pair.  8, not 16 (round 4): a wave's 64 lanes then fill from
// 2 polynomials, so cosac2's queue hands out work in half the size and its end-of-launch tail halves
// (configs[2] 61.3 K -> 62.4 K commits/s with the stream DAG, profiles/r05h_dag_ab.txt)
constexpr int kCosGroup = 8;

struct SampleArgs {
  JShape s;
  IdxDiv d_half, d_nm, d_cols;  // mlwe_noise_kernel's index split (pairs < 2^32)
  AesKey key[kNumDom];
  const uint32_t* te0;
  unsigned long long first_commit;
  // encode noise
  const uint32_t* digits;  // [B][cols+1][rows][d]
  const double* delta;     // deltaInv[exp] (encoder.go:50-67)
  CdtDev cdt_enc, cdt_mlwe;
  ZigDev zig;
  double sd_ecd, sd_ecd_blind, sd_mask, sd_mask_blind, sd_mask_mlwe;
  long long* enc_noise;   // [B][cols+1][rows][d]
  long long* mlwe_noise;  // [B][cols+1][nm][d]
  long long n_enc_pairs, n_ml_pairs;
  long long batch;
  // cdt2_noise_kernel's tail bounds: [2][128][size + 2], lower then upper; row c, entry j + 1 bounds
  // the reference's tail cdf sum_{x = tailLo}^{j} rho(x - cFrac) / norm, j = -1 .. size, over
  // cFrac in [c, c + 1] / 128 (host, rg_jindo_set_stddevs)
  const double* cdt_sbound;
  const int* cdt_jmax;  // [128]: v0 <= jmax[c0] decides the sample as v0 (cdt2_noise_kernel)
  double cdt_band;      // relative width of the band around the bounds that goes to the exact sum: 2^-40
  int* wq;              // [0] cdt2_noise_kernel's chunk counter, [2..3] cosac2's job counter (zeroed)
};

#pragma clang fp contract(off)
// centre of coefficient k of one encode: -fpSample[k] (encoder.go:153-165), the deltaInv
// convolution of the digit polynomial, summed term by term in Go's order
__device__ __forceinline__ double enc_centre(const SampleArgs& a, const uint32_t* dg, int k) {
  const JShape& S = a.s;
  double fp = 0.0;
  for (int i = 0; i < S.exp; ++i) {
    const double di = a.delta[i];
    if (di == 0.0) continue;
    const int dd = S.d - (i + 1) * S.slots;
    if (k >= dd)
      fp = fp + di * (double)dg[k - dd];
    else
      fp = fp - di * (double)dg[k + S.d - dd];
  }
  return -fp;
}
#pragma clang fp contract(on)

// ---- d = 256 encode noise, split by sampler -----------------------------------------------
// One kernel per sampler, so a wave never waits on the other sampler's slow path:
//   cdt2_noise_kernel   wave per TwinCDT polynomial, 4 coefficients per lane (2 AES blocks);
//                       digits staged in LDS for the deltaInv centres; one guide-table lookup
//                       per sample; tails decided inline;
//   cosac2_noise_kernel COSAC groups as a work queue through one state machine.
// The sampling entry points refuse shapes these kernels do not cover (d != 256, slots % 4 != 0,
// TwinCDT tables above kCdtLdsMaxSize entries: fields with exp >= 128, or caller stddevs far above
// NewParameters').  The round-2 kernels that covered them (enc_noise_kernel, cdt_noise_kernel +
// cdt_tail_kernel) are tools/experiments/legacy_samplers.patch.
#pragma clang fp contract(off)
constexpr int kCdtLdsMaxSize = 96;  // tables' high words + guide in LDS when size <= 96 (<= 145 KiB
                                    // per workgroup with the 64 KiB AES table; the waves' digit slots
                                    // take the rest: cdt2_waves)
constexpr int kCdtChunk = 8;        // consecutive polynomials per chunk (queue granularity; 32 / 16 / 8 A/B: profiles/r04q_queue_chunks_ab.txt)

__device__ __forceinline__ double rl_f64(double x, int lane) {
  const uint64_t b = __double_as_longlong(x);
  const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)b, lane);
  const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), lane);
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// lower_bound of u in one table: the high words from LDS, the full word from global on a tie;
// found -> index - 1 (slices.BinarySearch, twin_cdt.go:86-93)
__device__ __forceinline__ int cdt_search_hi(const uint32_t* hi, const uint64_t* full, int n, uint64_t u) {
  const uint32_t uh = (uint32_t)(u >> 32);
  int lo = 0, len = n;
  while (len > 0) {
    const int half = len >> 1, mid = lo + half;
    const uint32_t th = hi[mid];
    const bool less = th != uh ? th < uh : full[mid] < u;
    if (less) {
      lo = mid + 1;
      len -= half + 1;
    } else {
      len = half;
    }
  }
  const bool eq = lo < n && hi[lo] == uh && full[lo] == u;
  return eq ? lo - 1 : lo;
}

// dynamic LDS of cdt2_noise_kernel: high words [128][size] u32, guide [128][257] u8, key, then
// the waves' digit slots and jmax
__host__ __device__ constexpr int cdt_guide_off(int size) { return 128 * size * 4; }
__host__ __device__ constexpr int cdt_key_off(int size) { return cdt_guide_off(size) + ((128 * 257 + 3) & ~3); }

// ---- cdt2: TwinCDT for every encode polynomial, tails decided inline ----------------------
// Each wave owns a contiguous range of the batch's (commit, column, row) polynomials: TwinCDT
// polynomials are sampled; COSAC ones get their deltaInv centres (as doubles, in enc_noise)
// for cosac2_noise_kernel; skipped ones are zeroed.
// The round-2 form (cdt_noise_kernel) spent its time on (profiling variants) the deltaInv centres,
// 16 dependent global loads per polynomial, and eight table searches per lane; its v0 != v1
// tails go to a second kernel that sums up to 2 tailHi + 1 exp terms each.  Here:
//  * the polynomial's 256 digits are staged in a wave-private 1 KiB LDS slot (one 16-B store per
//    lane), the next polynomial's digits already in flight, and the 16 shifted digit quadruples a
//    lane needs are 16 independent ds_read_b128;
//  * one search per sample (table c0: guide by top byte, bisection on the high words); table c1
//    gives the same lower bound unless u lies between the two tables' entries around it (two
//    word compares; ~0.1% of samples search c1 in full);
//  * a v0 != v1 tail compares p = u / 2^64 with the reference's cdf = sum_{x <= v0} rho(x - cFrac)
//    / norm through bounds: cFrac lies in [c0, c0 + 1] / 128, and the host bounds that sum over the
//    interval from its values at the two ends (summed in the same order; rg_jindo_set_stddevs), so
//    lo[c0][v0] (1 - 2^-40) <= cdf <= hi[c0][v0] (1 + 2^-40) (2^-40 covers both libms and the float
//    sums).  Outside that band the comparison is decided; inside it (p ~ 1, unseen at NewParameters'
//    widths; a few tails in a hundred at widths below 0.5) the wave sums the terms in the
//    reference's order.  Results equal the reference's draw for draw.
// deltaInv centres of coefficients 4 lane + h (encoder.go:153-165, Go's summation order) from the
// polynomial's 256 digits in the wave's LDS slot dl: coefficient k reads digit (k + (i+1) slots)
// mod 256, added when that index wrapped; fp = the negated centres.  Leading zero deltas (12 of 16
// at the configs' shapes: b^i / p underflows the double grid) are skipped (i0); later zeros are
// added: fp starts at +0 and never becomes -0, so adding 0 * g changes nothing, and four digits'
// loads are in flight at once.  One definition for both kernels that need centres, so TwinCDT
// and COSAC polynomials see the same arithmetic (fp contract off).
typedef const __attribute__((address_space(4))) double* dconst_ptr;
__device__ __forceinline__ void enc_centres(const uint4* dl, int lane, const JShape& S, dconst_ptr dlt, int i0,
                                            double (&fp)[4]) {
  fp[0] = fp[1] = fp[2] = fp[3] = 0.0;
  auto cstep = [&](double di, int i, const uint4& q) {
    // slots % 4 == 0 (the launch condition) makes base a multiple of 4: base + h >= 256 for
    // all four coefficients or for none, so one sign per digit; fp + (-di) g == fp - di g
    const double sdi = 4 * lane + (i + 1) * S.slots >= 256 ? di : -di;
    fp[0] = fp[0] + sdi * (double)q.x;
    fp[1] = fp[1] + sdi * (double)q.y;
    fp[2] = fp[2] + sdi * (double)q.z;
    fp[3] = fp[3] + sdi * (double)q.w;
  };
  auto dslot = [&](int i) { return dl[((4 * lane + (i + 1) * S.slots) & 255) >> 2]; };
  int i = i0;
  for (; i + 4 <= S.exp; i += 4) {
    const uint4 q0 = dslot(i), q1 = dslot(i + 1), q2 = dslot(i + 2), q3 = dslot(i + 3);
    const double d0 = dlt[i], d1 = dlt[i + 1], d2 = dlt[i + 2], d3 = dlt[i + 3];
    cstep(d0, i, q0);
    cstep(d1, i + 1, q1);
    cstep(d2, i + 2, q2);
    cstep(d3, i + 3, q3);
  }
  for (; i < S.exp; ++i) cstep(dlt[i], i, dslot(i));
}

// The COSAC polynomials' centres (row 0 of the data columns, every row of the mask column: the
// stddevs other than ecdStdDev, prover.go:93-123), written as doubles into enc_noise for
// cosac2_noise_kernel: one wave per polynomial, jobs in cosac2's order.  A launch of its own
// (not part of cdt2_noise_kernel) so that the TwinCDT and COSAC samplers are independent and
// can run on two streams, each filling the other's tail.
constexpr int kCentreWaves = 4;
__global__ __launch_bounds__(64 * kCentreWaves) void cos_centre_kernel(SampleArgs a) {
  __shared__ uint4 dls[kCentreWaves][64];
  const int wl = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const JShape& S = a.s;
  const int per = S.cols + S.rows;
  const long long job = (long long)blockIdx.x * kCentreWaves + wl;
  if (job >= a.batch * per) return;
  const long long b = job / per;
  const int j = (int)(job % per);
  const int col = j < S.cols ? j : S.cols, row = j < S.cols ? 0 : j - S.cols;
  const double sd = col == S.cols ? (row == 0 ? a.sd_mask_blind : a.sd_mask) : (row == 0 ? a.sd_ecd_blind : a.sd_ecd);
  if (enc_skipped(S, col, row) || sd == a.sd_ecd) return;  // cdt2_noise_kernel's polynomials
  const long long poly = (b * (S.cols + 1) + col) * S.rows + row;
  const dconst_ptr dlt = (dconst_ptr)a.delta;
  int i0 = 0;
  while (i0 < S.exp && dlt[i0] == 0.0) ++i0;
  uint4* dl = dls[wl];
  dl[lane] = reinterpret_cast<const uint4*>(a.digits + poly * 256)[lane];
  wave_lds_fence();
  double fp[4];
  enc_centres(dl, lane, S, dlt, i0, fp);
  double2* out = reinterpret_cast<double2*>(a.enc_noise + poly * 256);
  out[2 * lane] = make_double2(-fp[0], -fp[1]);
  out[2 * lane + 1] = make_double2(-fp[2], -fp[3]);
}

constexpr int kCdt2Waves = 16;  // per workgroup; fewer where the tables leave no room for 16 digit slots
constexpr int kLdsBytes = 163840;
__host__ __device__ constexpr int cdt2_dig_off(int size) { return cdt_key_off(size) + kKeyWords * 4; }
__host__ __device__ constexpr int cdt2_jmax_off(int size, int waves) { return cdt2_dig_off(size) + waves * 1024; }
__host__ __device__ constexpr int cdt2_dyn_lds(int size, int waves) { return cdt2_jmax_off(size, waves) + 128 * 4; }
// the waves a workgroup runs at this table size: 16 up to 93 entries (NewParameters' tables have 89),
// 15 at 95 (the kernel's layout follows blockDim)
constexpr int cdt2_waves(int size) {
  int w = kCdt2Waves;
  while (w > 1 && cdt2_dyn_lds(size, w) + (int)sizeof(uint32_t) * kAesLds > kLdsBytes) --w;
  return w;
}
static_assert(cdt2_waves(89) == kCdt2Waves && cdt2_waves(kCdtLdsMaxSize) >= 14 &&
                  cdt2_dyn_lds(kCdtLdsMaxSize, cdt2_waves(kCdtLdsMaxSize)) + (int)sizeof(uint32_t) * kAesLds <= kLdsBytes,
              "every accepted table fits beside the AES table");

__global__ __launch_bounds__(64 * kCdt2Waves) void cdt2_noise_kernel(SampleArgs a) {
  __shared__ uint32_t lds[kAesLds];
  extern __shared__ uint32_t dyn[];
  const CdtDev& C = a.cdt_enc;
  const int n = C.size;
  uint32_t* thi = dyn;
  uint8_t* guide = reinterpret_cast<uint8_t*>(dyn) + cdt_guide_off(n);
  uint32_t* keyl = dyn + cdt_key_off(n) / 4;
  const int wl = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint4* dl = reinterpret_cast<uint4*>(reinterpret_cast<char*>(dyn) + cdt2_dig_off(n) + wl * 1024);
  int* jmax = reinterpret_cast<int*>(reinterpret_cast<char*>(dyn) + cdt2_jmax_off(n, (int)(blockDim.x >> 6)));
  aes_lds_fill(lds, a.te0);
  aes_key_fill(keyl, a.key[kDomEncCdt]);
  for (int i = threadIdx.x; i < 128 * n; i += blockDim.x) thi[i] = (uint32_t)(C.tables[i] >> 32);
  for (int i = threadIdx.x; i < 128 * 257; i += blockDim.x) guide[i] = C.guide[i];
  for (int i = threadIdx.x; i < 128; i += blockDim.x) jmax[i] = a.cdt_jmax[i];
  __syncthreads();
  const JShape& S = a.s;
  const long long npoly = a.batch * (S.cols + 1) * S.rows;
  const double norm = sqrt(2.0 * M_PI) * C.sigma;
  const double two_s2 = 2.0 * C.sigma * C.sigma;
  const LdsKey key{keyl};
  const int sstride = n + 2;
  // deltaInv through the constant address space: scalar loads (a plain global load waits on
  // vmcnt(0) per digit, as the kernel's stores defeat the no-clobber analysis)
  const dconst_ptr dlt = (dconst_ptr)a.delta;
  int i0 = 0;  // first nonzero deltaInv
  while (i0 < S.exp && dlt[i0] == 0.0) ++i0;
  // chunks from a counter: a wave that drew cheap polynomials (COSAC hand-offs, skipped ones)
  // takes more, so the workgroups -- one per CU, whose last wave holds its CU -- end together
  for (;;) {
    int ch = 0;
    if (lane == 0) ch = atomicAdd(a.wq, 1);
    const long long p0 = (long long)__builtin_amdgcn_readlane(ch, 0) * kCdtChunk;
    if (p0 >= npoly) break;
    const long long p1 = p0 + kCdtChunk < npoly ? p0 + kCdtChunk : npoly;
    int row = (int)(p0 % S.rows), col = (int)((p0 / S.rows) % (S.cols + 1));
    uint4 gnext = reinterpret_cast<const uint4*>(a.digits + p0 * 256)[lane];
    for (long long poly = p0; poly < p1; ++poly) {  // (b, col, row) flattened
      if (poly > p0 && ++row == S.rows) {
        row = 0;
        if (++col == S.cols + 1) col = 0;
      }
      const uint4 g = gnext;
      if (poly + 1 < p1) gnext = reinterpret_cast<const uint4*>(a.digits + (poly + 1) * 256)[lane];
      long long* out = a.enc_noise + poly * 256;
      if (enc_skipped(S, col, row)) {  // the reference draws nothing for these (prover.go:101-105,118-123)
        reinterpret_cast<longlong2*>(out)[2 * lane] = make_longlong2(0, 0);
        reinterpret_cast<longlong2*>(out)[2 * lane + 1] = make_longlong2(0, 0);
        continue;
      }
      const double sd =
          col == S.cols ? (row == 0 ? a.sd_mask_blind : a.sd_mask) : (row == 0 ? a.sd_ecd_blind : a.sd_ecd);
      if (sd != a.sd_ecd) continue;  // a COSAC polynomial: cos_centre_kernel writes its centres
      dl[lane] = g;
      wave_lds_fence();
      double fp[4];
      enc_centres(dl, lane, S, dlt, i0, fp);
      wave_lds_fence();  // the slot is rewritten for the next polynomial after these reads
      const unsigned long long gpoly =
          a.first_commit * (unsigned long long)(S.cols + 1) * S.rows + (unsigned long long)poly;
      uint64_t u[4];
      ks_words_x2(key, gpoly, (uint64_t)(2 * lane), (uint64_t)(2 * lane + 1), lds, u);
      // TwinCDTGaussianSampler.Sample (twin_cdt.go:77-111).  Fast path: the guide bucket of u's
      // top byte in table c0 holds <= 3 entries and none shares u's high word, so the lower bound
      // is lo + #(entries below u) with no equality (three LDS word compares); and v0 <= jmax[c0],
      // for which the reference returns v0 whatever v1 is: if v1 == v0 trivially, else because
      // p = u / 2^64 <= t_c0[v0 + 1] / 2^64 < (1 - 2^-40) lo[c0][v0] <= the cdf it compares
      // with (host-checked per table and index, rg_jindo_set_stddevs).  Other samples (a long
      // bucket, a high-word tie, an extreme v0) take the exact path below.
      int c0[4], v0[4];
      double cf[4], flo[4];
      uint32_t slow = 0;
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const double center = -fp[h];
        flo[h] = floor(center);
        cf[h] = center - flo[h];
        c0[h] = (int)((int64_t)floor(128.0 * cf[h]) % 128);
        const int t = (int)(u[h] >> 56);
        const int lo = guide[c0[h] * 257 + t];
        const int len = guide[c0[h] * 257 + t + 1] - lo;
        const uint32_t uh = (uint32_t)(u[h] >> 32);
        const uint32_t* th = thi + c0[h] * n + lo;
        int cnt = 0;
        bool tie = false;
#pragma unroll
        for (int k = 0; k < 3; ++k)
          if (k < len) {
            const uint32_t x = th[k];
            cnt += x < uh ? 1 : 0;
            tie |= x == uh;
          }
        v0[h] = lo + cnt;
        if (len > 3 || tie || v0[h] > jmax[c0[h]]) slow |= 1u << h;
      }
      int64_t res[4];
      uint32_t pend = 0;
#pragma unroll
      for (int h = 0; h < 4; ++h) res[h] = (int64_t)v0[h] + C.tail_lo + (int64_t)flo[h];
      if (__ballot(slow != 0)) {  // the exact path, literally (rare)
#pragma unroll
        for (int h = 0; h < 4; ++h)
          if ((slow >> h) & 1) {
            const int a0 = c0[h], a1 = (int)((int64_t)ceil(128.0 * cf[h]) % 128);
            const int w0 = cdt_search_hi(thi + a0 * n, C.tables + (long long)a0 * n, n, u[h]);
            const int w1 = a1 == a0 ? w0 : cdt_search_hi(thi + a1 * n, C.tables + (long long)a1 * n, n, u[h]);
            v0[h] = w0;
            res[h] = (int64_t)w1 + C.tail_lo + (int64_t)flo[h];
            if (w0 != w1) {  // the tail: p < cdf -> v0's value (twin_cdt.go:95-110)
              const double p = __ull2double_rn(u[h]) / 18446744073709551616.0;
              const double lo_b = a.cdt_sbound[a0 * sstride + w0 + 1] * (1.0 - a.cdt_band);
              const double hi_b = a.cdt_sbound[(128 + a0) * sstride + w0 + 1] * (1.0 + a.cdt_band);
              if (p < lo_b)
                res[h] = (int64_t)w0 + C.tail_lo + (int64_t)flo[h];
              else if (!(p >= hi_b))
                pend |= 1u << h;  // within the bounds' band: sum the terms below
            }
          }
      }
      for (;;) {  // the exact sums (p within ~1e-12 of the cdf), one sample at a time across the wave
        const uint64_t any = __ballot(pend != 0);
        if (!any) break;
        const int src = __builtin_amdgcn_readfirstlane(__builtin_ctzll(any));
        const int hs = __builtin_amdgcn_readlane(pend ? __builtin_ctz(pend) : 0, src);
        double c_frac = 0.0, p = 0.0;
        int vv = 0;
#pragma unroll
        for (int h = 0; h < 4; ++h)
          if (h == hs) {
            c_frac = cf[h];
            vv = v0[h];
            p = __ull2double_rn(u[h]) / 18446744073709551616.0;
          }
        c_frac = rl_f64(c_frac, src);
        vv = __builtin_amdgcn_readlane(vv, src);
        double cdf = 0.0;
        for (int64_t x0 = C.tail_lo; x0 <= vv; x0 += 64) {
          const double xf = (double)(x0 + lane);
          const double term = exp(-(xf - c_frac) * (xf - c_frac) / two_s2) / norm;
          const int nn = (int)std::min<int64_t>(64, (int64_t)vv - x0 + 1);
          for (int i = 0; i < nn; ++i) cdf += rl_f64(term, i);
        }
        if (lane == src) {
#pragma unroll
          for (int h = 0; h < 4; ++h)
            if (h == hs && p < cdf) res[h] = (int64_t)v0[h] + C.tail_lo + (int64_t)flo[h];
          pend &= pend - 1;
        }
      }
      reinterpret_cast<longlong2*>(out)[2 * lane] = make_longlong2(res[0], res[1]);
      reinterpret_cast<longlong2*>(out)[2 * lane + 1] = make_longlong2(res[2], res[3]);
    }
  }
}

// COSACSampler.Sample (gaussian_cosac.go:22-57) with its RoundedGaussianSampler's normFloat
// (gaussian_rounded.go:77-116) as a state machine in which every state consumes exactly one
// Sample() word, from the sampler's own instance (base) or the rounded sampler's (rnd):
enum { kCoStart = 0, kCoNorm, kCoTailU, kCoTailV, kCoWedge, kCoBit, kCoRR };
__device__ __forceinline__ int co_src(int st) { return (st >= kCoNorm && st <= kCoWedge) ? 1 : 0; }
__device__ __forceinline__ double float52(uint64_t w) { return (double)(w & 0xFFFFFFFFFFFFFull) * 2.220446049250313e-16; }

// ---- cosac2: COSAC samples through one state machine, one AES block per lane per step ------
// The COSAC samples of an encode polynomial come in groups of kCosGroup consecutive
// coefficients; group g of polynomial gpoly draws from instance gpoly * (d / kCosGroup) + g of
// both COSAC domains (the sampler's own UniformSampler and its RoundedGaussianSampler's), in
// coefficient order, each sample continuing the streams where the previous one stopped (as one
// Go COSACSampler would over those samples).  Per-sample instances (round 2) left the unused
// second word of each instance's last block behind: ~3.7 blocks per sample against ~3.0 here.
// Each wave's groups (its jobs' 16 groups each, in order) form a queue; a lane takes the next
// group when its current one is done, and every iteration
//   1. lets each lane consume its buffered word (the second word of its stream's last block)
//      while the state machine wants a word it has, then
//   2. computes ONE AES block per lane: the next block of whichever stream the lane's state
//      needs (keys selected per lane from LDS), and steps on its first word,
// so every lane with work computes a useful block on every iteration (a block is only ever
// computed when its first word is consumed at once).  The lane state is kept small (x / u / y
// share a register: each is live in disjoint states).
constexpr int kCos2Threads = 1024;
constexpr int kCos2KeyStride = kKeyWords + 4;  // keys of the two streams 4 banks apart

struct Cos2Lane {
  int g;                // queue index of the current group, -1: none
  int st;               // state | zi << 8 | zb << 15 | code << 16 | sample-in-group << 20
  unsigned long long oi;  // enc_noise index of the current sample
  uint32_t pos[2];      // next word of each stream's instance
  uint32_t have;        // bit s: spare[s] holds word pos[s]
  uint64_t spare[2];
  double c_int, c_frac, t, y_round;  // t: x (wedge), u (tail), y (bit / rr)
};

// One step of the state machine on word w; returns true when the sample is done (its output
// written).  Only the common states (Norm, Bit, RR without its exp) run unconditionally; the
// divisions and exp / log of the reference's comparisons sit in branches that only lanes
// needing them take:
//   START  r < exp(-(cFrac^2) / 2 sd^2) / (sqrt(2 pi) sd) can only hold when r < 1 / (sqrt(2 pi) sd)
//          (exp <= 1): the exp and division only then;
//   RR     rr < exp(arg), arg = -((yR + cFrac)^2 - y^2) / 2 sd^2 = -D / 2 sd^2: accepted when D <= 0
//          (arg >= +-0, exp >= 1 > rr), or when rr < (1 + a')(1 - 2^-48) with a' = -D (1 / 2 sd^2)
//          (1 + 2^-50) <= arg (the product form of the quotient, its rounding covered by the
//          2^-50) and exp(arg) >= 1 + arg (exp within an ulp, covered by the 2^-48); else the
//          reference's division and exp decide.
template <class Z>
__device__ __forceinline__ bool cos2_step(Cos2Lane& L, uint64_t w, const Z& Zg, const double* sdv, long long* en) {
  const double rn = 3.442619855899;
  const int st = L.st & 255, code = (L.st >> 16) & 3;
  const double fw = float52(w);
  bool have_nf = false, done = false;
  double nf = 0.0;
  int nst = st;
  if (st == kCoNorm) {  // gaussian_rounded.go:80-92
    const uint64_t b = w >> 63;
    const uint32_t i = (uint32_t)(w & 127u);
    const uint64_t j = (w >> 7) & 0xFFFFFFFFFFFFFull;
    const double x = (double)(int64_t)((j ^ (0ull - b)) + b) * Zg.wn[i];
    if (j < Zg.kn[i]) {
      nf = x;
      have_nf = true;
    } else if (i == 0) {
      L.st = (L.st & ~(1 << 15)) | ((int)b << 15);
      nst = kCoTailU;
    } else {
      L.st = (L.st & ~(127 << 8)) | ((int)i << 8);
      L.t = x;
      nst = kCoWedge;
    }
  } else if (st == kCoBit) {  // gaussian_cosac.go:43-50
    bool cmp;
    if ((w & 1) == 0) {
      L.y_round = round(L.t) - 1.0;
      cmp = L.y_round <= 0.5;
    } else {
      L.y_round = round(L.t) + 1.0;
      cmp = L.y_round >= -0.5;
    }
    nst = cmp ? kCoRR : kCoNorm;
  } else if (st == kCoRR) {  // gaussian_cosac.go:51-55
    const double D = (L.y_round + L.c_frac) * (L.y_round + L.c_frac) - L.t * L.t;
    bool acc = D <= 0.0;
    if (!acc) {
      const double ap = -D * sdv[4 * code + 1] * (1.0 + 8.881784197001252e-16);  // a' <= arg < 0
      acc = fw < (1.0 + ap) * 0.99999999999999644729;
      if (!acc) acc = fw < exp(-D / (2.0 * sdv[4 * code] * sdv[4 * code]));
    }
    if (acc) {
      en[L.oi] = (long long)L.y_round + (long long)L.c_int;
      done = true;
    } else {
      nst = kCoNorm;
    }
  } else if (st == kCoStart) {  // gaussian_cosac.go:36-40
    nst = kCoNorm;
    if (fw < sdv[4 * code + 3]) {  // r < 1 / lead: the reference's exp comparison decides
      const double sd = sdv[4 * code];
      if (fw < exp(-(L.c_frac * L.c_frac) / (2.0 * sd * sd)) / sdv[4 * code + 2]) {
        en[L.oi] = (long long)L.c_int;
        done = true;
      }
    }
  } else if (st == kCoWedge) {  // gaussian_rounded.go:109-113
    const int zi = (L.st >> 8) & 127;
    const double f0 = Zg.fn[zi - 1], f1 = Zg.fn[zi];
    if (fw * (f0 - f1) < exp(-0.5 * L.t * L.t) - f1) {
      nf = L.t;
      have_nf = true;
    } else {
      nst = kCoNorm;
    }
  } else {  // kCoTailU / kCoTailV, gaussian_rounded.go:94-101
    const double lg = -log(fw);
    if (st == kCoTailU) {
      L.t = lg * (1.0 / rn);
      nst = kCoTailV;
    } else if (lg + lg >= L.t * L.t) {
      const double uu = L.t + rn;
      nf = ((L.st >> 15) & 1) ? -uu : uu;
      have_nf = true;
    } else {
      nst = kCoTailU;
    }
  }
  if (have_nf) {
    L.t = sdv[4 * code] * nf;
    nst = kCoBit;
  }
  L.st = (L.st & ~255) | nst;
  return done;
}

__global__ __launch_bounds__(kCos2Threads, 1) void cosac2_noise_kernel(SampleArgs a) {
  __shared__ uint32_t lds[kAesLds];
  __shared__ uint32_t keys[2 * kCos2KeyStride];
  __shared__ uint64_t zig[384];  // kn, wn, fn
  __shared__ double sdv[12];     // per sd code: sd, 1 / (2 sd^2), sqrt(2 pi) sd, 1 / that
  aes_lds_fill(lds, a.te0);
  aes_key_fill(keys, a.key[kDomCosac]);
  aes_key_fill(keys + kCos2KeyStride, a.key[kDomCosacRnd]);
  for (int i = threadIdx.x; i < 128; i += blockDim.x) {
    zig[i] = a.zig.kn[i];
    zig[128 + i] = __double_as_longlong(a.zig.wn[i]);
    zig[256 + i] = __double_as_longlong(a.zig.fn[i]);
  }
  if (threadIdx.x < 3) {
    const double sd = threadIdx.x == 0 ? a.sd_ecd_blind : threadIdx.x == 1 ? a.sd_mask : a.sd_mask_blind;
    const double lead = sqrt(2.0 * M_PI) * sd;
    sdv[4 * threadIdx.x] = sd;
    sdv[4 * threadIdx.x + 1] = 1.0 / (2.0 * sd * sd);
    sdv[4 * threadIdx.x + 2] = lead;
    sdv[4 * threadIdx.x + 3] = 1.0 / lead;
  }
  __syncthreads();
  const ZigDev Z{zig, reinterpret_cast<const double*>(zig + 128), reinterpret_cast<const double*>(zig + 256)};
  const JShape& S = a.s;
  const int per = S.cols + S.rows;
  const long long njobs = a.batch * per;
  constexpr int NG = 256 / kCosGroup;  // groups per polynomial
  // a wave's queue is refilled kCos2Chunk jobs at a time from one counter (one atomic per chunk),
  // so waves whose groups drew few words take more jobs; results do not depend on which wave draws
  // a group
  constexpr int kCos2Chunk = 64 / NG;  // jobs per refill: one group per lane of the wave
  long long total = 0;   // groups in the wave's current chunk
  long long job0 = 0;    // the chunk's first job
  bool drained = false;  // the counter passed njobs
  unsigned long long* cq = reinterpret_cast<unsigned long long*>(a.wq + 2);
  const unsigned long long pbg = a.first_commit * (unsigned long long)(S.cols + 1) * S.rows * (unsigned long long)NG;
  auto mb = [](uint64_t m) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
  };
  auto start_sample = [&](Cos2Lane& L) {  // the group's next sample: its centre, state START
    const double center = __longlong_as_double(a.enc_noise[L.oi]);
    L.c_int = round(center);
    L.c_frac = L.c_int - center;
    L.st = (L.st & ~0xFFFF) | kCoStart;
  };
  Cos2Lane L;
  L.g = -1;
  L.st = 0;
  unsigned long long inst = 0;  // the group's instance (both streams)
  long long next = 0;
  for (;;) {
    bool can = L.g >= 0 && ((L.have >> co_src(L.st & 255)) & 1);
    uint64_t w = 0;
    if (!__ballot(can)) {
      // no lane can step on a buffered word: lanes without a group take the next ones of the
      // queue (groups of polynomials that draw nothing are dropped here), then every lane with
      // work computes the next block of the stream its state needs and steps on its first word
      for (;;) {
        const uint64_t need = __ballot(L.g < 0);
        if (!need) break;
        if (next >= total) {
          if (drained) break;
          unsigned long long base = 0;
          if ((threadIdx.x & 63) == 0) base = atomicAdd(cq, (unsigned long long)kCos2Chunk);
          job0 = (long long)(((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(base >> 32), 0) << 32) |
                             (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)base, 0));
          if (job0 >= njobs) {
            drained = true;
            break;
          }
          next = 0;
          total = (njobs - job0 < kCos2Chunk ? njobs - job0 : kCos2Chunk) * NG;
        }
        const int rank = mb(need);
        if (L.g < 0 && next + rank < total) {
          const long long g = next + rank;
          const long long job = job0 + g / NG;
          const long long b = job / per;
          const int j = (int)(job % per);
          const int col = j < S.cols ? j : S.cols, row = j < S.cols ? 0 : j - S.cols;
          const int code = col < S.cols ? 0 : (row == 0 ? 2 : 1);
          if (!enc_skipped(S, col, row) && sdv[4 * code] != a.sd_ecd) {
            const long long poly = (b * (S.cols + 1) + col) * S.rows + row;
            L.g = (int)g;
            L.oi = (unsigned long long)(poly * 256 + (g % NG) * kCosGroup);
            inst = pbg + (unsigned long long)(poly * NG + g % NG);
            L.st = code << 16;
            L.pos[0] = L.pos[1] = 0;
            L.have = 0;
            start_sample(L);
          }
        }
        next += __builtin_popcountll(need);
      }
      if (!__ballot(L.g >= 0)) break;
      if (L.g >= 0) {
        const int s = co_src(L.st & 255);
        const uint32_t p = L.pos[s];
        const LdsKey k{keys + s * kCos2KeyStride};
        if (p < 1024) {
          uint64_t w1;
          ks_words(k, inst, p / 2, lds, w, w1);
          if (s)
            L.spare[1] = w1;
          else
            L.spare[0] = w1;
        } else {  // past the first 8 KiB buffer: the XOR-accumulated refill (rare)
          w = uniform_word_at(k, lds, inst, p);
        }
        // spare[s] is word p + 1, the stream's next word once the step below has taken word p
        L.have = p < 1024 ? (L.have | (1u << s)) : (L.have & ~(1u << s));
        can = true;
      }
    } else if (can) {
      const int s = co_src(L.st & 255);
      w = s ? L.spare[1] : L.spare[0];
      L.have &= ~(1u << s);
    }
    if (can) {
      ++L.pos[co_src(L.st & 255)];
      if (cos2_step(L, w, Z, sdv, a.enc_noise)) {  // done: the group's next sample continues its streams
        const int kk = ((L.st >> 20) & 15) + 1;
        if (kk == kCosGroup) {
          L.g = -1;
        } else {
          L.st = (L.st & ~(15 << 20)) | (kk << 20);
          ++L.oi;
          start_sample(L);
        }
      }
    }
  }
}

#pragma clang fp contract(on)

// thread = (commit, column, MLWE polynomial, coefficient pair) (prover.go:130-139).  Two
// instantiations: ROUND = false covers the key columns (mlweSampler, one AES block and two table
// searches per pair), ROUND = true the mask column (the rounded Gaussian with its exp / log), so
// the table-search launch is not held at the rounded path's register count (238 VGPRs, 2 waves
// per SIMD, when both were one kernel).
constexpr int kMlweLdsTab = 512;  // mlweSampler's table in LDS up to this size (configs: 123 entries)
template <bool ROUND>
__global__ __launch_bounds__(512) void mlwe_noise_kernel(SampleArgs a) {
  __shared__ uint32_t lds[kAesLds];
  __shared__ uint32_t key[kKeyWords];
  __shared__ uint64_t mtab[ROUND ? 1 : kMlweLdsTab];
  aes_lds_fill(lds, a.te0);
  const bool tab_lds = a.cdt_mlwe.size <= kMlweLdsTab;  // else the binary search reads global memory
  if constexpr (ROUND) {
    aes_key_fill(key, a.key[kDomMlweRnd]);
  } else if (tab_lds) {
    for (int i = threadIdx.x; i < a.cdt_mlwe.size; i += blockDim.x) mtab[i] = a.cdt_mlwe.tables[i];
  }
  __syncthreads();
  const JShape& S = a.s;
  const int nm = S.in_msis + S.mlwe, half = S.d / 2;
  const int ncol = ROUND ? 1 : S.cols;  // columns this launch covers
  const long long n = a.n_ml_pairs / (S.cols + 1) * ncol;
  // grid-stride: a bounded grid fills the 64 KiB LDS tables once per workgroup, not once per 512 pairs
  for (long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x; gid < n;
       gid += (long long)gridDim.x * blockDim.x) {
    int m, j, col;
    long long b;
    if (n <= 0xffffffffLL) {
      const uint32_t g = (uint32_t)gid, r = idx_div(g, a.d_half), r2 = idx_div(r, a.d_nm);
      m = (int)(g - r * (uint32_t)half);
      j = (int)(r - r2 * (uint32_t)nm);
      if constexpr (ROUND) {
        col = S.cols;
        b = r2;
      } else {
        const uint32_t r3 = idx_div(r2, a.d_cols);
        col = (int)(r2 - r3 * (uint32_t)S.cols);
        b = r3;
      }
    } else {
      m = (int)(gid % half);
      const long long r = gid / half;
      j = (int)(r % nm);
      const long long r2 = r / nm;
      col = ROUND ? S.cols : (int)(r2 % S.cols);
      b = ROUND ? r2 : r2 / S.cols;
    }
    const long long poly = (b * (S.cols + 1) + col) * nm + j;  // (b, col, j)
    long long* out = a.mlwe_noise + poly * S.d;
    const unsigned long long gpoly = a.first_commit * (unsigned long long)(S.cols + 1) * nm + (unsigned long long)poly;
    if constexpr (!ROUND) {  // mlweSampler.Sample(0): centre 0, one table, no float tail
      uint64_t w0, w1;
      ks_words(a.key[kDomMlweCdt], gpoly, (uint64_t)m, lds, w0, w1);
      int64_t v0, v1;
      if (tab_lds) {
        v0 = cdt_search(mtab, a.cdt_mlwe.size, w0);
        v1 = cdt_search(mtab, a.cdt_mlwe.size, w1);
      } else {
        v0 = cdt_search(a.cdt_mlwe.tables, a.cdt_mlwe.size, w0);
        v1 = cdt_search(a.cdt_mlwe.tables, a.cdt_mlwe.size, w1);
      }
      out[2 * m] = v0 + a.cdt_mlwe.tail_lo;
      out[2 * m + 1] = v1 + a.cdt_mlwe.tail_lo;
    } else {  // roundedSampler.Sample(0, maskMLWEStdDev)
      for (int h = 0; h < 2; ++h) {
        const int k = 2 * m + h;
        Uniform u;
        u.init(key, lds, gpoly * S.d + k);
        out[k] = rounded_gauss(a.zig, u, 0.0, a.sd_mask_mlwe);
      }
    }
  }
}

// thread = one MustSetRandom draw: lastRow[0 .. cols*slots-2] (the last entry is zero, not
// drawn: prover.go:68-72) and the mask column's rows x slots elements (prover.go:93-115).
// Uint.SetRandom (element.go:299-343): read k = ceil(bitLen/8) bytes, clear the unused top
// bits, reject while >= q.
template <int L>
struct UniArgs {
  JShape s;
  AesKey key;
  const uint32_t* te0;
  FieldParams<L> F;
  int kbytes;
  uint32_t top_mask;
  unsigned long long first_commit;
  uint64_t* last_row;  // [B][cols*slots][L]
  uint64_t* mask;      // [B][rows][slots][L]
  long long total;     // B * (cols*slots + rows*slots)
  IdxDiv d_per;        // cols*slots + rows*slots, for total < 2^32
};

template <int L>
__global__ __launch_bounds__(512) void uniform_elems_kernel(UniArgs<L> a) {
  __shared__ uint32_t lds[kAesLds];
  __shared__ uint32_t key[kKeyWords];
  aes_lds_fill(lds, a.te0);
  aes_key_fill(key, a.key);
  __syncthreads();
  // grid-stride (see mlwe_noise_kernel); one draw per iteration
  for (long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x; gid < a.total;
       gid += (long long)gridDim.x * blockDim.x) [&] {
  const JShape& S = a.s;
  const long long nl = (long long)S.cols * S.slots, per = nl + (long long)S.rows * S.slots;
  long long b, i;
  if (a.total <= 0xffffffffLL) {
    b = idx_div((uint32_t)gid, a.d_per);
    i = gid - b * per;
  } else {
    b = gid / per;
    i = gid % per;
  }
  uint64_t* dst = i < nl ? a.last_row + (b * nl + i) * L : a.mask + (b * (per - nl) + (i - nl)) * L;
  if (i == nl - 1) {
    el_zero<L>(dst);
    return;
  }
  const unsigned long long inst = (a.first_commit + (unsigned long long)b) * (unsigned long long)per + (unsigned long long)i;
  uint64_t z[L];
  bool whole = false;  // whole words (e.g. q255: 32 bytes): a try = L/2 blocks, in parallel
  if constexpr (L % 2 == 0) {
    whole = a.kbytes == 8 * L;
    if (whole) set_random_whole<L>(LdsKey{key}, lds, inst, set_random_topm(a.top_mask), a.F, z);
  }
  if (!whole) set_random_bytes<L>(key, lds, inst, a.kbytes, a.top_mask, a.F, z);
  el_copy<L>(dst, z);
  }();
}

// Whole-word draws (kbytes = 8 L, e.g. q255) within the first 8 KiB of each instance: a try is
// L / 2 AES blocks in parallel, up to 1024 / L tries.  A draw that needs more (its probability is
// 0.475^256 at q255) is left as all-ones -- never a value below q -- and flagged for
// uniform_fix_kernel, so this kernel carries no XOR-accumulated refill: 112 VGPRs (4 waves/SIMD)
// against the general kernel's 164 (2 waves/SIMD with its 64 KiB of LDS).
template <int L>
__global__ __launch_bounds__(512) void uniform_whole_kernel(UniArgs<L> a, int* flag, int max_tries) {
  __shared__ uint32_t lds[kAesLds];
  __shared__ uint32_t key[kKeyWords];
  aes_lds_fill(lds, a.te0);
  aes_key_fill(key, a.key);
  __syncthreads();
  const JShape& S = a.s;
  const long long nl = (long long)S.cols * S.slots, per = nl + (long long)S.rows * S.slots;
  const uint64_t topm = ((uint64_t)a.top_mask << 56) | 0x00FFFFFFFFFFFFFFull;
  const long long stride = (long long)gridDim.x * blockDim.x;
  // One try per iteration, and a lane moves on to its next element (grid-stride) as soon as its
  // current one is accepted: the wave no longer waits, element by element, for its slowest lane
  // (a try is accepted with probability q / 2^bitlen(q-1), 0.52 at q255: the most tries among 64
  // lanes averages ~6 against 1.9 per lane).  Same draws: element i's try t reads the same blocks.
  long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t* dst = nullptr;
  unsigned long long inst = 0;
  int t = 0;
  auto next = [&]() {  // from gid: the element's destination and instance; skips lastRow's last entry
    while (gid < a.total) {
      long long b, i;
      if (a.total <= 0xffffffffLL) {
        b = idx_div((uint32_t)gid, a.d_per);
        i = gid - b * per;
      } else {
        b = gid / per;
        i = gid % per;
      }
      dst = i < nl ? a.last_row + (b * nl + i) * L : a.mask + (b * (per - nl) + (i - nl)) * L;
      if (i != nl - 1) {
        inst = (a.first_commit + (unsigned long long)b) * (unsigned long long)per + (unsigned long long)i;
        t = 0;
        return;
      }
      el_zero<L>(dst);  // genFirstLastRow leaves it zero
      gid += stride;
    }
  };
  next();
  static_assert(L % 2 == 0, "whole 16-byte blocks per try");
  while (gid < a.total) {
    uint64_t z[L];
    bool ok = false;
    if (max_tries > 0) {  // (0: every draw left to the fix-up, the experiments build's test)
      ok = set_random_whole_try<L>(LdsKey{key}, lds, inst, t, topm, a.F, z);
    }
    if (ok || t + 1 >= max_tries) {
      if (!ok) *flag = 1;
#pragma unroll
      for (int l = 0; l < L; ++l) dst[l] = ok ? z[l] : ~0ull;
      gid += stride;
      next();
    } else {
      ++t;
    }
  }
}

// uniform_whole_kernel's leftovers: nothing unless a draw was flagged; then every all-ones element
// is drawn again by the general kernel's loop, refill included
template <int L>
__global__ __launch_bounds__(512) void uniform_fix_kernel(UniArgs<L> a, const int* flag) {
  if (*flag == 0) return;
  __shared__ uint32_t lds[kAesLds];
  __shared__ uint32_t key[kKeyWords];
  aes_lds_fill(lds, a.te0);
  aes_key_fill(key, a.key);
  __syncthreads();
  const JShape& S = a.s;
  const long long nl = (long long)S.cols * S.slots, per = nl + (long long)S.rows * S.slots;
  const uint64_t topm = ((uint64_t)a.top_mask << 56) | 0x00FFFFFFFFFFFFFFull;
  for (long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x; gid < a.total;
       gid += (long long)gridDim.x * blockDim.x) {
    long long b, i;
    if (a.total <= 0xffffffffLL) {
      b = idx_div((uint32_t)gid, a.d_per);
      i = gid - b * per;
    } else {
      b = gid / per;
      i = gid % per;
    }
    uint64_t* dst = i < nl ? a.last_row + (b * nl + i) * L : a.mask + (b * (per - nl) + (i - nl)) * L;
    bool ones = i != nl - 1;
#pragma unroll
    for (int l = 0; l < L; ++l) ones = ones && dst[l] == ~0ull;
    if (!ones) continue;
    const unsigned long long inst = (a.first_commit + (unsigned long long)b) * (unsigned long long)per + (unsigned long long)i;
    uint64_t z[L];
    set_random_whole<L>(LdsKey{key}, lds, inst, topm, a.F, z);
    el_copy<L>(dst, z);
  }
}

// raw Sample() words of one UniformSampler instance (rg_uniform_words_dev)
__global__ __launch_bounds__(512) void uniform_words_kernel(AesKey key, const uint32_t* te0, unsigned long long inst,
                                                            unsigned long long first, long long n, uint64_t* out) {
  __shared__ uint32_t lds[kAesLds];
  __shared__ uint32_t kl[kKeyWords];
  aes_lds_fill(lds, te0);
  aes_key_fill(kl, key);
  __syncthreads();
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= n) return;
  Uniform u;
  u.init(kl, lds, inst);
  out[gid] = u.word_at(first + (unsigned long long)gid);
}

// ------------------------------------------------------------------------------------------
// host: keys, launches, the sampler stage and its scratch
// ------------------------------------------------------------------------------------------
static rg_status make_keys(const rg_jindo_seeds* seeds, AesKey* keys) {
  const uint8_t* sd[kNumDom] = {seeds->enc_cdt, seeds->enc_cosac, seeds->enc_cosac_round,
                                seeds->mlwe_cdt, seeds->mlwe_round, seeds->uniform};
  for (int i = 0; i < kNumDom; ++i) RG_TRY(derive_key(sd[i], 32, keys[i]));
  return RG_OK;
}

template <int L>
static rg_status launch_uniform(const rg_jindo* J, size_t batch, const AesKey& key, unsigned long long first,
                                uint64_t* last, uint64_t* mask, int* flag, hipStream_t st) {
  UniArgs<L> a;
  a.s = shape_of(J->p, 1);
  a.key = key;
  a.te0 = J->smp.te0.as<uint32_t>();
  a.F = field_params<L>(&J->field);
  set_random_shape(&J->field, a.kbytes, a.top_mask);
  a.first_commit = first;
  a.last_row = last;
  a.mask = mask;
  a.total = (long long)batch * ((long long)J->p.cols * J->p.slots + (long long)J->p.rows * J->p.slots);
  a.d_per = make_idxdiv((uint32_t)(J->p.cols * J->p.slots + J->p.rows * J->p.slots));
  const dim3 ug((unsigned)std::min<long long>((a.total + 511) / 512, 1024));
  // whole-word draws: about 4 elements per lane (the flattened try loop balances lanes only over
  // several elements), at least one workgroup per CU
  const dim3 ugw((unsigned)std::max<long long>(std::min<long long>((a.total + 512 * 4 - 1) / (512 * 4), 1024), std::min<long long>((a.total + 511) / 512, 256)));
  if constexpr (L % 2 == 0) {
    if (a.kbytes == 8 * L) {  // whole words: the common draws, then the (practically never) long ones
      const char* kt = knob(Knob::JindoUniTries);  // experiments build: cap the tries (fix-up test)
      const int tries = std::max(0, std::min(1024 / L, kt ? atoi(kt) : 1024 / L));
      RG_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
      hipLaunchKernelGGL(uniform_whole_kernel<L>, ugw, dim3(512), 0, st, a, flag, tries);
      RG_TRY(check_launch("jindo uniform (whole words)"));
      hipLaunchKernelGGL(uniform_fix_kernel<L>, ug, dim3(512), 0, st, a, (const int*)flag);
      return check_launch("jindo uniform (long draws)");
    }
  }
  hipLaunchKernelGGL(uniform_elems_kernel<L>, ug, dim3(512), 0, st, a);
  return check_launch("jindo uniform");
}

// lastRow/mask (crypto/rand), then digits, then every Gaussian sample of the batch
// Streams: st runs MustSetRandom, the digits, the COSAC centres and TwinCDT (cdt2); s_cos, once the
// centres are done (event e_dig), cosac2; s_ml, once st reaches this call (event e_start),
// the MLWE samplers, which need neither.  s_cos / s_ml may be st itself (one stream, no events).
// The caller joins s_cos and s_ml back into st before it reads their outputs.
static rg_status sample_stage(rg_jindo* J, size_t batch, const uint64_t* d_v, size_t nv, const rg_jindo_seeds* seeds,
                              unsigned long long first, uint64_t* d_last, uint64_t* d_mask, int64_t* d_en,
                              int64_t* d_mn, uint32_t* digits, rg_jindo_scratch* sc, hipStream_t st,
                              hipStream_t s_cos = nullptr, hipStream_t s_ml = nullptr, hipEvent_t e_start = nullptr,
                              hipEvent_t e_dig = nullptr) {
  if (!s_cos) s_cos = st;
  if (!s_ml) s_ml = st;
  const rg_jindo_params& p = J->p;
  if (!J->smp.ready) {
    set_last_error("rg_jindo_set_stddevs was not called on this handle");
    return RG_ERR_INVALID;
  }
  const rg_jindo_samplers& S = J->smp;
  // the shapes the device samplers cover (every NewParameters shape of a field with exp <= 64)
  if (p.d != 256 || p.slots % 4 != 0 || S.cdt_enc_size > kCdtLdsMaxSize) {
    set_last_error("device sampling needs d = 256, slots % 4 == 0 and an encode TwinCDT table of <= 96 entries (got d = " +
                   std::to_string(p.d) + ", slots = " + std::to_string(p.slots) + ", table " +
                   std::to_string(S.cdt_enc_size) + ")");
    return RG_ERR_UNSUPPORTED;
  }
  SampleArgs a;
  memset(&a, 0, sizeof(a));
  RG_TRY(make_keys(seeds, a.key));
  if (!sc->wq.p) {  // [0] cdt2's chunk counter, [2..3] cosac2's job counter, [4] uniform's long-draw flag
    std::lock_guard<std::mutex> lk(J->mu);
    RG_TRY(sc->wq.alloc(256));
  }
  int* uflag = sc->wq.as<int>() + 4;
  if (s_ml != st) {
    RG_HIP(hipEventRecord(e_start, st));
    RG_HIP(hipStreamWaitEvent(s_ml, e_start, 0));
  }
  RG_TRY(dispatch_limbs(p.field_limbs, [&](auto Lc) {
    return launch_uniform<Lc()>(J, batch, a.key[kDomUniform], first, d_last, d_mask, uflag, st);
  }));
  RG_TRY(digits_stage(J, batch, d_v, nv, d_last, d_mask, digits, st));
  a.s = shape_of(p, (long long)nv);
  a.te0 = S.te0.as<uint32_t>();
  a.first_commit = first;
  a.digits = digits;
  a.delta = S.delta.as<double>();
  a.cdt_enc = CdtDev{S.cdt_enc.as<uint64_t>(), S.cdt_guide.as<uint8_t>(), S.cdt_enc_size, S.tail_lo_enc, S.sd[0]};
  a.cdt_mlwe = CdtDev{S.cdt_mlwe.as<uint64_t>(), nullptr, S.cdt_mlwe_size, S.tail_lo_mlwe, S.sd[4]};
  const uint64_t* zg = S.zig.as<uint64_t>();
  a.zig = ZigDev{zg, reinterpret_cast<const double*>(zg + 128), reinterpret_cast<const double*>(zg + 256)};
  a.sd_ecd = S.sd[0];
  a.sd_ecd_blind = S.sd[1];
  a.sd_mask = S.sd[2];
  a.sd_mask_blind = S.sd[3];
  a.sd_mask_mlwe = S.sd[5];
  a.enc_noise = reinterpret_cast<long long*>(d_en);
  a.mlwe_noise = reinterpret_cast<long long*>(d_mn);
  const int nm = p.in_msis + p.mlwe;
  a.n_enc_pairs = (long long)batch * (p.cols + 1) * p.rows * (p.d / 2);
  a.n_ml_pairs = (long long)batch * (p.cols + 1) * nm * (p.d / 2);
  a.d_half = make_idxdiv((uint32_t)(p.d / 2));
  a.d_nm = make_idxdiv((uint32_t)nm);
  a.d_cols = make_idxdiv((uint32_t)std::max(p.cols, 1));
  a.batch = (long long)batch;
  {
    const long long npoly = (long long)batch * (p.cols + 1) * p.rows;
    const int cw = cdt2_waves(S.cdt_enc_size);
    const unsigned g = (unsigned)std::min<long long>((npoly + cw - 1) / cw, 256);
    a.cdt_sbound = S.cdt_sbound.as<double>();
    a.cdt_jmax = S.cdt_jmax.as<int>();
    // experiments build, RINGO_JINDO_CDT_PATH=sum: an infinite band, so neither bound decides (the
    // products are +-inf, or NaN at a zero sum) and every tail goes through the exact sum
    const char* kp = knob(Knob::JindoCdtPath);
    a.cdt_band = kp && !strcmp(kp, "sum") ? HUGE_VAL : 9.094947017729282e-13;
    a.wq = sc->wq.as<int>();
    RG_HIP(hipMemsetAsync(a.wq, 0, 4 * sizeof(int), st));  // [0]: cdt2's chunks, [2..3]: cosac2's jobs (u64)
    // the COSAC centres (small) ahead of cdt2 on st: launched on s_cos beside cdt2 they wait for
    // cdt2's one-per-CU workgroups to finish (configs[4]: 6.9 ms), and cosac2 with them
    const long long ncos = (long long)batch * (p.cols + p.rows);  // COSAC jobs
    hipLaunchKernelGGL(cos_centre_kernel, dim3((unsigned)((ncos + kCentreWaves - 1) / kCentreWaves)),
                       dim3(64 * kCentreWaves), 0, st, a);
    RG_TRY(check_launch("jindo enc noise (COSAC centres)"));
    if (s_cos != st) {
      RG_HIP(hipEventRecord(e_dig, st));
      RG_HIP(hipStreamWaitEvent(s_cos, e_dig, 0));
    }
    hipLaunchKernelGGL(cdt2_noise_kernel, dim3(g), dim3(64 * cw), cdt2_dyn_lds(S.cdt_enc_size, cw), st, a);
    RG_TRY(check_launch("jindo enc noise (TwinCDT)"));
    const long long w2 = kCos2Threads / 64;
    const unsigned g2 = (unsigned)std::min<long long>((ncos + w2 - 1) / w2, 256);
    hipLaunchKernelGGL(cosac2_noise_kernel, dim3(g2), dim3(kCos2Threads), 0, s_cos, a);
    RG_TRY(check_launch("jindo enc noise (COSAC)"));
  }
  {
    const long long per_col = a.n_ml_pairs / (p.cols + 1);
    if (p.cols > 0) {
      const long long n = per_col * p.cols;
      hipLaunchKernelGGL(mlwe_noise_kernel<false>, dim3((unsigned)std::min<long long>((n + 511) / 512, 1024)),
                         dim3(512), 0, s_ml, a);
      RG_TRY(check_launch("jindo mlwe noise (table)"));
    }
    hipLaunchKernelGGL(mlwe_noise_kernel<true>, dim3((unsigned)std::min<long long>((per_col + 511) / 512, 1024)),
                       dim3(512), 0, s_ml, a);
  }
  return check_launch("jindo mlwe noise (rounded)");
}

// scratch for the sampled randomness of `batch` commits
static rg_status sample_scratch(rg_jindo* J, size_t batch, rg_jindo_scratch* sc, hipStream_t st) {
  const JSizes z = sizes_of(J->p, batch);
  std::lock_guard<std::mutex> lk(J->mu);
  if (sc->last.bytes < z.last || sc->mask.bytes < z.mask || sc->en.bytes < z.en || sc->mn.bytes < z.mn)
    RG_HIP(hipStreamSynchronize(st));
  RG_TRY(sc->last.alloc(z.last));
  RG_TRY(sc->mask.alloc(z.mask));
  RG_TRY(sc->en.alloc(z.en));
  RG_TRY(sc->mn.alloc(z.mn));
  return RG_OK;
}

}  // namespace rg

using namespace rg;

extern "C" {

rg_status rg_jindo_set_stddevs(rg_jindo* J, const rg_jindo_stddevs* sd) {
  if (!J || !sd) return RG_ERR_INVALID;
  const double v[6] = {sd->ecd, sd->ecd_blind, sd->mask, sd->mask_blind, sd->mlwe, sd->mask_mlwe};
  for (double x : v)
    if (!(x > 0.0) || !std::isfinite(x)) return RG_ERR_INVALID;  // RoundedGaussianSampler panics on <= 0
  rg_jindo_samplers& S = J->smp;
  std::lock_guard<std::mutex> lk(J->mu);
  S.ready = false;
  memcpy(S.sd, v, sizeof(v));
  uint32_t te0[256];
  aes_te0(te0);
  RG_TRY(S.te0.upload(te0, sizeof(te0)));
  // Encoder.twinCDT: 128 centre tables at ecdStdDev (twin_cdt.go:48-58); Prover.mlweSampler:
  // the same at mlweStdDev, of which Sample(0) reads table 0
  std::vector<uint64_t> enc, ml;
  for (int c = 0; c < 128; ++c) {
    const std::vector<uint64_t> t = compute_cdt((double)c / 128.0, v[0]);
    enc.insert(enc.end(), t.begin(), t.end());
    S.cdt_enc_size = (int)t.size();
  }
  ml = compute_cdt(0.0, v[4]);
  S.cdt_mlwe_size = (int)ml.size();
  S.tail_lo_enc = -(int64_t)std::ceil(9.0 * v[0]);
  S.tail_lo_mlwe = -(int64_t)std::ceil(9.0 * v[4]);
  RG_TRY(S.cdt_enc.upload(enc.data(), enc.size() * 8));
  if (S.cdt_enc_size <= 255) {  // guide: per table, lower_bound of t * 2^56 for t = 0..256
    std::vector<uint8_t> guide(128 * 257);
    for (int c = 0; c < 128; ++c) {
      const uint64_t* t = enc.data() + (size_t)c * S.cdt_enc_size;
      for (int b = 0; b <= 256; ++b) {
        int i = 0;
        if (b == 256)
          i = S.cdt_enc_size;
        else
          while (i < S.cdt_enc_size && t[i] < ((uint64_t)b << 56)) ++i;
        guide[c * 257 + b] = (uint8_t)i;
      }
    }
    RG_TRY(S.cdt_guide.upload(guide.data(), guide.size()));
  }
  {  // cdt2's tail bounds: the reference's tail cdf (twin_cdt.go:101-105) at centres c / 128, c = 0..128
    const int n = S.cdt_enc_size;
    const double sigma = v[0], norm = std::sqrt(2.0 * M_PI) * sigma;
    std::vector<double> sb((size_t)129 * (n + 2));
    for (int c = 0; c <= 128; ++c) {
      const double cf = (double)c / 128.0;
      double cdf = 0.0;
      int64_t x = S.tail_lo_enc;
      for (int j = -1; j <= n; ++j) {  // entry j + 1: sum over x = tailLo .. j
        for (; x <= j; ++x) {
          const double xf = (double)x;
          cdf += std::exp(-(xf - cf) * (xf - cf) / (2.0 * sigma * sigma)) / norm;
        }
        sb[(size_t)c * (n + 2) + j + 1] = cdf;
      }
    }
    // Bounds of that sum f_j over cFrac in [c, c + 1] / 128 from its values at the two ends.  f_j
    // falls with the centre while the terms left of it dominate (every j at NewParameters' widths,
    // where f_j tracks the normal cdf), but not in general: at small widths the lattice sum itself
    // swings with the centre (sum_x rho(x - c) / norm ~ 1 + 2 exp(-2 pi^2 sigma^2) cos(2 pi c)), and
    // terms right of the centre rise with it.  So: min and max of the two ends, widened by the
    // chord's error h^2 / 8 max |f_j''|, h = 1/128, with |f_j''| <= sum_x |z^2 - 1| rho / (norm sigma^2)
    // (z = (x - c) / sigma) <= (2 + 1.14 / sigma) / sigma^2: (z^2 + 1) exp(-z^2 / 2) has integral
    // 2 sqrt(2 pi) and total variation < 2.85, which bounds its lattice sum.  7e-7 at ecdStdDev = 4.79.
    // (tests/test_oracle_sampler_paths.py checks the claim on a grid of centres.)  The lower bound is
    // clamped at 0: the cdf is not negative, and a negative bound times cdt_band's (1 - inf) would be +inf.
    const double chord = (2.0 + 1.14 / sigma) / (sigma * sigma) / (8.0 * 128.0 * 128.0);
    std::vector<double> lohi((size_t)2 * 128 * (n + 2));
    for (int c = 0; c < 128; ++c)
      for (int k = 0; k < n + 2; ++k) {
        const double s0 = sb[(size_t)c * (n + 2) + k], s1 = sb[(size_t)(c + 1) * (n + 2) + k];
        lohi[(size_t)c * (n + 2) + k] = std::max(0.0, std::min(s0, s1) - chord);
        lohi[(size_t)(128 + c) * (n + 2) + k] = std::max(s0, s1) + chord;
      }
    RG_TRY(S.cdt_sbound.upload(lohi.data(), lohi.size() * 8));
    // jmax[c]: the largest J with, for every v0 = j in [-1, J] of table c, the bound on p
    // (t_c[j + 1] / 2^64, or 1 past the table) below the smallest cdf the reference can compare it
    // with (the lower bound (1 - 2^-40)), again shrunk by 2^-40 for the double rounding of p
    std::vector<int> jm(128);
    for (int c = 0; c < 128; ++c) {
      const uint64_t* t = enc.data() + (size_t)c * n;
      int J = -2;
      for (int j = -1; j <= n; ++j) {
        const double pu = (j + 1 < n ? (double)t[j + 1] / 18446744073709551616.0 : 1.0) * (1.0 + 9.094947017729282e-13);
        if (!(pu < lohi[(size_t)c * (n + 2) + j + 1] * (1.0 - 9.094947017729282e-13))) break;
        J = j;
      }
      jm[c] = J;
    }
    // experiments build, RINGO_JINDO_CDT_PATH=exact | sum: no sample takes the guide-table fast path
    if (const char* kp = knob(Knob::JindoCdtPath); kp && (!strcmp(kp, "exact") || !strcmp(kp, "sum")))
      std::fill(jm.begin(), jm.end(), -2);
    RG_TRY(S.cdt_jmax.upload(jm.data(), jm.size() * 4));
  }
  RG_TRY(S.cdt_mlwe.upload(ml.data(), ml.size() * 8));
  const Ziggurat Z = make_ziggurat();
  std::vector<uint64_t> zg(384);
  memcpy(zg.data(), Z.kn, 128 * 8);
  memcpy(zg.data() + 128, Z.wn, 128 * 8);
  memcpy(zg.data() + 256, Z.fn, 128 * 8);
  RG_TRY(S.zig.upload(zg.data(), zg.size() * 8));
  S.h_delta = compute_delta_inv(J->p.base, J->p.exp);
  RG_TRY(S.delta.upload(S.h_delta.data(), S.h_delta.size() * 8));
  S.ready = true;
  return RG_OK;
}

rg_status rg_jindo_delta_inv(const rg_jindo* J, double* out) {
  if (!J || !out) return RG_ERR_INVALID;
  const std::vector<double> d = compute_delta_inv(J->p.base, J->p.exp);
  memcpy(out, d.data(), d.size() * 8);
  return RG_OK;
}

// Every sampler instance of commits [first, first + batch) must have a u64 number (so that no two
// instances share a window; csprng.hpp ks_words): the largest per-commit count of a domain is
// (cols+1) rows d (COSAC, per sample), (cols+1) (in_msis+mlwe) d (rounded MLWE, per sample) or
// (cols + rows) slots (MustSetRandom, per element).
static rg_status instances_in_range(const rg_jindo* J, unsigned long long first, size_t batch) {
  const rg_jindo_params& p = J->p;
  const unsigned __int128 per_enc = (unsigned __int128)(p.cols + 1) * p.rows * p.d;
  const unsigned __int128 per_ml = (unsigned __int128)(p.cols + 1) * (p.in_msis + p.mlwe) * p.d;
  const unsigned __int128 per_uni = (unsigned __int128)(p.cols + p.rows) * p.slots;
  const unsigned __int128 per = std::max(per_enc, std::max(per_ml, per_uni));
  const unsigned __int128 end = (unsigned __int128)first + batch;
  if (end > ((unsigned __int128)1 << 64) / per) {
    set_last_error("first_commit + batch: sampler instance numbers would exceed 2^64");
    return RG_ERR_INVALID;
  }
  return RG_OK;
}

rg_status rg_jindo_sample_dev(const rg_jindo* J, size_t batch, const uint64_t* d_v, size_t nv,
                              const rg_jindo_seeds* seeds, unsigned long long first_commit, uint64_t* d_last_row,
                              uint64_t* d_mask, int64_t* d_enc_noise, int64_t* d_mlwe_noise, void* stream) {
  if (!J || !seeds) return RG_ERR_INVALID;
  if (nv < 1 || nv > (size_t)J->p.rank) return RG_ERR_RANK;
  RG_TRY(instances_in_range(J, first_commit, batch));
  if (batch == 0) return RG_OK;
  if (!d_v || !d_last_row || !d_mask || !d_enc_noise || !d_mlwe_noise) return RG_ERR_INVALID;
  RG_TRY(on_device(J));
  rg_jindo* Jm = const_cast<rg_jindo*>(J);
  hipStream_t st = as_stream(stream);
  rg_jindo_scratch* sc = nullptr;
  RG_TRY(stream_scratch(Jm, batch, st, &sc));
  return sample_stage(Jm, batch, d_v, nv, seeds, first_commit, d_last_row, d_mask, d_enc_noise, d_mlwe_noise,
                      sc->digits.as<uint32_t>(), sc, st);
}

rg_status rg_jindo_commit_sampled_dev(const rg_jindo* J, size_t batch, const uint64_t* d_v, size_t nv,
                                      const rg_jindo_seeds* seeds, unsigned long long first_commit, uint64_t* d_incom,
                                      uint64_t* d_enc, uint64_t* d_mlwe, uint64_t* d_com, void* stream) {
  if (!J || !seeds) return RG_ERR_INVALID;
  if (nv < 1 || nv > (size_t)J->p.rank) return RG_ERR_RANK;
  RG_TRY(instances_in_range(J, first_commit, batch));
  if (batch == 0) return RG_OK;
  if (!d_v || !d_incom || !d_enc || !d_mlwe || !d_com) return RG_ERR_INVALID;
  RG_TRY(on_device(J));
  rg_jindo* Jm = const_cast<rg_jindo*>(J);
  hipStream_t st = as_stream(stream);
  rg_jindo_scratch* sc = nullptr;
  RG_TRY(stream_scratch(Jm, batch, st, &sc));
  RG_TRY(sample_scratch(Jm, batch, sc, st));
  uint32_t* digits = sc->digits.as<uint32_t>();
  int64_t *en = sc->en.as<int64_t>(), *mn = sc->mn.as<int64_t>();
  // The batch as one DAG over three streams (the caller's st and two helpers of this caller
  // stream), so that each sampler's tail overlaps other work instead of idling the chip:
  //   st:   MustSetRandom -> digits -> cdt2 (TwinCDT) ...................... -> prep(encode) -> core
  //   s[0]:                    (digits) -> COSAC centres -> cosac2 ----------^
  //   s[1]: mlwe samplers -> prep(MLWE) -------------------------------------^
  // Results do not depend on the schedule: every sampler instance is numbered per commit, and
  // each buffer has one writer ordered before its readers by the events.
  static const bool one_stream = [] {  // RINGO_JINDO_SPLIT=0: everything on st (per-kernel profiling)
    const char* e = knob(Knob::JindoSplit);
    return e && e[0] == '0';
  }();
  rg_jindo::Aux* ax = nullptr;
  if (!one_stream) {
    std::lock_guard<std::mutex> lk(Jm->mu);
    rg_jindo::Aux& x = Jm->aux[st];
    for (hipStream_t& s : x.s)
      if (!s) RG_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    for (hipEvent_t& e : x.e)
      if (!e) RG_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ax = &x;
  }
  hipStream_t s_cos = ax ? ax->s[0] : st, s_ml = ax ? ax->s[1] : st;
  rg_status s = sample_stage(Jm, batch, d_v, nv, seeds, first_commit, sc->last.as<uint64_t>(), sc->mask.as<uint64_t>(),
                             en, mn, digits, sc, st, s_cos, s_ml, ax ? ax->e[0] : nullptr, ax ? ax->e[1] : nullptr);
  if (s == RG_OK) s = prep_launch(Jm, batch, nv, digits, en, mn, d_enc, d_mlwe, kPrepMlwe, s_ml);
  // (the TwinCDT rows' prep right behind cdt2, beside cosac2, measured no faster: r05i)
  if (ax) {
    // join: the encode prep needs both samplers' noise; the core needs the MLWE prep.  Joined on
    // every exit path, so that after a failed launch the caller's stream still orders whatever
    // helper work was queued before this handle's scratch (wq, en, mn) is reused; the first error
    // is the one returned
    const hipError_t j[4] = {hipEventRecord(ax->e[2], s_cos), hipEventRecord(ax->e[3], s_ml),
                             hipStreamWaitEvent(st, ax->e[2], 0), hipStreamWaitEvent(st, ax->e[3], 0)};
    for (hipError_t e : j)
      if (e != hipSuccess && s == RG_OK) {
        set_last_error(std::string("jindo sampled commit: joining the helper streams: ") + hipGetErrorString(e));
        s = RG_ERR_DEVICE;
      }
  }
  RG_TRY(s);
  RG_TRY(prep_launch(Jm, batch, nv, digits, en, mn, d_enc, d_mlwe, kPrepEnc, st));
  return commit_core(Jm, batch, d_enc, d_mlwe, d_incom, d_com, sc, st);
}

rg_status rg_uniform_words_dev(const uint8_t* seed, size_t seed_len, unsigned long long instance,
                               unsigned long long first_word, size_t n, uint64_t* d_out, void* stream) {
  if ((!seed && seed_len) || (!d_out && n)) return RG_ERR_INVALID;
  if (n == 0) return RG_OK;
  AesKey K;
  RG_TRY(derive_key(seed, seed_len, K));
  uint32_t te0[256];
  aes_te0(te0);
  DevBuf t;
  RG_TRY(t.upload(te0, sizeof(te0)));
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(uniform_words_kernel, dim3((unsigned)((n + 511) / 512)), dim3(512), 0, st, K, t.as<uint32_t>(),
                     instance, first_word, (long long)n, d_out);
  RG_TRY(check_launch("uniform words"));
  RG_HIP(hipStreamSynchronize(st));  // `t` is freed on return
  return RG_OK;
}

}  // extern "C"
