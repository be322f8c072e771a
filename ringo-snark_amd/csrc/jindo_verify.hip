// jindo_verify.hip -- the device work of Verifier.Verify and of Prover.Evaluate (overview in
// jindo_commit.hip; shared definitions in jindo_impl.hpp).
// Evaluate: every MulCoeffsMontgomeryThenAdd loop is a J = 1 dot product on mac_kernel
// (rg_jindo_eval_*; dot_split_kernel for the batch combination), plus rns_reduce_kernel after a
// cross-GPU sum of partial openBatches.
// The inputs of both that depend on the transcript alone are built here too: leftVec / rightVec of
// the evaluation point with Encoder.encode of each left element (rg_jindo_eval_point_dev) and
// encodeChallengeTo of the challenge bytes (rg_jindo_encode_challenges_dev); for a batch of proofs,
// all of them in one call (rg_jindo_eval_point_multi_dev, rg_jindo_verify_inputs_multi_dev).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "chal_digits.hpp"
#include "digits_dc.hpp"
#include "host_field.hpp"
#include "jindo_impl.hpp"

namespace rg {

// ------------------------------------------------------------------------------------------
// Verifier.Verify (verifier.go:50-282), challenges injected.  The MACs run on mac_kernel
// (jindo_commit.hip), the lifted inner commitments on round_kernel (cut 0, ringQOut -> ringQ);
// these kernels add:
//   norm_kernel    workgroup per polynomial: IMForm, INTT, centred CRT, sum of squares
//                  (verifyNorm :262-276) -> kNormW words per polynomial
//   combine_kernel A * 2^cut - B per residue (MulRNSScalarMontgomery, ...ThenSub)
//   neq_kernel     any word of x != y -> flag (verifyConsistency :203-221)
//   decode_kernel  workgroup per polynomial: IMForm, INTT, centred CRT, SetBigInt mod p,
//                  Horner in base b over the slots (DecodeTo, encoder.go:203-219)
//   dot2_kernel    one workgroup: sum right * dcd and sum batchDcd[0] * y (verifyEval :224-259)
// ------------------------------------------------------------------------------------------
constexpr int kNormW = 10;  // words of a sum of squares (|value| < 2^240, <= 2^20 values)

struct NormArgs {
  int d;
  RingDev R;
  CrtDev crt;
  const uint64_t* in;  // [npoly] at stride in_stride, R.n limbs
  long long in_stride;
  uint64_t* out;       // [npoly][kNormW]
};

__device__ __forceinline__ void mw_add(uint64_t* a, const uint64_t* b, int n) {
  uint32_t c = 0;
  for (int i = 0; i < n; ++i) a[i] = addc(a[i], b[i], c);
}

__global__ __launch_bounds__(256) void norm_kernel(NormArgs a) {
  extern __shared__ uint64_t poly_lds[];
  const int d = a.d, tid = threadIdx.x, ns = a.R.n;
  auto poly = [&](int l) { return poly_lds + (long long)l * d; };
  const long long pid = blockIdx.x;
  const uint64_t* in = a.in + pid * a.in_stride;
  for (int k = tid; k < ns * d; k += blockDim.x) {
    const int l = k / d;
    const RnsPrime& P = a.R.p[l];
    poly(l)[k % d] = sh_mul(in[k], P.rinv, P.rinv_sh, P.q);  // IMForm
  }
  __syncthreads();
  const int half = blockDim.x >> 1;
  for (int l0 = 0; l0 < ns; l0 += 2) {
    const int l = l0 + (tid >= half ? 1 : 0);
    const bool active = l < ns;
    const int lc = active ? l : l0;
    intt_lds(poly(lc), d, a.R.bwd + (long long)lc * d, a.R.p[lc], tid % half, half, active);
  }
  uint64_t acc[kNormW];
  for (int i = 0; i < kNormW; ++i) acc[i] = 0;
  for (int k = tid; k < d; k += blockDim.x) {
    uint64_t r[kMaxQ], mag[4];
    for (int l = 0; l < ns; ++l) r[l] = poly(l)[k];
    crt_centred(a.crt, ns, r, mag);
    uint64_t sq[kNormW];
    for (int i = 0; i < kNormW; ++i) sq[i] = 0;
    for (int i = 0; i < 4; ++i) {
      uint64_t carry = 0;
      for (int j = 0; j < 4; ++j) {
        uint64_t lo, hi;
        mul_wide(mag[i], mag[j], lo, hi);
        uint32_t c = 0;
        lo = addc(lo, sq[i + j], c);
        hi += c;
        c = 0;
        lo = addc(lo, carry, c);
        hi += c;
        sq[i + j] = lo;
        carry = hi;
      }
      sq[i + 4] += carry;
    }
    mw_add(acc, sq, kNormW);
  }
  __syncthreads();  // poly_lds is reused for the reduction
  for (int i = 0; i < kNormW; ++i) poly_lds[tid * kNormW + i] = acc[i];
  __syncthreads();
  for (int s = blockDim.x >> 1; s > 0; s >>= 1) {
    if (tid < s) mw_add(poly_lds + tid * kNormW, poly_lds + (tid + s) * kNormW, kNormW);
    __syncthreads();
  }
  if (tid < kNormW) a.out[pid * kNormW + tid] = poly_lds[tid];
}

// out[p][l][k] = A[p][l][k] * c_l - B[p][l][k] mod q_l  (A, B, out: [npoly][nl][d] contiguous)
__global__ __launch_bounds__(256) void combine_kernel(const uint64_t* A, const uint64_t* B, uint64_t* out,
                                                      long long n, int nl, int d, RingDev R, uint64_t c0,
                                                      uint64_t c1, uint64_t c2, uint64_t c3) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int l = (int)((i / d) % nl);
  const RnsPrime& P = R.p[l];
  const uint64_t c = l == 0 ? c0 : l == 1 ? c1 : l == 2 ? c2 : c3;
  const uint64_t cp = (uint64_t)(((unsigned __int128)c << 64) / P.q);
  out[i] = mod_sub(sh_mul(A[i], c, cp, P.q), B[i], P.q);
}

__global__ __launch_bounds__(256) void neq_kernel(const uint64_t* x, const uint64_t* y, long long n, int* flag) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && x[i] != y[i]) atomicOr(flag, 1);
}

template <int L>
struct DecodeArgs {
  int d, slots, exp, nout;
  RingDev R;
  CrtDev crt;
  FieldParams<L> F;
  uint64_t pw[4][L];  // 2^(64 i) R^2 mod p: montmul(w, pw[i]) = w 2^(64 i) R
  uint64_t bmont[L];  // base in Montgomery form
  const uint64_t* in;  // [npoly][R.n][d]
  uint64_t* out;       // [npoly][nout][L]
};

template <int L>
__global__ __launch_bounds__(256) void decode_kernel(DecodeArgs<L> a) {
  extern __shared__ uint64_t poly_lds[];  // R.n * d words, then d * L words of coefficients
  const int d = a.d, tid = threadIdx.x, ns = a.R.n;
  auto poly = [&](int l) { return poly_lds + (long long)l * d; };
  uint64_t* ce = poly_lds + (long long)ns * d;
  const long long pid = blockIdx.x;
  const uint64_t* in = a.in + pid * ns * d;
  for (int k = tid; k < ns * d; k += blockDim.x) {
    const int l = k / d;
    const RnsPrime& P = a.R.p[l];
    poly(l)[k % d] = sh_mul(in[k], P.rinv, P.rinv_sh, P.q);  // IMForm
  }
  __syncthreads();
  const int half = blockDim.x >> 1;
  for (int l0 = 0; l0 < ns; l0 += 2) {
    const int l = l0 + (tid >= half ? 1 : 0);
    const bool active = l < ns;
    const int lc = active ? l : l0;
    intt_lds(poly(lc), d, a.R.bwd + (long long)lc * d, a.R.p[lc], tid % half, half, active);
  }
  for (int k = tid; k < d; k += blockDim.x) {  // reconstructTo, then SetBigInt (mod p)
    uint64_t r[kMaxQ], mag[4];
    for (int l = 0; l < ns; ++l) r[l] = poly(l)[k];
    const bool neg = crt_centred(a.crt, ns, r, mag);
    uint64_t v[L], t[L], w[L];
#pragma unroll
    for (int i = 0; i < L; ++i) v[i] = 0;
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < L; ++j) w[j] = j == 0 ? mag[i] : 0;
      if (L == 1) w[0] = mag[i] % a.F.q[0];  // a word may exceed a one-limb p
      f_mul<L>(t, w, a.pw[i], a.F);
      f_add<L>(v, v, t, a.F);
    }
    if (neg) f_neg<L>(v, v, a.F);
    el_copy<L>(ce + (long long)k * L, v);
  }
  __syncthreads();
  for (int i = tid; i < a.nout; i += blockDim.x) {  // Horner over j = exp-1 .. 0
    uint64_t v[L];
#pragma unroll
    for (int j = 0; j < L; ++j) v[j] = 0;
    for (int j = a.exp - 1; j >= 0; --j) {
      f_mul<L>(v, v, a.bmont, a.F);
      f_add<L>(v, v, ce + (long long)(j * a.slots + i) * L, a.F);
    }
    el_copy<L>(a.out + (pid * a.nout + i) * L, v);
  }
}

// one workgroup: out[0] = sum_i x1[i] * y1[i] (n1 terms), out[1] = sum_i x2[i] * y2[i] (n2)
template <int L>
__global__ __launch_bounds__(256) void dot2_kernel(FieldParams<L> F, const uint64_t* x1, const uint64_t* y1,
                                                   long long n1, const uint64_t* x2, const uint64_t* y2, long long n2,
                                                   uint64_t* out) {
  __shared__ uint64_t red[256 * L];
  for (int which = 0; which < 2; ++which) {
    const uint64_t* x = which ? x2 : x1;
    const uint64_t* y = which ? y2 : y1;
    const long long n = which ? n2 : n1;
    uint64_t acc[L], t[L];
#pragma unroll
    for (int j = 0; j < L; ++j) acc[j] = 0;
    for (long long i = threadIdx.x; i < n; i += blockDim.x) {
      f_mul<L>(t, x + i * L, y + i * L, F);
      f_add<L>(acc, acc, t, F);
    }
    el_copy<L>(red + threadIdx.x * L, acc);
    __syncthreads();
    for (int s = blockDim.x >> 1; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) f_add<L>(red + threadIdx.x * L, red + threadIdx.x * L, red + (threadIdx.x + s) * L, F);
      __syncthreads();
    }
    if (threadIdx.x < L) out[which * L + threadIdx.x] = red[threadIdx.x];
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------
// A batch of proofs of one handle (rg_jindo_verify_multi_dev).  The kernels above take every
// proof's polynomials in one launch as they are; the commit-key MACs run on mac_kernel with a
// column per proof.  The products whose two operands both belong to the proof (MacArgs has no
// per-column stride for A) and the per-proof decisions are these:
//   pdot_kernel         thread per (proof, output, limb * d + coeff): a J = 1 dot product with a proof
//                       stride on both operands and on the optional addend
//   consistency_kernel  thread per (proof, limb * d + coeff): both sides of verifyConsistency, never
//                       stored; a difference ORs the proof's flag
//   dot2_multi_kernel   dot2_kernel with a workgroup per proof
//   verdict_kernel      wave per proof: the two norm sums against their thresholds, the evaluation
//                       sides, the consistency flag -> the proof's record
// In the first two blockIdx.y is the proof (RG_JINDO_VERIFY_MAX_PROOFS = the grid's y extent).
// ------------------------------------------------------------------------------------------
template <bool WIDE>
__device__ __forceinline__ uint64_t pdot(const uint64_t* A, long long a_term, const uint64_t* B, long long b_term,
                                         int T, const RnsPrime& P) {
  Acc<WIDE> acc;
  acc.zero();
#pragma unroll 4
  for (int t = 0; t < T; ++t) acc.mac(A[t * a_term], B[t * b_term]);
  return acc.reduce(P);
}

struct PDotArgs {
  int d, nl, T, nout;  // degree, limbs, terms, outputs per proof
  const uint64_t* A;   // term t of proof p at p * a_proof + t * a_term
  long long a_proof, a_term;
  const uint64_t* B;   // term t of output o of proof p at p * b_proof + o * b_out + t * b_term
  long long b_proof, b_out, b_term;
  const uint64_t* C;   // added after reduction (nullable): p * c_proof + o * c_out
  long long c_proof, c_out;
  uint64_t* out;       // [proof][nout][nl][d]
  RnsPrime P[kMaxQ];
};

template <bool WIDE>
__global__ __launch_bounds__(256) void pdot_kernel(PDotArgs a) {
  const uint32_t per_col = (uint32_t)(a.nl * a.d);
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (uint32_t)a.nout * per_col) return;
  const uint32_t o = i / per_col, lk = i % per_col;
  const long long p = blockIdx.y;
  const RnsPrime& P = a.P[lk / a.d];
  uint64_t r = pdot<WIDE>(a.A + p * a.a_proof + lk, a.a_term, a.B + p * a.b_proof + o * a.b_out + lk, a.b_term, a.T, P);
  if (a.C) r = mod_add(a.C[p * a.c_proof + o * a.c_out + lk], r, P.q);
  a.out[(p * a.nout + o) * per_col + lk] = r;
}

struct ConsArgs {
  int d, nl, rows, cols;
  const uint64_t *left, *enc;       // [proof][rows][nl][d]
  const uint64_t *chals, *partial;  // [proof][cols][nl][d], [proof][cols + 1][nl][d]
  int* flag;                        // [proof], zero on entry
  RnsPrime P[kMaxQ];
};

// sum_i left[i] * Encode[i] != sum_i chals[i] * Partial[i] + PartialMask at any (limb, coeff)
template <bool WIDE>
__global__ __launch_bounds__(256) void consistency_kernel(ConsArgs a) {
  const long long per_col = (long long)a.nl * a.d;
  const long long lk = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (lk >= per_col) return;
  const long long p = blockIdx.y;
  const RnsPrime& P = a.P[(int)(lk / a.d)];
  const long long e0 = p * a.rows * per_col + lk;
  const uint64_t* part = a.partial + p * (a.cols + 1) * per_col + lk;
  const uint64_t lhs = pdot<WIDE>(a.left + e0, per_col, a.enc + e0, per_col, a.rows, P);
  uint64_t rhs = pdot<WIDE>(a.chals + p * a.cols * per_col + lk, per_col, part, per_col, a.cols, P);
  rhs = mod_add(part[a.cols * per_col], rhs, P.q);
  if (lhs != rhs) atomicOr(a.flag + p, 1);
}

// dot2_kernel for workgroup = proof: operand k of proof p starts p * s_k elements in, out [proof][2][L]
template <int L>
__global__ __launch_bounds__(256) void dot2_multi_kernel(FieldParams<L> F, const uint64_t* x1, long long s_x1,
                                                         const uint64_t* y1, long long s_y1, long long n1,
                                                         const uint64_t* x2, const uint64_t* y2, long long n2,
                                                         uint64_t* out) {
  __shared__ uint64_t red[256 * L];
  const long long p = blockIdx.x;
  for (int which = 0; which < 2; ++which) {
    const uint64_t* x = which ? x2 + p * n2 * L : x1 + p * s_x1 * L;
    const uint64_t* y = which ? y2 + p * n2 * L : y1 + p * s_y1 * L;
    const long long n = which ? n2 : n1;
    uint64_t acc[L], t[L];
#pragma unroll
    for (int j = 0; j < L; ++j) acc[j] = 0;
    for (long long i = threadIdx.x; i < n; i += blockDim.x) {
      f_mul<L>(t, x + i * L, y + i * L, F);
      f_add<L>(acc, acc, t, F);
    }
    el_copy<L>(red + threadIdx.x * L, acc);
    __syncthreads();
    for (int s = blockDim.x >> 1; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) f_add<L>(red + threadIdx.x * L, red + threadIdx.x * L, red + (threadIdx.x + s) * L, F);
      __syncthreads();
    }
    if (threadIdx.x < L) out[(p * 2 + which) * L + threadIdx.x] = red[threadIdx.x];
    __syncthreads();
  }
}

// a norm bound as norm_threshold built it: always = 0: S < k2; -1: no sum is below; +1: every sum is
struct NormBound {
  uint64_t k2[kNormW];
  int always;
};

constexpr int kVerdictSegs = 5;  // norm rows of pf_incom, C_out | pf_enc, pf_mlwe, C_in
constexpr int kVerdictOuter = 2;
static_assert(RG_JINDO_VERIFY_WORDS == 2 + 2 * kNormW + 2 * 16, "ok, flags, two norm sums, two 16-word sides");

struct VerdictArgs {
  int L;
  const uint64_t* norms[kVerdictSegs];  // [proof][cnt][kNormW] each
  int cnt[kVerdictSegs];
  NormBound bound[2];                   // outer, inner
  const uint64_t* lhs;                  // eval sides: element of proof p at p * stride
  const uint64_t* rhs;
  long long lhs_stride, rhs_stride;
  const int* flag;                      // [proof] verifyConsistency's difference
  uint64_t* out;                        // [proof][RG_JINDO_VERIFY_WORDS]
};

__global__ __launch_bounds__(64) void verdict_kernel(VerdictArgs a) {
  __shared__ uint64_t red[64 * kNormW];
  __shared__ uint64_t sum[2][kNormW];
  __shared__ int pass[4];  // outer, inner, consistency, eval
  const int tid = threadIdx.x;
  const long long p = blockIdx.x;
  for (int which = 0; which < 2; ++which) {
    uint64_t acc[kNormW];
    for (int i = 0; i < kNormW; ++i) acc[i] = 0;
    for (int s = which ? kVerdictOuter : 0; s < (which ? kVerdictSegs : kVerdictOuter); ++s) {
      const uint64_t* rows = a.norms[s] + p * a.cnt[s] * kNormW;
      for (int r = tid; r < a.cnt[s]; r += 64) mw_add(acc, rows + (long long)r * kNormW, kNormW);
    }
    for (int i = 0; i < kNormW; ++i) red[tid * kNormW + i] = acc[i];
    __syncthreads();
    for (int s = 32; s > 0; s >>= 1) {
      if (tid < s) mw_add(red + tid * kNormW, red + (tid + s) * kNormW, kNormW);
      __syncthreads();
    }
    if (tid < kNormW) sum[which][tid] = red[tid];
    __syncthreads();
  }
  const uint64_t* lhs = a.lhs + p * a.lhs_stride;
  const uint64_t* rhs = a.rhs + p * a.rhs_stride;
  if (tid < 2) {  // S < K^2, from the top word down
    const NormBound& b = a.bound[tid];
    int below = b.always > 0;
    if (b.always == 0) {
      for (int w = kNormW - 1; w >= 0; --w) {
        if (sum[tid][w] != b.k2[w]) {
          below = sum[tid][w] < b.k2[w];
          break;
        }
      }
    }
    pass[tid] = below;
  } else if (tid == 2) {
    pass[2] = a.flag[p] == 0;
  } else if (tid == 3) {
    int eq = 1;
    for (int i = 0; i < a.L; ++i) eq &= lhs[i] == rhs[i];
    pass[3] = eq;
  }
  __syncthreads();
  if (tid >= RG_JINDO_VERIFY_WORDS) return;
  uint64_t w;
  if (tid == 0) {
    w = pass[0] & pass[1] & pass[2] & pass[3];
  } else if (tid == 1) {
    w = pass[0] | pass[1] << 1 | pass[2] << 2 | pass[3] << 3;
  } else if (tid < 2 + 2 * kNormW) {
    w = sum[(tid - 2) / kNormW][(tid - 2) % kNormW];
  } else {
    const int i = (tid - 2 - 2 * kNormW) % 16;
    const uint64_t* side = tid < 2 + 2 * kNormW + 16 ? lhs : rhs;
    w = i < a.L ? side[i] : 0;
  }
  a.out[p * RG_JINDO_VERIFY_WORDS + tid] = w;
}

// ------------------------------------------------------------------------------------------
// Prover.Evaluate core (prover.go:205-324): the MulCoeffsMontgomeryThenAdd loops, with the
// Fiat-Shamir challenges (batch, left, chals) injected by the caller.  Every loop is a
// per-(limb, coeff) dot product, so each maps onto mac_kernel with J = 1 and the loop's own
// strides.
// ------------------------------------------------------------------------------------------
// Prover.Evaluate's batch combination (prover.go:254-266): a J = 1 dot product over the batch's
// T commits, out[col][lk] = (sum_t A[t][lk] B[col][t][lk]) 2^-64 mod q, read once from HBM.
// T = batch is the long axis (512 at the configs[4] shard) and the column count is modest (the
// 144 InCommit / 432 MLWE polynomials), so mac_kernel's thread per (4 columns, lk) left too few
// waves in flight for the opening stream.  Here a 256-thread workgroup owns 64 lk x NC columns
// and its 4 waves split the terms (wave w: t = w, w + 4, ...), each term's loads unrolled x2;
// the four exact 128-bit partial sums are added through LDS, then reduced once.
constexpr int kDotNC = 4;
__global__ __launch_bounds__(256) void dot_split_kernel(MacArgs a) {
  __shared__ uint64_t red[3][kDotNC][2][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long per_col = (long long)a.nl * a.d;
  const long long nlkb = per_col / 64;
  const long long lk = (blockIdx.x % nlkb) * 64 + lane;
  const long long col0 = (blockIdx.x / nlkb) * kDotNC;
  const int nc = (int)min((long long)kDotNC, a.ncols - col0);
  const int T = a.T1;
  Acc<false> acc[kDotNC];
#pragma unroll
  for (int c = 0; c < kDotNC; ++c) acc[c].zero();
  const uint64_t* A = a.A1 + lk;
  const uint64_t* Bp = a.B1 + lk;
#pragma unroll 2
  for (int t = w; t < T; t += 4) {
    const uint64_t av = A[(long long)t * per_col];
    uint64_t bv[kDotNC];
#pragma unroll
    for (int c = 0; c < kDotNC; ++c) bv[c] = c < nc ? Bp[(col0 + c) * a.b1_col + t * a.b1_term] : 0;
#pragma unroll
    for (int c = 0; c < kDotNC; ++c) acc[c].mac(av, bv[c]);
  }
  if (w > 0) {
#pragma unroll
    for (int c = 0; c < kDotNC; ++c) {
      red[w - 1][c][0][lane] = acc[c].lo;
      red[w - 1][c][1][lane] = acc[c].hi;
    }
  }
  __syncthreads();
  if (w != 0) return;
  const RnsPrime& P = a.P[(int)(lk / a.d)];
#pragma unroll
  for (int c = 0; c < kDotNC; ++c) {
#pragma unroll
    for (int v = 0; v < 3; ++v) {  // exact: (lo, hi) += (lo', hi'), the sum stays below 2^128
      uint32_t cy = 0;
      acc[c].lo = addc(acc[c].lo, red[v][c][0][lane], cy);
      acc[c].hi += red[v][c][1][lane] + cy;
    }
    if (c < nc) a.out[(col0 + c) * per_col + lk] = acc[c].reduce(P);
  }
}

static rg_status launch_dot(const MacArgs& m, hipStream_t st) {
  uint64_t qmax = 0;
  for (int l = 0; l < m.nl; ++l) qmax = std::max(qmax, m.P[l].q);
  const bool narrow = 2.0 * log2((double)(qmax - 1)) + log2((double)m.T1 + 1.0) < 127.5;
  if (m.J != 1 || m.T2 != 0 || m.C || !narrow || (m.nl * m.d) % 64 != 0)
    return launch_mac(m, st);
  const long long blocks = (m.ncols + kDotNC - 1) / kDotNC * ((long long)m.nl * m.d / 64);
  hipLaunchKernelGGL(dot_split_kernel, dim3((unsigned)blocks), dim3(256), 0, st, m);
  return check_launch("jindo eval dot");
}

static rg_status eval_batch(const rg_jindo* J, size_t batch, const uint64_t* incom, const uint64_t* enc,
                            const uint64_t* mlwe, const uint64_t* bq, const uint64_t* bo, uint64_t* ob_incom,
                            uint64_t* ob_enc, uint64_t* ob_mlwe, hipStream_t st) {
  const rg_jindo_params& p = J->p;
  const long long pq = (long long)p.nq * p.d, po = (long long)p.nqo * p.d, nm = p.in_msis + p.mlwe;
  const long long n_inc = p.dcmp, n_enc = (long long)(p.cols + 1) * p.rows, n_ml = (long long)(p.cols + 1) * nm;
  if (!bq) {  // params.batch == 1: openBatch = open[0] (prover.go:267-269)
    RG_HIP(hipMemcpyAsync(ob_incom, incom, 8 * n_inc * po, hipMemcpyDeviceToDevice, st));
    RG_HIP(hipMemcpyAsync(ob_enc, enc, 8 * n_enc * pq, hipMemcpyDeviceToDevice, st));
    RG_HIP(hipMemcpyAsync(ob_mlwe, mlwe, 8 * n_ml * pq, hipMemcpyDeviceToDevice, st));
    return RG_OK;
  }
  const int T = (int)batch;  // term i = commit i, scaled by its batch challenge (:254-266)
  RG_TRY(launch_dot(dot_args(J->ro, p.nqo, p.d, n_inc, T, bo, incom, po, n_inc * po, ob_incom), st));
  RG_TRY(launch_dot(dot_args(J->rq, p.nq, p.d, n_enc, T, bq, enc, pq, n_enc * pq, ob_enc), st));
  RG_TRY(launch_dot(dot_args(J->rq, p.nq, p.d, n_ml, T, bq, mlwe, pq, n_ml * pq, ob_mlwe), st));
  return RG_OK;
}

// x mod q over limb-planar polynomials (Shoup by 1 reduces any 64-bit word): folds the
// cross-GPU sum of partial openBatches (each < q, at most 2^64 / q of them) back to residues
__global__ __launch_bounds__(256) void rns_reduce_kernel(uint64_t* x, long long npoly, int nl, int d, RingDev R) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npoly * nl * d) return;
  const RnsPrime& P = R.p[(int)((i / d) % nl)];
  x[i] = sh_mul(x[i], 1, P.one_sh, P.q);
}

// ------------------------------------------------------------------------------------------
// The inputs Evaluate and Verify derive from the transcript (jindo/utils.go:20-82):
//   encode_left_kernel  workgroup per row j of leftVec: one lane takes the element out of Montgomery
//                       form and expands its base-b digits into coefficients i * slots
//                       (Encoder.encode of a one-element vector, encoder.go:105-146: slot 0 of an
//                       otherwise empty row, every other coefficient zero), MForm, then the NTT per
//                       ring prime -- the commit path's digits_kernel + prep_kernel for that element
//                       without noise
//   encode_chal_kernel  workgroup per challenge: one lane takes exp remainders of the 128-bit value
//                       by ChallengeBound (divMod64, utils.go:12-18), signs them, MForm, NTT
// ------------------------------------------------------------------------------------------
// NTT per limb of poly [R.n][d] in LDS (two limbs at a time on the halves of the workgroup, as
// prep_kernel), then the store; the caller has synchronised after filling poly
__device__ inline void ntt_store(uint64_t* poly, const RingDev& R, int d, uint64_t* dst) {
  const int tid = threadIdx.x, half = blockDim.x >> 1;
  for (int l0 = 0; l0 < R.n; l0 += 2) {
    const int l = l0 + (tid >= half ? 1 : 0);
    const bool active = l < R.n;
    const int lc = active ? l : l0;
    ntt_lds(poly + (long long)lc * d, d, R.fwd + (long long)lc * d, R.p[lc].q, tid % half, half, active);
  }
  for (int k = tid; k < R.n * d; k += blockDim.x) dst[k] = poly[k];
}

template <int L>
struct PointArgs {
  int d, slots, exp, rows;
  RingDev R;
  FieldParams<L> F;
  uint64_t base, base_inv;  // b and floor(2^64 / b)
  DigitDc dc;               // digits_dc.hpp constants; dc.exp != exp: the division loop
  const uint64_t* lp;       // [rows][L] skip^j
  const uint64_t* x;        // the point: left[rows - 1]
  uint64_t* out;            // [rows][R.n][d]
};

template <int L>
__global__ __launch_bounds__(256) void encode_left_kernel(PointArgs<L> a) {
  extern __shared__ uint64_t poly_lds[];
  const int d = a.d, tid = threadIdx.x, nl = a.R.n, row = blockIdx.x;
  for (int k = tid; k < nl * d; k += blockDim.x) poly_lds[k] = 0;
  __syncthreads();
  if (tid == 0) {
    // left[rows - 1] = x is written last (utils.go:70), also when skip^(rows-1) was there
    const uint64_t* e = row == a.rows - 1 ? a.x : a.lp + (long long)row * L;
    uint64_t xv[L], c[L];
    el_copy<L>(xv, e);
    f_redc<L>(c, xv, a.F);  // Slice = fromMont
    auto put = [&](int j, uint32_t dg) {  // MForm(digit) at coefficient j * slots (digit < 2^32 <= any word)
      for (int l = 0; l < nl; ++l) {
        const RnsPrime& P = a.R.p[l];
        poly_lds[(long long)l * d + j * a.slots] = sh_mul(dg, P.r64, P.r64_sh, P.q);
      }
    };
    bool done = false;
    if constexpr (L == 4 || L == 2) {
      if (a.dc.exp == a.exp) {
        dc_digits<L>(c, a.dc, put);
        done = true;
      }
    }
    if (!done) {  // exp - 1 remainders, then the last quotient (encoder.go:125-136)
      uint32_t w[2 * L];
#pragma unroll
      for (int l = 0; l < L; ++l) {
        w[2 * l] = (uint32_t)c[l];
        w[2 * l + 1] = (uint32_t)(c[l] >> 32);
      }
      for (int jd = 0; jd < a.exp - 1; ++jd) {
        uint64_t rem = 0;
        for (int k = 2 * L - 1; k >= 0; --k) w[k] = divstep((rem << 32) | w[k], a.base, a.base_inv, rem);
        put(jd, (uint32_t)rem);
      }
      put(a.exp - 1, w[0]);
    }
  }
  __syncthreads();
  ntt_store(poly_lds, a.R, d, a.out + (long long)row * nl * d);
}

struct ChalArgs {
  int d, slots, exp;
  RingDev R;
  uint64_t bound, bound_inv;  // ChallengeBound >= 1 and floor(2^64 / bound) (unused when bound = 1)
  const uint8_t* bytes;       // [n][16]
  uint64_t* out;              // [n][R.n][d]
};

__global__ __launch_bounds__(256) void encode_chal_kernel(ChalArgs a) {
  extern __shared__ uint64_t poly_lds[];
  const int d = a.d, tid = threadIdx.x, nl = a.R.n;
  for (int k = tid; k < nl * d; k += blockDim.x) poly_lds[k] = 0;
  __syncthreads();
  if (tid == 0 && a.bound > 1) {  // bound = 1: every remainder is 0 (utils.go:31-32)
    chal_digits(a.bytes + (long long)blockIdx.x * 16, a.bound, a.bound_inv, a.exp, [&](int i, uint64_t r, bool neg) {
      for (int l = 0; l < nl; ++l) {
        const RnsPrime& P = a.R.p[l];
        const uint64_t v = neg ? P.q - (a.bound - r) : r;
        poly_lds[(long long)l * d + i * a.slots] = sh_mul(v, P.r64, P.r64_sh, P.q);  // MForm
      }
    });
  }
  __syncthreads();
  ntt_store(poly_lds, a.R, d, a.out + (long long)blockIdx.x * nl * d);
}

// leftVec's powers live in the stream's scratch: x^0 .. x^(cols slots), then skip^0 .. skip^(rows-1)
static rg_status point_scratch(rg_jindo* J, hipStream_t st, uint64_t** out) {
  const rg_jindo_params& p = J->p;
  std::lock_guard<std::mutex> lk(J->mu);
  std::unique_ptr<rg_jindo_scratch>& S = J->scratch[st];
  if (!S) S.reset(new rg_jindo_scratch());
  RG_TRY(S->point.alloc(((size_t)p.cols * p.slots + 1 + p.rows) * p.field_limbs * 8));
  *out = S->point.as<uint64_t>();
  return RG_OK;
}

template <int L>
static rg_status launch_encode_left(const rg_jindo* J, const uint64_t* lp, const uint64_t* x, uint64_t* out,
                                    hipStream_t st) {
  const rg_jindo_params& p = J->p;
  PointArgs<L> a;
  memset(&a, 0, sizeof(a));
  a.d = p.d;
  a.slots = p.slots;
  a.exp = p.exp;
  a.rows = p.rows;
  a.R = ring_dev(J->rq, p.nq, J->rootsq_f, J->rootsq_b);
  a.F = field_params<L>(&J->field);
  a.base = p.base;
  a.base_inv = J->base_inv;
  a.dc = dc_constants((uint64_t)p.base, p.exp, L, field_bits(J->field));
  a.lp = lp;
  a.x = x;
  a.out = out;
  hipLaunchKernelGGL(encode_left_kernel<L>, dim3((unsigned)p.rows), dim3(256), (size_t)p.nq * p.d * 8, st, a);
  return check_launch("jindo encode left");
}

// ------------------------------------------------------------------------------------------
// The evaluation points of a batch of proofs (rg_jindo_eval_point_multi_dev): encode_left_kernel's
// work on a (rows, point) grid, point blockIdx.y at x + blockIdx.y * x_stride words.
//   point_powers_kernel       lane per element: leftVec[j] = x^(j cols slots) for j < rows - 1 by square and
//                             multiply (at most 2 log2(rank) dependent products, every lane busy), x itself
//                             for row rows - 1, and kRightPer successive powers of rightVec per further
//                             lane.  Montgomery products are fully reduced, so the words are those of the
//                             single entry's running-product tables.
//   encode_left_multi_kernel  encode_left_kernel with the element read from that table
// Measured against the single entry's two power tables per point (rg_buckler_powers_batch_dev twice
// and a strided copy: four stream items, each table 2 (log2 + 16) products deep) and against raising
// x in the encoding workgroups' one busy lane: profiles/jverify_inputs_timing.txt,
// tools/experiments/jindo_point_pow_arms.patch.
// ------------------------------------------------------------------------------------------
constexpr int kRightPer = 4;

// p = c^e
template <int L>
__device__ __forceinline__ void f_pow(uint64_t* p, const uint64_t* c, unsigned long long e, const uint64_t* one,
                                      const FieldParams<L>& F) {
  uint64_t sq[L];
  el_copy<L>(p, one);
  el_copy<L>(sq, c);
  for (; e; e >>= 1) {
    if (e & 1) f_mul<L>(p, p, sq, F);
    if (e > 1) f_mul<L>(sq, sq, sq, F);
  }
}

template <int L>
struct PointPowArgs {
  int rows;
  long long cs;        // cols * slots: rightVec's length, and skip = x^cs
  FieldParams<L> F;
  Elem<L> one;         // Montgomery 1
  const uint64_t* x;   // point k at x + k * x_stride
  long long x_stride;  // in words
  uint64_t* lp;        // [point][rows][L] leftVec
  uint64_t* right;     // [point][cs][L] rightVec, or nullptr: not written
};

template <int L>
__global__ __launch_bounds__(256) void point_powers_kernel(PointPowArgs<L> a) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x, pt = blockIdx.y;
  uint64_t cv[L], p[L];
  el_copy<L>(cv, a.x + pt * a.x_stride);
  if (t < a.rows) {  // leftVec (utils.go:63-72); left[rows - 1] = x is written last, also when rows == 1
    if (t == a.rows - 1)
      el_copy<L>(p, cv);
    else
      f_pow<L>(p, cv, (unsigned long long)t * (unsigned long long)a.cs, a.one.v, a.F);
    el_copy<L>(a.lp + (pt * a.rows + t) * L, p);
    return;
  }
  // rightVec (utils.go:75-82): right[i] = x^i
  const long long e0 = (t - a.rows) * kRightPer;
  if (!a.right || e0 >= a.cs) return;
  f_pow<L>(p, cv, (unsigned long long)e0, a.one.v, a.F);
  const long long e1 = min(a.cs, e0 + kRightPer);
  uint64_t* right = a.right + pt * a.cs * L;
  for (long long e = e0; e < e1; ++e) {
    el_copy<L>(right + e * L, p);
    if (e + 1 < e1) f_mul<L>(p, p, cv, a.F);
  }
}

// workgroup (row, point) of PointArgs with lp [point][rows][L] and out [point][rows][R.n][d]; a.x is unused
template <int L>
__global__ __launch_bounds__(256) void encode_left_multi_kernel(PointArgs<L> a) {
  extern __shared__ uint64_t poly_lds[];
  const int d = a.d, tid = threadIdx.x, nl = a.R.n;
  const long long el = (long long)blockIdx.y * a.rows + blockIdx.x;
  for (int k = tid; k < nl * d; k += blockDim.x) poly_lds[k] = 0;
  __syncthreads();
  if (tid == 0) {
    uint64_t xv[L], c[L];
    el_copy<L>(xv, a.lp + el * L);
    f_redc<L>(c, xv, a.F);  // Slice = fromMont
    auto put = [&](int j, uint32_t dg) {  // MForm(digit) at coefficient j * slots (digit < 2^32 <= any word)
      for (int l = 0; l < nl; ++l) {
        const RnsPrime& P = a.R.p[l];
        poly_lds[(long long)l * d + j * a.slots] = sh_mul(dg, P.r64, P.r64_sh, P.q);
      }
    };
    bool done = false;
    if constexpr (L == 4 || L == 2) {
      if (a.dc.exp == a.exp) {
        dc_digits<L>(c, a.dc, put);
        done = true;
      }
    }
    if (!done) {  // exp - 1 remainders, then the last quotient (encoder.go:125-136)
      uint32_t w[2 * L];
#pragma unroll
      for (int l = 0; l < L; ++l) {
        w[2 * l] = (uint32_t)c[l];
        w[2 * l + 1] = (uint32_t)(c[l] >> 32);
      }
      for (int jd = 0; jd < a.exp - 1; ++jd) {
        uint64_t rem = 0;
        for (int k = 2 * L - 1; k >= 0; --k) w[k] = divstep((rem << 32) | w[k], a.base, a.base_inv, rem);
        put(jd, (uint32_t)rem);
      }
      put(a.exp - 1, w[0]);
    }
  }
  __syncthreads();
  ntt_store(poly_lds, a.R, d, a.out + el * nl * d);
}

// The scratch of rg_jindo_eval_point_multi_dev in words: leftVec of every point, [N][rows][L]
static size_t point_multi_words(const rg_jindo_params& p, size_t N) {
  return N * (size_t)p.rows * p.field_limbs;
}

// the point pass of both batch entries, arguments checked by the caller: two launches
template <int L>
static rg_status point_multi_L(const rg_jindo* J, size_t N, const uint64_t* x, size_t x_stride, uint64_t* left,
                               uint64_t* right, uint64_t* lp, hipStream_t st) {
  const rg_jindo_params& p = J->p;
  PointPowArgs<L> w;
  memset(&w, 0, sizeof(w));
  w.rows = p.rows;
  w.cs = (long long)p.cols * p.slots;
  w.F = field_params<L>(&J->field);
  w.one = elem<L>(J->field.one);
  w.x = x;
  w.x_stride = (long long)(x_stride * L);
  w.lp = lp;
  w.right = right;
  const long long lanes = p.rows + (right ? (w.cs + kRightPer - 1) / kRightPer : 0);
  hipLaunchKernelGGL(point_powers_kernel<L>, dim3(grid256(lanes), (unsigned)N), dim3(256), 0, st, w);
  RG_TRY(check_launch("jindo point powers"));
  PointArgs<L> a;
  memset(&a, 0, sizeof(a));
  a.d = p.d;
  a.slots = p.slots;
  a.exp = p.exp;
  a.rows = p.rows;
  a.R = ring_dev(J->rq, p.nq, J->rootsq_f, J->rootsq_b);
  a.F = w.F;
  a.base = p.base;
  a.base_inv = J->base_inv;
  a.dc = dc_constants((uint64_t)p.base, p.exp, L, field_bits(J->field));
  a.lp = lp;
  a.out = left;
  hipLaunchKernelGGL(encode_left_multi_kernel<L>, dim3((unsigned)p.rows, (unsigned)N), dim3(256),
                     (size_t)p.nq * p.d * 8, st, a);
  return check_launch("jindo encode left multi");
}

static rg_status point_multi(const rg_jindo* J, size_t N, const uint64_t* x, size_t x_stride, uint64_t* left,
                             uint64_t* right, uint64_t* scratch, hipStream_t st) {
  return dispatch_limbs(J->p.field_limbs,
                        [&](auto Lc) { return point_multi_L<Lc()>(J, N, x, x_stride, left, right, scratch, st); });
}

}  // namespace rg

using namespace rg;

// ---- Verifier.Verify (verifier.go:50-282) ----------------------------------------------------
// nmTest < nm with nmTest = Float64(isqrt(S)) (verifyNorm :278-281), decided exactly: the test is
// S < K^2 with K the smallest integer whose float64 is >= nm (ceil(nm) up to 2^53; above, the
// midpoint below nm, + 1 when nm's mantissa is odd, as ties round to even).
// K^2 of the bound nm as 2 kNormW words, for both entries: the single one compares on the host
// (norm_below), the batch one hands the low half to verdict_kernel.  Returns 0 when the test is
// S < K2; -1 when !(nm > 0), no sum is below; +1 when K^2 does not fit the sum's 640 bits, every
// sum is below (K2 is then unspecified).
static int norm_threshold(double nm, uint64_t K2[2 * kNormW]) {
  constexpr int NW = kNormW;
  if (!(nm > 0)) return -1;
  uint64_t K[NW] = {0};
  memset(K2, 0, 2 * NW * sizeof(uint64_t));
  int e;
  const double fr = frexp(nm, &e);
  const uint64_t M = (uint64_t)ldexp(fr, 53);
  const int E = e - 53;
  if (E <= 0) {
    const double c = ceil(nm);
    if (c >= 18446744073709551616.0) return 1;
    K[0] = (uint64_t)c;
  } else {
    if (E / 64 >= NW) return 1;
    const int sub_e = (M == (1ull << 52)) ? E - 2 : E - 1;  // half the gap to the double below
    K[E / 64] = M << (E % 64);
    if (E % 64 && E / 64 + 1 < NW) K[E / 64 + 1] = M >> (64 - E % 64);
    uint64_t h[NW] = {0};
    if (sub_e >= 0) h[sub_e / 64] = 1ull << (sub_e % 64);
    HostField::sub_n(K, K, h, NW);
    if (M & 1)
      for (int k = 0; k < NW; ++k)
        if (++K[k]) break;
  }
  for (int a = 0; a < NW; ++a) {
    uint64_t c = 0;
    for (int b = 0; b < NW; ++b) {
      const unsigned __int128 t = (unsigned __int128)K[a] * K[b] + K2[a + b] + c;
      K2[a + b] = (uint64_t)t;
      c = (uint64_t)(t >> 64);
    }
    K2[a + NW] += c;
  }
  for (int w = 2 * NW - 1; w >= NW; --w)
    if (K2[w]) return 1;
  return 0;
}

static bool norm_below(const uint64_t* S, double nm) {
  uint64_t K2[2 * kNormW];
  const int always = norm_threshold(nm, K2);
  if (always) return always > 0;
  for (int w = kNormW - 1; w >= 0; --w)
    if (S[w] != K2[w]) return S[w] < K2[w];
  return false;
}

template <int L>
static rg_status launch_decode(const rg_jindo* J, const uint64_t* in, long long npoly, int nout, uint64_t* out,
                               hipStream_t st) {
  if (npoly == 0) return RG_OK;
  const rg_jindo_params& p = J->p;
  DecodeArgs<L> a;
  memset(&a, 0, sizeof(a));
  a.d = p.d;
  a.slots = p.slots;
  a.exp = p.exp;
  a.nout = nout;
  a.R = ring_dev(J->rq, p.nq, J->rootsq_f, J->rootsq_b);
  a.crt = J->crt_q;
  a.F = field_params<L>(&J->field);
  const HostField H(&J->field);
  uint64_t t32[16], t64[16];
  H.from_u64(t32, 1ull << 32);
  H.mul(t64, t32, t32);  // Montgomery form of 2^64
  memcpy(a.pw[0], J->field.r2, 8 * L);
  for (int i = 1; i < 4; ++i) H.mul(a.pw[i], a.pw[i - 1], t64);
  H.from_u64(a.bmont, p.base);
  a.in = in;
  a.out = out;
  const size_t lds = ((size_t)p.nq * p.d + (size_t)p.d * L) * 8;
  hipLaunchKernelGGL(decode_kernel<L>, dim3((unsigned)npoly), dim3(256), lds, st, a);
  return check_launch("jindo decode");
}

template <int L>
static rg_status launch_dot2(const rg_jindo* J, const uint64_t* x1, const uint64_t* y1, long long n1,
                             const uint64_t* x2, const uint64_t* y2, long long n2, uint64_t* out, hipStream_t st) {
  hipLaunchKernelGGL(dot2_kernel<L>, dim3(1), dim3(256), 0, st, field_params<L>(&J->field), x1, y1, n1, x2, y2, n2,
                     out);
  return check_launch("jindo dot");
}

static rg_status decode_any(const rg_jindo* J, const uint64_t* in, long long npoly, int nout, uint64_t* out,
                            hipStream_t st) {
  return dispatch_limbs(J->p.field_limbs, [&](auto Lc) { return launch_decode<Lc()>(J, in, npoly, nout, out, st); });
}
static rg_status dot2_any(const rg_jindo* J, const uint64_t* x1, const uint64_t* y1, long long n1, const uint64_t* x2,
                          const uint64_t* y2, long long n2, uint64_t* out, hipStream_t st) {
  return dispatch_limbs(J->p.field_limbs,
                        [&](auto Lc) { return launch_dot2<Lc()>(J, x1, y1, n1, x2, y2, n2, out, st); });
}

static rg_status launch_norm(const rg_jindo* J, bool outer, const uint64_t* in, long long npoly, long long stride,
                             uint64_t* out, hipStream_t st) {
  if (npoly == 0) return RG_OK;
  const rg_jindo_params& p = J->p;
  NormArgs a;
  memset(&a, 0, sizeof(a));
  a.d = p.d;
  a.R = outer ? ring_dev(J->ro, p.nqo, J->rootso_f, J->rootso_b) : ring_dev(J->rq, p.nq, J->rootsq_f, J->rootsq_b);
  a.crt = outer ? J->crt_o : J->crt_q;
  a.in = in;
  a.in_stride = stride;
  a.out = out;
  const size_t lds = std::max((size_t)a.R.n * p.d, (size_t)256 * kNormW) * 8;
  hipLaunchKernelGGL(norm_kernel, dim3((unsigned)npoly), dim3(256), lds, st, a);
  return check_launch("jindo norm");
}

static rg_status launch_combine(const RnsPrime* P, int nl, int d, int cut, const uint64_t* A, const uint64_t* B,
                                uint64_t* out, long long npoly, hipStream_t st) {
  uint64_t c[4] = {0, 0, 0, 0};
  RingDev R;
  memset(&R, 0, sizeof(R));
  R.n = nl;
  for (int l = 0; l < nl; ++l) {
    R.p[l] = P[l];
    unsigned __int128 x = 1;
    for (int i = 0; i < cut; ++i) x = (x * 2) % P[l].q;  // 2^cut mod q
    c[l] = (uint64_t)x;
  }
  const long long n = npoly * nl * d;
  hipLaunchKernelGGL(combine_kernel, dim3(grid256(n)), dim3(256), 0, st, A, B, out, n, nl, d, R, c[0],
                     c[1], c[2], c[3]);
  return check_launch("jindo combine");
}

extern "C" {

rg_status rg_jindo_eval_batch_dev(const rg_jindo* J, size_t batch, const uint64_t* d_incom, const uint64_t* d_enc,
                                  const uint64_t* d_mlwe, const uint64_t* d_bq, const uint64_t* d_bo,
                                  uint64_t* d_ob_incom, uint64_t* d_ob_enc, uint64_t* d_ob_mlwe, void* stream) {
  if (!J || batch == 0 || !d_incom || !d_enc || !d_mlwe || !d_ob_incom || !d_ob_enc || !d_ob_mlwe ||
      (!d_bq != !d_bo) || (!d_bq && batch != 1))
    return RG_ERR_INVALID;
  return eval_batch(J, batch, d_incom, d_enc, d_mlwe, d_bq, d_bo, d_ob_incom, d_ob_enc, d_ob_mlwe, as_stream(stream));
}

rg_status rg_jindo_eval_partial_dev(const rg_jindo* J, const uint64_t* d_ob_enc, const uint64_t* d_left,
                                    uint64_t* d_partial, void* stream) {
  if (!J || !d_ob_enc || !d_left || !d_partial) return RG_ERR_INVALID;
  const rg_jindo_params& p = J->p;
  const long long pq = (long long)p.nq * p.d;
  // out i in [0, cols]: sum_j left[j] * Enc[i][j] (prover.go:274-282); i = cols is PartialMask
  return launch_mac(dot_args(J->rq, p.nq, p.d, p.cols + 1, p.rows, d_left, d_ob_enc, (long long)p.rows * pq, pq,
                             d_partial),
                    as_stream(stream));
}

rg_status rg_jindo_eval_respond_dev(const rg_jindo* J, const uint64_t* d_ob_enc, const uint64_t* d_ob_mlwe,
                                    const uint64_t* d_chals, uint64_t* d_pf_enc, uint64_t* d_pf_mlwe, void* stream) {
  if (!J || !d_ob_enc || !d_ob_mlwe || !d_chals || !d_pf_enc || !d_pf_mlwe) return RG_ERR_INVALID;
  const rg_jindo_params& p = J->p;
  const long long pq = (long long)p.nq * p.d, nm = p.in_msis + p.mlwe;
  hipStream_t st = as_stream(stream);
  // pf.Encode[i] = Enc[cols][i] + sum_j chals[j] * Enc[j][i] (prover.go:300-306)
  MacArgs e = dot_args(J->rq, p.nq, p.d, p.rows, p.cols, d_chals, d_ob_enc, pq, (long long)p.rows * pq, d_pf_enc);
  e.C = d_ob_enc + (long long)p.cols * p.rows * pq;
  e.c_col = pq;
  RG_TRY(launch_mac(e, st));
  // pf.MLWE[i] = MLWE[cols][i] + sum_j chals[j] * MLWE[j][i] (:308-314)
  MacArgs m = dot_args(J->rq, p.nq, p.d, nm, p.cols, d_chals, d_ob_mlwe, pq, nm * pq, d_pf_mlwe);
  m.C = d_ob_mlwe + (long long)p.cols * nm * pq;
  m.c_col = pq;
  return launch_mac(m, st);
}

rg_status rg_jindo_verify_dev(const rg_jindo* J, size_t batch, const uint64_t* d_com, const uint64_t* d_bq,
                              const uint64_t* d_bo, const uint64_t* d_chals, const uint64_t* d_left,
                              const uint64_t* d_right, const uint64_t* d_y, const uint64_t* d_pf_incom,
                              const uint64_t* d_pf_partial, const uint64_t* d_pf_enc, const uint64_t* d_pf_mlwe,
                              double in_com_dcmp_two_nm, double res_two_nm, rg_jindo_verify_result* res,
                              void* stream) {
  if (!J || !res || !d_com || !d_chals || !d_left || !d_right || !d_y || !d_pf_incom || !d_pf_partial || !d_pf_enc ||
      !d_pf_mlwe)
    return RG_ERR_INVALID;
  if (batch < 1 || (batch > 1 && (!d_bq || !d_bo))) return RG_ERR_INVALID;
  RG_TRY(on_device(J));
  const rg_jindo_params& p = J->p;
  const int d = p.d, nq = p.nq, nqo = p.nqo, L = p.field_limbs;
  const long long pq = (long long)nq * d, po = (long long)nqo * d, nm = p.in_msis + p.mlwe;
  hipStream_t st = as_stream(stream);
  const long long n_out = p.dcmp + p.out_msis, n_in = p.rows + nm + p.in_msis;
  DevBuf a_out, b_out, c_out, lift, a_in, b_in, c_in, p1, p2, norms, flag, dcd, bd, ev;
  const size_t b_outer = sizes_of(p, 1).outer;  // one commit's outer commitment in ringQOut
  RG_TRY(a_out.alloc(b_outer));
  RG_TRY(b_out.alloc(b_outer));
  RG_TRY(c_out.alloc(b_outer));
  RG_TRY(lift.alloc(8 * p.dcmp * pq));
  RG_TRY(a_in.alloc(8 * p.in_msis * pq));
  RG_TRY(b_in.alloc(8 * p.in_msis * pq));
  RG_TRY(c_in.alloc(8 * p.in_msis * pq));
  RG_TRY(p1.alloc(8 * pq));
  RG_TRY(p2.alloc(8 * pq));
  RG_TRY(norms.alloc(8 * (n_out + n_in) * kNormW));
  RG_TRY(flag.alloc(sizeof(int)));
  RG_TRY(dcd.alloc(8 * (size_t)p.cols * p.slots * L));
  RG_TRY(bd.alloc(8 * (size_t)batch * L));
  RG_TRY(ev.alloc(8 * 2 * (size_t)L));
  uint64_t* nrm = norms.as<uint64_t>();
  // verifyOuterCommitment (:136-161): A = sum_j com[j][i] * batchOut[j] (or com[0][i]),
  // C = A * 2^logOutCut - sum_j Out[i][j] * Proof.InCommit[j]
  if (batch > 1) {
    MacArgs m = dot_args(J->ro, nqo, d, p.out_msis, (int)batch, d_bo, d_com, pq, (long long)p.out_msis * pq,
                         a_out.as<uint64_t>());
    RG_TRY(launch_mac(m, st));
  } else {
    RG_HIP(hipMemcpy2DAsync(a_out.p, 8 * po, d_com, 8 * pq, 8 * po, p.out_msis, hipMemcpyDeviceToDevice, st));
  }
  {
    MacArgs m = dot_args(J->ro, nqo, d, 1, p.dcmp, J->ck_out.as<uint64_t>(), d_pf_incom, 0, po, b_out.as<uint64_t>());
    m.J = p.out_msis;
    RG_TRY(launch_mac(m, st));
  }
  RG_TRY(launch_combine(J->ro, nqo, d, p.log_out_cut, a_out.as<uint64_t>(), b_out.as<uint64_t>(), c_out.as<uint64_t>(),
                        p.out_msis, st));
  RG_TRY(launch_norm(J, true, d_pf_incom, p.dcmp, po, nrm, st));
  RG_TRY(launch_norm(J, true, c_out.as<uint64_t>(), p.out_msis, po, nrm + p.dcmp * kNormW, st));
  // verifyInnerCommitment (:164-200): lift = MForm(NTT(ModUpQtoP(pfInv.InCommit))) (centred),
  // A = sum_{j<cols} lift[j in_msis + i] * chals[j] + lift[cols in_msis + i],
  // C = A * 2^logInCut - (sum In[i][j] * Encode[j] + sum MLWE_ck[i][j] * MLWE[j] + MLWE[mlwe + i])
  RG_TRY(launch_round(round_args(J, true, false, 0, d_pf_incom, lift.as<uint64_t>(), pq, nq), p.dcmp, st));
  {
    MacArgs m = dot_args(J->rq, nq, d, p.in_msis, p.cols, d_chals, lift.as<uint64_t>(), pq, (long long)p.in_msis * pq,
                         a_in.as<uint64_t>());
    m.C = lift.as<uint64_t>() + (long long)p.cols * p.in_msis * pq;
    m.c_col = pq;
    RG_TRY(launch_mac(m, st));
  }
  {
    MacArgs m = dot_args(J->rq, nq, d, 1, p.rows, J->ck_in.as<uint64_t>(), d_pf_enc, 0, pq, b_in.as<uint64_t>());
    m.J = p.in_msis;
    m.T2 = p.mlwe;
    m.A2 = J->ck_mlwe.as<uint64_t>();
    m.B2 = d_pf_mlwe;
    m.b2_term = pq;
    m.C = d_pf_mlwe + (long long)p.mlwe * pq;
    m.c_j = pq;
    RG_TRY(launch_mac(m, st));
  }
  RG_TRY(launch_combine(J->rq, nq, d, p.log_in_cut, a_in.as<uint64_t>(), b_in.as<uint64_t>(), c_in.as<uint64_t>(),
                        p.in_msis, st));
  uint64_t* nin = nrm + n_out * kNormW;
  RG_TRY(launch_norm(J, false, d_pf_enc, p.rows, pq, nin, st));
  RG_TRY(launch_norm(J, false, d_pf_mlwe, nm, pq, nin + p.rows * kNormW, st));
  RG_TRY(launch_norm(J, false, c_in.as<uint64_t>(), p.in_msis, pq, nin + (p.rows + nm) * kNormW, st));
  // verifyConsistency (:203-221): sum left[i] * Encode[i] == sum chals[i] * Partial[i] + PartialMask
  RG_TRY(launch_mac(dot_args(J->rq, nq, d, 1, p.rows, d_left, d_pf_enc, 0, pq, p1.as<uint64_t>()), st));
  {
    MacArgs m = dot_args(J->rq, nq, d, 1, p.cols, d_chals, d_pf_partial, 0, pq, p2.as<uint64_t>());
    m.C = d_pf_partial + (long long)p.cols * pq;
    RG_TRY(launch_mac(m, st));
  }
  RG_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), st));
  hipLaunchKernelGGL(neq_kernel, dim3(grid256(pq)), dim3(256), 0, st, p1.as<uint64_t>(),
                     p2.as<uint64_t>(), pq, flag.as<int>());
  RG_TRY(check_launch("jindo consistency"));
  // verifyEval (:224-259): sum_{i,j} right[i slots + j] * Decode(pfInv.Partial[i])[j] ==
  // sum_i Decode(INTT(IMForm(batch[i])))[0] * y[i]  (or y[0])
  RG_TRY(decode_any(J, d_pf_partial, p.cols, p.slots, dcd.as<uint64_t>(), st));
  const uint64_t* yb = d_y;
  if (batch > 1) {
    RG_TRY(decode_any(J, d_bq, (long long)batch, 1, bd.as<uint64_t>(), st));
    yb = bd.as<uint64_t>();
  }
  RG_TRY(dot2_any(J, d_right, dcd.as<uint64_t>(), (long long)p.cols * p.slots, yb, d_y, batch > 1 ? (long long)batch : 0,
                  ev.as<uint64_t>(), st));
  // results to the host
  std::vector<uint64_t> hn((size_t)(n_out + n_in) * kNormW), he(2 * L);
  int hf = 0;
  RG_HIP(hipMemcpyAsync(hn.data(), nrm, hn.size() * 8, hipMemcpyDeviceToHost, st));
  RG_HIP(hipMemcpyAsync(he.data(), ev.p, he.size() * 8, hipMemcpyDeviceToHost, st));
  RG_HIP(hipMemcpyAsync(&hf, flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
  RG_HIP(hipStreamSynchronize(st));
  memset(res, 0, sizeof(*res));
  for (long long i = 0; i < n_out; ++i) {
    uint32_t c = 0;
    for (int w = 0; w < kNormW; ++w) {
      const unsigned __int128 t = (unsigned __int128)res->outer_norm_sq[w] + hn[i * kNormW + w] + c;
      res->outer_norm_sq[w] = (uint64_t)t;
      c = (uint32_t)(t >> 64);
    }
  }
  for (long long i = n_out; i < n_out + n_in; ++i) {
    uint32_t c = 0;
    for (int w = 0; w < kNormW; ++w) {
      const unsigned __int128 t = (unsigned __int128)res->inner_norm_sq[w] + hn[i * kNormW + w] + c;
      res->inner_norm_sq[w] = (uint64_t)t;
      c = (uint32_t)(t >> 64);
    }
  }
  res->outer_ok = norm_below(res->outer_norm_sq, in_com_dcmp_two_nm);
  res->inner_ok = norm_below(res->inner_norm_sq, res_two_nm);
  res->consistency_ok = hf == 0;
  memcpy(res->eval_lhs, he.data(), 8 * L);
  if (batch > 1) {
    memcpy(res->eval_rhs, he.data() + L, 8 * L);
  } else {
    RG_HIP(hipMemcpy(res->eval_rhs, d_y, 8 * L, hipMemcpyDeviceToHost));
  }
  res->eval_ok = memcmp(res->eval_lhs, res->eval_rhs, 8 * L) == 0;
  res->ok = res->outer_ok && res->inner_ok && res->consistency_ok && res->eval_ok;
  return RG_OK;
}

}  // extern "C"

// ---- n_proofs proofs of one handle in one call -------------------------------------------------
static rg_status jvm_invalid(const std::string& why) {
  set_last_error("jindo verify multi: " + why);
  return RG_ERR_INVALID;
}

// launch_mac's accumulator choice for `terms` products below qmax^2
static bool acc_wide(const RnsPrime* P, int nl, int terms) {
  uint64_t qmax = 0;
  for (int l = 0; l < nl; ++l) qmax = std::max(qmax, P[l].q);
  return 2.0 * log2((double)(qmax - 1)) + log2((double)terms + 1.0) >= 127.5;
}

static rg_status launch_pdot(PDotArgs a, const RnsPrime* P, size_t n_proofs, hipStream_t st) {
  for (int l = 0; l < a.nl; ++l) a.P[l] = P[l];
  const dim3 grid(grid256((long long)a.nout * a.nl * a.d), (unsigned)n_proofs);
  if (acc_wide(P, a.nl, a.T))
    hipLaunchKernelGGL(pdot_kernel<true>, grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(pdot_kernel<false>, grid, dim3(256), 0, st, a);
  return check_launch("jindo verify multi dot");
}

template <int L>
static rg_status launch_dot2_multi(const rg_jindo* J, size_t n_proofs, const uint64_t* x1, long long s_x1,
                                   const uint64_t* y1, long long s_y1, long long n1, const uint64_t* x2,
                                   const uint64_t* y2, long long n2, uint64_t* out, hipStream_t st) {
  hipLaunchKernelGGL(dot2_multi_kernel<L>, dim3((unsigned)n_proofs), dim3(256), 0, st, field_params<L>(&J->field), x1,
                     s_x1, y1, s_y1, n1, x2, y2, n2, out);
  return check_launch("jindo verify multi eval");
}

// The scratch of rg_jindo_verify_multi_dev, offsets in words (N = n_proofs; every buffer proof-major):
//   a_out [N][out_msis][nqo][d]  sum_j batchOut[j] com[j][i], then C_out in place
//   b_out [N][out_msis][nqo][d]  sum_j Out[i][j] InCommit[j]
//   lift  [N][dcmp][nq][d]       the inner commitments in ringQ
//   a_in, b_in [N][in_msis][nq][d]  as a_out / b_out for verifyInnerCommitment (C_in in a_in)
//   norms [N][dcmp | out_msis | rows | in_msis + mlwe | in_msis][kNormW]  five arrays, in this order
//   dcd   [N][cols + 1][slots][L]  Decode of Partial and (unused) PartialMask
//   bd    [N][batch][L]            Decode(batch[i])[0]; absent for batch == 1
//   ev    [N][2][L]                both sides of verifyEval
//   flag  [N] int, rounded up to a word
struct JvmScratch {
  size_t a_out, b_out, lift, a_in, b_in, norms[kVerdictSegs], dcd, bd, ev, flag, words;
};
static JvmScratch jvm_scratch(const rg_jindo_params& p, size_t N, size_t batch) {
  const size_t pq = (size_t)p.nq * p.d, po = (size_t)p.nqo * p.d, L = p.field_limbs;
  const size_t cnt[kVerdictSegs] = {(size_t)p.dcmp, (size_t)p.out_msis, (size_t)p.rows, (size_t)(p.in_msis + p.mlwe),
                                    (size_t)p.in_msis};
  JvmScratch s;
  size_t at = 0;
  auto take = [&](size_t words) {
    const size_t here = at;
    at += words;
    return here;
  };
  s.a_out = take(N * p.out_msis * po);
  s.b_out = take(N * p.out_msis * po);
  s.lift = take(N * p.dcmp * pq);
  s.a_in = take(N * p.in_msis * pq);
  s.b_in = take(N * p.in_msis * pq);
  for (int i = 0; i < kVerdictSegs; ++i) s.norms[i] = take(N * cnt[i] * kNormW);
  s.dcd = take(N * (p.cols + 1) * p.slots * L);
  s.bd = take(batch > 1 ? N * batch * L : 0);
  s.ev = take(N * 2 * L);
  s.flag = take((N * sizeof(int) + 7) / 8);
  s.words = at;
  return s;
}

extern "C" {

size_t rg_jindo_verify_multi_scratch_bytes(const rg_jindo* J, size_t n_proofs, size_t batch) {
  if (!J || n_proofs == 0 || n_proofs > RG_JINDO_VERIFY_MAX_PROOFS || batch < 1) return 0;
  return jvm_scratch(J->p, n_proofs, batch).words * 8;
}

rg_status rg_jindo_verify_multi_dev(const rg_jindo* J, size_t n_proofs, size_t batch, const uint64_t* d_com,
                                    const uint64_t* d_bq, const uint64_t* d_bo, const uint64_t* d_chals,
                                    const uint64_t* d_left, const uint64_t* d_right, const uint64_t* d_y,
                                    const uint64_t* d_pf_incom, const uint64_t* d_pf_partial, const uint64_t* d_pf_enc,
                                    const uint64_t* d_pf_mlwe, double in_com_dcmp_two_nm, double res_two_nm,
                                    uint64_t* d_out, void* d_scratch, void* stream) {
  if (!J) return jvm_invalid("NULL handle");
  if (n_proofs == 0 || n_proofs > RG_JINDO_VERIFY_MAX_PROOFS)
    return jvm_invalid("n_proofs " + std::to_string(n_proofs) + " is not in [1, RG_JINDO_VERIFY_MAX_PROOFS]");
  if (batch < 1) return jvm_invalid("batch < 1");
  if (!d_com || !d_chals || !d_left || !d_right || !d_y || !d_pf_incom || !d_pf_partial || !d_pf_enc || !d_pf_mlwe)
    return jvm_invalid("NULL input");
  if (!d_out || !d_scratch) return jvm_invalid("NULL output or scratch");
  if ((batch == 1) != (!d_bq && !d_bo) || !d_bq != !d_bo)
    return jvm_invalid("d_bq and d_bo are both NULL iff batch == 1");
  const rg_jindo_params& p = J->p;
  const int d = p.d, nq = p.nq, nqo = p.nqo, L = p.field_limbs;
  const long long pq = (long long)nq * d, po = (long long)nqo * d, nm = p.in_msis + p.mlwe;
  const long long N = (long long)n_proofs, B = (long long)batch, cs = (long long)p.cols * p.slots;
  if (batch > 0x7fffffffull) return jvm_invalid("batch out of range");
  const JvmScratch S = jvm_scratch(p, n_proofs, batch);
  {  // d_out and d_scratch overlap no input, nor each other
    struct Span {
      const void* p;
      size_t words;
    };
    const Span in[] = {{d_com, (size_t)(N * B * p.out_msis * pq)}, {d_bq, (size_t)(N * B * pq)},
                       {d_bo, (size_t)(N * B * po)},             {d_chals, (size_t)(N * p.cols * pq)},
                       {d_left, (size_t)(N * p.rows * pq)},      {d_right, (size_t)(N * cs * L)},
                       {d_y, (size_t)(N * B * L)},               {d_pf_incom, (size_t)(N * p.dcmp * po)},
                       {d_pf_partial, (size_t)(N * (p.cols + 1) * pq)}, {d_pf_enc, (size_t)(N * p.rows * pq)},
                       {d_pf_mlwe, (size_t)(N * nm * pq)}};
    const Span outs[] = {{d_out, n_proofs * RG_JINDO_VERIFY_WORDS}, {d_scratch, S.words}};
    auto overlap = [](const Span& a, const Span& b) {
      const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
      return a.p && b.p && a0 < b0 + 8 * b.words && b0 < a0 + 8 * a.words;
    };
    if (overlap(outs[0], outs[1])) return jvm_invalid("d_scratch aliases d_out");
    for (const Span& o : outs)
      for (const Span& i : in)
        if (overlap(o, i)) return jvm_invalid("d_out or d_scratch aliases an input");
  }
  RG_TRY(on_device(J));
  hipStream_t st = as_stream(stream);
  uint64_t* scr = static_cast<uint64_t*>(d_scratch);
  uint64_t *a_out = scr + S.a_out, *b_out = scr + S.b_out, *lift = scr + S.lift, *a_in = scr + S.a_in,
           *b_in = scr + S.b_in, *dcd = scr + S.dcd, *bd = scr + S.bd, *ev = scr + S.ev;
  int* flag = reinterpret_cast<int*>(scr + S.flag);
  auto nrm = [&](int seg) { return scr + S.norms[seg]; };
  // verifyOuterCommitment (:136-161), every proof: A, B, C = A * 2^logOutCut - B in place, the norms
  if (batch > 1) {
    PDotArgs a;
    memset(&a, 0, sizeof(a));
    a.d = d, a.nl = nqo, a.T = (int)batch, a.nout = p.out_msis;
    a.A = d_bo, a.a_proof = B * po, a.a_term = po;
    a.B = d_com, a.b_proof = B * p.out_msis * pq, a.b_out = pq, a.b_term = (long long)p.out_msis * pq;
    a.out = a_out;
    RG_TRY(launch_pdot(a, J->ro, n_proofs, st));
  } else {
    RG_HIP(hipMemcpy2DAsync(a_out, 8 * po, d_com, 8 * pq, 8 * po, N * p.out_msis, hipMemcpyDeviceToDevice, st));
  }
  {
    MacArgs m = dot_args(J->ro, nqo, d, N, p.dcmp, J->ck_out.as<uint64_t>(), d_pf_incom, p.dcmp * po, po, b_out);
    m.J = p.out_msis;
    RG_TRY(launch_mac(m, st));
  }
  RG_TRY(launch_combine(J->ro, nqo, d, p.log_out_cut, a_out, b_out, a_out, N * p.out_msis, st));
  RG_TRY(launch_norm(J, true, d_pf_incom, N * p.dcmp, po, nrm(0), st));
  RG_TRY(launch_norm(J, true, a_out, N * p.out_msis, po, nrm(1), st));
  // verifyInnerCommitment (:164-200)
  RG_TRY(launch_round(round_args(J, true, false, 0, d_pf_incom, lift, pq, nq), N * p.dcmp, st));
  {
    PDotArgs a;
    memset(&a, 0, sizeof(a));
    a.d = d, a.nl = nq, a.T = p.cols, a.nout = p.in_msis;
    a.A = d_chals, a.a_proof = p.cols * pq, a.a_term = pq;
    a.B = lift, a.b_proof = p.dcmp * pq, a.b_out = pq, a.b_term = p.in_msis * pq;
    a.C = lift + (long long)p.cols * p.in_msis * pq, a.c_proof = p.dcmp * pq, a.c_out = pq;
    a.out = a_in;
    RG_TRY(launch_pdot(a, J->rq, n_proofs, st));
  }
  {
    MacArgs m = dot_args(J->rq, nq, d, N, p.rows, J->ck_in.as<uint64_t>(), d_pf_enc, p.rows * pq, pq, b_in);
    m.J = p.in_msis;
    m.T2 = p.mlwe;
    m.A2 = J->ck_mlwe.as<uint64_t>();
    m.B2 = d_pf_mlwe;
    m.b2_col = nm * pq;
    m.b2_term = pq;
    m.C = d_pf_mlwe + (long long)p.mlwe * pq;
    m.c_col = nm * pq;
    m.c_j = pq;
    RG_TRY(launch_mac(m, st));
  }
  RG_TRY(launch_combine(J->rq, nq, d, p.log_in_cut, a_in, b_in, a_in, N * p.in_msis, st));
  RG_TRY(launch_norm(J, false, d_pf_enc, N * p.rows, pq, nrm(2), st));
  RG_TRY(launch_norm(J, false, d_pf_mlwe, N * nm, pq, nrm(3), st));
  RG_TRY(launch_norm(J, false, a_in, N * p.in_msis, pq, nrm(4), st));
  // verifyConsistency (:203-221)
  RG_HIP(hipMemsetAsync(flag, 0, n_proofs * sizeof(int), st));
  {
    ConsArgs a;
    memset(&a, 0, sizeof(a));
    a.d = d, a.nl = nq, a.rows = p.rows, a.cols = p.cols;
    a.left = d_left, a.enc = d_pf_enc, a.chals = d_chals, a.partial = d_pf_partial;
    a.flag = flag;
    for (int l = 0; l < nq; ++l) a.P[l] = J->rq[l];
    const dim3 grid(grid256(pq), (unsigned)n_proofs);
    if (acc_wide(J->rq, nq, std::max(p.rows, p.cols)))
      hipLaunchKernelGGL(consistency_kernel<true>, grid, dim3(256), 0, st, a);
    else
      hipLaunchKernelGGL(consistency_kernel<false>, grid, dim3(256), 0, st, a);
    RG_TRY(check_launch("jindo verify multi consistency"));
  }
  // verifyEval (:224-259): Decode of every proof's Partial (PartialMask's row is decoded and left unread)
  RG_TRY(decode_any(J, d_pf_partial, N * (p.cols + 1), p.slots, dcd, st));
  if (batch > 1) RG_TRY(decode_any(J, d_bq, N * B, 1, bd, st));
  RG_TRY(dispatch_limbs(L, [&](auto Lc) {
    return launch_dot2_multi<Lc()>(J, n_proofs, d_right, cs, dcd, (long long)(p.cols + 1) * p.slots, cs, bd, d_y,
                                   batch > 1 ? B : 0, ev, st);
  }));
  // the records
  VerdictArgs v;
  memset(&v, 0, sizeof(v));
  v.L = L;
  const int cnt[kVerdictSegs] = {p.dcmp, p.out_msis, p.rows, (int)nm, p.in_msis};
  for (int i = 0; i < kVerdictSegs; ++i) {
    v.norms[i] = nrm(i);
    v.cnt[i] = cnt[i];
  }
  const double nms[2] = {in_com_dcmp_two_nm, res_two_nm};
  for (int i = 0; i < 2; ++i) {
    uint64_t K2[2 * kNormW];
    v.bound[i].always = norm_threshold(nms[i], K2);
    if (v.bound[i].always == 0) memcpy(v.bound[i].k2, K2, sizeof(v.bound[i].k2));
  }
  v.lhs = ev;
  v.lhs_stride = 2 * L;
  v.rhs = batch > 1 ? ev + L : d_y;  // batch == 1: yBatch = y[0] (:244-246)
  v.rhs_stride = batch > 1 ? 2 * L : L;
  v.flag = flag;
  v.out = d_out;
  hipLaunchKernelGGL(verdict_kernel, dim3((unsigned)n_proofs), dim3(64), 0, st, v);
  return check_launch("jindo verify multi verdict");
}

rg_status rg_jindo_verify_unpack(const uint64_t* words, int field_limbs, rg_jindo_verify_result* res) {
  if (!words || !res) return jvm_invalid("unpack: NULL record or result");
  if (!limbs_supported(field_limbs))
    return jvm_invalid("unpack: no field of " + std::to_string(field_limbs) + " limbs is built");
  memset(res, 0, sizeof(*res));
  res->ok = words[0] != 0;
  res->outer_ok = (words[1] >> 0) & 1;
  res->inner_ok = (words[1] >> 1) & 1;
  res->consistency_ok = (words[1] >> 2) & 1;
  res->eval_ok = (words[1] >> 3) & 1;
  memcpy(res->outer_norm_sq, words + 2, 8 * kNormW);
  memcpy(res->inner_norm_sq, words + 2 + kNormW, 8 * kNormW);
  memcpy(res->eval_lhs, words + 2 + 2 * kNormW, 8 * (size_t)field_limbs);
  memcpy(res->eval_rhs, words + 2 + 2 * kNormW + 16, 8 * (size_t)field_limbs);
  return RG_OK;
}

// ---- the transcript-derived inputs of Evaluate and Verify (utils.go:20-82) -------------------
rg_status rg_jindo_challenge_bound(const rg_jindo_params* p, uint64_t* bound) {
  if (!p || !bound) {
    set_last_error("jindo challenge bound: NULL argument");
    return RG_ERR_INVALID;
  }
  if (p->exp < 1 || p->base < 2) {
    set_last_error("jindo challenge bound: exp < 1 or base < 2");
    return RG_ERR_INVALID;
  }
  *bound = challenge_bound(p->base, p->exp);
  if (*bound == 0) {  // the reference divides by zero (utils.go:12-18)
    set_last_error("jindo challenge bound: ChallengeBound() = min(base, 1 << (120 / exp)) / 2 is 0 at exp = " +
                   std::to_string(p->exp) + " (exp > 120 or 120 / exp >= 64)");
    return RG_ERR_INVALID;
  }
  return RG_OK;
}

rg_status rg_jindo_eval_point_dev(const rg_jindo* J, const uint64_t* d_x, uint64_t* d_left, uint64_t* d_right,
                                  void* stream) {
  if (!J || !d_x || !d_left) {
    set_last_error("jindo eval point: NULL handle, point or left buffer");
    return RG_ERR_INVALID;
  }
  RG_TRY(on_device(J));
  const rg_jindo_params& p = J->p;
  const size_t cs = (size_t)p.cols * p.slots, L = p.field_limbs;
  hipStream_t st = as_stream(stream);
  uint64_t* pw = nullptr;
  RG_TRY(point_scratch(const_cast<rg_jindo*>(J), st, &pw));
  uint64_t* lp = pw + (cs + 1) * L;
  // rightVec: right[i] = x^i (utils.go:75-82); one more power is leftVec's skip = x^(cols slots)
  RG_TRY(rg_buckler_powers_dev(&J->field, d_x, cs + 1, pw, stream));
  if (d_right) RG_HIP(hipMemcpyAsync(d_right, pw, cs * L * 8, hipMemcpyDeviceToDevice, st));
  // leftVec: left[i] = skip^i, then left[rows - 1] = x (utils.go:63-72; the kernel takes x for that row)
  RG_TRY(rg_buckler_powers_dev(&J->field, pw + cs * L, p.rows, lp, stream));
  return dispatch_limbs((int)L, [&](auto Lc) { return launch_encode_left<Lc()>(J, lp, d_x, d_left, st); });
}

rg_status rg_jindo_encode_challenges_dev(const rg_jindo* J, int ring, const uint8_t* d_bytes, size_t n,
                                         uint64_t* d_out, void* stream) {
  if (ring != 0 && ring != 1) {
    set_last_error("jindo encode challenges: ring " + std::to_string(ring) + " is neither 0 (ringQ) nor 1 (ringQOut)");
    return RG_ERR_INVALID;
  }
  if (!J || (n && (!d_bytes || !d_out))) {
    set_last_error("jindo encode challenges: NULL handle or buffer");
    return RG_ERR_INVALID;
  }
  if (n > 0x7fffffffull) {
    set_last_error("jindo encode challenges: n out of range");
    return RG_ERR_INVALID;
  }
  const rg_jindo_params& p = J->p;
  ChalArgs a;
  memset(&a, 0, sizeof(a));
  RG_TRY(rg_jindo_challenge_bound(&p, &a.bound));
  if (n == 0) return RG_OK;
  RG_TRY(on_device(J));
  a.d = p.d;
  a.slots = p.slots;
  a.exp = p.exp;
  a.R = ring ? ring_dev(J->ro, p.nqo, J->rootso_f, J->rootso_b) : ring_dev(J->rq, p.nq, J->rootsq_f, J->rootsq_b);
  a.bound_inv = a.bound > 1 ? (uint64_t)(((unsigned __int128)1 << 64) / a.bound) : 0;
  a.bytes = d_bytes;
  a.out = d_out;
  hipLaunchKernelGGL(encode_chal_kernel, dim3((unsigned)n), dim3(256), (size_t)a.R.n * p.d * 8, as_stream(stream), a);
  return check_launch("jindo encode challenges");
}

}  // extern "C"

// ---- the inputs of a batch verification: every proof's point and challenges in one call -------
namespace {

struct Span {
  const char* name;
  const void* p;
  size_t bytes;
};

bool spans_overlap(const Span& a, const Span& b) {
  const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
  return a.p && b.p && a.bytes && b.bytes && a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

// no output overlaps another output or an input; the reason names the pair
rg_status check_disjoint(const char* who, const Span* outs, size_t n_out, const Span* ins, size_t n_in) {
  for (size_t i = 0; i < n_out; ++i) {
    for (size_t k = 0; k < i; ++k)
      if (spans_overlap(outs[i], outs[k])) {
        set_last_error(std::string(who) + ": " + outs[i].name + " overlaps " + outs[k].name);
        return RG_ERR_INVALID;
      }
    for (size_t k = 0; k < n_in; ++k)
      if (spans_overlap(outs[i], ins[k])) {
        set_last_error(std::string(who) + ": " + outs[i].name + " overlaps " + ins[k].name);
        return RG_ERR_INVALID;
      }
  }
  return RG_OK;
}

constexpr size_t kPointMaxStride = (size_t)1 << 30;  // rg_buckler_powers_batch_dev's limit on a base stride

// what both entries ask of the points; n > 0
rg_status check_points(const char* who, size_t n, const uint64_t* d_x, size_t x_stride) {
  auto invalid = [&](const std::string& why) {
    set_last_error(std::string(who) + ": " + why);
    return RG_ERR_INVALID;
  };
  if (n > RG_JINDO_POINT_MAX_POINTS)
    return invalid(std::to_string(n) + " points: at most RG_JINDO_POINT_MAX_POINTS, a point per grid row");
  if (!d_x) return invalid("NULL d_x");
  if (x_stride == 0 || x_stride > kPointMaxStride) return invalid("x_stride is not in [1, 2^30]");
  return RG_OK;
}

}  // namespace

extern "C" {

size_t rg_jindo_eval_point_multi_scratch_bytes(const rg_jindo* J, size_t n_points) {
  if (!J || n_points == 0 || n_points > RG_JINDO_POINT_MAX_POINTS) return 0;
  return point_multi_words(J->p, n_points) * 8;
}

rg_status rg_jindo_eval_point_multi_dev(const rg_jindo* J, size_t n_points, const uint64_t* d_x, size_t x_stride,
                                        uint64_t* d_left, uint64_t* d_right, void* d_scratch, void* stream) {
  static const char who[] = "jindo eval point multi";
  if (!J) {
    set_last_error(std::string(who) + ": NULL handle");
    return RG_ERR_INVALID;
  }
  if (n_points == 0) return RG_OK;
  RG_TRY(check_points(who, n_points, d_x, x_stride));
  if (!d_left || !d_scratch) {
    set_last_error(std::string(who) + ": NULL d_left or d_scratch");
    return RG_ERR_INVALID;
  }
  const rg_jindo_params& p = J->p;
  const size_t N = n_points, L = p.field_limbs, pq = (size_t)p.nq * p.d;
  const Span outs[] = {{"d_left", d_left, N * p.rows * pq * 8},
                       {"d_right", d_right, N * p.cols * p.slots * L * 8},
                       {"d_scratch", d_scratch, point_multi_words(p, N) * 8}};
  const Span ins[] = {{"the points of d_x", d_x, ((N - 1) * x_stride + 1) * L * 8}};
  RG_TRY(check_disjoint(who, outs, 3, ins, 1));
  RG_TRY(on_device(J));
  return point_multi(J, N, d_x, x_stride, d_left, d_right, static_cast<uint64_t*>(d_scratch), as_stream(stream));
}

size_t rg_jindo_verify_inputs_multi_scratch_bytes(const rg_jindo* J, size_t n_proofs) {
  return rg_jindo_eval_point_multi_scratch_bytes(J, n_proofs);
}

rg_status rg_jindo_verify_inputs_multi_dev(const rg_jindo* J, size_t n_proofs, size_t batch, const uint64_t* d_x,
                                           size_t x_stride, const uint8_t* d_batch_bytes, const uint8_t* d_chal_bytes,
                                           uint64_t* d_bq, uint64_t* d_bo, uint64_t* d_chals, uint64_t* d_left,
                                           uint64_t* d_right, void* d_scratch, void* stream) {
  static const char who[] = "jindo verify inputs multi";
  auto invalid = [&](const std::string& why) {
    set_last_error(std::string(who) + ": " + why);
    return RG_ERR_INVALID;
  };
  if (!J) return invalid("NULL handle");
  if (n_proofs == 0) return RG_OK;
  RG_TRY(check_points(who, n_proofs, d_x, x_stride));
  if (batch < 1 || batch > 0x7fffffffull / RG_JINDO_POINT_MAX_POINTS) return invalid("batch out of range");
  if (!d_chal_bytes || !d_chals || !d_left || !d_scratch) return invalid("NULL d_chal_bytes, d_chals, d_left or d_scratch");
  if ((batch == 1) != (!d_batch_bytes && !d_bq && !d_bo) || !d_bq != !d_bo || !d_bq != !d_batch_bytes)
    return invalid("d_batch_bytes, d_bq and d_bo are all NULL iff batch == 1");
  const rg_jindo_params& p = J->p;
  uint64_t bound = 0;
  RG_TRY(rg_jindo_challenge_bound(&p, &bound));
  const size_t N = n_proofs, L = p.field_limbs, pq = (size_t)p.nq * p.d, po = (size_t)p.nqo * p.d;
  const Span outs[] = {{"d_bq", d_bq, N * batch * pq * 8},
                       {"d_bo", d_bo, N * batch * po * 8},
                       {"d_chals", d_chals, N * p.cols * pq * 8},
                       {"d_left", d_left, N * p.rows * pq * 8},
                       {"d_right", d_right, N * p.cols * p.slots * L * 8},
                       {"d_scratch", d_scratch, point_multi_words(p, N) * 8}};
  const Span ins[] = {{"the points of d_x", d_x, ((N - 1) * x_stride + 1) * L * 8},
                      {"d_batch_bytes", d_batch_bytes, N * batch * 16},
                      {"d_chal_bytes", d_chal_bytes, N * p.cols * 16}};
  RG_TRY(check_disjoint(who, outs, 6, ins, 3));
  RG_TRY(on_device(J));
  if (batch > 1) {  // batch[i] in ringQ and batchOut[i] in ringQOut (verifier.go:74-80)
    RG_TRY(rg_jindo_encode_challenges_dev(J, 0, d_batch_bytes, N * batch, d_bq, stream));
    RG_TRY(rg_jindo_encode_challenges_dev(J, 1, d_batch_bytes, N * batch, d_bo, stream));
  }
  RG_TRY(rg_jindo_encode_challenges_dev(J, 0, d_chal_bytes, N * p.cols, d_chals, stream));
  return point_multi(J, N, d_x, x_stride, d_left, d_right, static_cast<uint64_t*>(d_scratch), as_stream(stream));
}

rg_status rg_jindo_eval_reduce_dev(const rg_jindo* J, uint64_t* d_ob_incom, uint64_t* d_ob_enc, uint64_t* d_ob_mlwe,
                                   void* stream) {
  if (!J || !d_ob_incom || !d_ob_enc || !d_ob_mlwe) return RG_ERR_INVALID;
  const rg_jindo_params& p = J->p;
  hipStream_t st = as_stream(stream);
  const long long nm = p.in_msis + p.mlwe, n_enc = (long long)(p.cols + 1) * p.rows, n_ml = (long long)(p.cols + 1) * nm;
  const RingDev rq = ring_dev(J->rq, p.nq, J->rootsq_f, J->rootsq_b), ro = ring_dev(J->ro, p.nqo, J->rootso_f, J->rootso_b);
  auto go = [&](uint64_t* x, long long npoly, int nl, const RingDev& R) {
    const long long n = npoly * nl * p.d;
    hipLaunchKernelGGL(rns_reduce_kernel, dim3(grid256(n)), dim3(256), 0, st, x, npoly, nl, p.d, R);
    return check_launch("jindo eval reduce");
  };
  RG_TRY(go(d_ob_incom, p.dcmp, p.nqo, ro));
  RG_TRY(go(d_ob_enc, n_enc, p.nq, rq));
  return go(d_ob_mlwe, n_ml, p.nq, rq);
}

}  // extern "C"

// ---- Prover.Evaluate for n_proofs proofs of one handle, in two calls around the transcript ----
// rg_jindo_eval_open_multi_dev (prover.go:227-289) and rg_jindo_eval_respond_multi_dev (:296-316).
// The challenge encodings and the point pass are the kernels above with n = n_proofs * batch (or
// cols) and a point per proof; the InCommit and MLWE combinations and the response products are
// pdot_kernel with the proof stride on both operands.  What is new is
//   eval_open_kernel  workgroup per (proof, column i, tile of 64 limb * coeff positions), its waves (4, or
//                     16 from kEvalManyRows rows on: one proof alone has only (cols + 1) * tiles workgroups)
//                     splitting the rows j as dot_split_kernel splits its terms.  Per row a wave forms
//                     openBatch.Encode[i][j] = sum_t batch[t] * open[t].Encode[i][j] exactly, reduces it,
//                     stores it and multiplies it by left[j] into a second exact accumulator, so
//                     Partial[i] = sum_j left[j] * openBatch.Encode[i][j] never reads openBatch.Encode
//                     back; the waves' sums are added through LDS and reduced once.  The proof's
//                     batch-challenge tile sits in LDS up to kEvalLdsBatch commits (16 KB) and is read
//                     from global memory (L2) above.  WB / WR: the third accumulator word for the sum
//                     over the batch / over the rows, each by launch_mac's criterion.
//   gather_kernel     batch == 1: Proof.InCommit = open[0].InCommit of every proof, a strided copy
namespace rg {

constexpr int kEvalLdsBatch = 32;
constexpr int kEvalManyRows = 32;  // from here on 16 waves split the rows, below 4

struct EvalOpenArgs {
  int d, nl, rows, cols, batch;
  const uint64_t* enc;               // opening t of proof p at p * enc_proof + t * enc_commit words
  long long enc_proof, enc_commit;
  const uint64_t* bq;                // [proof][batch][nl][d]
  const uint64_t* left;              // [proof][rows][nl][d]
  uint64_t* ob_enc;                  // [proof][cols + 1][rows][nl][d]
  uint64_t* partial;                 // [proof][cols + 1][nl][d]
  RnsPrime P[kMaxQ];
};

// dynamic LDS: the batch-challenge tile [batch][64] (LDSB), then the waves' sums [waves - 1][3][64]
template <bool WB, bool WR, bool LDSB>
__global__ __launch_bounds__(1024) void eval_open_kernel(EvalOpenArgs a) {
  extern __shared__ uint64_t eval_lds[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  uint64_t(*bt)[64] = reinterpret_cast<uint64_t(*)[64]>(eval_lds);
  uint64_t(*red)[3][64] = reinterpret_cast<uint64_t(*)[3][64]>(eval_lds + (LDSB ? a.batch * 64 : 0));
  const long long per_col = (long long)a.nl * a.d;
  const unsigned ntile = (unsigned)((per_col + 63) / 64);
  const long long lk = (long long)(blockIdx.x % ntile) * 64 + lane;
  const long long col = blockIdx.x / ntile, p = blockIdx.y;
  const bool ok = lk < per_col;  // nl * d need not be a multiple of 64 (d = 8)
  const uint64_t* bq = a.bq + p * a.batch * per_col + lk;
  if constexpr (LDSB) {
    for (int t = w; t < a.batch; t += nw) bt[t][lane] = ok ? bq[t * per_col] : 0;
    __syncthreads();
  }
  Acc<WR> part;
  part.zero();
  if (ok) {
    const RnsPrime& P = a.P[(int)(lk / a.d)];
    const uint64_t* e0 = a.enc + p * a.enc_proof + col * a.rows * per_col + lk;
    const uint64_t* left = a.left + p * a.rows * per_col + lk;
    uint64_t* ob = a.ob_enc + (p * (a.cols + 1) + col) * a.rows * per_col + lk;
    for (int j = w; j < a.rows; j += nw) {
      const uint64_t* e = e0 + j * per_col;
      const uint64_t lv = left[j * per_col];
      Acc<WB> s;
      s.zero();
#pragma unroll 4
      for (int t = 0; t < a.batch; ++t) {
        uint64_t b;
        if constexpr (LDSB)
          b = bt[t][lane];
        else
          b = bq[t * per_col];
        s.mac(b, e[t * a.enc_commit]);
      }
      const uint64_t v = s.reduce(P);
      ob[j * per_col] = v;
      part.mac(lv, v);
    }
  }
  if (w > 0) {
    red[w - 1][0][lane] = part.lo;
    red[w - 1][1][lane] = part.hi;
    red[w - 1][2][lane] = part.top;
  }
  __syncthreads();
  if (w != 0 || !ok) return;
  for (int v = 0; v < nw - 1; ++v) {  // exact: the whole sum over the rows fits the width chosen for it
    uint32_t c1 = 0;
    part.lo = addc(part.lo, red[v][0][lane], c1);
    if constexpr (WR) {
      uint32_t c2 = 0, c3 = 0;
      part.hi = addc(part.hi, red[v][1][lane], c2);
      part.hi = addc(part.hi, (uint64_t)c1, c3);
      part.top += (uint32_t)red[v][2][lane] + c2 + c3;
    } else {
      part.hi += red[v][1][lane] + c1;
    }
  }
  a.partial[(p * (a.cols + 1) + col) * per_col + lk] = part.reduce(a.P[(int)(lk / a.d)]);
}

// out [proof][words] = in[proof * in_stride ..]; blockIdx.y is the proof
__global__ __launch_bounds__(256) void gather_kernel(const uint64_t* in, long long in_stride, uint64_t* out,
                                                     long long words) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < words) out[blockIdx.y * words + i] = in[blockIdx.y * in_stride + i];
}

static rg_status launch_eval_open(const EvalOpenArgs& a, size_t n_proofs, hipStream_t st) {
  const bool wb = acc_wide(a.P, a.nl, a.batch), wr = acc_wide(a.P, a.nl, a.rows), lds = a.batch <= kEvalLdsBatch;
  const unsigned ntile = (unsigned)(((long long)a.nl * a.d + 63) / 64);
  const dim3 grid(ntile * (unsigned)(a.cols + 1), (unsigned)n_proofs);
  const int nw = a.rows >= kEvalManyRows ? 16 : 4;
  const size_t shmem = ((lds ? (size_t)a.batch * 64 : 0) + (size_t)(nw - 1) * 3 * 64) * 8;
  auto go = [&](auto WB, auto WR, auto LDSB) {
    hipLaunchKernelGGL((eval_open_kernel<WB(), WR(), LDSB()>), grid, dim3(64 * nw), shmem, st, a);
  };
  auto pick_lds = [&](auto WB, auto WR) {
    if (lds)
      go(WB, WR, std::true_type{});
    else
      go(WB, WR, std::false_type{});
  };
  auto pick_wr = [&](auto WB) {
    if (wr)
      pick_lds(WB, std::true_type{});
    else
      pick_lds(WB, std::false_type{});
  };
  if (wb)
    pick_wr(std::true_type{});
  else
    pick_wr(std::false_type{});
  return check_launch("jindo eval multi open");
}

// The scratch of rg_jindo_eval_open_multi_dev in words (N = n_proofs): bq [N][batch][nq][d] and bo
// [N][batch][nqo][d] (absent for batch == 1), left [N][rows][nq][d], then the point pass's own
struct JemScratch {
  size_t bq, bo, left, lp, words;
};
static JemScratch jem_scratch(const rg_jindo_params& p, size_t N, size_t batch) {
  const size_t pq = (size_t)p.nq * p.d, po = (size_t)p.nqo * p.d;
  JemScratch s;
  s.bq = 0;
  s.bo = s.bq + (batch > 1 ? N * batch * pq : 0);
  s.left = s.bo + (batch > 1 ? N * batch * po : 0);
  s.lp = s.left + N * p.rows * pq;
  s.words = s.lp + point_multi_words(p, N);
  return s;
}

constexpr size_t kEvalMaxBatch = 0x7fffffffull / RG_JINDO_EVAL_MAX_PROOFS;  // n_proofs * batch encodings in one grid
constexpr size_t kEvalMaxStride = (size_t)1 << 31;

// bytes from the first word of a strided array of `openings` openings of `words` words to its last
// opening's end; 0 where that passes 2^62 (refused by the callers)
static size_t strided_bytes(unsigned __int128 openings, size_t words) {
  const unsigned __int128 b = openings * words * 8;
  return b >> 62 ? 0 : (size_t)b;
}

}  // namespace rg

extern "C" {

size_t rg_jindo_eval_open_multi_scratch_bytes(const rg_jindo* J, size_t n_proofs, size_t batch) {
  if (!J || n_proofs == 0 || n_proofs > RG_JINDO_EVAL_MAX_PROOFS || batch < 1 || batch > kEvalMaxBatch) return 0;
  return jem_scratch(J->p, n_proofs, batch).words * 8;
}

rg_status rg_jindo_eval_open_multi_dev(const rg_jindo* J, size_t n_proofs, size_t batch, const uint64_t* d_incom,
                                       const uint64_t* d_enc, const uint64_t* d_mlwe, size_t open_proof_stride,
                                       size_t open_commit_stride, const uint64_t* d_x, size_t x_stride,
                                       const uint8_t* d_batch_bytes, uint64_t* d_ob_enc, uint64_t* d_ob_mlwe,
                                       uint64_t* d_pf_incom, uint64_t* d_pf_partial, void* d_scratch, void* stream) {
  static const char who[] = "jindo eval multi open";
  auto invalid = [&](const std::string& why) {
    set_last_error(std::string(who) + ": " + why);
    return RG_ERR_INVALID;
  };
  if (!J) return invalid("NULL handle");
  if (n_proofs == 0 || n_proofs > RG_JINDO_EVAL_MAX_PROOFS)
    return invalid("n_proofs " + std::to_string(n_proofs) + " is not in [1, RG_JINDO_EVAL_MAX_PROOFS]");
  if (batch < 1 || batch > kEvalMaxBatch) return invalid("batch is not in [1, " + std::to_string(kEvalMaxBatch) + "]");
  if (!d_incom || !d_enc || !d_mlwe) return invalid("NULL d_incom, d_enc or d_mlwe");
  if (open_proof_stride == 0 || open_commit_stride == 0 || open_proof_stride > kEvalMaxStride ||
      open_commit_stride > kEvalMaxStride)
    return invalid("open_proof_stride and open_commit_stride are not in [1, 2^31]");
  RG_TRY(check_points(who, n_proofs, d_x, x_stride));
  if (!d_pf_incom || !d_pf_partial || !d_scratch) return invalid("NULL d_pf_incom, d_pf_partial or d_scratch");
  if ((batch == 1) != (!d_batch_bytes && !d_ob_enc && !d_ob_mlwe) || !d_ob_enc != !d_ob_mlwe ||
      !d_ob_enc != !d_batch_bytes)
    return invalid("d_batch_bytes, d_ob_enc and d_ob_mlwe are all NULL iff batch == 1");
  const rg_jindo_params& p = J->p;
  uint64_t bound = 0;
  if (rg_jindo_challenge_bound(&p, &bound) != RG_OK) return invalid("ChallengeBound() is 0 (exp > 120)");
  const size_t N = n_proofs, L = p.field_limbs, pq = (size_t)p.nq * p.d, po = (size_t)p.nqo * p.d;
  const size_t nm = (size_t)p.in_msis + p.mlwe, w_inc = (size_t)p.dcmp * po, w_enc = (size_t)(p.cols + 1) * p.rows * pq,
               w_ml = (size_t)(p.cols + 1) * nm * pq;
  const JemScratch S = jem_scratch(p, N, batch);
  {
    const unsigned __int128 openings =
        (unsigned __int128)(N - 1) * open_proof_stride + (unsigned __int128)(batch - 1) * open_commit_stride + 1;
    const Span ins[] = {{"d_incom", d_incom, strided_bytes(openings, w_inc)},
                        {"d_enc", d_enc, strided_bytes(openings, w_enc)},
                        {"d_mlwe", d_mlwe, strided_bytes(openings, w_ml)},
                        {"the points of d_x", d_x, ((N - 1) * x_stride + 1) * L * 8},
                        {"d_batch_bytes", d_batch_bytes, N * batch * 16}};
    for (int i = 0; i < 3; ++i)
      if (!ins[i].bytes) return invalid("the openings' extent is out of range");
    const Span outs[] = {{"d_ob_enc", d_ob_enc, N * w_enc * 8},
                         {"d_ob_mlwe", d_ob_mlwe, N * w_ml * 8},
                         {"d_pf_incom", d_pf_incom, N * w_inc * 8},
                         {"d_pf_partial", d_pf_partial, N * (p.cols + 1) * pq * 8},
                         {"d_scratch", d_scratch, S.words * 8}};
    RG_TRY(check_disjoint(who, outs, 5, ins, 5));
  }
  RG_TRY(on_device(J));
  hipStream_t st = as_stream(stream);
  uint64_t* scr = static_cast<uint64_t*>(d_scratch);
  uint64_t *bq = scr + S.bq, *bo = scr + S.bo, *left = scr + S.left;
  const long long ps = (long long)open_proof_stride, cs = (long long)open_commit_stride;
  RG_TRY(point_multi(J, N, d_x, x_stride, left, nullptr, scr + S.lp, st));
  if (batch == 1) {  // openBatch = open[0] (:267-269): InCommit copied, the partials straight from d_enc
    hipLaunchKernelGGL(gather_kernel, dim3(grid256((long long)w_inc), (unsigned)N), dim3(256), 0, st, d_incom,
                       ps * (long long)w_inc, d_pf_incom, (long long)w_inc);
    RG_TRY(check_launch("jindo eval multi incommit"));
    PDotArgs a;
    memset(&a, 0, sizeof(a));
    a.d = p.d, a.nl = p.nq, a.T = p.rows, a.nout = p.cols + 1;
    a.A = left, a.a_proof = (long long)p.rows * pq, a.a_term = pq;
    a.B = d_enc, a.b_proof = ps * (long long)w_enc, a.b_out = (long long)p.rows * pq, a.b_term = pq;
    a.out = d_pf_partial;
    return launch_pdot(a, J->rq, N, st);
  }
  // batch[i] into ringQ and ringQOut (:228-252)
  RG_TRY(rg_jindo_encode_challenges_dev(J, 0, d_batch_bytes, N * batch, bq, stream));
  RG_TRY(rg_jindo_encode_challenges_dev(J, 1, d_batch_bytes, N * batch, bo, stream));
  {  // openBatch.InCommit and openBatch.MLWE (:254-266), a J = 1 dot product over the proof's commits
    PDotArgs a;
    memset(&a, 0, sizeof(a));
    a.d = p.d, a.nl = p.nqo, a.T = (int)batch, a.nout = p.dcmp;
    a.A = bo, a.a_proof = (long long)(batch * po), a.a_term = po;
    a.B = d_incom, a.b_proof = ps * (long long)w_inc, a.b_out = po, a.b_term = cs * (long long)w_inc;
    a.out = d_pf_incom;
    RG_TRY(launch_pdot(a, J->ro, N, st));
    a.nl = p.nq, a.nout = (int)((p.cols + 1) * nm);
    a.A = bq, a.a_proof = (long long)(batch * pq), a.a_term = pq;
    a.B = d_mlwe, a.b_proof = ps * (long long)w_ml, a.b_out = pq, a.b_term = cs * (long long)w_ml;
    a.out = d_ob_mlwe;
    RG_TRY(launch_pdot(a, J->rq, N, st));
  }
  EvalOpenArgs e;
  memset(&e, 0, sizeof(e));
  e.d = p.d, e.nl = p.nq, e.rows = p.rows, e.cols = p.cols, e.batch = (int)batch;
  e.enc = d_enc, e.enc_proof = ps * (long long)w_enc, e.enc_commit = cs * (long long)w_enc;
  e.bq = bq, e.left = left, e.ob_enc = d_ob_enc, e.partial = d_pf_partial;
  for (int l = 0; l < p.nq; ++l) e.P[l] = J->rq[l];
  return launch_eval_open(e, N, st);
}

size_t rg_jindo_eval_respond_multi_scratch_bytes(const rg_jindo* J, size_t n_proofs) {
  if (!J || n_proofs == 0 || n_proofs > RG_JINDO_EVAL_MAX_PROOFS) return 0;
  return n_proofs * J->p.cols * J->p.nq * J->p.d * 8;  // chals [N][cols][nq][d]
}

rg_status rg_jindo_eval_respond_multi_dev(const rg_jindo* J, size_t n_proofs, const uint64_t* d_ob_enc,
                                          const uint64_t* d_ob_mlwe, size_t ob_proof_stride,
                                          const uint8_t* d_chal_bytes, uint64_t* d_pf_enc, uint64_t* d_pf_mlwe,
                                          void* d_scratch, void* stream) {
  static const char who[] = "jindo eval multi respond";
  auto invalid = [&](const std::string& why) {
    set_last_error(std::string(who) + ": " + why);
    return RG_ERR_INVALID;
  };
  if (!J) return invalid("NULL handle");
  if (n_proofs == 0 || n_proofs > RG_JINDO_EVAL_MAX_PROOFS)
    return invalid("n_proofs " + std::to_string(n_proofs) + " is not in [1, RG_JINDO_EVAL_MAX_PROOFS]");
  if (!d_ob_enc || !d_ob_mlwe || !d_chal_bytes) return invalid("NULL d_ob_enc, d_ob_mlwe or d_chal_bytes");
  if (ob_proof_stride == 0 || ob_proof_stride > kEvalMaxStride) return invalid("ob_proof_stride is not in [1, 2^31]");
  if (!d_pf_enc || !d_pf_mlwe || !d_scratch) return invalid("NULL d_pf_enc, d_pf_mlwe or d_scratch");
  const rg_jindo_params& p = J->p;
  uint64_t bound = 0;
  if (rg_jindo_challenge_bound(&p, &bound) != RG_OK) return invalid("ChallengeBound() is 0 (exp > 120)");
  if ((unsigned long long)n_proofs * p.cols > 0x7fffffffull) return invalid("n_proofs * cols out of range");
  const size_t N = n_proofs, pq = (size_t)p.nq * p.d, nm = (size_t)p.in_msis + p.mlwe;
  const size_t w_enc = (size_t)(p.cols + 1) * p.rows * pq, w_ml = (size_t)(p.cols + 1) * nm * pq;
  {
    const unsigned __int128 openings = (unsigned __int128)(N - 1) * ob_proof_stride + 1;
    const Span ins[] = {{"d_ob_enc", d_ob_enc, strided_bytes(openings, w_enc)},
                        {"d_ob_mlwe", d_ob_mlwe, strided_bytes(openings, w_ml)},
                        {"d_chal_bytes", d_chal_bytes, N * p.cols * 16}};
    if (!ins[0].bytes || !ins[1].bytes) return invalid("the openBatches' extent is out of range");
    const Span outs[] = {{"d_pf_enc", d_pf_enc, N * p.rows * pq * 8},
                         {"d_pf_mlwe", d_pf_mlwe, N * nm * pq * 8},
                         {"d_scratch", d_scratch, N * p.cols * pq * 8}};
    RG_TRY(check_disjoint(who, outs, 3, ins, 3));
  }
  RG_TRY(on_device(J));
  hipStream_t st = as_stream(stream);
  uint64_t* chals = static_cast<uint64_t*>(d_scratch);
  RG_TRY(rg_jindo_encode_challenges_dev(J, 0, d_chal_bytes, N * p.cols, chals, stream));
  const long long ps = (long long)ob_proof_stride;
  PDotArgs a;
  memset(&a, 0, sizeof(a));
  // pf.Encode[i] = Enc[cols][i] + sum_j chals[j] * Enc[j][i] (prover.go:300-306)
  a.d = p.d, a.nl = p.nq, a.T = p.cols, a.nout = p.rows;
  a.A = chals, a.a_proof = (long long)(p.cols * pq), a.a_term = pq;
  a.B = d_ob_enc, a.b_proof = ps * (long long)w_enc, a.b_out = pq, a.b_term = (long long)(p.rows * pq);
  a.C = d_ob_enc + (size_t)p.cols * p.rows * pq, a.c_proof = a.b_proof, a.c_out = pq;
  a.out = d_pf_enc;
  RG_TRY(launch_pdot(a, J->rq, N, st));
  // pf.MLWE[i] = MLWE[cols][i] + sum_j chals[j] * MLWE[j][i] (:308-314)
  a.nout = (int)nm;
  a.B = d_ob_mlwe, a.b_proof = ps * (long long)w_ml, a.b_term = (long long)(nm * pq);
  a.C = d_ob_mlwe + (size_t)p.cols * nm * pq, a.c_proof = a.b_proof;
  a.out = d_pf_mlwe;
  return launch_pdot(a, J->rq, N, st);
}

}  // extern "C"
