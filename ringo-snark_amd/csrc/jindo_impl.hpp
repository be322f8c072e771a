// jindo_impl.hpp -- what the Jindo units (jindo_setup.hip, jindo_commit.hip, jindo_sample.hip,
// jindo_verify.hip) share: the device-side ring constants and kernel argument structs, the
// __device__ helpers that kernels of more than one unit inline (there is no relocatable device
// code, so a kernel never calls across units), the handle, the byte sizes of the per-commit
// buffers, and the host functions that cross units.  Dependencies point one way: sample -> commit
// -> setup, verify -> commit and setup.  The pipeline overview is at the top of jindo_commit.hip.
#pragma once
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "common.hpp"
#include "field.hpp"

namespace rg {

constexpr int kMaxQ = 4;     // RNS limbs per ring
constexpr int kMaxD = 1024;  // ring degree supported by the LDS kernels
constexpr int kMaxJ = 32;    // MSIS rank accumulated per thread

struct RnsPrime {
  uint64_t q;
  uint64_t rinv, rinv_sh;    // 2^-64 mod q (IMForm)
  uint64_t r64, r64_sh;      // 2^64 mod q (MForm)
  uint64_t one_sh;           // floor(2^64 / q): x mod q = shoup(x, 1)
  uint64_t ninv, ninv_sh;    // d^-1 mod q
  uint64_t bmod, bmod_sh;    // base mod q
  uint64_t rw1, rw1_sh;      // 2^64 w1 mod q, w1 = the forward table's first-stage root (prep256 stage 0)
};

struct RingDev {
  int n;                    // limbs
  RnsPrime p[kMaxQ];
  const ulonglong2* fwd;    // [n][d] (w, w') psi^brv
  const ulonglong2* bwd;    // [n][d] psi^-brv
};

// CRT (Garner) constants for a source ring
struct CrtDev {
  int n;
  uint64_t q[kMaxQ];
  uint64_t inv[kMaxQ][kMaxQ], inv_sh[kMaxQ][kMaxQ];  // inv[j][k] = q_k^-1 mod q_j (k < j)
  uint64_t Q[4], Qhalf[4];                            // product (4 words) and floor(Q/2)
};

// destination mod constants: 2^(64k) mod q' for multiword reduction
struct DstDev {
  int n;
  uint64_t pw[kMaxQ][4], pw_sh[kMaxQ][4];
};

// The shape of one commit as the kernels see it (shape_of below)
struct JShape {
  int rank, rows, cols, slots, exp, d, in_msis, out_msis, mlwe, dcmp, log_in_cut, log_out_cut;
  int nq, nqo;
  uint64_t base;
  long long nv;
};

// ------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t sh_mul(uint64_t y, uint64_t w, uint64_t wp, uint64_t q) {
  return shoup_mul(y, w, wp, q);
}

// x R^-1 mod q (Slice = fromMont, element.go): Montgomery reduction alone, L^2 word products
// instead of the 2 L^2 of f_mul(x, 1).  For any x < R, (x + m q) / R < q + 1, so one conditional
// subtraction of q leaves the canonical residue (a non-canonical word such as x = q gives 0, as
// f_mul(x, 1) did).
template <int L>
__device__ __forceinline__ void f_redc(uint64_t* z, const uint64_t* x, const FieldParams<L>& F) {
  uint64_t t[L];
#pragma unroll
  for (int i = 0; i < L; ++i) t[i] = x[i];
#pragma unroll
  for (int i = 0; i < L; ++i) {
    const uint64_t m = t[0] * F.qinv;
    uint64_t lo, hi;
    mul_wide(m, F.q[0], lo, hi);
    uint32_t c0 = 0;
    addc(lo, t[0], c0);  // == 0 mod 2^64; only the carry is kept
    uint64_t carry = hi + c0;
#pragma unroll
    for (int j = 1; j < L; ++j) {
      mul_wide(m, F.q[j], lo, hi);
      uint32_t c = 0;
      lo = addc(lo, t[j], c);
      hi += c;
      c = 0;
      lo = addc(lo, carry, c);
      t[j - 1] = lo;
      carry = hi + c;
    }
    t[L - 1] = carry;
  }
  uint64_t d[L];
  uint32_t br = 0;
#pragma unroll
  for (int i = 0; i < L; ++i) d[i] = subb(t[i], F.q[i], br);
#pragma unroll
  for (int i = 0; i < L; ++i) z[i] = br ? t[i] : d[i];
}

// Encodes the reference does not perform (prover.go:101-105, 118-123): data rows j in
// [1, rows-2] of column i whose first index j*cols*slots (+ i*slots) is past len(v); their
// Opening.Encode stays zero.  The start index grows with j, so the reference's `break`
// is the same as testing each row.
__device__ __forceinline__ bool enc_skipped(const JShape& S, int col, int row) {
  if (row < 1 || row > S.rows - 2) return false;
  const long long cs = (long long)S.cols * S.slots;
  const long long start = row * cs + (col == S.cols ? 0 : (long long)col * S.slots);
  return start > S.nv;
}

// orders a wave's LDS accesses around a wave-private exchange (no workgroup barrier)
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
}

// d-point negacyclic NTT (Lattigo ordering: natural -> bit-reversed) of one limb held in LDS,
// by `nt` threads (thread index `ti`); synchronises the whole workgroup between stages.
__device__ inline void ntt_lds(uint64_t* p, int d, const ulonglong2* roots, uint64_t q, int ti, int nt, bool active) {
  int lt = 0;
  while ((2 << lt) < d) ++lt;  // log2(d/2)
  for (int m = 1, t = d >> 1; m < d; m <<= 1, t >>= 1, --lt) {
    if (active) {
      for (int k = ti; k < (d >> 1); k += nt) {
        const int i = k >> lt, j = (i << (lt + 1)) + (k & (t - 1));
        const ulonglong2 w = roots[m + i];
        const uint64_t u = p[j], v = sh_mul(p[j + t], w.x, w.y, q);
        p[j] = mod_add(u, v, q);
        p[j + t] = mod_sub(u, v, q);
      }
    }
    __syncthreads();
  }
}

// d-point inverse negacyclic NTT (GS, bit-reversed -> natural), times d^-1, of one limb held in
// LDS, by `nt` threads (thread index `ti`); synchronises the whole workgroup between stages
__device__ inline void intt_lds(uint64_t* p, int d, const ulonglong2* roots, const RnsPrime& P, int ti, int nt,
                                bool active) {
  const uint64_t q = P.q;
  for (int m = d >> 1, t = 1, lt = 0; m >= 1; m >>= 1, t <<= 1, ++lt) {
    if (active) {
      for (int k = ti; k < (d >> 1); k += nt) {
        const int i = k >> lt, j = (i << (lt + 1)) + (k & (t - 1));
        const ulonglong2 w = roots[m + i];
        const uint64_t u = p[j], v = p[j + t];
        p[j] = mod_add(u, v, q);
        p[j + t] = sh_mul(mod_sub(u, v, q), w.x, w.y, q);
      }
    }
    __syncthreads();
  }
  if (active)
    for (int k = ti; k < d; k += nt) p[k] = sh_mul(p[k], P.ninv, P.ninv_sh, q);
  __syncthreads();
}

struct MacArgs {
  int d, nl, J;            // degree, limbs, outputs per column
  long long ncols;         // B * columns
  int T1, T2;              // terms from operand set 1 / 2
  const uint64_t* A1;      // [J][T1][nl][d]   commit key
  const uint64_t* B1;      // [ncols][T1][nl][d] (stride b1_col per column, b1_term per term)
  long long b1_col, b1_term;
  const uint64_t* A2;      // [J][T2][nl][d]
  const uint64_t* B2;
  long long b2_col, b2_term;
  const uint64_t* C;       // added after reduction: [ncols][...] + j * c_j  (nullable)
  long long c_col, c_j;
  uint64_t* out;           // [ncols][J][nl][d]
  RnsPrime P[kMaxQ];
};

// acc += a * b as an exact multiword sum; WIDE keeps a third word (needed only when
// (q-1)^2 * terms could reach 2^128: decided per launch on the host).
template <bool WIDE>
struct Acc {
  uint64_t lo, hi;
  uint32_t top;
  __device__ __forceinline__ void zero() {
    lo = hi = 0;
    top = 0;
  }
  __device__ __forceinline__ void mac(uint64_t a, uint64_t b) {
    uint64_t pl, ph;
    mul_wide(a, b, pl, ph);
    uint32_t c = 0;
    lo = addc(lo, pl, c);
    if constexpr (WIDE) {
      uint32_t c2 = 0;
      hi = addc(hi, ph, c2);
      uint32_t c3 = 0;
      hi = addc(hi, (uint64_t)c, c3);
      top += c2 + c3;
    } else {
      hi += ph + c;
    }
  }
  // (lo + hi 2^64 + top 2^128) * 2^-64 mod q = lo 2^-64 + hi + top 2^64
  __device__ __forceinline__ uint64_t reduce(const RnsPrime& P) const {
    const uint64_t q = P.q;
    uint64_t r = sh_mul(lo, P.rinv, P.rinv_sh, q);
    r = mod_add(r, sh_mul(hi, 1, P.one_sh, q), q);
    if constexpr (WIDE) r = mod_add(r, sh_mul((uint64_t)top, P.r64, P.r64_sh, q), q);
    return r;
  }
};

struct RoundArgs {
  int d, cut;
  RingDev src, dst;
  CrtDev crt;
  DstDev dm;
  const uint64_t* in;  // [npoly][src.n][d]
  uint64_t* out;       // [npoly] at stride out_stride, dst.n limbs (+ zero rows up to out_rows)
  long long out_stride;
  int out_rows;
  long long npoly;     // round256_kernel's polynomials (round_kernel: the grid)
};

__device__ __forceinline__ void mw_muladd(uint64_t* v, int nw, uint64_t m, uint64_t add) {
  uint64_t carry = add;
  for (int i = 0; i < nw; ++i) {
    uint64_t lo, hi;
    mul_wide(v[i], m, lo, hi);
    uint32_t c = 0;
    lo = addc(lo, carry, c);
    v[i] = lo;
    carry = hi + c;
  }
}

// reconstructTo (rns.go:76-105) of one coefficient's residues r[ns] (coefficient domain): the
// centred value as sign (returned) and 4-word magnitude
__device__ __forceinline__ bool crt_centred(const CrtDev& crt, int ns, const uint64_t* r, uint64_t mag[4]) {
  bool neg;
  mag[0] = mag[1] = mag[2] = mag[3] = 0;
  if (ns == 1) {  // reconstructTo fast path: toBalanced (rns.go:68-73,78-91)
    const uint64_t q = crt.q[0];
    neg = r[0] > (q >> 1);
    mag[0] = neg ? q - r[0] : r[0];
  } else {  // Garner: V = x0 + q0 (x1 + q1 (x2 + ...)) in [0, Q)  (rns.go:93-99)
    uint64_t x[kMaxQ];
    for (int j = 0; j < ns; ++j) {
      const uint64_t qj = crt.q[j];
      uint64_t v = r[j];
      for (int kk = 0; kk < j; ++kk) {
        uint64_t xk = x[kk];
        // x_k < q_k must be below q_j for mod_sub: one subtraction where q_k < 2 q_j (primes of
        // one bit size, every NewParameters ring), x_k % q_j for any other pair of primes
        if (xk >= qj) xk = (xk - qj >= qj) ? xk % qj : xk - qj;
        v = mod_sub(v, xk, qj);
        v = sh_mul(v, crt.inv[j][kk], crt.inv_sh[j][kk], qj);
      }
      x[j] = v;
    }
    uint64_t V[4] = {x[ns - 1], 0, 0, 0};
    for (int j = ns - 2; j >= 0; --j) mw_muladd(V, 4, crt.q[j], x[j]);
    // V >= floor(Q/2) -> V - Q (rns.go:100-102)
    bool ge = true;
    for (int i = 3; i >= 0; --i) {
      if (V[i] != crt.Qhalf[i]) {
        ge = V[i] > crt.Qhalf[i];
        break;
      }
    }
    neg = ge;
    if (neg) {
      uint32_t br = 0;
      for (int i = 0; i < 4; ++i) mag[i] = subb(crt.Q[i], V[i], br);
    } else {
      for (int i = 0; i < 4; ++i) mag[i] = V[i];
    }
  }
  return neg;
}

}  // namespace rg

// ------------------------------------------------------------------------------------------
// the handle
// ------------------------------------------------------------------------------------------
// Scratch of one commit stream: digits [B][cols+1][rows][d] u32, inner commitments
// [B][cols+1][inMSIS][nq][d], outer [B][outMSIS][nqo][d].  One per stream, so calls on
// different streams never share scratch (calls on one stream are ordered by the stream).
struct rg_jindo_scratch {
  rg::DevBuf digits, com, ocom;
  rg::DevBuf last, mask, en, mn;  // the sampled randomness of rg_jindo_commit_sampled_dev
  rg::DevBuf wq;                  // cdt2_noise_kernel's chunk counter
  rg::DevBuf point;               // rg_jindo_eval_point_dev: x^0 .. x^(cols slots), then leftVec [rows]
};

// Sampler setup (rg_jindo_set_stddevs): the reference's six standard deviations and the tables
// derived from them on the host (csprng_host.hpp)
struct rg_jindo_samplers {
  bool ready = false;
  double sd[6];  // ecd, ecd_blind, mask, mask_blind, mlwe, mask_mlwe
  rg::DevBuf te0, cdt_enc, cdt_guide, cdt_sbound, cdt_jmax, cdt_mlwe, zig, delta;
  int cdt_enc_size = 0, cdt_mlwe_size = 0;
  int64_t tail_lo_enc = 0, tail_lo_mlwe = 0;
  std::vector<double> h_delta;
};

struct rg_jindo {
  rg_jindo_params p;
  rg_field field;
  int device = 0;  // the handle's buffers live on this device
  rg::RnsPrime rq[rg::kMaxQ], ro[rg::kMaxQ];
  rg::DevBuf rootsq_f, rootsq_b, rootso_f, rootso_b;
  rg::CrtDev crt_q, crt_o;
  rg::DstDev dst_o, dst_q;
  rg::DevBuf ck_in, ck_mlwe, ck_out;  // the commit key, device-resident (entities.go:21-73 layouts)
  rg::DevBuf ckm_in, ckm_out;  // the same as base-256 digits for mac_mfma (inner, outer)
  int mfma_q = 0, mfma_o = 0;  // digits per residue of the MFMA MAC (0: mac_kernel)
  uint64_t base_inv;
  std::mutex mu;  // guards `scratch` and `aux`
  std::map<hipStream_t, std::unique_ptr<rg_jindo_scratch>> scratch;
  rg_jindo_samplers smp;
  // the sampled commit's helper streams and events, one set per caller stream (lazily created):
  // s[0] runs the COSAC centres + cosac2, s[1] the MLWE samplers and their prep (commit_sampled_dev)
  struct Aux {
    hipStream_t s[2] = {nullptr, nullptr};
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
  };
  std::map<hipStream_t, Aux> aux;
  ~rg_jindo() {
    for (auto& kv : aux) {
      for (hipStream_t x : kv.second.s)
        if (x) (void)hipStreamDestroy(x);
      for (hipEvent_t x : kv.second.e)
        if (x) (void)hipEventDestroy(x);
    }
  }
};

namespace rg {

// bit length of the L-word value x (0 for x = 0)
inline int bit_length(const uint64_t* x, int L) {
  for (int l = L - 1; l >= 0; --l)
    if (x[l]) return 64 * l + 64 - __builtin_clzll(x[l]);
  return 0;
}

// bit length of the field modulus
inline int field_bits(const rg_field& f) { return bit_length(f.q, f.L); }

inline JShape shape_of(const rg_jindo_params& p, long long nv) {
  JShape s;
  s.rank = p.rank;
  s.rows = p.rows;
  s.cols = p.cols;
  s.slots = p.slots;
  s.exp = p.exp;
  s.d = p.d;
  s.in_msis = p.in_msis;
  s.out_msis = p.out_msis;
  s.mlwe = p.mlwe;
  s.dcmp = p.dcmp;
  s.log_in_cut = p.log_in_cut;
  s.log_out_cut = p.log_out_cut;
  s.nq = p.nq;
  s.nqo = p.nqo;
  s.base = p.base;
  s.nv = nv;
  return s;
}

// Byte sizes of the per-commit buffers of `batch` commits (layouts: include/ringo.h), in one place
// for the stream scratch, the host entry points' staging buffers and the verifier
struct JSizes {
  size_t digits;        // [B][cols+1][rows][d] u32
  size_t inner, outer;  // the MACs' sums before rounding: [B][cols+1][inMSIS][nq][d], [B][outMSIS][nqo][d]
  size_t last, mask;    // [B][cols*slots][L], [B][rows][slots][L]
  size_t en, mn;        // the noise, i64: [B][cols+1][rows][d], [B][cols+1][nm][d] (nm = inMSIS + mlwe)
  size_t enc, mlwe;     // Opening.Encode [B][cols+1][rows][nq][d], Opening.MLWE [B][cols+1][nm][nq][d]
  size_t incom, com;    // Opening.InCommit [B][dcmp][nqo][d], Commitment.Value [B][outMSIS][nq][d]
  // what stream_scratch allocates for every commit (rg_jindo_scratch_bytes)
  size_t scratch() const { return digits + inner + outer; }
};
inline JSizes sizes_of(const rg_jindo_params& p, size_t batch) {
  const size_t d = p.d, L = p.field_limbs, nm = p.in_msis + p.mlwe, c1 = batch * (p.cols + 1);
  JSizes z;
  z.digits = c1 * p.rows * d * 4;
  z.inner = c1 * p.in_msis * p.nq * d * 8;
  z.outer = batch * p.out_msis * p.nqo * d * 8;
  z.last = batch * p.cols * p.slots * L * 8;
  z.mask = batch * p.rows * p.slots * L * 8;
  z.en = c1 * p.rows * d * 8;
  z.mn = c1 * nm * d * 8;
  z.enc = c1 * p.rows * p.nq * d * 8;
  z.mlwe = c1 * nm * p.nq * d * 8;
  z.incom = batch * p.dcmp * p.nqo * d * 8;
  z.com = batch * p.out_msis * p.nq * d * 8;
  return z;
}

// ---- jindo_setup.hip ----
RingDev ring_dev(const RnsPrime* P, int n, const DevBuf& f, const DevBuf& b);
rg_status on_device(const rg_jindo* J);
// the calling stream's scratch, grown to `batch` commits
rg_status stream_scratch(rg_jindo* J, size_t batch, hipStream_t st, rg_jindo_scratch** out);
struct MfmaPrime;  // mac_mfma.hpp
MfmaPrime mfma_prime(const RnsPrime& P);

// ---- jindo_commit.hip ----
rg_status launch_mac(const MacArgs& m, hipStream_t st);
// a CRT rounding from ring Q_out (src_o) or Q into Q_out (dst_o) or Q
RoundArgs round_args(const rg_jindo* J, bool src_o, bool dst_o, int cut, const uint64_t* in, uint64_t* out,
                     long long out_stride, int out_rows);
rg_status launch_round(RoundArgs ra, long long npoly, hipStream_t st);
MacArgs dot_args(const RnsPrime* P, int nl, int d, long long nout, int T, const uint64_t* A, const uint64_t* B,
                 long long b_out, long long b_term, uint64_t* out);
// the commit's stages, as the sampled commit's stream DAG (jindo_sample.hip) schedules them
rg_status digits_stage(rg_jindo* J, size_t batch, const uint64_t* d_v, size_t nv, const uint64_t* d_last,
                       const uint64_t* d_mask, uint32_t* digits, hipStream_t st);
enum PrepPart { kPrepAll = 3, kPrepEnc = 1, kPrepMlwe = 2 };
rg_status prep_launch(rg_jindo* J, size_t batch, size_t nv, const uint32_t* digits, const int64_t* d_en,
                      const int64_t* d_mn, uint64_t* d_enc, uint64_t* d_mlwe, int part, hipStream_t st);
rg_status commit_core(rg_jindo* J, size_t batch, const uint64_t* d_enc, const uint64_t* d_mlwe, uint64_t* d_incom,
                      uint64_t* d_com, rg_jindo_scratch* sc, hipStream_t st);

}  // namespace rg
