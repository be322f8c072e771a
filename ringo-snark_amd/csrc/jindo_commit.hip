// jindo_commit.hip -- the Jindo commitment (jindo/prover.go:45-202) on gfx950, batched over
// independent commits, with the prover's randomness injected (include/ringo.h) or sampled on the
// device (jindo_sample.hip).  The handle and its tables are jindo_setup.hip.
//
// Commit pipeline per batch of B commits (all device-resident, one stream):
//   1. digits_kernel   thread per (commit, column, row, slot): source element (v, firstRow =
//                      v - lastRow shifted, lastRow, mask; prover.go:65-128) -> fromMont ->
//                      base-b digits (encoder.go:120-146, utils.go:12-19), two per long
//                      division by b^2, into the encode's coefficient slots j*slots+i.
//   2. prep256_kernel  wave per ring polynomial (d = 256; prep_kernel, a workgroup per
//                      polynomial, covers other d): the randEncode tail (encoder.go:166-200:
//                      MForm(noise), X^slots negacyclic shift, - b*s, + MForm(digits)) or the
//                      MLWE finalize (prover.go:130-141), then the 256-point negacyclic NTT per
//                      RNS limb in registers (Lattigo ordering/roots).
//   3. the inner Ajtai product, a per-(limb, coeff) modular GEMM
//                      sum_k In[j][k]*Enc[k] + sum_k CK.MLWE[j][k]*MLWE[k] + MLWE[mlwe+j]
//                      (prover.go:149-157): exact sums reduced once (MulCoeffsMontgomeryThenAdd
//                      summed == (sum a*b) * 2^-64 mod q).  mac_mfma_kernel (mac_mfma.hip, the
//                      matrix cores) where its digit bound holds (every configs shape); else
//                      mac_kernel (exact 128/160-bit sums, any prime and J).  Round 2-5's VALU
//                      Karatsuba MAC (mac3h) is tools/experiments/jindo_knob_kernels.patch.
//   4. round_kernel    workgroup per polynomial: IMForm, INTT, centred CRT (Garner, up to 4
//                      primes), floor shift by the cut, Euclidean mod q', MForm, NTT in the
//                      destination ring (prover.go:164-176, rns.go:76-114).
//   5. the MAC + round_kernel again for the outer commitment (prover.go:180-202).
// The sampled commit (jindo_sample.hip, section 6) draws the randomness first and runs these
// stages as a DAG over three streams.
// Evaluate and Verifier.Verify: every MulCoeffsMontgomeryThenAdd loop is a J = 1 dot product on
// mac_kernel; their entry points and the verifier's norm, decode and dot kernels are
// jindo_verify.hip (shared definitions: jindo_impl.hpp).
// All residues are canonical, so results are bit-exact against the reference's Lattigo
// calls given the same primes (Lattigo conventions restated: see DESIGN.md, "parity").
#include <algorithm>
#include <cmath>
#include <cstring>

#include "digits_dc.hpp"
#include "jindo_impl.hpp"
#include "mac_mfma.hpp"
#include "ntt64.hpp"

namespace rg {

__device__ __forceinline__ uint64_t signed_residue(long long c, uint64_t q) {
  // setCoeffSigned (utils.go:49-61): c >= 0 -> c ; else Go's c%q + q (== q when q | c; the
  // following MForm maps that to 0 either way)
  if (c >= 0) return (uint64_t)c < q ? (uint64_t)c : (uint64_t)c % q;
  const uint64_t a = (uint64_t)(-(c + 1)) + 1;
  return a < q ? q - a : q - a % q;
}

// ------------------------------------------------------------------------------------------
// 1. digits
// ------------------------------------------------------------------------------------------
template <int L>
struct DigitArgs {
  JShape s;
  FieldParams<L> F;
  uint64_t base_inv;  // floor(2^64 / base)
  uint64_t b2, b2_inv;  // base^2 and floor(2^64 / base^2) when base^2 < 2^32, else 0
  DigitDc dc;           // divide-and-conquer constants (digits_dc.hpp); dc.exp = 0: the loop below
  const uint64_t* v;         // [B][nv][L]
  const uint64_t* last_row;  // [B][cols*slots][L]
  const uint64_t* mask;      // [B][rows][slots][L]
  uint32_t* digits;          // [B][cols+1][rows][d]
  long long total;           // B * (cols+1) * rows * slots
  IdxDiv d_slots, d_rows, d_cols1;  // total < 2^32: the index split by idx_div (else 64-bit division)
};

// divstep's step (digits_dc.hpp) for a divisor d in (2^31, 2^32) (b^2 of every configs field: 60272^2, 60256^2),
// whose reciprocal is 2^32 + B0: hi64(num (2^32 + B0)) = r + hi32(r B0 + n0 + hi32(n0 B0)) for
// num = r 2^32 + n0 -- three 32-bit multiplies instead of a 64 x 64 high product and a 64-bit
// product
__device__ __forceinline__ uint32_t divstep_b2(uint32_t r, uint32_t n0, uint32_t d, uint32_t B0, uint32_t& rem) {
  const uint64_t t = mad64(r, B0, (uint64_t)n0 + __umulhi(n0, B0));
  uint32_t qt = r + (uint32_t)(t >> 32);
  uint64_t rm = (((uint64_t)r << 32) | n0) - (uint64_t)qt * d;
  if (rm >= d) {
    rm -= d;
    ++qt;
  }
  rem = (uint32_t)rm;
  return qt;
}

template <int L>
__global__ __launch_bounds__(256) void digits_kernel(DigitArgs<L> a) {
  const JShape& S = a.s;
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= a.total) return;
  int slot, row, col;
  long long b;
  if (a.total <= 0xffffffffLL) {  // (slot, row, col, b) without 64-bit divisions
    const uint32_t g = (uint32_t)gid, q1 = idx_div(g, a.d_slots), q2 = idx_div(q1, a.d_rows),
                   q3 = idx_div(q2, a.d_cols1);
    slot = (int)(g - q1 * a.d_slots.d);
    row = (int)(q1 - q2 * a.d_rows.d);
    col = (int)(q2 - q3 * a.d_cols1.d);
    b = q3;
  } else {
    slot = (int)(gid % S.slots);
    long long r = gid / S.slots;
    row = (int)(r % S.rows);
    r /= S.rows;
    col = (int)(r % (S.cols + 1));
    b = r / (S.cols + 1);
  }
  const long long cs = (long long)S.cols * S.slots;
  const uint64_t* vb = a.v + b * S.nv * L;
  uint32_t* out = a.digits + (((b * (S.cols + 1) + col) * S.rows + row) * (long long)S.d);

  // which element feeds this slot (prover.go:89-128); `have` = false -> zero slot
  uint64_t x[L];
  bool have = true;
  if (col == S.cols) {  // mask column: every slot present
    const uint64_t* m = a.mask + ((b * S.rows + row) * S.slots + slot) * L;
    el_copy<L>(x, m);
  } else if (row == S.rows - 1) {  // last row
    const uint64_t* m = a.last_row + (b * cs + (long long)col * S.slots + slot) * L;
    el_copy<L>(x, m);
  } else if (row == 0) {  // first row: v[i] - lastRow[i-1] (genFirstLastRow :74-83)
    const long long i = (long long)col * S.slots + slot;
    uint64_t vi[L], lr[L];
#pragma unroll
    for (int l = 0; l < L; ++l) vi[l] = (i < S.nv) ? vb[i * L + l] : 0;
    if (i == 0) {
#pragma unroll
      for (int l = 0; l < L; ++l) x[l] = vi[l];
    } else {
      const uint64_t* m = a.last_row + (b * cs + i - 1) * L;
      el_copy<L>(lr, m);
      f_sub<L>(x, vi, lr, a.F);
    }
  } else {  // data row: v[row*cs + col*slots + slot] when < nv
    const long long i = row * cs + (long long)col * S.slots + slot;
    have = i < S.nv;
#pragma unroll
    for (int l = 0; l < L; ++l) x[l] = have ? vb[i * L + l] : 0;
  }
  // canonical limbs (Slice = fromMont)
  uint64_t c[L];
  f_redc<L>(c, x, a.F);
  if (!have) {
#pragma unroll
    for (int l = 0; l < L; ++l) c[l] = 0;
  }
  // base-b digits: exp-1 remainders then the final quotient (encoder.go:125-136)
  if constexpr (L == 4 || L == 2) {
    if (a.dc.exp == S.exp) {  // every configs field: by divide and conquer (digits_dc.hpp)
      dc_digits<L>(c, a.dc, [&](int j, uint32_t dg) { out[j * S.slots + slot] = dg; });
      return;
    }
  }
  uint32_t w[2 * L];
#pragma unroll
  for (int l = 0; l < L; ++l) {
    w[2 * l] = (uint32_t)c[l];
    w[2 * l + 1] = (uint32_t)(c[l] >> 32);
  }
  int jd = 0;
  if (a.b2) {  // two digits per long division: divide by b^2 (< 2^32), split the remainder
    // words above `top` are zero (the value shrinks ~2 log2(b) bits a pass); the word loop stays
    // unrolled with a predicate so w[] is never indexed dynamically (registers, not scratch)
    auto top_of = [&]() {
      int tp = 0;
#pragma unroll
      for (int k = 1; k < 2 * L; ++k) tp = w[k] ? k : tp;
      return tp;
    };
    int top = top_of();
    const bool b2fast = (a.b2_inv >> 32) == 1;  // uniform: d in (2^31, 2^32)
    for (; jd + 1 < S.exp - 1; jd += 2) {
      uint64_t rem = 0;
      if (b2fast) {
        uint32_t r32 = 0;
#pragma unroll
        for (int k = 2 * L - 1; k >= 0; --k)
          if (k <= top) w[k] = divstep_b2(r32, w[k], (uint32_t)a.b2, (uint32_t)a.b2_inv, r32);
        rem = r32;
      } else {
#pragma unroll
        for (int k = 2 * L - 1; k >= 0; --k)
          if (k <= top) w[k] = divstep((rem << 32) | w[k], a.b2, a.b2_inv, rem);
      }
      top = top_of();
      uint64_t lo;
      const uint32_t hi = divstep(rem, S.base, a.base_inv, lo);
      out[jd * S.slots + slot] = (uint32_t)lo;
      out[(jd + 1) * S.slots + slot] = hi;
    }
  }
  for (; jd < S.exp - 1; ++jd) {
    uint64_t rem = 0;
#pragma unroll
    for (int k = 2 * L - 1; k >= 0; --k) w[k] = divstep((rem << 32) | w[k], S.base, a.base_inv, rem);
    out[jd * S.slots + slot] = (uint32_t)rem;
  }
  out[(S.exp - 1) * S.slots + slot] = w[0];
}

// Coefficients [slots * exp, d) of a digit polynomial belong to no slot (slots * exp < d: never a
// NewParameters shape, but rg_jindo_create accepts it); launch_digits zeroes the buffer then.

// ------------------------------------------------------------------------------------------
// 2. prep: encode tail / MLWE finalize + NTT
// ------------------------------------------------------------------------------------------
struct PrepArgs {
  JShape s;
  RingDev R;
  const uint32_t* digits;     // [B][cols+1][rows][d]
  const long long* enc_noise;  // [B][cols+1][rows][d]
  const long long* mlwe_noise; // [B][cols+1][nm][d]
  uint64_t* enc;               // [B][cols+1][rows][nq][d]
  uint64_t* mlwe;              // [B][cols+1][nm][nq][d]
  long long n_enc;             // B * (cols+1) * rows
  long long n_ml;              // B * (cols+1) * (inMSIS + mlwe)
  long long clim;              // |noise| bound for the one-integer encode form: 2^61 / base
};

__global__ __launch_bounds__(256) void prep_kernel(PrepArgs a) {
  __shared__ uint64_t poly[kMaxQ][kMaxD];
  const JShape& S = a.s;
  const int d = S.d, nq = S.nq, tid = threadIdx.x;
  const int nm = S.in_msis + S.mlwe;
  const long long job = blockIdx.x;
  const bool is_enc = job < a.n_enc;
  uint64_t* dst;
  if (is_enc) {
    const long long pj = job;
    const int cr = (int)(pj % ((long long)(S.cols + 1) * S.rows));
    dst = a.enc + pj * nq * d;
    if (enc_skipped(S, cr / S.rows, cr % S.rows)) {  // Opening.Encode[i][j] stays zero
      for (int k = tid; k < nq * d; k += blockDim.x) dst[k] = 0;
      return;
    }
    const uint32_t* dg = a.digits + pj * d;
    const long long* nz = a.enc_noise + pj * d;
    for (int k = tid; k < d; k += blockDim.x) {
      const long long c = nz[k];
      // the X^slots shift: coefficient k receives s[k - slots] (k >= slots) or -s[k + d - slots]
      const int ks = k - S.slots;
      const long long cs = ks >= 0 ? nz[ks] : nz[ks + d];
      const uint64_t dgk = dg[k];
      for (int l = 0; l < nq; ++l) {
        const RnsPrime& P = a.R.p[l];
        const uint64_t q = P.q;
        const uint64_t sm = sh_mul(signed_residue(c, q), P.r64, P.r64_sh, q);    // MForm(s) :184
        uint64_t sh = sh_mul(signed_residue(cs, q), P.r64, P.r64_sh, q);
        if (ks < 0) sh = mod_neg(sh, q);  // wrapped coefficients negate (:191-195)
        sh = mod_sub(sh, sh_mul(sm, P.bmod, P.bmod_sh, q), q);                   // :196
        const uint64_t dm = sh_mul(dgk, P.r64, P.r64_sh, q);  // MForm(digits) :198 (digit <= b < q)
        poly[l][k] = mod_add(dm, sh, q);                                          // :199
      }
    }
  } else {
    const long long mj = job - a.n_enc;  // (b, col, j) flattened
    dst = a.mlwe + mj * nq * d;
    const long long* nz = a.mlwe_noise + mj * d;
    for (int k = tid; k < d; k += blockDim.x) {
      const long long c = nz[k];
      for (int l = 0; l < nq; ++l) {
        const RnsPrime& P = a.R.p[l];
        poly[l][k] = sh_mul(signed_residue(c, P.q), P.r64, P.r64_sh, P.q);  // MForm (prover.go:140)
      }
    }
    (void)nm;
  }
  __syncthreads();
  // NTT per limb: two limbs at a time on the two halves of the workgroup
  const int half = blockDim.x >> 1;
  for (int l0 = 0; l0 < nq; l0 += 2) {
    const int l = l0 + (tid >= half ? 1 : 0);
    const bool active = l < nq;
    const int lc = active ? l : l0;
    ntt_lds(poly[lc], d, a.R.fwd + (long long)lc * d, a.R.p[lc].q, tid % half, half, active);
  }
  for (int k = tid; k < nq * d; k += blockDim.x) dst[k] = poly[k / d][k % d];
}

// Wave-per-polynomial prep for d = 256 (every Jindo parameter set): one wave owns one job and two
// RNS limbs at a time (lanes 0-31 limb l0, 32-63 limb l0+1), 8 coefficients per lane; the
// 256-point negacyclic NTT runs as rounds of 3 + 3 + 2 radix-2 stages in registers with
// wave-local LDS exchanges (no workgroup barrier; ntt64.hpp's ROW index algebra with hi = 0),
// lazy [0, 2q) Shoup arithmetic, canonical output.  Same results as prep_kernel.
constexpr int kPrepWaves = 4;

// The index algebra of the wave transforms (prep256_kernel, round256_kernel), in one place.
// A lane (t = lane & 31) holds 8 points e[0..8) of its half-wave's 256-point limb in one of three
// patterns PAT: H (point t + 32 rho), M (rho in bits 2-4) and L (point 8 t + rho).  A round of RK
// radix-2 stages on bits LO .. LO + RK - 1 runs in registers; wave_pairs hands every butterfly's
// register pair and twiddle index to bfly(rho0, rho1, wi), stage by stage from stage SP0 (forward:
// high bit first; INV: low bit first).
template <int RK, int LO, int PAT, bool INV, int SP0, class F>
__device__ __forceinline__ void wave_pairs(uint32_t t, F&& bfly) {
  auto xof = [&](int rho) -> uint32_t {
    if (PAT == 0) return t + 32u * rho;
    if (PAT == 1) return ((t >> 2) << 5) | ((uint32_t)rho << 2) | (t & 3u);
    return 8u * t + rho;
  };
  constexpr int NPK = 1 << RK;
#pragma unroll
  for (int sp = SP0; sp < RK; ++sp) {
    const int bw = INV ? sp : RK - 1 - sp, b = LO + bw, k = 7 - b, half = 1 << bw;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int grp = j / (NPK / 2), jj = j % (NPK / 2);
      const int rho0 = grp * NPK + ((jj >> bw) << (bw + 1)) + (jj & (half - 1));
      bfly(rho0, rho0 + half, (1u << k) + (xof(rho0) >> (b + 1)));
    }
  }
}

// Between rounds the points move through the wave's 288-word LDS row at `row` (ntt64.hpp's ROW
// index algebra with hi = 0): lane t's offsets for the H pattern (+ 36 y padded, + 33 y or + 32 y
// natural order), the M pattern (+ 4 y, + (y >> 1) padded) and the L pattern (9 t + r padded,
// 8 t + (t >> 2) + r)
struct WaveRows {
  uint32_t H, M, L9, L8;
};
__device__ __forceinline__ WaveRows wave_rows(uint32_t row, uint32_t t) {
  return WaveRows{row + t, row + 36 * (t >> 2) + (t & 3), row + 9 * t, row + 8 * t + (t >> 2)};
}

template <int RK, int LO, int PAT, int SP0 = 0, bool LAZY = false>
__device__ __forceinline__ void prep_round(uint64_t (&e)[8], const ulonglong2* roots, uint64_t q, uint64_t q2,
                                           uint32_t t) {
  wave_pairs<RK, LO, PAT, false, SP0>(t, [&](int rho0, int rho1, uint32_t wi) {
    const ulonglong2 w = roots[wi];  // the limb's table, staged in LDS
    // Harvey with a 4q-wide twiddle product: values in [0, 8q) (ring primes < 2^61), x
    // reduced to [0, 4q), t = y w - Q' q in [0, 4q) with Q' the Shoup quotient less the low
    // cross products (Q - 2 <= Q' <= Q): three 32-bit multiplies for the quotient, not four
    // x >= 4q ? x - 4q : x, on the borrow (q2 = 4q here); LAZY (36 q < 2^64): x unreduced, each
    // stage widens the bound by 4q, [0, 8q) after stage 0 -> [0, 36q) after stage 7
    const uint64_t x = LAZY ? e[rho0] : canon_x(e[rho0], q2);
    const uint64_t y = e[rho1];
    const uint32_t y0 = (uint32_t)y, y1 = (uint32_t)(y >> 32), p0 = (uint32_t)w.y, p1 = (uint32_t)(w.y >> 32);
    const uint64_t qa = mad64(y1, p1, __umulhi(y1, p0)) + __umulhi(y0, p1);
    const uint64_t tt = y * w.x - qa * q;
    e[rho0] = x + tt;
    e[rho1] = x + q2 - tt;
  });
}

// y w mod q in [0, 3q) for any 64-bit y: prep_round's Shoup product with the 3-multiply quotient
__device__ __forceinline__ uint64_t shoup3(uint64_t y, uint64_t w, uint64_t wp, uint64_t q) {
  const uint32_t y0 = (uint32_t)y, y1 = (uint32_t)(y >> 32), p0 = (uint32_t)wp, p1 = (uint32_t)(wp >> 32);
  const uint64_t qa = mad64(y1, p1, __umulhi(y1, p0)) + __umulhi(y0, p1);
  return y * w - qa * q;
}

// signed integer -> residue in [0, q) without division (Shoup by 1 reduces any 64-bit value)
__device__ __forceinline__ uint64_t red_signed(long long c, const RnsPrime& P) {
  const uint64_t ac = c < 0 ? (uint64_t)(-(c + 1)) + 1 : (uint64_t)c;
  const uint64_t m = sh_mul(ac, 1, P.one_sh, P.q);
  return c < 0 ? mod_neg(m, P.q) : m;
}

template <int MINW, bool PAIR1, int WAVES = kPrepWaves, bool LAZY = false>
__global__ __launch_bounds__(64 * WAVES, MINW) void prep256_kernel(PrepArgs a) {
  __shared__ uint64_t lds_all[WAVES][2 * 288];
  extern __shared__ ulonglong2 tw_lds[];  // the nq limbs' forward tables (w, w'), [nq][256]: dynamic LDS
  const JShape& S = a.s;
  const int nq = S.nq;
  const uint32_t lane = threadIdx.x & 63u, t = lane & 31u, hs = lane >> 5;
  const int wv = threadIdx.x >> 6;
  uint64_t* lds = lds_all[wv];
  const long long job = (long long)blockIdx.x * WAVES + wv;
  const bool has = job < a.n_enc + a.n_ml;
  const bool is_enc = job < a.n_enc;
  uint64_t* dst = nullptr;
  const uint32_t* dg = nullptr;
  const long long* nz = nullptr;
  bool skip = false;
  if (has && is_enc) {
    const long long pj = job;
    const int cr = (int)(pj % ((long long)(S.cols + 1) * S.rows));
    dst = a.enc + pj * nq * 256;
    skip = enc_skipped(S, cr / S.rows, cr % S.rows);  // Opening.Encode[i][j] stays zero
    dg = a.digits + pj * 256;
    nz = a.enc_noise + pj * 256;
  } else if (has) {
    const long long mj = job - a.n_enc;
    dst = a.mlwe + mj * nq * 256;
    nz = a.mlwe_noise + mj * 256;
  }
  // the job's inputs (noise, shifted noise, digits).  PAIR1 (nq <= 2, every configs ring): loaded
  // ahead of the table staging so the two loads' latencies overlap (configs[2] +1.4%); otherwise
  // read per limb pair after it, rather than held across the NTT
  long long cv[8], csv[8];
  uint32_t dv[8];
  auto load_in = [&]() {
#pragma unroll
    for (int y = 0; y < 8; ++y) {
      const int k = (int)t + 32 * y;
      cv[y] = nz[k];
      if (is_enc) {
        const int ks = k - S.slots;
        csv[y] = ks >= 0 ? nz[ks] : nz[ks + 256];
        dv[y] = dg[k];
      } else {
        csv[y] = 0;
        dv[y] = 0;
      }
    }
  };
  if (PAIR1 && has && !skip) load_in();
  // slot 0 of each limb's table (unused by the transform) holds (2^64 w1, Shoup) for stage 0
  for (int i = threadIdx.x; i < nq * 256; i += blockDim.x)
    tw_lds[i] = (i & 255) ? a.R.fwd[i] : make_ulonglong2(a.R.p[i >> 8].rw1, a.R.p[i >> 8].rw1_sh);
  __syncthreads();
  if (!has) return;
  if (skip) {
    for (int k = (int)lane; k < nq * 256; k += 64) dst[k] = 0;
    return;
  }
  const WaveRows wr = wave_rows(288 * hs, t);
  auto pair = [&](const int l0) {
    const int limb = l0 + (int)hs;
    const bool active = limb < nq;
    const int lc = active ? limb : l0;
    const RnsPrime& P = a.R.p[lc];
    const uint64_t q = P.q, q2 = 4 * q;  // prep_round's lazy bound: values in [0, 2 q2)
    const ulonglong2* roots = tw_lds + lc * 256;
    // The encode tail MForm(dg) + MForm(+-s') - MForm(s) b (encoder.go:184-199) is MForm of ONE
    // signed integer v = dg +- s' - s b when that fits (|s| <= 2^61 / b, |s'| < 2^61); the MLWE
    // finalize is MForm(setCoeffSigned(s)) (prover.go:130-141): v = s.  MForm is a factor 2^64 on
    // every coefficient, so it rides on NTT stage 0: e holds v mod q (one add when |v| < q), and
    // stage 0 multiplies by 2^64 and 2^64 w1 instead of w1.
    uint64_t e[8];
    uint32_t big = 0;  // bit y: coefficient t + 32 y takes the term-by-term reduction
#pragma unroll
    for (int y = 0; y < 8; ++y) {
      const int k = (int)t + 32 * y;
      const long long c = cv[y];
      long long v = c;
      bool ok = true;
      if (is_enc) {
        const long long cs = csv[y];
        const uint64_t s2 = k < S.slots ? 0ull - (uint64_t)cs : (uint64_t)cs;  // wrapped coefficients negate
        ok = c >= -a.clim && c <= a.clim && cs > -(1LL << 61) && cs < (1LL << 61);
        v = (long long)((uint64_t)dv[y] + s2 - (uint64_t)c * S.base);
      }
      const uint64_t r = v < 0 ? (uint64_t)v + q : (uint64_t)v;  // v mod q when -q <= v < q
      ok = ok && r < q;
      big |= ok ? 0u : (1u << y);
      e[y] = r;
    }
    if (big) {  // rare (huge injected noise): every term reduced separately, same residue
      for (int y = 0; y < 8; ++y) {
        if (!((big >> y) & 1u)) continue;
        const int k = (int)t + 32 * y;
        if (is_enc) {
          const int ks = k - S.slots;
          const uint64_t cm = red_signed(nz[k], P);
          uint64_t s2 = red_signed(ks >= 0 ? nz[ks] : nz[ks + 256], P);
          if (k < S.slots) s2 = mod_neg(s2, q);
          const uint64_t val = mod_add(sh_mul(dg[k], 1, P.one_sh, q), s2, q);
          e[y] = mod_sub(val, sh_mul(cm, P.bmod, P.bmod_sh, q), q);
        } else {
          e[y] = red_signed(nz[k], P);
        }
      }
    }
    {  // stage 0 (pairs y, y + 4 of the H pattern, root w1) times 2^64: inputs in [0, q), outputs
       // in [0, 8q) like every later stage's
      const ulonglong2 rw = roots[0];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint64_t xr = shoup3(e[j], P.r64, P.r64_sh, q), yr = shoup3(e[j + 4], rw.x, rw.y, q);
        e[j] = xr + yr;
        e[j + 4] = xr + q2 - yr;
      }
    }
    // NTT: H round (stages 1-2; 0 above), H->M, M round (3-5), M->L, L round (6-7), L->H, store
    prep_round<3, 5, 0, 1, LAZY>(e, roots, q, q2, t);
#pragma unroll
    for (int y = 0; y < 8; ++y) lds[wr.H + 36 * y] = e[y];
    wave_lds_fence();
#pragma unroll
    for (int y = 0; y < 8; ++y) e[y] = lds[wr.M + 4 * y];
    prep_round<3, 2, 1, 0, LAZY>(e, roots, q, q2, t);
    wave_lds_fence();
#pragma unroll
    for (int y = 0; y < 8; ++y) lds[wr.M + 4 * y + (y >> 1)] = e[y];
    wave_lds_fence();
#pragma unroll
    for (int r = 0; r < 8; ++r) e[r] = lds[wr.L9 + r];
    prep_round<2, 0, 2, 0, LAZY>(e, roots, q, q2, t);
    wave_lds_fence();
#pragma unroll
    for (int r = 0; r < 8; ++r)  // [0, 8q) (LAZY: [0, 36q), Shoup by 1) -> [0, q)
      lds[wr.L8 + r] = LAZY ? shoup_mul(e[r], 1, P.one_sh, q) : canon_x(canon_x(canon_x(e[r], q2), 2 * q), q);
    wave_lds_fence();
    if (active) {
      uint64_t* o = dst + (long long)limb * 256;
#pragma unroll
      for (int y = 0; y < 8; ++y) o[t + 32 * y] = lds[wr.H + 33 * y];
    }
    wave_lds_fence();
  };
  if constexpr (PAIR1) {
    pair(0);
  } else {
    for (int l0 = 0; l0 < nq; l0 += 2) {
      load_in();
      pair(l0);
    }
  }
}

// ------------------------------------------------------------------------------------------
// 3. multiply-accumulate (inner / outer Ajtai products)
// ------------------------------------------------------------------------------------------
// Thread = (column group of NC columns, limb*coeff).  Per term: JB commit-key words are loaded
// once and reused for NC columns, NC data words reused for JB outputs (register tiling of the
// per-(limb, coeff) modular GEMM  out[j][col] = sum_t A[j][t] B[t][col]).
template <int JB, int NC, bool WIDE>
__global__ __launch_bounds__(256) void mac_kernel(MacArgs a, int j0) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long per_col = (long long)a.nl * a.d;
  const long long ngroups = (a.ncols + NC - 1) / NC;
  if (gid >= ngroups * per_col) return;
  const long long cg = gid / per_col;
  const int lk = (int)(gid % per_col);  // limb * d + coeff
  const int l = lk / a.d;
  const int J = min(JB, a.J - j0);
  const long long col0 = cg * NC;
  const int nc = (int)min((long long)NC, a.ncols - col0);
  Acc<WIDE> acc[NC][JB];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int j = 0; j < JB; ++j) acc[c][j].zero();
  for (int set = 0; set < 2; ++set) {
    const int T = set ? a.T2 : a.T1;
    if (!T) continue;
    const uint64_t* A = (set ? a.A2 : a.A1) + lk;
    const uint64_t* Bp = (set ? a.B2 : a.B1) + lk;
    const long long bcol = set ? a.b2_col : a.b1_col, bterm = set ? a.b2_term : a.b1_term;
    // J = 1 (Prover.Evaluate's dot products): unrolled so each thread keeps 4 terms' loads in
    // flight -- one term's 1 + NC loads per iteration left the opening stream latency-bound
    constexpr int kUnr = JB == 1 ? 4 : 1;
#pragma unroll kUnr
    for (int t = 0; t < T; ++t) {
      uint64_t av[JB], bv[NC];
#pragma unroll
      for (int j = 0; j < JB; ++j) av[j] = (j < J) ? A[((long long)(j0 + j) * T + t) * per_col] : 0;
#pragma unroll
      for (int c = 0; c < NC; ++c) bv[c] = (c < nc) ? Bp[(col0 + c) * bcol + t * bterm] : 0;
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int j = 0; j < JB; ++j) acc[c][j].mac(av[j], bv[c]);
    }
  }
  const RnsPrime& P = a.P[l];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (c >= nc) continue;
    const long long col = col0 + c;
#pragma unroll
    for (int j = 0; j < JB; ++j) {
      if (j >= J) continue;
      uint64_t r = acc[c][j].reduce(P);
      if (a.C) r = mod_add(a.C[col * a.c_col + (long long)(j0 + j) * a.c_j + lk], r, P.q);
      a.out[(col * a.J + j0 + j) * per_col + lk] = r;
    }
  }
}

constexpr int kMacNC = 4;

template <int JB, bool WIDE>
static rg_status launch_mac_jb(const MacArgs& m, int j0, hipStream_t st) {
  const long long groups = (m.ncols + kMacNC - 1) / kMacNC;
  const long long threads = groups * m.nl * m.d;
  hipLaunchKernelGGL((mac_kernel<JB, kMacNC, WIDE>), dim3(grid256(threads)), dim3(256), 0, st, m, j0);
  return check_launch("jindo mac");
}

template <bool WIDE>
static rg_status launch_mac_w(const MacArgs& m, int jb, int j0, hipStream_t st) {
  switch (jb) {
    case 1: return launch_mac_jb<1, WIDE>(m, j0, st);
    case 2: return launch_mac_jb<2, WIDE>(m, j0, st);
    case 3: return launch_mac_jb<3, WIDE>(m, j0, st);
    case 4: return launch_mac_jb<4, WIDE>(m, j0, st);
    case 5: return launch_mac_jb<5, WIDE>(m, j0, st);
    case 6: return launch_mac_jb<6, WIDE>(m, j0, st);
    case 7: return launch_mac_jb<7, WIDE>(m, j0, st);
    default: return launch_mac_jb<8, WIDE>(m, j0, st);
  }
}

// J outputs split into ceil(J/8) launches of equal width
rg_status launch_mac(const MacArgs& m, hipStream_t st) {
  uint64_t qmax = 0;
  for (int l = 0; l < m.nl; ++l) qmax = std::max(qmax, m.P[l].q);
  const double bits = 2.0 * log2((double)(qmax - 1)) + log2((double)(m.T1 + m.T2) + 1.0);
  const bool wide = bits >= 127.5;
  const int passes = (m.J + 7) / 8;
  const int jb = (m.J + passes - 1) / passes;
  for (int j0 = 0; j0 < m.J; j0 += jb) RG_TRY(wide ? launch_mac_w<true>(m, jb, j0, st) : launch_mac_w<false>(m, jb, j0, st));
  return RG_OK;
}

// ------------------------------------------------------------------------------------------
// 4. round: IMForm -> INTT -> centred CRT -> floor shift -> mod q' -> MForm -> NTT
// ------------------------------------------------------------------------------------------
// The rounding tail of one coefficient (floor shift by the cut with the toward-minus-infinity fix,
// the zero test, the Euclidean residue per destination prime, MForm) is written out in both round
// kernels: change the two copies together.  (One __forceinline__ helper compiles to different code
// in both: profiles/r08b_jindo_split_commit_ab.txt.)
__global__ __launch_bounds__(256) void round_kernel(RoundArgs a) {
  // LDS sized per launch (max(ns, nd) limbs x d words), not for kMaxQ x kMaxD: occupancy is then
  // register-limited (7 waves/SIMD) instead of LDS-limited (5)
  extern __shared__ uint64_t poly_lds[];
  const int d = a.d, tid = threadIdx.x, ns = a.src.n, nd = a.dst.n;
  auto poly = [&](int l) { return poly_lds + (long long)l * d; };
  const long long pid = blockIdx.x;
  const uint64_t* in = a.in + pid * ns * d;
  for (int k = tid; k < ns * d; k += blockDim.x) {
    const int l = k / d;
    const RnsPrime& P = a.src.p[l];
    poly(l)[k % d] = sh_mul(in[k], P.rinv, P.rinv_sh, P.q);  // IMForm
  }
  __syncthreads();
  const int half = blockDim.x >> 1;
  for (int l0 = 0; l0 < ns; l0 += 2) {
    const int l = l0 + (tid >= half ? 1 : 0);
    const bool active = l < ns;
    const int lc = active ? l : l0;
    intt_lds(poly(lc), d, a.src.bwd + (long long)lc * d, a.src.p[lc], tid % half, half, active);
  }
  // CRT per coefficient
  for (int k = tid; k < d; k += blockDim.x) {
    uint64_t r[kMaxQ];
    for (int l = 0; l < ns; ++l) r[l] = poly(l)[k];
    uint64_t mag[4];
    bool neg = crt_centred(a.crt, ns, r, mag);
    // floor(value / 2^cut) (big.Int.Rsh on a signed value rounds toward -inf)
    bool lost = false;
    int cut = a.cut;
    while (cut > 0) {
      const int sft = cut > 63 ? 63 : cut;
      lost |= (mag[0] & ((1ull << sft) - 1)) != 0;
      for (int i = 0; i < 4; ++i) mag[i] = (mag[i] >> sft) | (i + 1 < 4 ? mag[i + 1] << (64 - sft) : 0);
      cut -= sft;
    }
    if (neg && lost) {
      for (int i = 0; i < 4; ++i)
        if (++mag[i]) break;
    }
    const bool zero = !(mag[0] | mag[1] | mag[2] | mag[3]);
    // setBigCoeffTo: Euclidean mod each destination prime (rns.go:108-114), then MForm
    for (int l = 0; l < nd; ++l) {
      const RnsPrime& P = a.dst.p[l];
      const uint64_t q = P.q;
      uint64_t m = 0;
      for (int i = 0; i < 4; ++i) m = mod_add(m, sh_mul(mag[i], a.dm.pw[l][i], a.dm.pw_sh[l][i], q), q);
      if (neg && !zero) m = mod_neg(m, q);
      r[l] = sh_mul(m, P.r64, P.r64_sh, q);
    }
    for (int l = 0; l < nd; ++l) poly(l)[k] = r[l];  // each thread owns coefficient k
  }
  __syncthreads();
  for (int l0 = 0; l0 < nd; l0 += 2) {
    const int l = l0 + (tid >= half ? 1 : 0);
    const bool active = l < nd;
    const int lc = active ? l : l0;
    ntt_lds(poly(lc), d, a.dst.fwd + (long long)lc * d, a.dst.p[lc].q, tid % half, half, active);
  }
  uint64_t* out = a.out + pid * a.out_stride;
  for (int k = tid; k < a.out_rows * d; k += blockDim.x) out[k] = (k / d < nd) ? poly(k / d)[k % d] : 0;
}

// Wave-per-polynomial round for d = 256 (every Jindo shape): one wave owns one polynomial, a
// limb pair at a time in its two half-waves (lanes 0-31 limb l0, 32-63 limb l0 + 1), 8 points per
// lane in registers.  The inverse and forward 256-point transforms run as rounds of 3 + 3 + 2
// radix-2 stages (ntt64.hpp's ROW index algebra, lazy [0, 2q) Shoup butterflies) with wave-private
// LDS exchanges and no workgroup barrier; the CRT step reads each coefficient's residues from the
// wave's limb rows.  round_kernel (a workgroup per polynomial, a barrier per stage) does the same
// arithmetic; results are the same canonical residues.
constexpr int kRoundWaves = 4;
template <int RK, int LO, int PAT, bool INV>
__device__ __forceinline__ void wround(uint64_t (&e)[8], const ulonglong2* roots, const Q64& Q, uint32_t t) {
  wave_pairs<RK, LO, PAT, INV, 0>(t, [&](int rho0, int rho1, uint32_t wi) {
    const ulonglong2 w = roots[wi];
    if constexpr (INV)
      inv_bfly_lazy<false>(e[rho0], e[rho1], w.x, w.y, Q);
    else
      fwd_bfly_lazy<false>(e[rho0], e[rho1], w.x, w.y, Q);
  });
}

__global__ __launch_bounds__(64 * kRoundWaves) void round256_kernel(RoundArgs a) {
  // dynamic LDS: the limbs' tables (ns inverse, then nd forward; [l][256]), then per wave `rows`
  // rows of 288 words: limb l's exchanges and its natural-order coefficients in row l
  extern __shared__ ulonglong2 rtab[];
  const int ns = a.src.n, nd = a.dst.n, rows = (std::max(ns, nd) + 1) & ~1;
  for (int i = threadIdx.x; i < (ns + nd) * 256; i += blockDim.x)
    rtab[i] = i < ns * 256 ? a.src.bwd[i] : a.dst.fwd[i - ns * 256];
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u, t = lane & 31u, hs = lane >> 5;
  const int wv = threadIdx.x >> 6;
  uint64_t* wl = reinterpret_cast<uint64_t*>(rtab + (ns + nd) * 256) + (size_t)wv * rows * 288;
  const long long pid = (long long)blockIdx.x * kRoundWaves + wv;
  if (pid >= a.npoly) return;
  const uint64_t* in = a.in + pid * ns * 256;
  // 1. IMForm, inverse NTT (Gentleman-Sande, bit-reversed -> natural), times 256^-1, per limb pair
  for (int l0 = 0; l0 < ns; l0 += 2) {
    const int limb = l0 + (int)hs, lc = limb < ns ? limb : l0;
    const RnsPrime& P = a.src.p[lc];
    const Q64 Q = make_q64(P.q);
    const ulonglong2* roots = rtab + lc * 256;
    const uint32_t row = 288u * (uint32_t)(l0 + (int)hs);
    const WaveRows wr = wave_rows(row, t);
    uint64_t e[8];
#pragma unroll
    for (int y = 0; y < 8; ++y) e[y] = sh_mul(in[lc * 256 + t + 32 * y], P.rinv, P.rinv_sh, P.q);
#pragma unroll
    for (int y = 0; y < 8; ++y) wl[wr.H + 33 * y] = e[y];  // H -> L (pad x >> 5)
    wave_lds_fence();
#pragma unroll
    for (int r = 0; r < 8; ++r) e[r] = wl[wr.L8 + r];
    wround<2, 0, 2, true>(e, roots, Q, t);
    wave_lds_fence();
#pragma unroll
    for (int r = 0; r < 8; ++r) wl[wr.L9 + r] = e[r];  // L -> M
    wave_lds_fence();
#pragma unroll
    for (int y = 0; y < 8; ++y) e[y] = wl[wr.M + 4 * y + (y >> 1)];
    wround<3, 2, 1, true>(e, roots, Q, t);
    wave_lds_fence();
#pragma unroll
    for (int y = 0; y < 8; ++y) wl[wr.M + 4 * y] = e[y];  // M -> H
    wave_lds_fence();
#pragma unroll
    for (int y = 0; y < 8; ++y) e[y] = wl[wr.H + 36 * y];
    wround<3, 5, 0, true>(e, roots, Q, t);
    wave_lds_fence();
#pragma unroll
    for (int y = 0; y < 8; ++y) wl[row + t + 32 * y] = sh_mul(e[y], P.ninv, P.ninv_sh, P.q);  // natural order
    wave_lds_fence();
  }
  // 2. CRT per coefficient (4 per lane), floor shift, the destination residues in MForm
  for (int i = 0; i < 4; ++i) {
    const int k = (int)lane + 64 * i;
    uint64_t r[kMaxQ];
    for (int l = 0; l < ns; ++l) r[l] = wl[288 * l + k];
    uint64_t mag[4];
    const bool neg = crt_centred(a.crt, ns, r, mag);
    bool lost = false;
    int cut = a.cut;
    while (cut > 0) {
      const int sft = cut > 63 ? 63 : cut;
      lost |= (mag[0] & ((1ull << sft) - 1)) != 0;
      for (int w = 0; w < 4; ++w) mag[w] = (mag[w] >> sft) | (w + 1 < 4 ? mag[w + 1] << (64 - sft) : 0);
      cut -= sft;
    }
    if (neg && lost) {
      for (int w = 0; w < 4; ++w)
        if (++mag[w]) break;
    }
    const bool zero = !(mag[0] | mag[1] | mag[2] | mag[3]);
    for (int l = 0; l < nd; ++l) {
      const RnsPrime& P = a.dst.p[l];
      const uint64_t q = P.q;
      uint64_t m = 0;
      for (int w = 0; w < 4; ++w) m = mod_add(m, sh_mul(mag[w], a.dm.pw[l][w], a.dm.pw_sh[l][w], q), q);
      if (neg && !zero) m = mod_neg(m, q);
      r[l] = sh_mul(m, P.r64, P.r64_sh, q);
    }
    for (int l = 0; l < nd; ++l) wl[288 * l + k] = r[l];
  }
  wave_lds_fence();
  // 3. forward NTT (Cooley-Tukey, natural -> bit-reversed) per destination limb pair, stored in H
  uint64_t* out = a.out + pid * a.out_stride;
  for (int l0 = 0; l0 < nd; l0 += 2) {
    const int limb = l0 + (int)hs, lc = limb < nd ? limb : l0;
    const Q64 Q = make_q64(a.dst.p[lc].q);
    const ulonglong2* roots = rtab + (ns + lc) * 256;
    const uint32_t row = 288u * (uint32_t)(l0 + (int)hs);
    const WaveRows wr = wave_rows(row, t);
    uint64_t e[8];
#pragma unroll
    for (int y = 0; y < 8; ++y) e[y] = wl[288 * lc + t + 32 * y];
    wave_lds_fence();
    wround<3, 5, 0, false>(e, roots, Q, t);
#pragma unroll
    for (int y = 0; y < 8; ++y) wl[wr.H + 36 * y] = e[y];  // H -> M
    wave_lds_fence();
#pragma unroll
    for (int y = 0; y < 8; ++y) e[y] = wl[wr.M + 4 * y];
    wround<3, 2, 1, false>(e, roots, Q, t);
    wave_lds_fence();
#pragma unroll
    for (int y = 0; y < 8; ++y) wl[wr.M + 4 * y + (y >> 1)] = e[y];  // M -> L
    wave_lds_fence();
#pragma unroll
    for (int r = 0; r < 8; ++r) e[r] = wl[wr.L9 + r];
    wround<2, 0, 2, false>(e, roots, Q, t);
    wave_lds_fence();
#pragma unroll
    for (int r = 0; r < 8; ++r) wl[wr.L8 + r] = canon(e[r], Q);  // L -> H, canonical
    wave_lds_fence();
    if (limb < nd) {
#pragma unroll
      for (int y = 0; y < 8; ++y) out[limb * 256 + t + 32 * y] = wl[wr.H + 33 * y];
    }
    wave_lds_fence();
  }
  for (int k = nd * 256 + (int)lane; k < a.out_rows * 256; k += 64) out[k] = 0;
}

// ------------------------------------------------------------------------------------------
// host: the launchers and the stages
// ------------------------------------------------------------------------------------------
template <int L>
static rg_status launch_digits(const rg_jindo* J, size_t batch, const uint64_t* v, long long nv, const uint64_t* last,
                               const uint64_t* mask, uint32_t* digits, hipStream_t st) {
  DigitArgs<L> a;
  a.s = shape_of(J->p, nv);
  a.F = field_params<L>(&J->field);
  a.base_inv = J->base_inv;
  const uint64_t b2 = (uint64_t)J->p.base * J->p.base;
  a.b2 = (b2 >> 32) ? 0 : b2;
  a.b2_inv = a.b2 ? (uint64_t)(((unsigned __int128)1 << 64) / b2) : 0;
  a.dc = dc_constants((uint64_t)J->p.base, J->p.exp, L, field_bits(J->field));
  a.v = v;
  a.last_row = last;
  a.mask = mask;
  a.digits = digits;
  a.total = (long long)batch * (J->p.cols + 1) * J->p.rows * J->p.slots;
  a.d_slots = make_idxdiv((uint32_t)J->p.slots);
  a.d_rows = make_idxdiv((uint32_t)J->p.rows);
  a.d_cols1 = make_idxdiv((uint32_t)(J->p.cols + 1));
  if (J->p.slots * J->p.exp < J->p.d)  // the coefficients no thread writes read as zero digits (baseEncodeTo)
    RG_HIP(hipMemsetAsync(digits, 0, sizes_of(J->p, batch).digits, st));
  hipLaunchKernelGGL(digits_kernel<L>, dim3(grid256(a.total)), dim3(256), 0, st, a);
  return check_launch("jindo digits");
}

// MacArgs (legacy kernel layout) -> MfmaMacArgs over the digit key `key` (mac_mfma_key_dev)
static MfmaMacArgs mfma_args(const MacArgs& m, const DevBuf& key) {
  MfmaMacArgs a;
  memset(&a, 0, sizeof(a));
  a.per_col = (long long)m.nl * m.d;
  a.ncols = m.ncols;
  a.J = m.J;
  a.T1 = m.T1;
  a.T2 = m.T2;
  a.Tc = (m.T1 + m.T2 + 7) / 8;
  mac_mfma_key_ptrs(key, a.per_col, m.T1 + m.T2, &a.Ak, &a.corr);
  a.B1 = m.B1;
  a.b1_col = m.b1_col;
  a.b1_term = m.b1_term;
  a.B2 = m.B2;
  a.b2_col = m.b2_col;
  a.b2_term = m.b2_term;
  a.C = m.C;
  a.c_col = m.c_col;
  a.c_j = m.c_j;
  a.out = m.out;
  a.d = m.d;
  for (int l = 0; l < m.nl && l < kMfmaMaxQ; ++l) a.P[l] = mfma_prime(m.P[l]);
  return a;
}

RoundArgs round_args(const rg_jindo* J, bool src_o, bool dst_o, int cut, const uint64_t* in, uint64_t* out,
                     long long out_stride, int out_rows) {
  auto ring = [&](bool o) {
    return o ? ring_dev(J->ro, J->p.nqo, J->rootso_f, J->rootso_b) : ring_dev(J->rq, J->p.nq, J->rootsq_f, J->rootsq_b);
  };
  RoundArgs ra;
  memset(&ra, 0, sizeof(ra));
  ra.d = J->p.d;
  ra.cut = cut;
  ra.src = ring(src_o);
  ra.dst = ring(dst_o);
  ra.crt = src_o ? J->crt_o : J->crt_q;
  ra.dm = dst_o ? J->dst_o : J->dst_q;
  ra.in = in;
  ra.out = out;
  ra.out_stride = out_stride;
  ra.out_rows = out_rows;
  return ra;
}

// CRT rounding of `npoly` polynomials: round256_kernel (a wave per polynomial) for d = 256 and
// primes below 2^62 (its lazy butterflies need 2q < 2^63), round_kernel otherwise.  round256
// against round_kernel at configs[4]: 429 vs 513 us per launch (profiles/r05s_round_wave_ab.txt)
rg_status launch_round(RoundArgs ra, long long npoly, hipStream_t st) {
  ra.npoly = npoly;
  bool small = ra.d == 256;
  for (int l = 0; l < ra.src.n; ++l) small = small && ra.src.p[l].q < (1ull << 62);
  for (int l = 0; l < ra.dst.n; ++l) small = small && ra.dst.p[l].q < (1ull << 62);
  if (small) {
    const int rows = (std::max(ra.src.n, ra.dst.n) + 1) & ~1;
    const size_t lds = (size_t)(ra.src.n + ra.dst.n) * 256 * sizeof(ulonglong2) + (size_t)kRoundWaves * rows * 288 * 8;
    hipLaunchKernelGGL(round256_kernel, dim3((unsigned)((npoly + kRoundWaves - 1) / kRoundWaves)), dim3(64 * kRoundWaves),
                       lds, st, ra);
  } else {
    hipLaunchKernelGGL(round_kernel, dim3((unsigned)npoly), dim3(256),
                       (size_t)std::max(ra.src.n, ra.dst.n) * ra.d * 8, st, ra);
  }
  return check_launch("jindo round");
}

// The deterministic Ajtai core (prover.go:144-202) over a batch of NTT-domain openings:
// inner MAC, rounding into Opening.InCommit, outer MAC and rounding into Commitment.Value.
rg_status commit_core(rg_jindo* J, size_t batch, const uint64_t* d_enc, const uint64_t* d_mlwe, uint64_t* d_incom,
                      uint64_t* d_com, rg_jindo_scratch* sc, hipStream_t st) {
  const rg_jindo_params& p = J->p;
  const int nm = p.in_msis + p.mlwe;
  const long long pq = (long long)p.nq * p.d, po = (long long)p.nqo * p.d;
  // 3. inner MAC: sum_k In[j][k] Enc[k] + sum_k CK.MLWE[j][k] MLWE[k] + MLWE[mlwe + j]
  MacArgs ma = dot_args(J->rq, p.nq, p.d, (long long)batch * (p.cols + 1), p.rows, J->ck_in.as<uint64_t>(), d_enc,
                        p.rows * pq, pq, sc->com.as<uint64_t>());
  ma.J = p.in_msis;
  ma.T2 = p.mlwe;
  ma.A2 = J->ck_mlwe.as<uint64_t>();
  ma.B2 = d_mlwe;
  ma.b2_col = nm * pq;
  ma.b2_term = pq;
  ma.C = d_mlwe + p.mlwe * pq;  // MLWE[i][mlwe + j]
  ma.c_col = nm * pq;
  ma.c_j = pq;
  if (J->mfma_q) {
    RG_TRY(launch_mac_mfma(mfma_args(ma, J->ckm_in), J->mfma_q, st));
  } else {
    RG_TRY(launch_mac(ma, st));
  }
  // 4. inner round -> Opening.InCommit (column i, j -> index i*inMSIS + j)
  {
    const long long npoly = (long long)batch * (p.cols + 1) * p.in_msis;  // == batch * dcmp, same order
    RG_TRY(launch_round(round_args(J, false, true, p.log_in_cut, sc->com.as<uint64_t>(), d_incom, po, p.nqo), npoly,
                        st));
  }
  // 5. outer MAC + round -> Commitment.Value (ringQ-shaped rows, rows >= nqo zero)
  MacArgs mo = dot_args(J->ro, p.nqo, p.d, (long long)batch, p.dcmp, J->ck_out.as<uint64_t>(), d_incom, p.dcmp * po, po,
                        sc->ocom.as<uint64_t>());
  mo.J = p.out_msis;
  if (J->mfma_o) {
    RG_TRY(launch_mac_mfma(mfma_args(mo, J->ckm_out), J->mfma_o, st));
  } else {
    RG_TRY(launch_mac(mo, st));
  }
  RG_TRY(launch_round(round_args(J, true, true, p.log_out_cut, sc->ocom.as<uint64_t>(), d_com, pq, p.nq),
                      (long long)batch * p.out_msis, st));
  RG_TRY(check_launch("jindo round(out)"));
  return RG_OK;
}

// 1. digits of every encode's source elements into the stream's scratch.  (rg_jindo_create's
// validate admits only the five limb counts, so dispatch_limbs' refusal is never reached here.)
rg_status digits_stage(rg_jindo* J, size_t batch, const uint64_t* d_v, size_t nv, const uint64_t* d_last,
                       const uint64_t* d_mask, uint32_t* digits, hipStream_t st) {
  return dispatch_limbs(J->p.field_limbs, [&](auto Lc) {
    return launch_digits<Lc()>(J, batch, d_v, (long long)nv, d_last, d_mask, digits, st);
  });
}

// 2. encode tails + MLWE finalize with their NTTs (prep256_kernel): jobs [0, n_enc) are the encode
// polynomials, [n_enc, n_enc + n_ml) the MLWE ones; `part` (PrepPart) selects both or one of the two sets
rg_status prep_launch(rg_jindo* J, size_t batch, size_t nv, const uint32_t* digits, const int64_t* d_en,
                      const int64_t* d_mn, uint64_t* d_enc, uint64_t* d_mlwe, int part, hipStream_t st) {
  const rg_jindo_params& p = J->p;
  const int d = p.d, nq = p.nq, nm = p.in_msis + p.mlwe;
  PrepArgs pa;
  pa.s = shape_of(p, (long long)nv);
  pa.R = ring_dev(J->rq, nq, J->rootsq_f, J->rootsq_b);
  pa.digits = digits;
  pa.enc_noise = reinterpret_cast<const long long*>(d_en);
  pa.mlwe_noise = reinterpret_cast<const long long*>(d_mn);
  pa.enc = d_enc;
  pa.mlwe = d_mlwe;
  pa.n_enc = (part & kPrepEnc) ? (long long)batch * (p.cols + 1) * p.rows : 0;
  const long long n_ml = (part & kPrepMlwe) ? (long long)batch * (p.cols + 1) * nm : 0;
  pa.n_ml = n_ml;
  pa.clim = (long long)(((uint64_t)1 << 61) / p.base);
  if (pa.n_enc + n_ml == 0) return RG_OK;
  bool q61 = true;  // prep256's lazy [0, 8q) needs q < 2^61 (every configs ring prime is <= 59 bits)
  for (int l = 0; l < nq; ++l) q61 = q61 && J->rq[l].q < (1ull << 61);
  if (d == 256 && q61) {  // else prep_kernel: a workgroup per polynomial, any d and q
    const long long jobs = pa.n_enc + n_ml;
    const dim3 g((unsigned)((jobs + kPrepWaves - 1) / kPrepWaves)), b(64 * kPrepWaves);
    const size_t twl = (size_t)nq * 256 * sizeof(ulonglong2);
    // large launches (configs[4]'s encode prep, 2.4 M jobs): 12-wave workgroups, so each table
    // staging serves 12 polynomials instead of 4 (configs[4] +1.2%; at configs[2]'s 0.3 M jobs the
    // 4-wave form is 1% faster: profiles/r05ao_prep_workgroup_ab.txt)
    constexpr int kBigWaves = 12;
    // (minimum waves per SIMD 8 or 1 instead of 6, round 2-5's RINGO_JINDO_PREP_W: slower at both
    // configs shapes, removed in round 6)
    bool lazy = true;  // every ring prime below 2^64 / 36: prep_round skips its x reductions
    for (int l = 0; l < nq; ++l) lazy = lazy && J->rq[l].q < ~0ull / 36;
    if (nq <= 2 && jobs >= (1LL << 20)) {
      const dim3 gb((unsigned)((jobs + kBigWaves - 1) / kBigWaves)), bb(64 * kBigWaves);
      if (lazy)
        hipLaunchKernelGGL((prep256_kernel<2, true, kBigWaves, true>), gb, bb, twl, st, pa);
      else
        hipLaunchKernelGGL((prep256_kernel<2, true, kBigWaves>), gb, bb, twl, st, pa);
    } else if (nq <= 2 && lazy)
      hipLaunchKernelGGL((prep256_kernel<6, true, kPrepWaves, true>), g, b, twl, st, pa);
    else if (nq <= 2)
      hipLaunchKernelGGL((prep256_kernel<6, true>), g, b, twl, st, pa);
    else
      hipLaunchKernelGGL((prep256_kernel<6, false>), g, b, twl, st, pa);
  } else {
    hipLaunchKernelGGL(prep_kernel, dim3((unsigned)(pa.n_enc + n_ml)), dim3(256), 0, st, pa);
  }
  return check_launch("jindo prep");
}

// 1.-5.: the digits, then from them and the randomness the encode tails + MLWE finalize with their
// NTTs, then the core
static rg_status commit_dev(rg_jindo* J, size_t batch, const uint64_t* d_v, size_t nv, const uint64_t* d_last,
                            const uint64_t* d_mask, const int64_t* d_en, const int64_t* d_mn, uint64_t* d_incom,
                            uint64_t* d_enc, uint64_t* d_mlwe, uint64_t* d_com, hipStream_t st) {
  const rg_jindo_params& p = J->p;
  if (nv < 1 || nv > (size_t)p.rank) return RG_ERR_RANK;
  if (batch == 0) return RG_OK;
  RG_TRY(on_device(J));
  rg_jindo_scratch* sc = nullptr;
  RG_TRY(stream_scratch(J, batch, st, &sc));
  uint32_t* digits = sc->digits.as<uint32_t>();
  RG_TRY(digits_stage(J, batch, d_v, nv, d_last, d_mask, digits, st));
  RG_TRY(prep_launch(J, batch, nv, digits, d_en, d_mn, d_enc, d_mlwe, kPrepAll, st));
  return commit_core(J, batch, d_enc, d_mlwe, d_incom, d_com, sc, st);
}

// MacArgs of a J = 1 dot product over T terms with the caller's strides (Prover.Evaluate's and the
// verifier's loops); the commit's two products start from it and set J and their second operand set
MacArgs dot_args(const RnsPrime* P, int nl, int d, long long nout, int T, const uint64_t* A, const uint64_t* B,
                 long long b_out, long long b_term, uint64_t* out) {
  MacArgs m;
  memset(&m, 0, sizeof(m));
  m.d = d;
  m.nl = nl;
  m.J = 1;
  m.ncols = nout;
  m.T1 = T;
  m.A1 = A;
  m.B1 = B;
  m.b1_col = b_out;
  m.b1_term = b_term;
  m.out = out;
  for (int l = 0; l < nl; ++l) m.P[l] = P[l];
  return m;
}

}  // namespace rg

using namespace rg;

extern "C" {

rg_status rg_jindo_commit_dev(const rg_jindo* J, size_t batch, const uint64_t* d_v, size_t nv, const uint64_t* d_last,
                              const uint64_t* d_mask, const int64_t* d_en, const int64_t* d_mn, uint64_t* d_incom,
                              uint64_t* d_enc, uint64_t* d_mlwe, uint64_t* d_com, void* stream) {
  if (!J) return RG_ERR_INVALID;
  if (batch && (!d_v || !d_last || !d_mask || !d_en || !d_mn || !d_incom || !d_enc || !d_mlwe || !d_com))
    return RG_ERR_INVALID;
  return commit_dev(const_cast<rg_jindo*>(J), batch, d_v, nv, d_last, d_mask, d_en, d_mn, d_incom, d_enc, d_mlwe, d_com,
                    as_stream(stream));
}

rg_status rg_jindo_commit_core_dev(const rg_jindo* J, size_t batch, const uint64_t* d_enc, const uint64_t* d_mlwe,
                                   uint64_t* d_incom, uint64_t* d_com, void* stream) {
  if (!J) return RG_ERR_INVALID;
  if (batch == 0) return RG_OK;
  if (!d_enc || !d_mlwe || !d_incom || !d_com) return RG_ERR_INVALID;
  RG_TRY(on_device(J));
  rg_jindo* Jm = const_cast<rg_jindo*>(J);
  hipStream_t st = as_stream(stream);
  rg_jindo_scratch* sc = nullptr;
  RG_TRY(stream_scratch(Jm, batch, st, &sc));
  return commit_core(Jm, batch, d_enc, d_mlwe, d_incom, d_com, sc, st);
}

rg_status rg_jindo_commit_core(const rg_jindo* J, const uint64_t* enc, const uint64_t* mlwe, uint64_t* o_incom,
                               uint64_t* o_com) {
  if (!J || !enc || !mlwe || !o_incom || !o_com) return RG_ERR_INVALID;
  const JSizes z = sizes_of(J->p, 1);
  DevBuf enc_, ml_, inc_, com_;
  RG_TRY(enc_.upload(enc, z.enc));
  RG_TRY(ml_.upload(mlwe, z.mlwe));
  RG_TRY(inc_.alloc(z.incom));
  RG_TRY(com_.alloc(z.com));
  RG_TRY(rg_jindo_commit_core_dev(J, 1, enc_.as<uint64_t>(), ml_.as<uint64_t>(), inc_.as<uint64_t>(),
                                  com_.as<uint64_t>(), nullptr));
  RG_HIP(hipMemcpy(o_incom, inc_.p, z.incom, hipMemcpyDeviceToHost));
  RG_HIP(hipMemcpy(o_com, com_.p, z.com, hipMemcpyDeviceToHost));
  return RG_OK;
}

rg_status rg_jindo_commit(const rg_jindo* J, const uint64_t* v, size_t nv, const uint64_t* last_row,
                          const uint64_t* mask, const int64_t* enc_noise, const int64_t* mlwe_noise, uint64_t* o_incom,
                          uint64_t* o_enc, uint64_t* o_mlwe, uint64_t* o_com) {
  if (!J || !v || !last_row || !mask || !enc_noise || !mlwe_noise || !o_incom || !o_enc || !o_mlwe || !o_com)
    return RG_ERR_INVALID;
  const rg_jindo_params& p = J->p;
  if (nv < 1 || nv > (size_t)p.rank) return RG_ERR_RANK;
  const JSizes z = sizes_of(p, 1);
  DevBuf v_, l_, m_, en_, mn_, inc_, enc_, ml_, com_;
  RG_TRY(v_.upload(v, nv * p.field_limbs * 8));
  RG_TRY(l_.upload(last_row, z.last));
  RG_TRY(m_.upload(mask, z.mask));
  RG_TRY(en_.upload(enc_noise, z.en));
  RG_TRY(mn_.upload(mlwe_noise, z.mn));
  RG_TRY(inc_.alloc(z.incom));
  RG_TRY(enc_.alloc(z.enc));
  RG_TRY(ml_.alloc(z.mlwe));
  RG_TRY(com_.alloc(z.com));
  RG_TRY(rg_jindo_commit_dev(J, 1, v_.as<uint64_t>(), nv, l_.as<uint64_t>(), m_.as<uint64_t>(), en_.as<int64_t>(),
                             mn_.as<int64_t>(), inc_.as<uint64_t>(), enc_.as<uint64_t>(), ml_.as<uint64_t>(),
                             com_.as<uint64_t>(), nullptr));
  RG_HIP(hipMemcpy(o_incom, inc_.p, z.incom, hipMemcpyDeviceToHost));
  RG_HIP(hipMemcpy(o_enc, enc_.p, z.enc, hipMemcpyDeviceToHost));
  RG_HIP(hipMemcpy(o_mlwe, ml_.p, z.mlwe, hipMemcpyDeviceToHost));
  RG_HIP(hipMemcpy(o_com, com_.p, z.com, hipMemcpyDeviceToHost));
  return RG_OK;
}

}  // extern "C"
