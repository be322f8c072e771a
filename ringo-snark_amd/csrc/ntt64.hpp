// ntt64.hpp -- single-word (q < 2^63, L = 1) NTT arithmetic for gfx950: lazy butterflies.
//
// The bound is q < 2^63 (2q fits a word), not 2^64/3: the sum of two lazy values, < 4q < 2^65, is
// compared against 2q through its carry bit (lazy_add's c, fwd_bfly_x / inv_bfly_x's c2), so 3q
// may pass 2^64.  ntt_route.hpp's Lazy64 route gates on exactly this;
// tests/test_gpu_ntt_synthetic.py runs q = 0x7ffffff900000001 (3q > 2^64) through every pass.
// Values between butterfly stages live in [0, 2q) ("Harvey" lazy form); only the last stage of
// a transform maps them to the canonical residues the reference produces (gnark fully reduces,
// jindo/internal/zp/element.go:397-466), so every output limb is bit-identical to ntt.go.
// The twiddle product is Shoup's precomputed-quotient multiply, exact for any 64-bit input:
//   wp = floor(w 2^64 / q),  qh = floor(y wp / 2^64),  y w - qh q  in [0, 2q).
// q mod 2^32 == 1 (every jindo-modulus prime: p - 1 = b^(2^e) with b even) turns lo64(qh q)
// into qh + ((qh_lo q_hi) << 32): one 32-bit multiply instead of three.
// Cost model (tools/ubench, MI355X): 32-bit multiplies, 64-bit shifts/adds and carry ops issue
// at ~4.4 cycles per wave64 instruction, plain v_add/v_sub/v_and/v_mov at ~2.4; a butterfly is
// 8 multiplies + ~13 adds/selects.
// Moduli with q / 2^64 <= 0.2808 (ntt64_mont_ok: the config-2 prime 47104^4 + 1) take the
// Montgomery product below instead (the MONT kernels): 6 multiplies + 3 borrow ops on single-word
// twiddles in the reference's own Montgomery form, 19 (forward) / 20 (inverse) half-rate ops per
// butterfly against 23.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "field.hpp"
#include "ntt_route.hpp"
#include "ntt_tile.hpp"

namespace rg {

struct Q64 {
  uint64_t q, q2;  // q, 2q (2q < 2^64 needs q < 2^63; the lazy add below keeps the sum's 65th bit)
  uint32_t qhi;    // q >> 32
  uint32_t qlo1;   // q mod 2^32 == 1
};

RG_HD Q64 make_q64(uint64_t q) {
  Q64 Q;
  Q.q = q;
  Q.q2 = 2 * q;
  Q.qhi = (uint32_t)(q >> 32);
  Q.qlo1 = (uint32_t)q == 1u;
  return Q;
}

// ---- Montgomery twiddle product with a subtractive REDC (the lazy 2^16 passes, MONT) ----
// q = q1 2^32 + 1, y in [0, 2q), w < q a twiddle in Montgomery form (w' 2^64 mod q, the form the
// reference's tables already have).  T = y w + 2^64 + (q - 1) 2^64 = y w + q 2^64 (the two
// constants ride in the high words of the addends of p1 and p3: they add q to the result and keep
// it positive), T0, T1 its low words.  q == 1 (mod 2^32) makes
// -q^-1 == -1 (mod 2^32), so REDC's two quotient words are m0 = T0 and m1 = T1 - lo(T0 q1), and
//   t = (T - T0 q - m1 q 2^32) / 2^64      (exact: both low words cancel)
//     = p3 - W - b1,   Z = T0 q1,  W = m1 q1 + hi(Z),  b1 = borrow of T1 - lo(Z),
// because T0 q = T0 + Z 2^32 and m1 q 2^32 = m1 2^32 + m1 q1 2^64: word 0 is T0 - T0 = 0, word 1
// is T1 - lo(Z) - m1 = 0 with borrow b1 into word 2, and hi(Z) joins m1 q1 in W.
// Result: t == y w 2^-64 (mod q) and, as T0 q + m1 q 2^32 < q 2^64,
//   0 < t < q + ceil(2 q^2 / 2^64)                      (1.534 q for q = 47104^4 + 1).
// No 64-bit intermediate overflows, and the forward butterfly's x + t (x < 2q) fits 64 bits,
// when 3q + ceil(2 q^2 / 2^64) + 2^33 < 2^64: p2 = y0 w1 + y1 w0 + hi(p0) + 2^32 < 3q + 2^33,
// p3 < y1 w1 + 2^32 + q < 2q^2/2^64 + q + 2^33, x + t < 3q + ceil(2 q^2 / 2^64).  That is
// q1 <= 0x47e0f66a (q / 2^64 <= 0.28078): kMontMaxQ1 and ntt64_mont_ok of ntt_route.hpp, where the
// plan's route is decided; tests/test_mont64_host.py checks the constant against the inequality and
// the product against integers at both ends.

// portable form (host tables, tests); the device kernels use mont_x below
RG_HD uint64_t mont64(uint64_t y, uint64_t w, uint32_t q1) {
  const uint32_t y0 = (uint32_t)y, y1 = (uint32_t)(y >> 32), w0 = (uint32_t)w, w1 = (uint32_t)(w >> 32);
  const uint64_t p0 = (uint64_t)y0 * w0;
  const uint64_t p1 = (uint64_t)y0 * w1 + ((p0 >> 32) | (1ull << 32));
  const uint64_t p2 = (uint64_t)y1 * w0 + p1;
  const uint64_t p3 = (uint64_t)y1 * w1 + ((p2 >> 32) | ((uint64_t)q1 << 32));
  const uint64_t Z = (uint64_t)(uint32_t)p0 * q1;
  const uint32_t m1 = (uint32_t)p2 - (uint32_t)Z;
  const uint64_t b1 = (uint32_t)p2 < (uint32_t)Z;
  const uint64_t W = (uint64_t)m1 * q1 + (Z >> 32);
  return p3 - W - b1;
}

#if defined(__HIPCC__)

// y * w mod q in [0, 2q), exact Shoup for any y < 2^64
template <bool QLO1>
__device__ __forceinline__ uint64_t shoup2(uint64_t y, uint64_t w, uint64_t wp, const Q64& Q) {
  const uint32_t y0 = (uint32_t)y, y1 = (uint32_t)(y >> 32);
  const uint32_t p0 = (uint32_t)wp, p1 = (uint32_t)(wp >> 32);
  // qh = hi64(y * wp): mid = y0 p1 + y1 p0 + hi(y0 p0) < 2^65 carries at most once
  unsigned long long c1, c2;
  const uint64_t mid0 = __builtin_addcll((uint64_t)y0 * p1, (uint64_t)y1 * p0, 0ull, &c1);
  const uint64_t mid = __builtin_addcll(mid0, (uint64_t)__umulhi(y0, p0), 0ull, &c2);
  const uint64_t qh = (uint64_t)y1 * p1 + ((mid >> 32) | ((uint64_t)(c1 | c2) << 32));
  const uint32_t w0 = (uint32_t)w, w1 = (uint32_t)(w >> 32);
  if constexpr (QLO1) {
    const uint64_t l = (uint64_t)y0 * w0;
    const uint32_t hi = (uint32_t)(l >> 32) + y0 * w1 + y1 * w0 - (uint32_t)qh * Q.qhi;
    return (((uint64_t)hi << 32) | (uint32_t)l) - qh;
  } else {
    return y * w - qh * Q.q;
  }
}

// [0, 4q) sum as (value mod 2^64, carry) -> [0, 2q)
__device__ __forceinline__ uint64_t lazy_add(uint64_t x, uint64_t y, const Q64& Q) {
  unsigned long long c, b;
  const uint64_t s = __builtin_addcll(x, y, 0ull, &c);
  const uint64_t t = __builtin_subcll(s, Q.q2, 0ull, &b);
  return (c | (b ^ 1ull)) ? t : s;
}
// x - y + 2q (x, y in [0, 2q)) -> [0, 2q)
__device__ __forceinline__ uint64_t lazy_sub(uint64_t x, uint64_t y, const Q64& Q) {
  unsigned long long b;
  const uint64_t d = __builtin_subcll(x, y, 0ull, &b);
  return b ? d + Q.q2 : d;
}
// [0, 2q) -> [0, q)
__device__ __forceinline__ uint64_t canon(uint64_t x, const Q64& Q) {
  unsigned long long b;
  const uint64_t t = __builtin_subcll(x, Q.q, 0ull, &b);
  return b ? x : t;
}

// Cooley-Tukey (ntt.go:254-259): (x, y) <- (x + w y, x - w y), lazy in and out
template <bool QLO1 = true>
__device__ __forceinline__ void fwd_bfly_lazy(uint64_t& x, uint64_t& y, uint64_t w, uint64_t wp, const Q64& Q) {
  const uint64_t t = shoup2<QLO1>(y, w, wp, Q);
  const uint64_t a = x;
  x = lazy_add(a, t, Q);
  y = lazy_sub(a, t, Q);
}
// Gentleman-Sande (ntt.go:365-370): (x, y) <- (x + y, (x - y) w), lazy in and out
template <bool QLO1 = true>
__device__ __forceinline__ void inv_bfly_lazy(uint64_t& x, uint64_t& y, uint64_t w, uint64_t wp, const Q64& Q) {
  const uint64_t a = x, b = y;
  x = lazy_add(a, b, Q);
  y = shoup2<QLO1>(lazy_sub(a, b, Q), w, wp, Q);
}


// ---- explicit-carry forms (VOP3b carry outputs in SGPR lane masks; the compiler keeps the
// 32-bit halves of 64-bit values as sub-registers, so no pair is ever rebuilt) ----
typedef unsigned long long lmask;  // wave64 lane mask (SGPR pair)

__device__ __forceinline__ uint64_t mad_co(uint32_t a, uint32_t b, uint64_t c, lmask& co) {
  uint64_t d;
  asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(d), "=s"(co) : "v"(a), "v"(b), "v"(c));
  return d;
}
__device__ __forceinline__ uint32_t add_co(uint32_t a, uint32_t b, lmask& co) {
  uint32_t d;
  asm("v_add_co_u32 %0, %1, %2, %3" : "=v"(d), "=s"(co) : "v"(a), "v"(b));
  return d;
}
__device__ __forceinline__ uint32_t addc_co(uint32_t a, uint32_t b, lmask ci, lmask& co) {
  uint32_t d;
  asm("v_addc_co_u32 %0, %1, %2, %3, %4" : "=v"(d), "=s"(co) : "v"(a), "v"(b), "s"(ci));
  return d;
}
__device__ __forceinline__ uint32_t sub_co(uint32_t a, uint32_t b, lmask& bo) {
  uint32_t d;
  asm("v_sub_co_u32 %0, %1, %2, %3" : "=v"(d), "=s"(bo) : "v"(a), "v"(b));
  return d;
}
__device__ __forceinline__ uint32_t subb_co(uint32_t a, uint32_t b, lmask bi, lmask& bo) {
  uint32_t d;
  asm("v_subb_co_u32 %0, %1, %2, %3, %4" : "=v"(d), "=s"(bo) : "v"(a), "v"(b), "s"(bi));
  return d;
}
__device__ __forceinline__ uint32_t sel(lmask m, uint32_t if1, uint32_t if0) {
  uint32_t d;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(d) : "v"(if0), "v"(if1), "s"(m));
  return d;
}
__device__ __forceinline__ uint64_t pk(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; }
__device__ __forceinline__ uint32_t lo32(uint64_t v) { return (uint32_t)v; }
__device__ __forceinline__ uint32_t hi32(uint64_t v) { return (uint32_t)(v >> 32); }

// Shoup y * w mod q in [0, 2q), q mod 2^32 == 1; nqhi = -(q >> 32) mod 2^32
__device__ __forceinline__ uint64_t shoup_x(uint64_t y, uint64_t w, uint64_t wp, uint32_t nqhi) {
  const uint32_t y0 = lo32(y), y1 = hi32(y), p0 = lo32(wp), p1 = hi32(wp);
  lmask cb, k;
  const uint64_t a = (uint64_t)y0 * p1 + __umulhi(y0, p0);   // < 2^64
  const uint64_t b = mad_co(y1, p0, a, cb);                  // y1 p0 + a, carry into 2^96
  const uint64_t c = (uint64_t)y1 * p1 + hi32(b);            // < 2^64 (qh fits)
  const uint32_t qh0 = lo32(c);
  const uint32_t qh1 = addc_co(hi32(c), 0u, cb, k);
  const uint64_t l = (uint64_t)y0 * lo32(w);
  const uint32_t hi = hi32(l) + y0 * hi32(w) + y1 * lo32(w) + qh0 * nqhi;
  lmask br;
  const uint32_t r0 = sub_co(lo32(l), qh0, br);
  const uint32_t r1 = subb_co(hi, qh1, br, k);
  return pk(r0, r1);
}
// (x, y) <- (x + w y, x - w y), lazy [0, 2q) in and out; q2 = 2q
__device__ __forceinline__ void fwd_bfly_x(uint64_t& x, uint64_t& y, uint64_t w, uint64_t wp, uint64_t q2,
                                           uint32_t nqhi) {
  const uint64_t t = shoup_x(y, w, wp, nqhi);
  lmask c, c2, b, b2, e, e2;
  const uint32_t s0 = add_co(lo32(x), lo32(t), c);
  const uint32_t s1 = addc_co(hi32(x), hi32(t), c, c2);
  const uint32_t u0 = sub_co(s0, lo32(q2), b);
  const uint32_t u1 = subb_co(s1, hi32(q2), b, b2);
  const lmask m = c2 | ~b2;  // s >= 2q (65-bit)
  const uint32_t d0 = sub_co(lo32(x), lo32(t), e);
  const uint32_t d1 = subb_co(hi32(x), hi32(t), e, e2);
  const uint64_t d = pk(d0, d1);
  const uint64_t f = d + q2;
  x = pk(sel(m, u0, s0), sel(m, u1, s1));
  y = pk(sel(e2, lo32(f), d0), sel(e2, hi32(f), d1));
}


// (x, y) <- (x + y, (x - y) w), lazy [0, 2q) in and out
__device__ __forceinline__ void inv_bfly_x(uint64_t& x, uint64_t& y, uint64_t w, uint64_t wp, uint64_t q2,
                                           uint32_t nqhi) {
  lmask c, c2, b, b2, e, e2;
  const uint32_t s0 = add_co(lo32(x), lo32(y), c);
  const uint32_t s1 = addc_co(hi32(x), hi32(y), c, c2);
  const uint32_t u0 = sub_co(s0, lo32(q2), b);
  const uint32_t u1 = subb_co(s1, hi32(q2), b, b2);
  const lmask m = c2 | ~b2;
  const uint32_t d0 = sub_co(lo32(x), lo32(y), e);
  const uint32_t d1 = subb_co(hi32(x), hi32(y), e, e2);
  const uint64_t d = pk(d0, d1);
  const uint64_t f = d + q2;
  x = pk(sel(m, u0, s0), sel(m, u1, s1));
  y = shoup_x(pk(sel(e2, lo32(f), d0), sel(e2, hi32(f), d1)), w, wp, nqhi);
}
// ---- Montgomery product (derivation and bounds at the top of the file): 6 multiplies and
// 3 borrow ops, no quotient word.  The three addends {hi(p0), 1}, {hi(p2), q1}, {hi(Z), 0} are
// 64-bit register pairs whose high word never changes.  MontK keeps one such pair per addend
// alive for the whole tile and mont_x only rewrites its low word (one v_mov each): built afresh,
// each pair costs two moves, which spends what the shorter product saves.  mont_k hides the pairs
// behind an empty asm so the compiler cannot see (and rematerialise) the constant halves.  The asm
// is not volatile: a volatile one counts as a possible store, after which the H round's uniform
// twiddle loads are no longer provably unclobbered and turn from scalar loads into vector ones.
struct MontK {
  uint64_t c1, cq, c0;  // high words 1, q1, 0; low words scratch
  uint32_t q1;
};
__device__ __forceinline__ MontK mont_k(uint32_t q1) {
  MontK K;
  K.c1 = 1ull << 32;
  K.cq = (uint64_t)q1 << 32;
  K.c0 = 0;
  K.q1 = q1;
  asm("" : "+v"(K.c1), "+v"(K.cq), "+v"(K.c0));
  return K;
}
// (lo, hi) as one register pair the compiler cannot take apart again: a 64-bit add of pk(lo, hi)
// is otherwise split into an add of {lo, 0} and a 32-bit add of hi (two more full-rate ops)
__device__ __forceinline__ uint64_t pair(uint32_t lo, uint32_t hi) {
  uint64_t v = pk(lo, hi);
  asm("" : "+v"(v));
  return v;
}
__device__ __forceinline__ uint64_t with_lo(uint64_t v, uint32_t lo) { return (v & 0xffffffff00000000ull) | lo; }

// v_mad_u64_u32 with a wave-uniform second factor taken straight from an SGPR (no copy to a VGPR)
__device__ __forceinline__ uint64_t mad_co_s(uint32_t a, uint32_t b, uint64_t c, lmask& co) {
  uint64_t d;
  asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(d), "=s"(co) : "v"(a), "s"(b), "v"(c));
  return d;
}
// y w 2^-64 mod q in (0, q + ceil(2 q^2 / 2^64)), y in [0, 2q), w < q; ntt64_mont_ok(q)
// SW: w is wave-uniform and lives in SGPRs (the H round's scalar-loaded twiddles, N^-1, w1n)
template <bool SW = false>
__device__ __forceinline__ uint64_t mont_x(uint64_t y, uint64_t w, MontK& K) {
  const uint32_t y0 = lo32(y), y1 = hi32(y), w0 = lo32(w), w1 = hi32(w);
  const uint64_t p0 = (uint64_t)y0 * w0;
  K.c1 = with_lo(K.c1, hi32(p0));
  lmask b1, b2;
  const uint64_t p1 = SW ? mad_co_s(y0, w1, K.c1, b1) : mad_co(y0, w1, K.c1, b1);  // asm: as C++ the two middle products are summed first and c1 added last
  const uint64_t p2 = (uint64_t)y1 * w0 + p1;
  K.cq = with_lo(K.cq, hi32(p2));
  const uint64_t p3 = (uint64_t)y1 * w1 + K.cq;
  const uint64_t Z = (uint64_t)lo32(p0) * K.q1;
  const uint32_t m1 = sub_co(lo32(p2), lo32(Z), b1);
  K.c0 = with_lo(K.c0, hi32(Z));
  const uint64_t W = (uint64_t)m1 * K.q1 + K.c0;
  const uint32_t r0 = subb_co(lo32(p3), lo32(W), b1, b2);
  const uint32_t r1 = subb_co(hi32(p3), hi32(W), b2, b1);
  return pair(r0, r1);
}
// (x, y) <- (x + w y, x - w y), lazy [0, 2q) in and out.  x + t < 3q + ceil(2 q^2 / 2^64) < 2^64
// under the gate, so the sum needs no 65th bit and the borrow of s - 2q is the select mask.
template <bool SW = false>
__device__ __forceinline__ void fwd_bfly_m(uint64_t& x, uint64_t& y, uint64_t w, uint64_t q2, MontK& K) {
  const uint64_t t = mont_x<SW>(y, w, K);
  lmask b, b2, e, e2;
  const uint64_t s = x + t;
  const uint32_t u0 = sub_co(lo32(s), lo32(q2), b);
  const uint32_t u1 = subb_co(hi32(s), hi32(q2), b, b2);
  const uint32_t d0 = sub_co(lo32(x), lo32(t), e);
  const uint32_t d1 = subb_co(hi32(x), hi32(t), e, e2);
  const uint64_t d = pair(d0, d1);
  const uint64_t f = d + q2;
  x = pk(sel(b2, lo32(s), u0), sel(b2, hi32(s), u1));
  y = pk(sel(e2, lo32(f), lo32(d)), sel(e2, hi32(f), hi32(d)));
}
// (x, y) <- (x + y, (x - y) w), lazy [0, 2q) in and out (x + y can reach 4q: the carry form)
template <bool SW = false>
__device__ __forceinline__ void inv_bfly_m(uint64_t& x, uint64_t& y, uint64_t w, uint64_t q2, MontK& K) {
  lmask c, c2, b, b2, e, e2;
  const uint32_t s0 = add_co(lo32(x), lo32(y), c);
  const uint32_t s1 = addc_co(hi32(x), hi32(y), c, c2);
  const uint32_t u0 = sub_co(s0, lo32(q2), b);
  const uint32_t u1 = subb_co(s1, hi32(q2), b, b2);
  const lmask m = c2 | ~b2;
  const uint32_t d0 = sub_co(lo32(x), lo32(y), e);
  const uint32_t d1 = subb_co(hi32(x), hi32(y), e, e2);
  const uint64_t d = pair(d0, d1);
  const uint64_t f = d + q2;
  x = pk(sel(m, u0, s0), sel(m, u1, s1));
  y = mont_x<SW>(pk(sel(e2, lo32(f), lo32(d)), sel(e2, hi32(f), hi32(d))), w, K);
}
// [0, 2q) -> [0, q)
__device__ __forceinline__ uint64_t canon_x(uint64_t x, uint64_t q) {
  lmask b, b2;
  const uint32_t t0 = sub_co(lo32(x), lo32(q), b);
  const uint32_t t1 = subb_co(hi32(x), hi32(q), b, b2);
  return pk(sel(b2, lo32(x), t0), sel(b2, hi32(x), t1));
}

// ----------------------------------------------------------------------------------------
// Pass kernel: 8 consecutive radix-2 stages [G0, G0+8) of a 2^logN-point transform, as 2^(logN-8)
// independent 256-point sub-transforms per polynomial whose points sit at stride S =
// 2^(logN-G0-8): COL (S >= 16, G0 = 0) or ROW (S = 1).  A 512-thread workgroup owns a tile of
// 16 sub-transforms x 256 points = 32 KiB; each thread holds 8 points in registers and runs
// three rounds of 3 + 3 + 2 stages with two LDS exchanges (plus one transpose for coalesced
// ROW stores/loads).  Index algebra (ntt.go:98-115 forward, :357-466 inverse): local stage k
// combines bit b = 7-k of the in-sub-transform index x and uses
//     tw[2^(G0+k) + (hi << k) + (x >> (b+1))],   hi = sub-transform prefix (ROW: row index).
// Register patterns per round (t = lane's slot, y / r = register):
//     H: x = t + 32 y   (window bits [5,8))       M: x = (t>>2)<<5 | y<<2 | (t&3)   (bits [2,5))
//     L: x = 8 t + r    (window bits [0,2), r>>2 = x bit 2)
// ----------------------------------------------------------------------------------------
struct Ntt64Args {
  const uint64_t* in;
  uint64_t* out;
  // (w, floor(w 2^64 / q)) pairs, forward or inverse: [N] in the reference order tw[m + i]
  // (ntt.go:153-203), then for N = 2^16 a lane-ordered copy of the ROW pass's last two stages:
  // row r, stage 14: [r*192 + 32 g + t] = tw[2^14 + 64 r + 2 t + g]       (g < 2,  t < 32)
  //        stage 15: [r*192 + 64 + 32 j + t] = tw[2^15 + 128 r + 4 t + j] (j < 4)
  // MONT kernels: the same two tables as single words in Montgomery form (w 2^64 mod q, the
  // reference's own representation), 8 B per entry, same indices; behind the inverse one, at
  // kNttFoldBase, rank_inv and rank_inv twInv[1 .. 16) (ntt_tile.hpp: the fold of the last round)
  const uint64_t* tw;
  uint64_t q, q2;
  uint32_t nqhi, q1;      // -(q >> 32) mod 2^32 (Shoup), q >> 32 (MONT)
  uint64_t ninv, ninv_p;  // N^-1 and its Shoup quotient (inverse, last stage); MONT: N^-1 in Montgomery form, ninv_p unused
  uint64_t w1n, w1n_p;    // twInv[1] N^-1, likewise
  long long total_sub;    // batch * 2^(logN - 8)
  int logN, G0;
  int rev;  // 1: tiles in reverse order (a transform's second pass: Infinity Cache reuse, rg_bstore)
};

// ----------------------------------------------------------------------------------------
// N = 2^16 pass kernel: compile-time strides, buffer addressing (one VGPR offset per access
// pattern, per-access constants in SGPR soffsets / immediates) and one tile per workgroup, so
// no address is held in registers across the tile.  COL = global stages [0, 8) on the 256
// columns (stride 256), ROW = [8, 16) on the 256 rows.
// Tiles: COL = 16 adjacent columns of one polynomial.  ROW = 16 rows; with RP ("row-major over
// polynomials", batch % 16 == 0) the 16 rows are the SAME row of 16 consecutive polynomials,
// so every twiddle of the tile is shared by all 16 sub-transforms (as in COL): the first
// round's twiddles come from scalar loads and the others are loaded once per lane slot t,
// shared by both half-waves.  Without RP the 16 rows are 16 consecutive rows of one poly.
// ----------------------------------------------------------------------------------------
typedef unsigned int rg_u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int rg_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rg_buf(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, 0x7fffffff, 0x00020000);
}
// cache policy of the transform's data: loads nt, stores default.  A transform's second pass
// runs its tiles in reverse order (Ntt64Args::rev), so it starts on the polynomials its first pass
// wrote last, which the default-policy stores left in the 256 MiB Infinity Cache; the next call's
// first pass (forward order) likewise starts where this second pass ended.  Round 5: 0.902 ->
// 0.889 ms per step against nt stores in forward order (nt on both, in forward order, had been
// -3% against the default in round 2; the default alone without the reversal is +5%).  The
// M- and L-round twiddles are staged in LDS per tile for COL and RP
// tiles (L round -0.6% per step, M round a further -2.3%, against per-lane global loads that
// queue behind the tile's HBM traffic); s_setprio on the tile loads (+6%) or on the
// butterflies (+5%) measured slower.
constexpr int kNttAux = 2, kNttAuxSt = 0;
__device__ __forceinline__ uint64_t rg_bload(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
  const rg_u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, kNttAux);
  return pk(v.x, v.y);
}
__device__ __forceinline__ void rg_bstore(uint64_t x, __amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
  rg_u32x2 v;
  v.x = lo32(x);
  v.y = hi32(x);
  __builtin_amdgcn_raw_buffer_store_b64(v, r, voff, soff, kNttAuxSt);
}

// PROBE (tuning only; production = 0): 1 = twiddles from registers (no table loads),
// 2 = butterflies replaced by one add (memory / LDS / twiddle-load floor), 3 = both,
// 4 = no global data loads / stores (the tile is synthesised from the thread index and its
// result kept live by a store that never fires): the compute floor (butterflies, twiddle loads,
// LDS exchanges) of the same launch, timed by bench.py through rg_set_probe
// LTW / MTW: the L round (PAT 2) and the M round (PAT 1) read their twiddles from the tile's LDS
// copy `ltw` (248 entries staged by ntt16_tile: COL tw[8, 256); RP the row's lane-ordered L-round
// copy, then its 56 stage 3-5 entries) instead of per-lane global loads
// MONT: the Montgomery product (mont_x) on single-word twiddles in Montgomery form, for moduli
// that pass ntt64_mont_ok; every table entry, staged word and LDS slot is 8 B instead of a 16-B
// (w, quotient) pair, and N^-1 / w1n stay in Montgomery form.  !MONT: Shoup's product (shoup_x).
template <bool MONT>
using tw_t = std::conditional_t<MONT, uint64_t, ulonglong2>;
__device__ __forceinline__ void tw_put(uint64_t& w, uint64_t& wp, const ulonglong2& v) {
  w = v.x;
  wp = v.y;
}
__device__ __forceinline__ void tw_put(uint64_t& w, uint64_t& wp, uint64_t v) {
  w = v;
  wp = 0;
}
// table entry idx through the buffer resource
template <bool MONT>
__device__ __forceinline__ tw_t<MONT> tw_bload(__amdgpu_buffer_rsrc_t twr, uint32_t idx) {
  if constexpr (MONT) {
    const rg_u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(twr, idx * 8u, 0, 0);
    return pk(v.x, v.y);
  } else {
    const rg_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(twr, idx * 16u, 0, 0);
    return ulonglong2{pk(v.x, v.y), pk(v.z, v.w)};
  }
}

template <bool MONT, int RK, int LO, int PAT, bool INV, bool SCALE, bool COL, bool RP, int PROBE>
__device__ __forceinline__ void ntt16_round(const Ntt64Args& a, __amdgpu_buffer_rsrc_t twr, uint64_t (&e)[8],
                                            uint32_t hi, uint32_t t, [[maybe_unused]] MontK& K,
                                            const tw_t<MONT>* ltw = nullptr) {  // K: MONT only (dead in the Shoup kernels)
  constexpr bool LTW = PAT == 2 && (COL || RP);
  constexpr int G0 = COL ? 0 : 8;
  // twiddle index independent of the lane: the H round of COL / RP tiles.  (The M round of COL
  // tiles is wave-uniform too, x >> (b + 1) depending on t >> 2 = tid >> 6 only, but scalar loads
  // there measured no faster: their lgkmcnt waits also wait for the exchange's LDS traffic.)
  constexpr bool UNIFORM = (COL || RP) && PAT == 0;
  constexpr bool MTW = PAT == 1 && (COL || RP) && (PROBE & 1) == 0;
  auto xof = [&](int rho) -> uint32_t { return ntt8_xof(PAT, t, rho); };
  // rank_inv folded into this round's y-branch twiddles (ntt_tile.hpp): the round that holds global
  // stage 0 of a MONT inverse.  The scaled twiddles are scalar loads from behind the table, like the
  // round's plain ones; register 0 keeps w1n and the explicit product, as kernel arguments.
  constexpr bool FOLD = MONT && INV && SCALE && COL && PAT == 0 && (PROBE & 1) == 0;
#pragma unroll
  for (int sp = 0; sp < RK; ++sp) {
    const int bw = ntt_round_bw(INV, RK, sp);
    const int b = LO + bw;
    const int k = 7 - b;
    const int half = 1 << bw;
    const bool last = INV && SCALE && k == 0;  // SCALE: this pass holds global stage 0
    uint64_t w[4], wp[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int rho0 = ntt_pair_rho0(RK, bw, j);
      const bool scaled = FOLD && ntt_fold_scaled(rho0, bw);
      // same x >> (b+1) as the previous pair, and the same variant of it
      if ((rho0 & (half - 1)) != 0 && !(FOLD && ntt_fold_scaled(ntt_pair_rho0(RK, bw, j - 1), bw))) {
        w[j] = w[j - 1];
        wp[j] = wp[j - 1];
        continue;
      }
      if (last && (!FOLD || scaled)) {
        w[j] = a.w1n;
        wp[j] = a.w1n_p;
        continue;
      }
      if constexpr ((PROBE & 1) != 0) {
        w[j] = a.w1n + (xof(rho0) >> (b + 1)) + hi;
        wp[j] = a.w1n_p;
      } else if constexpr (UNIFORM) {
        const uint32_t idx = ntt_tw_index(G0, b, hi, xof(rho0)) + (scaled ? kNttFoldBase : 0u);
        const uint32_t iu = __builtin_amdgcn_readfirstlane(idx);
        tw_put(w[j], wp[j], reinterpret_cast<const tw_t<MONT>*>(a.tw)[iu]);
      } else if constexpr (LTW && COL) {
        tw_put(w[j], wp[j], ltw[(1u << k) + (xof(rho0) >> (b + 1)) - 8u]);
      } else if constexpr (LTW) {
        tw_put(w[j], wp[j], ltw[(k == 6 ? 32u * (rho0 >> 2) : 64u + 32u * (rho0 >> 1)) + t]);
      } else if constexpr (MTW) {  // M round: COL tw[8, 64) ahead of the L round's; RP the row's stage 3-5 entries after them
        tw_put(w[j], wp[j],
               COL ? ltw[(1u << k) + (xof(rho0) >> (b + 1)) - 8u]
                   : ltw[192u + (k == 3 ? 0u : k == 4 ? 8u : 24u) + (xof(rho0) >> (b + 1))]);
      } else if constexpr (!COL && PAT == 2) {
        // ROW last round (stages 14, 15): lane-ordered copy after the natural table, lane t's
        // j-th twiddle at t + 32 j, so every load is one coalesced 512-B (MONT: 256-B) run
        const uint32_t pos = (kNttRowCopyBase + hi * 192u) + (k == 6 ? 32u * (rho0 >> 2) : 64u + 32u * (rho0 >> 1)) + t;
        tw_put(w[j], wp[j], tw_bload<MONT>(twr, pos));
      } else {
        tw_put(w[j], wp[j], tw_bload<MONT>(twr, ntt_tw_index(G0, b, hi, xof(rho0))));
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int rho0 = ntt_pair_rho0(RK, bw, j);
      const int rho1 = rho0 + half;
      if constexpr ((PROBE & 2) != 0) {
        e[rho0] += e[rho1] ^ w[j] ^ wp[j];
      } else if constexpr (MONT) {
        // scalar twiddles (the H round's scalar loads; w1n and N^-1 are kernel arguments) feed
        // the asm multiply from their SGPRs
        constexpr bool SW = UNIFORM && (PROBE & 1) == 0;
        if constexpr (!INV) {
          fwd_bfly_m<SW>(e[rho0], e[rho1], w[j], a.q2, K);
        } else {
          if (last && (!FOLD || ntt_fold_product(rho0, bw, RK))) {
            inv_bfly_m<true>(e[rho0], e[rho1], w[j], a.q2, K);
            e[rho0] = mont_x<true>(e[rho0], a.ninv, K);
          } else {
            inv_bfly_m<SW>(e[rho0], e[rho1], w[j], a.q2, K);
          }
        }
      } else if constexpr (!INV) {
        fwd_bfly_x(e[rho0], e[rho1], w[j], wp[j], a.q2, a.nqhi);
      } else {
        inv_bfly_x(e[rho0], e[rho1], w[j], wp[j], a.q2, a.nqhi);
        if (last) e[rho0] = shoup_x(e[rho0], a.ninv, a.ninv_p, a.nqhi);
      }
    }
  }
}

// One 16 x 256 tile.  LDS images (u64 index):
//   COL: transposed [x][s] image 16 x + s + 16 (x >> 3) for every exchange; per pattern this is
//        a lane base plus compile-time offsets: H (x = t + 32 y): 16t + s + 16(t>>3) + 576 y;
//        M (x = 32(t>>2) + 4y + (t&3)): s + 16(t&3) + 576(t>>2) + 64 y + 16(y>>1);
//        L (x = 8t + r): 144 t + s + 16 r.
//   ROW: [s][x] rows of 288 with a per-exchange pad: H<->M pad 4(x>>5), M<->L pad (x>>3),
//        L<->H pad (x>>5).
// Every pattern pair was checked conflict-free for ds_*_b64 half-wave groups
// (SQ_LDS_BANK_CONFLICT = 0 for COL in profiles/r01_ntt16_pmc_summary.txt).
template <bool MONT, bool INV, bool COL, bool SCALE, bool CANON, bool RP, int PROBE = 0>
__device__ __forceinline__ void ntt16_tile(const Ntt64Args& a, uint32_t tile, uint64_t* lds, tw_t<MONT>* ltw) {
  const uint32_t tid = threadIdx.x;
  const uint32_t s = COL ? (tid & 15u) : (tid >> 5);
  const uint32_t t = COL ? (tid >> 4) : (tid & 31u);
  // tile base (elements) and the stride between the tile's ROW sub-transforms
  //   COL: poly * 2^16 + column block * 16
  //   ROW: 16 consecutive rows (tile * 4096), or RP: row (tile & 255) of polys 16 (tile >> 8) + s
  const size_t tbase = COL  ? (((size_t)(tile >> 4) << 16) + ((tile & 15u) << 4))
                       : RP ? (((size_t)(tile >> 8) << 20) + ((tile & 255u) << 8))
                            : ((size_t)tile << 12);
  constexpr uint32_t RSH = RP ? 16 : 8;  // log2 of the ROW sub-transform stride (elements)
  const __amdgpu_buffer_rsrc_t rin = rg_buf(a.in + tbase);
  const __amdgpu_buffer_rsrc_t rout = rg_buf(a.out + tbase);
  const __amdgpu_buffer_rsrc_t twr = rg_buf(a.tw);
  const uint32_t hi = COL ? 0u : RP ? (uint32_t)__builtin_amdgcn_readfirstlane(tile & 255u) : (((tile << 4) + s) & 255u);
  uint64_t e[8];
  constexpr bool LTW = (COL || RP) && (PROBE & 1) == 0;
  // The M and L rounds' 248 twiddle pairs, one 8-B word per thread (496 threads; MONT: 248
  // single words, 248 threads): the word is loaded after the tile's data loads and written to
  // LDS just before the first barrier, so no wave waits for it before issuing its data loads
  // (the first load's latency would otherwise open every tile).  COL: tw[8, 256); RP: the row's
  // lane-ordered L-round copy, then its 56 stage 3-5 entries.
  const bool stv_on = LTW && tid < (MONT ? 248u : 496u);
  uint32_t st_src = 0, st_dst = tid;
  if constexpr (MONT) {
    if constexpr (COL) {
      st_src = 8u + tid;
    } else if (tid < 192u) {
      st_src = 65536u + hi * 192u + tid;
    } else {
      const uint32_t ent = tid - 192u;
      const uint32_t kk = ent < 8u ? 3u : ent < 24u ? 4u : 5u, j = ent - (kk == 3u ? 0u : kk == 4u ? 8u : 24u);
      st_src = (1u << (8u + kk)) + (hi << kk) + j;
    }
  } else if constexpr (COL) {
    st_src = 16u + tid;
  } else if (tid < 384u) {
    st_src = 2u * (65536u + hi * 192u) + tid;
  } else {
    const uint32_t wd = tid - 384u, ent = wd >> 1;
    const uint32_t kk = ent < 8u ? 3u : ent < 24u ? 4u : 5u, j = ent - (kk == 3u ? 0u : kk == 4u ? 8u : 24u);
    st_src = 2u * ((1u << (8u + kk)) + (hi << kk) + j) + (wd & 1u);
    st_dst = 2u * (192u + ent) + (wd & 1u);
  }
  uint64_t stv = 0;
  auto stage_write = [&]() {
    if (stv_on) reinterpret_cast<uint64_t*>(ltw)[st_dst] = stv;
  };
  // ---- global load
  if constexpr ((PROBE & 4) != 0) {
#pragma unroll
    for (int y = 0; y < 8; ++y) e[y] = (uint64_t)(tid * 0x9E3779B9u + tile * 8u + (uint32_t)y);
  } else if constexpr (COL) {
    if constexpr (!INV) {
      const uint32_t vo = ((t << 8) + s) * 8u;
#pragma unroll
      for (int y = 0; y < 8; ++y) e[y] = rg_bload(rin, vo, (uint32_t)y << 16);
    } else {
      const uint32_t vo = ((t << 11) + s) * 8u;
#pragma unroll
      for (int r = 0; r < 8; ++r) e[r] = rg_bload(rin, vo, (uint32_t)r << 11);
    }
  } else {
    const uint32_t vo = ((s << RSH) + t) * 8u;
#pragma unroll
    for (int y = 0; y < 8; ++y) e[y] = rg_bload(rin, vo + 256u * y, 0);
  }
  if (stv_on) stv = reinterpret_cast<const uint64_t*>(a.tw)[st_src];
  // PROBE & 4: the result stays live through a store that never fires (values are < 2q < 2^64 - 1)
  auto st64 = [&](uint64_t x, uint32_t voff, uint32_t soff) {
    if constexpr ((PROBE & 4) != 0) {
      if (x == ~0ull) rg_bstore(x, rout, voff, soff);
    } else {
      rg_bstore(x, rout, voff, soff);
    }
  };
  const uint32_t bH = 16 * t + s + 16 * (t >> 3), bM = s + 16 * (t & 3) + 576 * (t >> 2), bL = 144 * t + s;
  auto offM = [](int y) { return 64 * y + 16 * (y >> 1); };
  const uint32_t rH = 288 * s + t, rM = 288 * s + 36 * (t >> 2) + (t & 3), rL9 = 288 * s + 9 * t,
                 rL8 = 288 * s + 8 * t + (t >> 2);
  MontK K{};  // the Shoup kernels carry it unused
  if constexpr (MONT) K = mont_k(a.q1);
  if constexpr (!INV) {
    ntt16_round<MONT, 3, 5, 0, false, false, COL, RP, PROBE>(a, twr, e, hi, t, K);
    stage_write();
    // exchange H -> M
#pragma unroll
    for (int y = 0; y < 8; ++y) lds[COL ? bH + 576 * y : rH + 36 * y] = e[y];
    __syncthreads();
#pragma unroll
    for (int y = 0; y < 8; ++y) e[y] = lds[COL ? bM + offM(y) : rM + 4 * y];
    ntt16_round<MONT, 3, 2, 1, false, false, COL, RP, PROBE>(a, twr, e, hi, t, K, ltw);
    __syncthreads();
    // exchange M -> L
#pragma unroll
    for (int y = 0; y < 8; ++y) lds[COL ? bM + offM(y) : rM + 4 * y + (y >> 1)] = e[y];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; ++r) e[r] = lds[COL ? bL + 16 * r : rL9 + r];
    ntt16_round<MONT, 2, 0, 2, false, false, COL, RP, PROBE>(a, twr, e, hi, t, K, ltw);
    if (CANON) {
#pragma unroll
      for (int r = 0; r < 8; ++r) e[r] = canon_x(e[r], a.q);
    }
    if constexpr (COL) {
      const uint32_t vo = ((t << 11) + s) * 8u;
#pragma unroll
      for (int r = 0; r < 8; ++r) st64(e[r], vo, (uint32_t)r << 11);
    } else {  // L -> H through LDS (pad x >> 5), then coalesced rows
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 8; ++r) lds[rL8 + r] = e[r];
      __syncthreads();
      const uint32_t vo = ((s << RSH) + t) * 8u;
#pragma unroll
      for (int y = 0; y < 8; ++y) st64(lds[rH + 33 * y], vo + 256u * y, 0);
    }
  } else {
    stage_write();
    if constexpr (!COL) {  // ROW inverse: loaded in H, transpose to L (pad x >> 5)
#pragma unroll
      for (int y = 0; y < 8; ++y) lds[rH + 33 * y] = e[y];
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 8; ++r) e[r] = lds[rL8 + r];
      __syncthreads();
    }
    if constexpr (COL && LTW) __syncthreads();  // the staged twiddles (ROW's transpose has its barrier)
    ntt16_round<MONT, 2, 0, 2, true, SCALE, COL, RP, PROBE>(a, twr, e, hi, t, K, ltw);
    // exchange L -> M
#pragma unroll
    for (int r = 0; r < 8; ++r) lds[COL ? bL + 16 * r : rL9 + r] = e[r];
    __syncthreads();
#pragma unroll
    for (int y = 0; y < 8; ++y) e[y] = lds[COL ? bM + offM(y) : rM + 4 * y + (y >> 1)];
    ntt16_round<MONT, 3, 2, 1, true, SCALE, COL, RP, PROBE>(a, twr, e, hi, t, K, ltw);
    __syncthreads();
    // exchange M -> H
#pragma unroll
    for (int y = 0; y < 8; ++y) lds[COL ? bM + offM(y) : rM + 4 * y] = e[y];
    __syncthreads();
#pragma unroll
    for (int y = 0; y < 8; ++y) e[y] = lds[COL ? bH + 576 * y : rH + 36 * y];
    ntt16_round<MONT, 3, 5, 0, true, SCALE, COL, RP, PROBE>(a, twr, e, hi, t, K);
    if (CANON) {
#pragma unroll
      for (int y = 0; y < 8; ++y) e[y] = canon_x(e[y], a.q);
    }
    if constexpr (COL) {
      const uint32_t vo = ((t << 8) + s) * 8u;
#pragma unroll
      for (int y = 0; y < 8; ++y) st64(e[y], vo, (uint32_t)y << 16);
    } else {
      const uint32_t vo = ((s << RSH) + t) * 8u;
#pragma unroll
      for (int y = 0; y < 8; ++y) st64(e[y], vo + 256u * y, 0);
    }
  }
}

// ----------------------------------------------------------------------------------------
// The same tile with 16 points per thread, for the two MONT passes that measured faster on it
// (DESIGN.md section 4.2): ROW forward on RP tiles and COL inverse.  256 threads, rounds of 4 + 4
// stages, A (window [4, 8), x = t + 16 y) and B ([0, 4), x = 16 t + r): COL has one LDS exchange
// instead of two, ROW two with its transpose instead of three, and the butterflies are the same.
// Round A's 15 twiddles are uniform over the tile (scalar loads), round B's 15 per lane come from
// the tile's LDS copy (ntt_tile.hpp: ntt16_stage_src, ntt16_ltw_pos, and the LDS images).  COL
// forward and ROW inverse measured no faster on this tile and stay on 8 points; their halves of this
// tile are tools/experiments/ntt16_tile16_all_passes.patch.
// ----------------------------------------------------------------------------------------
template <int PAT, bool INV, bool SCALE, bool COL, int PROBE>
__device__ __forceinline__ void ntt16x_round(const Ntt64Args& a, uint64_t (&e)[16], uint32_t hi, uint32_t t, MontK& K,
                                             const uint64_t* ltw) {
  constexpr int G0 = COL ? 0 : 8, RK = 4, LO = PAT == 0 ? 4 : 0;
  constexpr bool TOP = INV && SCALE && COL && PAT == 0;  // the round that holds global stage 0
  constexpr bool FOLD = TOP && (PROBE & 1) == 0;
  constexpr bool SW = PAT == 0 && (PROBE & 1) == 0;  // twiddles in SGPRs
#pragma unroll
  for (int sp = 0; sp < RK; ++sp) {
    const int bw = ntt_round_bw(INV, RK, sp);
    const int b = LO + bw;
    const int half = 1 << bw;
    const bool last = TOP && b == 7;
    uint64_t w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int rho0 = ntt_pair_rho0(RK, bw, j);
      const bool scaled = FOLD && ntt_fold_scaled(rho0, bw);
      if ((rho0 & (half - 1)) != 0 && !(FOLD && ntt_fold_scaled(ntt_pair_rho0(RK, bw, j - 1), bw))) {
        w[j] = w[j - 1];
        continue;
      }
      if (last && (!FOLD || scaled)) {
        w[j] = a.w1n;
        continue;
      }
      const uint32_t x = ntt16_xof(PAT, t, rho0);
      if constexpr ((PROBE & 1) != 0) {
        w[j] = a.w1n + (x >> (b + 1)) + hi;
      } else if constexpr (PAT == 0) {
        const uint32_t idx = ntt_tw_index(G0, b, hi, x) + (scaled ? kNttFoldBase : 0u);
        w[j] = a.tw[__builtin_amdgcn_readfirstlane(idx)];
      } else {
        w[j] = ltw[ntt16_ltw_pos((1u << (7 - b)) + (x >> (b + 1)))];
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int rho0 = ntt_pair_rho0(RK, bw, j);
      const int rho1 = rho0 + half;
      if constexpr ((PROBE & 2) != 0) {
        e[rho0] += e[rho1] ^ w[j];
      } else if constexpr (!INV) {
        fwd_bfly_m<SW>(e[rho0], e[rho1], w[j], a.q2, K);
      } else if (last && (!FOLD || ntt_fold_product(rho0, bw, RK))) {
        inv_bfly_m<true>(e[rho0], e[rho1], w[j], a.q2, K);
        e[rho0] = mont_x<true>(e[rho0], a.ninv, K);
      } else {
        inv_bfly_m<SW>(e[rho0], e[rho1], w[j], a.q2, K);
      }
    }
  }
}

template <bool INV, bool COL, bool SCALE, bool CANON, int PROBE>
__device__ __forceinline__ void ntt16x_tile(const Ntt64Args& a, uint32_t tile, uint64_t* lds, uint64_t* ltw) {
  static_assert(INV == COL, "ROW forward and COL inverse");
  const uint32_t tid = threadIdx.x;
  const uint32_t s = ntt16_s_of(COL, tid), t = ntt16_t_of(COL, tid);
  // COL: poly * 2^16 + column block * 16; ROW: row (tile & 255) of polys 16 (tile >> 8) + s
  const size_t tbase = COL ? (((size_t)(tile >> 4) << 16) + ((tile & 15u) << 4))
                           : (((size_t)(tile >> 8) << 20) + ((tile & 255u) << 8));
  const __amdgpu_buffer_rsrc_t rin = rg_buf(a.in + tbase);
  const __amdgpu_buffer_rsrc_t rout = rg_buf(a.out + tbase);
  const uint32_t hi = COL ? 0u : (uint32_t)__builtin_amdgcn_readfirstlane(tile & 255u);
  uint64_t e[16];
  // round B's 240 twiddles, one word per thread, loaded after the tile's data loads and written to
  // LDS before the first barrier
  const bool stv_on = (PROBE & 1) == 0 && tid < 240u;
  const uint32_t st_src = ntt16_stage_src(COL, hi, 16u + tid), st_dst = ntt16_ltw_pos(16u + tid);
  // global accesses, one VGPR offset per pattern.  COL: element x * 256 + s, loaded in the B
  // pattern (rows r apart: soffset r << 11) and stored in the A pattern (rows 16 y apart: y << 15);
  // ROW: element (s << 16) + x, both ways in the A pattern (128-B runs 16 y elements apart:
  // immediate 128 y)
  const uint32_t gA = COL ? ((t << 8) + s) * 8u : ((s << 16) + t) * 8u;
  if constexpr ((PROBE & 4) != 0) {
#pragma unroll
    for (int y = 0; y < 16; ++y) e[y] = (uint64_t)(tid * 0x9E3779B9u + tile * 16u + (uint32_t)y);
  } else if constexpr (COL) {
    const uint32_t gB = ((t << 12) + s) * 8u;
#pragma unroll
    for (int r = 0; r < 16; ++r) e[r] = rg_bload(rin, gB, (uint32_t)r << 11);
  } else {
#pragma unroll
    for (int y = 0; y < 16; ++y) e[y] = rg_bload(rin, gA + 128u * y, 0);
  }
  uint64_t stv = 0;
  if (stv_on) stv = a.tw[st_src];
  const uint32_t pA = ntt16_lds_pos(COL, s, t), pB = ntt16_lds_pos(COL, s, 16u * t);
  constexpr int oA = COL ? 272 : 17, oB = COL ? 16 : 1;
  MontK K = mont_k(a.q1);
  if constexpr (!INV) {  // ROW forward
    ntt16x_round<0, false, false, COL, PROBE>(a, e, hi, t, K, ltw);
    if (stv_on) ltw[st_dst] = stv;
#pragma unroll
    for (int y = 0; y < 16; ++y) lds[pA + oA * y] = e[y];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) e[r] = lds[pB + oB * r];
    ntt16x_round<1, false, false, COL, PROBE>(a, e, hi, t, K, ltw);
    if (CANON) {
#pragma unroll
      for (int r = 0; r < 16; ++r) e[r] = canon_x(e[r], a.q);
    }
    __syncthreads();  // B -> A through LDS, then 128-B runs
#pragma unroll
    for (int r = 0; r < 16; ++r) lds[pB + oB * r] = e[r];
    __syncthreads();
#pragma unroll
    for (int y = 0; y < 16; ++y) e[y] = lds[pA + oA * y];
  } else {  // COL inverse
    if (stv_on) ltw[st_dst] = stv;
    __syncthreads();  // the staged twiddles
    ntt16x_round<1, true, SCALE, COL, PROBE>(a, e, hi, t, K, ltw);
#pragma unroll
    for (int r = 0; r < 16; ++r) lds[pB + oB * r] = e[r];
    __syncthreads();
#pragma unroll
    for (int y = 0; y < 16; ++y) e[y] = lds[pA + oA * y];
    ntt16x_round<0, true, SCALE, COL, PROBE>(a, e, hi, t, K, ltw);
    if (CANON) {
#pragma unroll
      for (int y = 0; y < 16; ++y) e[y] = canon_x(e[y], a.q);
    }
  }
#pragma unroll
  for (int y = 0; y < 16; ++y) {
    const uint32_t vo = COL ? gA : gA + 128u * y, so = COL ? (uint32_t)y << 15 : 0u;
    if constexpr ((PROBE & 4) != 0) {  // the result stays live through a store that never fires
      if (e[y] == ~0ull) rg_bstore(e[y], rout, vo, so);
    } else {
      rg_bstore(e[y], rout, vo, so);
    }
  }
}

// PTS: points per thread, 8 (512 threads) or 16 (256 threads; MONT, ROW forward on RP tiles or COL inverse)
template <bool MONT, bool INV, bool COL, bool SCALE, bool CANON, bool RP = false, int MINW = 1, int PTS = 8, int PROBE = 0>
__global__ __launch_bounds__(PTS == 16 ? 256 : 512, MINW) void ntt16_pass(Ntt64Args a) {
  const uint32_t tile = a.rev ? gridDim.x - 1u - blockIdx.x : blockIdx.x;
  if constexpr (PTS == 16) {
    static_assert(MONT && INV == COL && (COL || RP), "the 16-point tile serves MONT ROW forward (RP) and COL inverse");
    __shared__ uint64_t lds[kNtt16LdsLen];
    __shared__ uint64_t ltw[kNtt16LtwLen];  // 35.9 KiB per workgroup with lds: 4 per CU
    ntt16x_tile<INV, COL, SCALE, CANON, PROBE>(a, tile, lds, ltw);
  } else {
    __shared__ uint64_t lds[16 * 288];
    __shared__ tw_t<MONT> ltw[COL || RP ? 248 : 1];  // 39.9 KiB (MONT: 37.9 KiB) per workgroup with lds: 4 per CU
    ntt16_tile<MONT, INV, COL, SCALE, CANON, RP, PROBE>(a, tile, lds, ltw);
  }
}

#endif  // __HIPCC__

}  // namespace rg
