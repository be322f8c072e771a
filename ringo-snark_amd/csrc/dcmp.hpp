// dcmp.hpp -- the arithmetic core of the Buckler norm decomposition: decomposeBig
// (buckler/utils.go:34-56) on one field element, in sign-magnitude form.
//
// The reference works on a centred big integer.  With x = plain(w) in [0, q):
//   xs = x > (q >> 1) ? x - q : x
//   for each base element b_j in order:   xs >= b_j: digit +1, xs -= b_j
//                                         xs <= -b_j: digit -1, xs += b_j
//                                         otherwise:  digit 0
// Here the value is held as a sign s and a magnitude m that never change roles:
//   s = [x > q >> 1],  m = s ? q - x : x        (q odd: m <= (q - 1) / 2, and s = 1 gives m >= 1)
//   for each b_j in order:   m >= b_j: digit s ? -1 : +1, m -= b_j;   otherwise digit 0
// which is one L-limb subtract with borrow and a select per step, with no signed arithmetic.
//
// Equivalence, by induction on the invariant xs = s ? -m : m with m >= 0, for b_j >= 1:
//   s = 0: xs = m >= 0.  The reference's first case is m >= b_j: digit +1 and xs - b_j = m - b_j
//          >= 0, the invariant again.  Its second case needs xs <= -b_j < 0: never.  So digit 0
//          iff m < b_j.
//   s = 1, m >= 1: xs = -m < 0.  The first case needs xs >= b_j >= 1: never.  The second is
//          -m <= -b_j, i.e. m >= b_j: digit -1 and xs + b_j = -(m - b_j) <= 0, the invariant again.
//   s = 1, m = 0 (a step has brought the magnitude to zero): xs = 0.  0 >= b_j and 0 <= -b_j are
//          both false for b_j >= 1: digit 0.  Here m >= b_j is false as well: digit 0, m stays 0.
// So a step never changes the sign, and both loops emit the same digit at every step.  Nothing in
// the argument bounds x: for |xs| > sum of the base the loop ends with the residual m > 0, exactly
// as the reference ends with xs != 0 and reports no error.  b_j = 0 is outside both the proof and
// the reference's intent (its two cases overlap at xs = 0): the library refuses such a base.
// A base element above (q - 1) / 2 is never reached, so an element too wide for L limbs may be
// given as 2^(64L) - 1 without changing a digit.
//
// The input is a Montgomery element: the core first multiplies by 1 (fromMont).  The digits leave
// as field elements, as SetInt64 makes them: 0, R mod q or q - (R mod q); a lane picks
// c = s ? q - R : R once, and each digit is c or 0.
//
// RG_HD: the same source is compiled for the host by tests/test_dcmp_host.py and compared there
// with the loop-by-loop restatement of the reference.
#pragma once
#include <stdint.h>

#include "field.hpp"

namespace rg {

// The sign-magnitude state of one coefficient.
template <int L>
struct Dcmp {
  uint64_t m[L];  // |xs|
  bool s;         // xs < 0
};

// x = plain(w), s = [x > q >> 1], m = s ? q - x : x
template <int L>
RG_HD void dcmp_init(Dcmp<L>& d, const uint64_t* w, const FieldParams<L>& F) {
  uint64_t one[L], x[L], t[L];
#pragma unroll
  for (int i = 0; i < L; ++i) one[i] = i == 0;
  f_mul<L>(x, w, one, F);
  uint32_t br = 0;
#pragma unroll
  for (int i = 0; i + 1 < L; ++i)  // (q >> 1) - x borrows iff x > q >> 1
    (void)subb((F.q[i] >> 1) | (F.q[i + 1] << 63), x[i], br);
  (void)subb(F.q[L - 1] >> 1, x[L - 1], br);
  d.s = br != 0;
  br = 0;
#pragma unroll
  for (int i = 0; i < L; ++i) t[i] = subb(F.q[i], x[i], br);
#pragma unroll
  for (int i = 0; i < L; ++i) d.m[i] = d.s ? t[i] : x[i];
}

// One step: returns [m >= b] and subtracts b if so.  The digit is then s ? -1 : +1, else 0.
template <int L>
RG_HD bool dcmp_step(Dcmp<L>& d, const uint64_t* b) {
  uint64_t t[L];
  uint32_t br = 0;
#pragma unroll
  for (int i = 0; i < L; ++i) t[i] = subb(d.m[i], b[i], br);
  const bool ge = br == 0;
#pragma unroll
  for (int i = 0; i < L; ++i) d.m[i] = ge ? t[i] : d.m[i];
  return ge;
}

// The nonzero digit of this coefficient as a field element: SetInt64(s ? -1 : +1)
template <int L>
RG_HD void dcmp_unit(uint64_t* c, const Dcmp<L>& d, const uint64_t* one, const uint64_t* neg_one) {
#pragma unroll
  for (int i = 0; i < L; ++i) c[i] = d.s ? neg_one[i] : one[i];
}

}  // namespace rg
