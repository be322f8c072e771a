// chal_digits.hpp -- the digits of encodeChallengeTo (jindo/utils.go:20-46): the 16 challenge bytes
// as a 128-bit value, exp successive remainders by ChallengeBound (divMod64, utils.go:12-18).
// bound < 2^31, so each division of the 128-bit value is four 32-bit long-division steps.
//
// RG_HD: the same source is compiled for the host by tests/test_chal_digits_host.py (a stand-alone
// program, run under the address and undefined-behaviour sanitizers) and checked there against
// 128-bit integer division.
#pragma once
#include <stdint.h>

#include "digits_dc.hpp"

namespace rg {

// Parameters.ChallengeBound (params.go:357-360): min(base, 1 << (120 / exp)) / 2 in uint64, where
// Go's shift by 64 or more gives 0; exp >= 1.  0 is the reference's division by zero.
inline uint64_t challenge_bound(uint64_t base, int exp) {
  const int sh = 120 / exp;
  const uint64_t pw = sh >= 64 ? 0 : 1ull << sh;
  return (base < pw ? base : pw) / 2;
}

// put(i, r, neg) for i < exp: r the i-th remainder, neg when r > bound / 2 (the coefficient is then
// q_l - (bound - r), utils.go:32-36).  bytes: two big-endian words, the first the low word of
// divMod64's little-endian pair.  bound >= 2, bound_inv = floor(2^64 / bound).
template <class Put>
RG_HD void chal_digits(const uint8_t* bytes, uint64_t bound, uint64_t bound_inv, int exp, Put put) {
  uint64_t c0 = 0, c1 = 0;
  for (int i = 0; i < 8; ++i) {
    c0 = (c0 << 8) | bytes[i];
    c1 = (c1 << 8) | bytes[8 + i];
  }
  uint32_t w3 = (uint32_t)(c1 >> 32), w2 = (uint32_t)c1, w1 = (uint32_t)(c0 >> 32), w0 = (uint32_t)c0;
  for (int i = 0; i < exp; ++i) {
    uint64_t r = 0;
    w3 = divstep((r << 32) | w3, bound, bound_inv, r);
    w2 = divstep((r << 32) | w2, bound, bound_inv, r);
    w1 = divstep((r << 32) | w1, bound, bound_inv, r);
    w0 = divstep((r << 32) | w0, bound, bound_inv, r);
    put(i, r, r > bound / 2);
  }
}

}  // namespace rg
