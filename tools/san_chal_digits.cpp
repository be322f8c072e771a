// san_chal_digits.cpp -- a stand-alone host program over csrc/chal_digits.hpp, the digit routine of
// rg_jindo_encode_challenges_dev, meant to be built with -fsanitize=address,undefined and run on the
// CPU (tests/test_chal_digits_host.py does both): every ChallengeBound the parameter sets give and the
// extremes of the routine's range, on all-zero, all-one, boundary and pseudo-random 128-bit values,
// against 128-bit integer division; and ChallengeBound itself against its definition.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I ringo-snark_amd/csrc tools/san_chal_digits.cpp -o san_chal_digits && ./san_chal_digits
#include <cstdio>
#include <cstring>
#include <vector>

#include "chal_digits.hpp"

typedef unsigned __int128 u128;

static int check(u128 v, uint64_t bound, int exp) {
  uint8_t b[16];
  const uint64_t lo = (uint64_t)v, hi = (uint64_t)(v >> 64);
  for (int i = 0; i < 8; ++i) {
    b[i] = (uint8_t)(lo >> (56 - 8 * i));
    b[8 + i] = (uint8_t)(hi >> (56 - 8 * i));
  }
  std::vector<uint64_t> got(exp, ~0ull);
  std::vector<int> neg(exp, -1);
  const uint64_t inv = (uint64_t)(((u128)1 << 64) / bound);
  rg::chal_digits(b, bound, inv, exp, [&](int i, uint64_t r, bool n) {
    got[i] = r;
    neg[i] = n;
  });
  for (int i = 0; i < exp; ++i) {
    const uint64_t r = (uint64_t)(v % bound);
    v /= bound;
    if (got[i] != r || neg[i] != (r > bound / 2)) {
      std::printf("bound %llu digit %d: got %llu (neg %d), want %llu\n", (unsigned long long)bound, i,
                  (unsigned long long)got[i], neg[i], (unsigned long long)r);
      return 1;
    }
  }
  return 0;
}

int main() {
  int bad = 0;
  // ChallengeBound: (base, exp) -> min(base, 2^(120 / exp)) / 2, 0 where the reference divides by zero
  const struct {
    uint64_t base;
    int exp;
    uint64_t want;
  } cb[] = {{60272, 16, 64}, {60256, 8, 16384}, {47104, 4, 23552}, {13694, 64, 1}, {13512, 32, 4}, {7000, 5, 3500},
            {60272, 120, 1}, {60272, 121, 0}, {60272, 100000, 0}, {60272, 1, 0}, {60272, 2, 30136}, {3, 2, 1},
            {0xffffffffull, 3, 0x7fffffffull}};
  for (const auto& c : cb)
    if (rg::challenge_bound(c.base, c.exp) != c.want) {
      std::printf("challenge_bound(%llu, %d) = %llu, want %llu\n", (unsigned long long)c.base, c.exp,
                  (unsigned long long)rg::challenge_bound(c.base, c.exp), (unsigned long long)c.want);
      ++bad;
    }
  const uint64_t bounds[] = {2, 3, 4, 5, 64, 3500, 3501, 16384, 23552, 35000, 0x7fffffffull, 0x7ffffffeull, 0x40000000ull};
  const int exps[] = {1, 2, 4, 5, 8, 16, 32, 64, 120};
  uint64_t s = 0x9e3779b97f4a7c15ull;
  auto next = [&]() {  // xorshift64*
    s ^= s >> 12;
    s ^= s << 25;
    s ^= s >> 27;
    return s * 0x2545f4914f6cdd1dull;
  };
  for (uint64_t bound : bounds)
    for (int exp : exps) {
      bad += check(0, bound, exp);
      bad += check(~(u128)0, bound, exp);
      bad += check((u128)1 << 127, bound, exp);
      bad += check(((u128)1 << 64) - 1, bound, exp);
      bad += check((u128)1 << 64, bound, exp);
      // every digit at 0, bound/2, bound/2 + 1, bound - 1 in turn (while the value fits 128 bits)
      const uint64_t edge[4] = {0, bound / 2, bound / 2 + 1 < bound ? bound / 2 + 1 : bound - 1, bound - 1};
      for (int rot = 0; rot < 4; ++rot) {
        u128 v = 0, pw = 1;
        for (int i = 0; i < exp; ++i) {
          if (pw > (~(u128)0) / bound) break;
          v += pw * edge[(i + rot) & 3];
          pw *= bound;
        }
        bad += check(v, bound, exp);
      }
      for (int k = 0; k < 200; ++k) bad += check(((u128)next() << 64) | next(), bound, exp);
    }
  if (bad) {
    std::printf("%d mismatches\n", bad);
    return 1;
  }
  std::printf("chal_digits ok\n");
  return 0;
}
