// keccak.hpp -- Keccak-f[1600] and the SHAKE128 sponge's index algebra (FIPS 202), shared by the
// kernels of xof.hip and by the host checks.
//
// Lane (x, y) of the state is word x + 5 y; a stream position p of the rate is byte p % 8 of word
// p / 8 (little-endian lanes, as golang.org/x/crypto/sha3 and hashlib hold them).  SHAKE128: rate 168
// bytes (21 words), domain byte 0x1F at the position the message ends on, final bit 0x80 in byte 167;
// the two fall on one byte (0x9F) when that position is 167.
//
// RG_HD: the same source is compiled for the host by tests/test_keccak_host.py (the stand-alone
// program tools/san_keccak.cpp, run under the address and undefined-behaviour sanitizers) and checked
// there against hashlib.shake_128.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#ifndef RG_HD
#define RG_HD __host__ __device__ __forceinline__
#endif
#else
#ifndef RG_HD
#define RG_HD inline
#endif
#endif

namespace rg {
namespace keccak {

constexpr int kWords = 25;
constexpr int kRounds = 24;
constexpr int kRate = 168;           // SHAKE128: 1600 / 8 - 2 * 128 / 8
constexpr int kRateWords = kRate / 8;
constexpr uint8_t kDomain = 0x1F;    // SHAKE's 1111 suffix and the first padding bit
constexpr uint8_t kFinalBit = 0x80;  // the last padding bit, in byte kRate - 1

// iota's round constants
RG_HD uint64_t round_constant(int r) {
  constexpr uint64_t rc[kRounds] = {
      0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull,
      0x000000000000808bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
      0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
      0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull,
      0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
      0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
  return rc[r];
}

// rho: the left rotation of word i = x + 5 y
RG_HD int rho_offset(int i) {
  constexpr uint8_t rho[kWords] = {0,  1,  62, 28, 27, 36, 44, 6,  55, 20, 3,  10, 43,
                                   25, 39, 41, 45, 15, 21, 8,  18, 2,  61, 56, 14};
  return rho[i];
}

// pi: word i = x + 5 y moves to (y, 2 x + 3 y); pi_source is the inverse, the word that lands on i
RG_HD int pi_dest(int i) {
  const int x = i % 5, y = i / 5;
  return y + 5 * ((2 * x + 3 * y) % 5);
}
RG_HD int pi_source(int i) {
  const int x = i % 5, y = i / 5;
  return (x + 3 * y) % 5 + 5 * x;
}

RG_HD uint64_t rotl64(uint64_t v, int n) { return n ? (v << n) | (v >> (64 - n)) : v; }

// One round on 25 words held by one thread.  Fully unrolled, so every index is a constant.
RG_HD void round1600(uint64_t* a, uint64_t rc) {
  uint64_t c[5], b[kWords];
#pragma unroll
  for (int x = 0; x < 5; ++x) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
  for (int x = 0; x < 5; ++x) {
    const uint64_t d = c[(x + 4) % 5] ^ rotl64(c[(x + 1) % 5], 1);
#pragma unroll
    for (int y = 0; y < 5; ++y) a[x + 5 * y] ^= d;
  }
#pragma unroll
  for (int i = 0; i < kWords; ++i) {
    b[pi_dest(i)] = rotl64(a[i], rho_offset(i));
  }
#pragma unroll
  for (int y = 0; y < 5; ++y) {
#pragma unroll
    for (int x = 0; x < 5; ++x) a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
  }
  a[0] ^= rc;
}

// Keccak-f[1600] on 25 words
RG_HD void f1600(uint64_t* a) {
  for (int r = 0; r < kRounds; ++r) round1600(a, round_constant(r));
}

// ---- the sponge's index algebra ------------------------------------------------------------------
// Position p of the rate: its word and the shift of its byte inside the word.
RG_HD int word_of(int p) { return p >> 3; }
RG_HD int shift_of(int p) { return (p & 7) * 8; }

// The padding of a message that ends on position p (0 <= p < kRate): what to xor into word w.
RG_HD uint64_t pad_word(int p, int w) {
  uint64_t v = 0;
  if (w == word_of(p)) v ^= (uint64_t)kDomain << shift_of(p);
  if (w == kRateWords - 1) v ^= (uint64_t)kFinalBit << 56;
  return v;
}

// A run of `len` bytes that starts on position `pos` (0 <= pos < kRate while absorbing, 0 <= pos <=
// kRate while squeezing) of the current block:
//   blocks it touches, full_blocks of them completed by it (each followed by a permutation while
//   absorbing), and the position it leaves behind.
struct Run {
  size_t blocks, full_blocks;
  int end_pos;
};
RG_HD Run split_run(int pos, size_t len) {
  Run r;
  const size_t end = (size_t)pos + len;
  r.full_blocks = end / kRate;
  r.end_pos = (int)(end % kRate);
  r.blocks = r.full_blocks + (r.end_pos != 0 ? 1 : 0);
  return r;
}
// Block b of such a run covers run bytes [lo, hi): lo = max(0, b kRate - pos), hi = min(len, (b + 1) kRate - pos)
RG_HD void block_range(int pos, size_t len, size_t b, size_t& lo, size_t& hi) {
  const size_t s = b * kRate;
  lo = s > (size_t)pos ? s - (size_t)pos : 0;
  const size_t e = s + kRate - (size_t)pos;
  hi = e < len ? e : len;
}
// Run byte m sits on position (pos + m) % kRate of block (pos + m) / kRate; word w of block b
// starts at run byte b kRate + 8 w - pos (negative before the run's start).
RG_HD long long word_start(int pos, size_t b, int w) { return (long long)(b * kRate) + 8 * w - pos; }

// ---- a plain one-state sponge over the above (host checks, and the model the kernels follow) -----
struct Sponge {
  uint64_t a[kWords];
  int pos;         // absorbing: the position the message ends on; squeezing: bytes of the block read
  bool squeezing;
};
RG_HD void sponge_reset(Sponge& s) {
  for (int i = 0; i < kWords; ++i) s.a[i] = 0;
  s.pos = 0;
  s.squeezing = false;
}
// false: absorbing after a squeeze (the reference panics)
RG_HD bool sponge_absorb(Sponge& s, const uint8_t* p, size_t len) {
  if (s.squeezing) return false;
  const Run r = split_run(s.pos, len);
  for (size_t b = 0; b < r.blocks; ++b) {
    size_t lo, hi;
    block_range(s.pos, len, b, lo, hi);
    for (size_t m = lo; m < hi; ++m) {
      const int q = (int)(((size_t)s.pos + m) % kRate);
      s.a[word_of(q)] ^= (uint64_t)p[m] << shift_of(q);
    }
    if (b < r.full_blocks) f1600(s.a);
  }
  s.pos = r.end_pos;
  return true;
}
RG_HD void sponge_squeeze(Sponge& s, uint8_t* out, size_t len) {
  if (!s.squeezing) {
    for (int w = 0; w < kRateWords; ++w) s.a[w] ^= pad_word(s.pos, w);
    s.pos = kRate;  // nothing of a block to read yet: the first byte permutes
    s.squeezing = true;
  }
  for (size_t m = 0; m < len; ++m) {
    if (s.pos == kRate) {
      f1600(s.a);
      s.pos = 0;
    }
    out[m] = (uint8_t)(s.a[word_of(s.pos)] >> shift_of(s.pos));
    ++s.pos;
  }
}

}  // namespace keccak
}  // namespace rg
