// san_eval_args.cpp -- a stand-alone host program over the argument checks of
// rg_poly_evaluate_batch[_dev] and rg_poly_evaluate_batch_scratch_bytes (csrc/poly_eval.hip), meant
// to be built with the host side under -fsanitize=address,undefined and run on the CPU.  Every call
// below returns before its first device call, so no GPU is needed; rg_buckler_powers_dev, which
// poly_eval.hip calls after its checks, is a stub here so that the rest of the library stays out.
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=all ringo-snark_amd/csrc/poly_eval.hip \
//       ringo-snark_amd/csrc/capi.hip ringo-snark_amd/csrc/knobs.hip tools/san_eval_args.cpp \
//       -fsanitize=address,undefined -o san_eval_args && ./san_eval_args
#include <cstdio>
#include <cstring>

#include "../include/ringo.h"

extern "C" rg_status rg_buckler_powers_dev(const rg_field*, const uint64_t*, size_t, uint64_t*, void*) {
  return RG_ERR_DEVICE;  // never reached: every call below fails its checks first
}

static int bad = 0;
#define EXPECT(expr, want, text)                                                                  \
  do {                                                                                            \
    const long long got_ = (long long)(expr);                                                     \
    if (got_ != (long long)(want) || (text && !strstr(rg_last_error(), text))) {                  \
      std::printf("%s: got %lld \"%s\", want %lld \"%s\"\n", #expr, got_, rg_last_error(), (long long)(want), \
                  text ? text : "");                                                              \
      ++bad;                                                                                      \
    }                                                                                             \
  } while (0)

int main() {
  const uint64_t q1[1] = {0x7fffffffffffffe7ull};  // any odd word: the checks read the limb count alone
  const uint64_t q3[3] = {5, 0, 4};
  rg_field *f = nullptr, *g = nullptr;
  EXPECT(rg_field_create(1, q1, &f), RG_OK, nullptr);
  EXPECT(rg_field_create(3, q3, &g), RG_OK, nullptr);
  uint64_t* const A = (uint64_t*)0x10000;  // made-up device addresses: a call that read them would crash
  uint64_t* const B = (uint64_t*)0x20000;
  uint64_t* const C = (uint64_t*)0x30000;
  void* const D = (void*)0x40000;
  uint64_t h[8] = {1, 2, 3, 4, 5, 6, 7, 8}, o[8];
  EXPECT(rg_poly_evaluate_batch_dev(nullptr, A, 4, 4, 1, B, C, D, nullptr), RG_ERR_INVALID, "NULL field");
  EXPECT(rg_poly_evaluate_batch(nullptr, h, 4, 4, 1, h, o), RG_ERR_INVALID, "NULL field");
  EXPECT(rg_poly_evaluate_batch_dev(g, A, 4, 4, 1, B, C, D, nullptr), RG_ERR_UNSUPPORTED, "3 limbs");
  EXPECT(rg_poly_evaluate_batch(g, h, 1, 1, 1, h, o), RG_ERR_UNSUPPORTED, "3 limbs");
  EXPECT(rg_poly_evaluate_batch_dev(f, A, 5, 4, 1, B, C, D, nullptr), RG_ERR_INVALID, "stride 4 < n 5");
  EXPECT(rg_poly_evaluate_batch(f, h, 5, 4, 1, h, o), RG_ERR_INVALID, "stride 4 < n 5");
  EXPECT(rg_poly_evaluate_batch_dev(f, nullptr, 4, 4, 1, B, C, D, nullptr), RG_ERR_INVALID, "NULL buffer");
  EXPECT(rg_poly_evaluate_batch_dev(f, A, 4, 4, 1, nullptr, C, D, nullptr), RG_ERR_INVALID, "NULL buffer");
  EXPECT(rg_poly_evaluate_batch_dev(f, A, 4, 4, 1, B, nullptr, D, nullptr), RG_ERR_INVALID, "NULL buffer");
  EXPECT(rg_poly_evaluate_batch_dev(f, A, 4, 4, 1, B, C, nullptr, nullptr), RG_ERR_INVALID, "NULL scratch");
  EXPECT(rg_poly_evaluate_batch(f, nullptr, 4, 4, 1, h, o), RG_ERR_INVALID, "NULL buffer");
  EXPECT(rg_poly_evaluate_batch_dev(f, A, 4, (size_t)1 << 41, 1, B, C, D, nullptr), RG_ERR_INVALID, "out of range");
  EXPECT(rg_poly_evaluate_batch_dev(f, A, 4, (size_t)1 << 30, (size_t)1 << 21, B, C, D, nullptr), RG_ERR_INVALID,
         "out of range");
  EXPECT(rg_poly_evaluate_batch_dev(f, A, (size_t)1 << 40, (size_t)1 << 40, 16, B, C, D, nullptr), RG_ERR_INVALID,
         "out of range");  // 2^28 tiles x 16 polynomials: past a 1-D grid
  EXPECT(rg_poly_evaluate_batch_dev(f, A, 4, 4, 0, B, C, D, nullptr), RG_OK, nullptr);
  EXPECT(rg_poly_evaluate_batch(f, nullptr, 4, 4, 0, nullptr, nullptr), RG_OK, nullptr);
  EXPECT(rg_poly_evaluate_batch_scratch_bytes(nullptr, 4, 1), 0, nullptr);
  size_t prev = 0;
  for (size_t n : {(size_t)0, (size_t)1, (size_t)4095, (size_t)4096, (size_t)4097, (size_t)1 << 16}) {
    const size_t s = rg_poly_evaluate_batch_scratch_bytes(f, n, 3);
    if (s < prev || (n && !s)) {
      std::printf("scratch bytes not monotone at n = %zu\n", n);
      ++bad;
    }
    prev = s;
  }
  rg_field_destroy(f);
  rg_field_destroy(g);
  if (bad) return 1;
  std::printf("eval args ok\n");
  return 0;
}
