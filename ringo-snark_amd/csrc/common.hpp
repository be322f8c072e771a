// common.hpp -- shared host-side plumbing of libringo: status codes, HIP error capture,
// device buffers, the launch and field-check helpers of every unit (grid256, elem, is_pow2,
// same_field, dispatch_limbs / limbs_supported), and the opaque handle definitions behind
// include/ringo.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/ringo.h"
#include "field.hpp"

namespace rg {

void set_last_error(const std::string& msg);

// Measurement / A-B switches.  libringo.so links knobs.hip, where every knob is unset (nullptr:
// the production choice) and the probe is 0.  Only the experiments build, libringo_exp.so
// (tools/experiments/knobs_env.hip), reads them from the RINGO_* environment and honours
// rg_set_probe; the production library has no environment access at all.  The two NTT knobs are
// read when a plan is created (ntt.hip finalize()) and hold for the plan's life; the probe is read
// by every call.
enum class Knob : int {
  NttKernel,   // RINGO_NTT_KERNEL   r*: generic single-word / q255 pass kernels; stage: wide fields per stage;
               //                    w3: wide fields in three passes from 2^3 up (ntt_route.hpp ntt_wide_long)
  NttChunkMb,  // RINGO_NTT_CHUNK_MB polys per pass pair bounded to this many MiB
  JindoMac,    // RINGO_JINDO_MAC    l: mac_kernel instead of the MFMA MAC
  JindoSplit,  // RINGO_JINDO_SPLIT  0: commit_sampled on the caller's stream only
  JindoUniTries,  // RINGO_JINDO_UNI_TRIES n: uniform_whole_kernel gives up after n tries (tests the fix-up path)
  JindoCdtPath,   // RINGO_JINDO_CDT_PATH exact: cdt2_noise_kernel's exact path for every sample; sum: and its
                  //                      exact sum for every v0 != v1 tail (tests the paths draws never reach)
  XofLayout,      // RINGO_XOF_LAYOUT     lane: the SHAKE128 sponges one state per lane (xof.hip), read when a
                  //                      handle is created
  Count
};
const char* knob(Knob k);
// rg_set_probe's value on the calling thread (always 0 in libringo.so)
int measure_probe();

#define RG_HIP(call)                                                                            \
  do {                                                                                          \
    hipError_t e_ = (call);                                                                     \
    if (e_ != hipSuccess) {                                                                     \
      ::rg::set_last_error(std::string(#call) + ": " + hipGetErrorString(e_) + " @" + __FILE__ + \
                           ":" + std::to_string(__LINE__));                                     \
      return RG_ERR_DEVICE;                                                                     \
    }                                                                                           \
  } while (0)

#define RG_TRY(expr)          \
  do {                        \
    rg_status s_ = (expr);    \
    if (s_ != RG_OK) return s_; \
  } while (0)

inline rg_status check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_last_error(std::string("launch ") + what + ": " + hipGetErrorString(e));
    return RG_ERR_DEVICE;
  }
  return RG_OK;
}

// RAII device buffer
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  rg_status alloc(size_t n) {
    if (p && bytes >= n) return RG_OK;
    if (p) {
      (void)hipFree(p);
      p = nullptr;
      bytes = 0;
    }
    if (n == 0) return RG_OK;
    hipError_t e = hipMalloc(&p, n);
    if (e != hipSuccess) {
      set_last_error(std::string("hipMalloc ") + std::to_string(n) + ": " + hipGetErrorString(e));
      p = nullptr;
      return RG_ERR_NOMEM;
    }
    bytes = n;
    return RG_OK;
  }
  rg_status upload(const void* src, size_t n) {
    RG_TRY(alloc(n));
    RG_HIP(hipMemcpy(p, src, n, hipMemcpyHostToDevice));
    return RG_OK;
  }
  rg_status download(void* dst, size_t n) const {  // the buffer's first n bytes (a blocking copy)
    RG_HIP(hipMemcpy(dst, p, n, hipMemcpyDeviceToHost));
    return RG_OK;
  }
  template <class T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
};

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// blocks of 256 lanes that cover n items
inline unsigned grid256(long long n) { return (unsigned)((n + 255) / 256); }

inline bool is_pow2(long long n) { return n > 0 && (n & (n - 1)) == 0; }

// an element of L words as a kernel argument
template <int L>
inline Elem<L> elem(const uint64_t* x) {
  Elem<L> e;
  el_copy<L>(e.v, x);
  return e;
}

// Compile-time loop: f(std::integral_constant<int, i>) for i in [0, N), so a body indexes its
// register arrays with constants (a rolled loop the unroller leaves alone indexes them dynamically)
template <class F, int... I>
__host__ __device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__host__ __device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// Division of a 32-bit index by a launch-constant divisor through the double unit: q = floor(n / d)
// as trunc((n + 1/2) / d); (n + 1/2) / d keeps 1 / (2 d) from both neighbouring integers, far more
// than the few-ulp error of one fma on n < 2^32.  3 VALU against ~100 for a 64-bit integer division.
struct IdxDiv {
  uint32_t d;
  double inv, half_inv;  // 1 / d and (1 / d) / 2
};
inline IdxDiv make_idxdiv(uint32_t d) {
  IdxDiv f;
  f.d = d;
  f.inv = 1.0 / (double)d;
  f.half_inv = 0.5 * f.inv;
  return f;
}
__host__ __device__ __forceinline__ uint32_t idx_div(uint32_t n, const IdxDiv& f) {
  return (uint32_t)fma((double)n, f.inv, f.half_inv);
}

}  // namespace rg

// ------------------------------------------------------------------------------------------
// handle definitions
// ------------------------------------------------------------------------------------------
struct rg_field {
  int L;
  uint64_t q[16];
  uint64_t qinv;
  uint64_t r2[16];
  uint64_t one[16];
  bool spare_bit;  // q < 2^(64L-1)
};

namespace rg {

// the kernel-argument form of a field handle
template <int L>
inline FieldParams<L> field_params(const rg_field* f) {
  FieldParams<L> F;
  memcpy(F.q, f->q, 8 * L);
  F.qinv = f->qinv;
  return F;
}

// The one switch on a field's limb count: f(std::integral_constant<int, L>) for the five counts
// the kernels are instantiated for, e.g.
//   dispatch_limbs(f->L, [&](auto Lc) { return vec_L<Lc()>(f, ...); });
template <class F>
inline rg_status dispatch_limbs(int L, F&& f) {
  switch (L) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 7: return f(std::integral_constant<int, 7>{});
    case 14: return f(std::integral_constant<int, 14>{});
    default: return RG_ERR_UNSUPPORTED;
  }
}
// "is this limb count built?", read off that switch
inline bool limbs_supported(int L) {
  return dispatch_limbs(L, [](auto) { return RG_OK; }) == RG_OK;
}

inline bool same_field(const rg_field* a, const rg_field* b) {
  return a->L == b->L && memcmp(a->q, b->q, 8 * a->L) == 0;
}

}  // namespace rg
