// xof.hip -- SHAKE128 sponges on the device for the Jindo transcript (jindo/prover.go:220-302,
// verifier.go:56-96) and the projection XOF (buckler/prover.go:165-176).
//
// n_states sponges move in lockstep: every state absorbs and squeezes the same number of bytes in
// every call, so the position in the block and the phase are host-side facts of the handle and only
// the [n_states][25] words live on the device.  The work is a serial chain per state (one
// Keccak-f[1600] per 168 bytes) over few states, so the kernels are written for latency per
// permutation:
//
//   cooperative (the product)   one state per 32-lane half-wave, lane i < 25 holding word i = x + 5 y.
//       theta is four independent cross-lane reads down the column and two along the row, pi one
//       read, chi two; rho is a per-lane variable rotate: 18 ds_bpermute_b32 and 25 VALU on a
//       round's chain, and each lane of the rate loads (stores) its own word of a block.
//   lane per state (libringo_exp.so, RINGO_XOF_LAYOUT=lane)   keccak.hpp's scalar permutation, 25
//       words in one lane's registers, no cross-lane traffic, 288 VALU a round on the chain.
// Measured: 6.0-6.8 us against 14.4-15.1 us per permutation, at 1 and at 64 states.
//
// Both walk the same wave-uniform segment list and load the next block's words before the current
// block's rounds, so the global-memory round trip is off the chain.  A word whose eight bytes lie in
// one segment is read as one aligned uint64 (or two, funnel-shifted, when the source is not 8-byte
// aligned: both words hold bytes of the segment); the words at a segment's ends are gathered bytewise.
#include <new>

#include "common.hpp"
#include "keccak.hpp"

namespace rg {
namespace kk = keccak;

constexpr size_t kXofMaxSegs = 65536;

// a segment of a message as the kernels read it; start = bytes of the message before it
struct XofSeg {
  unsigned long long offset, stride, len, start;
  int base;  // RG_XOF_LITERAL or an index into the call's bases
  int pad_;
};

// where a call's bytes are: a device list of segments, or the single segment `one`
struct XofSrc {
  const XofSeg* segs;  // nullptr: `one`
  unsigned n_segs;
  XofSeg one;
  const uint8_t* bases[RG_XOF_MAX_BASES + 1];  // [0] the literal blob, [1 + b] base b
};

struct XofAbsorbArgs {
  uint64_t* lanes;
  size_t n_states;
  int pos;       // position of the block the run starts on
  size_t total;  // bytes of the run
  XofSrc src;
};

struct XofSqueezeArgs {
  uint64_t* lanes;
  size_t n_states;
  uint8_t* out;
  size_t out_stride, len;
  int pad_pos;  // >= 0: the message ended on this position and is not padded yet
  int pos;      // bytes of the current block already read (kRate: none left)
};

__device__ __forceinline__ XofSeg seg_at(const XofSrc& S, unsigned i) { return S.segs ? S.segs[i] : S.one; }

// The word made of bytes [m0, m0 + 8) of the `len` bytes at src, little-endian; bytes outside [0, len)
// read as 0 and are not touched.
__device__ __forceinline__ uint64_t gather_word(const uint8_t* src, long long m0, long long len) {
  if (m0 <= -8 || m0 >= len) return 0;
  if (m0 >= 0 && m0 + 8 <= len) {
    const uintptr_t a = (uintptr_t)(src + m0);
    const unsigned sh = (unsigned)(a & 7) * 8;
    const uint64_t* w = reinterpret_cast<const uint64_t*>(a & ~(uintptr_t)7);
    const uint64_t lo = w[0];
    if (sh == 0) return lo;
    return (lo >> sh) | (w[1] << (64 - sh));  // w[1] holds byte m0 + 7
  }
  uint64_t v = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const long long m = m0 + k;
    if (m >= 0 && m < len) v |= (uint64_t)src[m] << (8 * k);
  }
  return v;
}

// Bytes [j0, j0 + 8) of the output take word v where they fall inside [lo, hi)
__device__ __forceinline__ void scatter_word(uint8_t* out, long long j0, long long lo, long long hi, uint64_t v) {
  if (j0 + 8 <= lo || j0 >= hi) return;
  if (j0 >= lo && j0 + 8 <= hi && ((uintptr_t)(out + j0) & 7) == 0) {
    *reinterpret_cast<uint64_t*>(out + j0) = v;
    return;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const long long j = j0 + k;
    if (j >= lo && j < hi) out[j] = (uint8_t)(v >> (8 * k));
  }
}

// Words w0 .. w0 + NW - 1 of block b of the run, for one state.  `first` is the first segment that can
// reach the block and only moves forward; every trip count depends on the run alone, so the walk is
// the same in every lane, and only `live` lanes read memory.
template <int NW>
__device__ __forceinline__ void block_words(const XofSrc& S, unsigned& first, int pos, size_t total, size_t b,
                                            size_t state, int w0, bool live, uint64_t (&out)[NW]) {
  size_t lo, hi;
  kk::block_range(pos, total, b, lo, hi);
#pragma unroll
  for (int i = 0; i < NW; ++i) out[i] = 0;
  unsigned si = first;
  while (si < S.n_segs) {
    const XofSeg g = seg_at(S, si);
    if (g.start + g.len > lo) break;
    ++si;
  }
  first = si;
  for (unsigned j = si; j < S.n_segs; ++j) {
    const XofSeg g = seg_at(S, j);
    if (g.start >= hi) break;
    if (g.len == 0 || !live) continue;
    const uint8_t* src = S.bases[g.base + 1] + g.offset + (g.base >= 0 ? state * g.stride : 0);
#pragma unroll
    for (int i = 0; i < NW; ++i)
      out[i] ^= gather_word(src, kk::word_start(pos, b, w0 + i) - (long long)g.start, (long long)g.len);
  }
}

// ---- cooperative layout ---------------------------------------------------------------------------
// byte addresses (lane * 4) of the lanes a lane reads in a round, and its rho rotation
struct CoopIdx {
  int y1, y2, y3, y4;  // the other four words of the column
  int xm1, xp1, xp2;   // the row's words x - 1, x + 1, x + 2
  int pi;              // the word that pi moves here
  int rho;
};

__device__ __forceinline__ CoopIdx coop_idx(int lane, int half_base) {
  CoopIdx ix;
  const auto addr = [&](int l) { return (l + half_base) * 4; };
  if (lane < kk::kWords) {
    const int x = lane % 5, row = lane - x;
    ix.y1 = addr((lane + 5) % 25);
    ix.y2 = addr((lane + 10) % 25);
    ix.y3 = addr((lane + 15) % 25);
    ix.y4 = addr((lane + 20) % 25);
    ix.xm1 = addr(row + (x + 4) % 5);
    ix.xp1 = addr(row + (x + 1) % 5);
    ix.xp2 = addr(row + (x + 2) % 5);
    ix.pi = addr(kk::pi_source(lane));
    ix.rho = kk::rho_offset(lane);
  } else {  // the seven idle lanes of a half read themselves
    ix.y1 = ix.y2 = ix.y3 = ix.y4 = ix.xm1 = ix.xp1 = ix.xp2 = ix.pi = addr(lane);
    ix.rho = 0;
  }
  return ix;
}

__device__ __forceinline__ uint64_t lane_read(int addr, uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)(uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t coop_f1600(uint64_t a, const CoopIdx& ix, bool word0) {
  for (int r = 0; r < kk::kRounds; ++r) {
    // theta
    const uint64_t p = a ^ lane_read(ix.y1, a) ^ lane_read(ix.y2, a) ^ lane_read(ix.y3, a) ^ lane_read(ix.y4, a);
    const uint64_t right = lane_read(ix.xp1, p);
    a ^= lane_read(ix.xm1, p) ^ ((right << 1) | (right >> 63));
    // rho, pi
    const uint64_t t = (a << ix.rho) | (a >> ((64 - ix.rho) & 63));
    const uint64_t b = lane_read(ix.pi, t);
    // chi, iota
    a = b ^ (~lane_read(ix.xp1, b) & lane_read(ix.xp2, b));
    if (word0) a ^= kk::round_constant(r);
  }
  return a;
}

struct CoopLane {
  int lane;      // word of the state
  size_t state;
  bool have;     // a word of an existing state
  CoopIdx ix;
};
__device__ __forceinline__ CoopLane coop_lane(size_t n_states) {
  CoopLane c;
  c.lane = threadIdx.x & 31;
  c.state = (size_t)blockIdx.x * 2 + (threadIdx.x >> 5);
  c.have = c.state < n_states && c.lane < kk::kWords;
  c.ix = coop_idx(c.lane, threadIdx.x & 32);
  return c;
}

__global__ __launch_bounds__(64) void xof_absorb_coop_kernel(XofAbsorbArgs A) {
  const CoopLane c = coop_lane(A.n_states);
  const bool live = c.have && c.lane < kk::kRateWords;
  uint64_t a = c.have ? A.lanes[c.state * kk::kWords + c.lane] : 0;
  const kk::Run run = kk::split_run(A.pos, A.total);
  unsigned first = 0;
  uint64_t w[1], nx[1];
  block_words<1>(A.src, first, A.pos, A.total, 0, c.state, c.lane, live, w);
  for (size_t b = 0; b < run.blocks; ++b) {
    nx[0] = 0;
    if (b + 1 < run.blocks) block_words<1>(A.src, first, A.pos, A.total, b + 1, c.state, c.lane, live, nx);
    a ^= w[0];
    if (b < run.full_blocks) a = coop_f1600(a, c.ix, c.lane == 0);
    w[0] = nx[0];
  }
  if (c.have) A.lanes[c.state * kk::kWords + c.lane] = a;
}

__global__ __launch_bounds__(64) void xof_squeeze_coop_kernel(XofSqueezeArgs A) {
  const CoopLane c = coop_lane(A.n_states);
  const bool live = c.have && c.lane < kk::kRateWords;
  uint64_t a = c.have ? A.lanes[c.state * kk::kWords + c.lane] : 0;
  if (A.pad_pos >= 0 && live) a ^= kk::pad_word(A.pad_pos, c.lane);
  uint8_t* out = A.out + c.state * A.out_stride;
  int pos = A.pos;
  for (size_t m = 0; m < A.len;) {
    if (pos == kk::kRate) {
      a = coop_f1600(a, c.ix, c.lane == 0);
      pos = 0;
    }
    const size_t left = A.len - m;
    const size_t n = left < (size_t)(kk::kRate - pos) ? left : (size_t)(kk::kRate - pos);
    if (live) scatter_word(out, (long long)m - pos + 8 * c.lane, (long long)m, (long long)(m + n), a);
    m += n;
    pos += (int)n;
  }
  if (c.have) A.lanes[c.state * kk::kWords + c.lane] = a;
}

// ---- lane per state (the experiments build's alternative) ------------------------------------------
__global__ __launch_bounds__(64) void xof_absorb_lane_kernel(XofAbsorbArgs A) {
  const size_t state = (size_t)blockIdx.x * 64 + threadIdx.x;
  const bool live = state < A.n_states;
  uint64_t a[kk::kWords];
#pragma unroll
  for (int i = 0; i < kk::kWords; ++i) a[i] = live ? A.lanes[state * kk::kWords + i] : 0;
  const kk::Run run = kk::split_run(A.pos, A.total);
  unsigned first = 0;
  uint64_t w[kk::kRateWords], nx[kk::kRateWords];
  block_words<kk::kRateWords>(A.src, first, A.pos, A.total, 0, state, 0, live, w);
  for (size_t b = 0; b < run.blocks; ++b) {
#pragma unroll
    for (int i = 0; i < kk::kRateWords; ++i) nx[i] = 0;
    if (b + 1 < run.blocks) block_words<kk::kRateWords>(A.src, first, A.pos, A.total, b + 1, state, 0, live, nx);
#pragma unroll
    for (int i = 0; i < kk::kRateWords; ++i) a[i] ^= w[i];
    if (b < run.full_blocks) kk::f1600(a);
#pragma unroll
    for (int i = 0; i < kk::kRateWords; ++i) w[i] = nx[i];
  }
  if (live) {
#pragma unroll
    for (int i = 0; i < kk::kWords; ++i) A.lanes[state * kk::kWords + i] = a[i];
  }
}

__global__ __launch_bounds__(64) void xof_squeeze_lane_kernel(XofSqueezeArgs A) {
  const size_t state = (size_t)blockIdx.x * 64 + threadIdx.x;
  const bool live = state < A.n_states;
  uint64_t a[kk::kWords];
#pragma unroll
  for (int i = 0; i < kk::kWords; ++i) a[i] = live ? A.lanes[state * kk::kWords + i] : 0;
  if (A.pad_pos >= 0) {
#pragma unroll
    for (int i = 0; i < kk::kRateWords; ++i) a[i] ^= kk::pad_word(A.pad_pos, i);
  }
  uint8_t* out = A.out + state * A.out_stride;
  int pos = A.pos;
  for (size_t m = 0; m < A.len;) {
    if (pos == kk::kRate) {
      kk::f1600(a);
      pos = 0;
    }
    const size_t left = A.len - m;
    const size_t n = left < (size_t)(kk::kRate - pos) ? left : (size_t)(kk::kRate - pos);
    if (live) {
#pragma unroll
      for (int i = 0; i < kk::kRateWords; ++i)
        scatter_word(out, (long long)m - pos + 8 * i, (long long)m, (long long)(m + n), a[i]);
    }
    m += n;
    pos += (int)n;
  }
  if (live) {
#pragma unroll
    for (int i = 0; i < kk::kWords; ++i) A.lanes[state * kk::kWords + i] = a[i];
  }
}

static rg_status xof_invalid(const std::string& why) {
  set_last_error("xof: " + why);
  return RG_ERR_INVALID;
}

}  // namespace rg

struct rg_xof {
  size_t n_states = 0;
  uint64_t* d_lanes = nullptr;
  int pos = 0;           // absorbing: where the message ends; squeezing: bytes of the block read
  bool squeezing = false;
  int pad_pos = -1;      // squeezing, and the padding is still to be applied by the next launch
  bool lane_layout = false;
};

struct rg_xof_plan {
  rg::XofSeg* d_segs = nullptr;
  uint8_t* d_literals = nullptr;
  size_t n_segs = 0, total = 0;
  int max_base = -1;
};

using namespace rg;

static rg_status launch_absorb(rg_xof* x, const XofSrc& src, size_t total, hipStream_t st) {
  XofAbsorbArgs A;
  A.lanes = x->d_lanes;
  A.n_states = x->n_states;
  A.pos = x->pos;
  A.total = total;
  A.src = src;
  if (x->lane_layout)
    hipLaunchKernelGGL(xof_absorb_lane_kernel, dim3((unsigned)((x->n_states + 63) / 64)), dim3(64), 0, st, A);
  else
    hipLaunchKernelGGL(xof_absorb_coop_kernel, dim3((unsigned)((x->n_states + 1) / 2)), dim3(64), 0, st, A);
  RG_TRY(check_launch("xof_absorb"));
  x->pos = kk::split_run(x->pos, total).end_pos;
  return RG_OK;
}

extern "C" {

rg_status rg_xof_create(size_t n_states, rg_xof** out) {
  if (!out) return xof_invalid("NULL out");
  *out = nullptr;
  if (n_states == 0) return xof_invalid("n_states is 0");
  if (n_states > (1u << 30)) return xof_invalid("n_states above 2^30");
  rg_xof* x = new (std::nothrow) rg_xof();
  if (!x) return RG_ERR_NOMEM;
  x->n_states = n_states;
  const char* layout = knob(Knob::XofLayout);
  x->lane_layout = layout && layout[0] == 'l';
  const size_t bytes = n_states * kk::kWords * 8;
  hipError_t e = hipMalloc((void**)&x->d_lanes, bytes);
  if (e != hipSuccess) {
    set_last_error(std::string("xof: hipMalloc: ") + hipGetErrorString(e));
    delete x;
    return RG_ERR_NOMEM;
  }
  e = hipMemset(x->d_lanes, 0, bytes);
  if (e != hipSuccess) {
    set_last_error(std::string("xof: hipMemset: ") + hipGetErrorString(e));
    (void)hipFree(x->d_lanes);
    delete x;
    return RG_ERR_DEVICE;
  }
  *out = x;
  return RG_OK;
}

void rg_xof_destroy(rg_xof* x) {
  if (!x) return;
  if (x->d_lanes) (void)hipFree(x->d_lanes);
  delete x;
}

rg_status rg_xof_reset_dev(rg_xof* x, void* stream) {
  if (!x) return xof_invalid("NULL handle");
  RG_HIP(hipMemsetAsync(x->d_lanes, 0, x->n_states * kk::kWords * 8, as_stream(stream)));
  x->pos = 0;
  x->squeezing = false;
  x->pad_pos = -1;
  return RG_OK;
}

rg_status rg_xof_copy_dev(rg_xof* dst, const rg_xof* src, void* stream) {
  if (!dst || !src) return xof_invalid("NULL handle");
  if (dst->n_states != src->n_states) return xof_invalid("copy between handles of different n_states");
  if (dst == src) return RG_OK;
  RG_HIP(hipMemcpyAsync(dst->d_lanes, src->d_lanes, src->n_states * kk::kWords * 8, hipMemcpyDeviceToDevice,
                        as_stream(stream)));
  dst->pos = src->pos;
  dst->squeezing = src->squeezing;
  dst->pad_pos = src->pad_pos;
  return RG_OK;
}

rg_status rg_xof_absorb_dev(rg_xof* x, const uint8_t* d_bytes, size_t len, size_t state_stride, void* stream) {
  if (!x) return xof_invalid("NULL handle");
  if (x->squeezing) return xof_invalid("absorb after squeeze");
  if (len == 0) return RG_OK;
  if (!d_bytes) return xof_invalid("NULL d_bytes");
  XofSrc src;
  memset(&src, 0, sizeof(src));
  src.n_segs = 1;
  src.one.base = 0;
  src.one.stride = state_stride;
  src.one.len = len;
  src.bases[1] = d_bytes;
  return launch_absorb(x, src, len, as_stream(stream));
}

rg_status rg_xof_plan_create(const rg_xof_seg* segs, size_t n_segs, const uint8_t* literals, size_t literal_len,
                             rg_xof_plan** out) {
  if (!out) return xof_invalid("NULL out");
  *out = nullptr;
  if (n_segs && !segs) return xof_invalid("NULL segs");
  if (literal_len && !literals) return xof_invalid("NULL literals");
  if (n_segs > kXofMaxSegs) return xof_invalid("more than 65536 segments");
  std::vector<XofSeg> v(n_segs);
  size_t total = 0;
  int max_base = -1;
  for (size_t i = 0; i < n_segs; ++i) {
    const rg_xof_seg& s = segs[i];
    if (s.base < RG_XOF_LITERAL || s.base >= RG_XOF_MAX_BASES)
      return xof_invalid("segment " + std::to_string(i) + ": base " + std::to_string(s.base) + " out of range");
    if (s.base == RG_XOF_LITERAL && (s.offset > literal_len || s.len > literal_len - s.offset))
      return xof_invalid("segment " + std::to_string(i) + ": literal run past the blob");
    if (total + s.len < total) return xof_invalid("plan length overflows");
    v[i].offset = s.offset;
    v[i].stride = s.base == RG_XOF_LITERAL ? 0 : s.state_stride;
    v[i].len = s.len;
    v[i].start = total;
    v[i].base = s.base;
    v[i].pad_ = 0;
    total += s.len;
    if (s.len && s.base > max_base) max_base = s.base;
  }
  rg_xof_plan* p = new (std::nothrow) rg_xof_plan();
  if (!p) return RG_ERR_NOMEM;
  p->n_segs = n_segs;
  p->total = total;
  p->max_base = max_base;
  hipError_t e = hipSuccess;
  if (n_segs) e = hipMalloc((void**)&p->d_segs, n_segs * sizeof(XofSeg));
  if (e == hipSuccess && literal_len) e = hipMalloc((void**)&p->d_literals, literal_len);
  if (e != hipSuccess) {
    set_last_error(std::string("xof: hipMalloc: ") + hipGetErrorString(e));
    rg_xof_plan_destroy(p);
    return RG_ERR_NOMEM;
  }
  if (n_segs) e = hipMemcpy(p->d_segs, v.data(), n_segs * sizeof(XofSeg), hipMemcpyHostToDevice);
  if (e == hipSuccess && literal_len) e = hipMemcpy(p->d_literals, literals, literal_len, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    set_last_error(std::string("xof: hipMemcpy: ") + hipGetErrorString(e));
    rg_xof_plan_destroy(p);
    return RG_ERR_DEVICE;
  }
  *out = p;
  return RG_OK;
}

void rg_xof_plan_destroy(rg_xof_plan* p) {
  if (!p) return;
  if (p->d_segs) (void)hipFree(p->d_segs);
  if (p->d_literals) (void)hipFree(p->d_literals);
  delete p;
}

size_t rg_xof_plan_bytes(const rg_xof_plan* p) { return p ? p->total : 0; }

rg_status rg_xof_absorb_plan_dev(rg_xof* x, const rg_xof_plan* p, const void* const* d_bases, size_t n_bases,
                                 void* stream) {
  if (!x || !p) return xof_invalid("NULL handle");
  if (n_bases > RG_XOF_MAX_BASES) return xof_invalid("n_bases above RG_XOF_MAX_BASES");
  if (n_bases && !d_bases) return xof_invalid("NULL d_bases");
  if (p->max_base >= (int)n_bases)
    return xof_invalid("a segment's base " + std::to_string(p->max_base) + " is outside [-1, n_bases)");
  for (int b = 0; b <= p->max_base; ++b)
    if (!d_bases[b]) return xof_invalid("NULL base " + std::to_string(b));
  if (x->squeezing) return xof_invalid("absorb after squeeze");
  if (p->total == 0) return RG_OK;
  XofSrc src;
  memset(&src, 0, sizeof(src));
  src.segs = p->d_segs;
  src.n_segs = (unsigned)p->n_segs;
  src.bases[0] = p->d_literals;
  for (size_t b = 0; b < n_bases; ++b) src.bases[1 + b] = static_cast<const uint8_t*>(d_bases[b]);
  return launch_absorb(x, src, p->total, as_stream(stream));
}

rg_status rg_xof_squeeze_dev(rg_xof* x, uint8_t* d_out, size_t len, size_t out_stride, void* stream) {
  if (!x) return xof_invalid("NULL handle");
  if (len && !d_out) return xof_invalid("NULL d_out");
  if (x->n_states > 1 && out_stride < len) return xof_invalid("out_stride < len");
  if (!x->squeezing) {  // the padding goes in with the first launch
    x->pad_pos = x->pos;
    x->pos = kk::kRate;
    x->squeezing = true;
  }
  if (len == 0) return RG_OK;
  XofSqueezeArgs A;
  A.lanes = x->d_lanes;
  A.n_states = x->n_states;
  A.out = d_out;
  A.out_stride = out_stride;
  A.len = len;
  A.pad_pos = x->pad_pos;
  A.pos = x->pos;
  hipStream_t st = as_stream(stream);
  if (x->lane_layout)
    hipLaunchKernelGGL(xof_squeeze_lane_kernel, dim3((unsigned)((x->n_states + 63) / 64)), dim3(64), 0, st, A);
  else
    hipLaunchKernelGGL(xof_squeeze_coop_kernel, dim3((unsigned)((x->n_states + 1) / 2)), dim3(64), 0, st, A);
  RG_TRY(check_launch("xof_squeeze"));
  x->pad_pos = -1;
  // the position after len more bytes: a block is read to its end before the next permutation
  const size_t in_block = (size_t)(kk::kRate - x->pos);
  x->pos = len <= in_block ? x->pos + (int)len : (int)((len - in_block - 1) % kk::kRate) + 1;
  return RG_OK;
}

}  // extern "C"
