// buckler_sample.hip -- the Buckler prover's MustSetRandom draws on the device, on any built field,
// for gfx950: the reference reads them from crypto/rand one Uint.SetRandom at a time
// (buckler/prover.go:136-153, 210-240, 381-397); here they come from a seeded UniformSampler
// (csprng.hpp) of which every field element has its own instance, so a value is a pure function of
// (seed, instance, q) and no draw order exists that a result could depend on.
//   * rg_fsampler: the key of NewUniformSamplerWithSeed(seed) with what SetRandom needs of the field
//     (k bytes, the top byte's mask); the Te0 table reaches the device at the first call that runs a
//     kernel.
//   * rg_field_sampler_elems_dev: element i of d_out [n][L] is SetRandom reading instance
//     first_instance + i.  The draw itself is csprng.hpp's, by its two routes, the one the Jindo
//     kernels (jindo_sample.hip) call:
//       - fs_elems_kernel: the byte-serial route, a lane per element (grid-stride);
//       - fs_whole_kernel + fs_fix_kernel: the whole-word route (q255) as uniform_whole_kernel has
//         it: one try per iteration, a lane moves on as soon as its element is accepted, a draw past
//         the tries cap is left all-ones and flagged (the flag lives in the caller's scratch) for the
//         fix-up, which runs the draw to its end, refill included.
//   * rg_buckler_sumcheck_mask_batch_sampled_dev: sumCheckMask of n_proofs proofs with the draws made
//     inside the mask kernel, so they never exist as a buffer.  A lane owns residue class c = k mod
//     rank of one proof and walks k = c, c + rank, ...: it holds the previous draw r_j, writes
//     mask[k_j] = r_j - r_{j+1} when r_{j+1} is accepted, the last r_j as it is, and then the zeros
//     of its class up to emb_rank.  Every draw is made once and every output word has one writer.
//       - mask_sampled_whole_kernel: the whole-word route, one try per iteration, lanes moving on
//         to their next draw or chain as soon as a try is accepted.  A chain that meets a draw past
//         the tries cap is left where it stands (nothing from that draw on is written) and flagged;
//       - mask_sampled_chain_kernel<WHOLE = true> (only when flagged) walks every chain with draws
//         run to their end and writes exactly what the first kernel left out: from the chain's
//         first draw past the cap on.  <WHOLE = false> is the byte-serial route: the same walk,
//         writing everything.
// No atomics; workgroups of up to 512 lanes with the T-tables in 64 KiB of LDS (two per CU).
#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <string>

#include "common.hpp"
#include "csprng.hpp"
#include "csprng_host.hpp"
#include "field.hpp"

struct rg_fsampler {
  rg_field f;
  rg::AesKey key;
  int kbytes = 0;
  uint32_t top_mask = 0;
  bool whole = false;  // even L and kbytes = 8 L: the whole-word route
  uint32_t te0[256];
  mutable std::mutex mu;
  mutable bool uploaded = false;
  mutable rg::DevBuf d_te0;
};

namespace rg {

constexpr size_t kFsScratchBytes = 256;  // [0] the whole-word route's long-draw flag (int)

template <int L>
struct FsArgs {
  AesKey key;
  const uint32_t* te0;
  FieldParams<L> F;
  int kbytes;
  uint32_t top_mask;
  unsigned long long first, n;
  uint64_t* out;  // [n][L]
};

template <int L>
__global__ __launch_bounds__(512) void fs_elems_kernel(FsArgs<L> a) {
  __shared__ uint32_t lds[kAesLds];
  __shared__ uint32_t key[kKeyWords];
  aes_lds_fill(lds, a.te0);
  aes_key_fill(key, a.key);
  __syncthreads();
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
    uint64_t z[L];
    set_random_bytes<L>(key, lds, a.first + i, a.kbytes, a.top_mask, a.F, z);
    el_copy<L>(a.out + i * L, z);
  }
}

template <int L>
__global__ __launch_bounds__(512) void fs_whole_kernel(FsArgs<L> a, int* flag, int max_tries) {
  __shared__ uint32_t lds[kAesLds];
  __shared__ uint32_t key[kKeyWords];
  aes_lds_fill(lds, a.te0);
  aes_key_fill(key, a.key);
  __syncthreads();
  const uint64_t topm = set_random_topm(a.top_mask);
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  int t = 0;
  while (i < a.n) {
    uint64_t z[L];
    bool ok = false;
    if (max_tries > 0) ok = set_random_whole_try<L>(LdsKey{key}, lds, a.first + i, t, topm, a.F, z);
    if (ok || t + 1 >= max_tries) {
      if (!ok) *flag = 1;
#pragma unroll
      for (int l = 0; l < L; ++l) a.out[i * L + l] = ok ? z[l] : ~0ull;  // all-ones: never a value below q
      i += stride;
      t = 0;
    } else {
      ++t;
    }
  }
}

template <int L>
__global__ __launch_bounds__(512) void fs_fix_kernel(FsArgs<L> a, const int* flag) {
  if (*flag == 0) return;
  __shared__ uint32_t lds[kAesLds];
  __shared__ uint32_t key[kKeyWords];
  aes_lds_fill(lds, a.te0);
  aes_key_fill(key, a.key);
  __syncthreads();
  const uint64_t topm = set_random_topm(a.top_mask);
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
    uint64_t* dst = a.out + i * L;
    bool ones = true;
#pragma unroll
    for (int l = 0; l < L; ++l) ones = ones && dst[l] == ~0ull;
    if (!ones) continue;
    uint64_t z[L];
    set_random_whole<L>(LdsKey{key}, lds, a.first + i, topm, a.F, z);
    el_copy<L>(dst, z);
  }
}

// ---- sumCheckMask (prover.go:381-397) with its draws made in place --------------------------------
template <int L>
struct MsArgs {
  AesKey key;
  const uint32_t* te0;
  FieldParams<L> F;
  int kbytes;
  uint32_t top_mask;
  unsigned long long first;  // draw k of proof p: instance first + p mask_rank + k
  unsigned long long rank, mask_rank, emb, n_proofs;
  uint64_t* mask;      // [n_proofs][emb][L]
  uint64_t* mask_com;  // [n_proofs][mask_rank][L] or null
  uint64_t* mask_sum;  // [n_proofs][L]
};

// mask[k] of proof p, k < mask_rank, in both layouts
template <int L>
__device__ __forceinline__ void ms_store(const MsArgs<L>& a, unsigned long long p, unsigned long long k,
                                         const uint64_t* x) {
  el_copy<L>(a.mask + (p * a.emb + k) * L, x);
  if (a.mask_com) el_copy<L>(a.mask_com + (p * a.mask_rank + k) * L, x);
}
// the chain's end: its last draw as it is (entry k), then the zeros of its class up to emb
template <int L>
__device__ __forceinline__ void ms_finish(const MsArgs<L>& a, unsigned long long p, unsigned long long k,
                                          const uint64_t* prev) {
  ms_store<L>(a, p, k, prev);
  for (k += a.rank; k < a.emb; k += a.rank) el_zero<L>(a.mask + (p * a.emb + k) * L);
}

template <int L>
__global__ __launch_bounds__(512) void mask_sampled_whole_kernel(MsArgs<L> a, int* flag, int max_tries) {
  __shared__ uint32_t lds[kAesLds];
  __shared__ uint32_t key[kKeyWords];
  aes_lds_fill(lds, a.te0);
  aes_key_fill(key, a.key);
  __syncthreads();
  const uint64_t topm = set_random_topm(a.top_mask);
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x, total = a.n_proofs * a.rank;
  // One try per iteration, as uniform_whole_kernel: an accepted try moves the lane to its chain's
  // next draw, or to its next chain (grid-stride over (proof, class)), at once
  unsigned long long item = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long p = 0, c = 0, k = 0;  // the chain and its current draw's index
  uint64_t prev[L];
  int t = 0;
  auto start = [&]() {
    if (item < total) {
      p = item / a.rank;
      c = k = item - p * a.rank;
      t = 0;
    }
  };
  start();
  while (item < total) {
    uint64_t z[L];
    bool ok = false;
    if (max_tries > 0) ok = set_random_whole_try<L>(LdsKey{key}, lds, a.first + p * a.mask_rank + k, t, topm, a.F, z);
    if (ok) {
      if (k == 0) el_copy<L>(a.mask_sum + p * L, z);  // maskSum := mask.Coeffs[0] before the loop
      if (k != c) {
        uint64_t d[L];
        f_sub<L>(d, prev, z, a.F);
        ms_store<L>(a, p, k - a.rank, d);
      }
      el_copy<L>(prev, z);
      t = 0;
      k += a.rank;
      if (k >= a.mask_rank) {
        ms_finish<L>(a, p, k - a.rank, prev);
        item += stride;
        start();
      }
    } else if (t + 1 >= max_tries) {  // a long draw: the rest of the chain is mask_sampled_chain_kernel's
      *flag = 1;
      item += stride;
      start();
    } else {
      ++t;
    }
  }
}

// Every chain walked with draws run to their end.  WHOLE: only when the first kernel flagged a long
// draw, and then only what it left out is written: it stopped a chain at its first draw of more than
// max_tries tries, before that draw's outputs (maskSum for draw 0, the difference that ends in it).
template <int L, bool WHOLE>
__global__ __launch_bounds__(512) void mask_sampled_chain_kernel(MsArgs<L> a, const int* flag, int max_tries) {
  if (WHOLE && *flag == 0) return;
  __shared__ uint32_t lds[kAesLds];
  __shared__ uint32_t key[kKeyWords];
  aes_lds_fill(lds, a.te0);
  aes_key_fill(key, a.key);
  __syncthreads();
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x, total = a.n_proofs * a.rank;
  for (unsigned long long item = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; item < total;
       item += stride) {
    const unsigned long long p = item / a.rank, c = item - p * a.rank;
    bool open = !WHOLE;  // this kernel writes from here on
    uint64_t prev[L];
    unsigned long long k = c;
    for (; k < a.mask_rank; k += a.rank) {
      const unsigned long long inst = a.first + p * a.mask_rank + k;
      uint64_t z[L];
      if constexpr (WHOLE) {
        const uint64_t tries = set_random_whole<L>(LdsKey{key}, lds, inst, set_random_topm(a.top_mask), a.F, z);
        open = open || tries > (uint64_t)max_tries;
      } else {
        set_random_bytes<L>(key, lds, inst, a.kbytes, a.top_mask, a.F, z);
      }
      if (open) {
        if (k == 0) el_copy<L>(a.mask_sum + p * L, z);
        if (k != c) {
          uint64_t d[L];
          f_sub<L>(d, prev, z, a.F);
          ms_store<L>(a, p, k - a.rank, d);
        }
      }
      el_copy<L>(prev, z);
    }
    if (open) ms_finish<L>(a, p, k - a.rank, prev);
  }
}

// ---- host ---------------------------------------------------------------------------------------
static rg_status fs_invalid(const std::string& why) {
  set_last_error("field sampler: " + why);
  return RG_ERR_INVALID;
}
static rg_status ms_invalid(const std::string& why) {
  set_last_error("buckler mask sampled: " + why);
  return RG_ERR_INVALID;
}

static bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && x < y + nb && y < x + na;
}

// instances first .. first + n - 1 stay below 2^64 - 1
static bool instances_ok(unsigned long long first, unsigned __int128 n) {
  return (unsigned __int128)first + n <= (unsigned __int128)~0ull;
}

// the Te0 table on the device: the first caller uploads it (to the device current then) and waits
static rg_status fs_table(const rg_fsampler* s, const uint32_t** te0) {
  std::lock_guard<std::mutex> lock(s->mu);
  if (!s->uploaded) {
    RG_TRY(s->d_te0.upload(s->te0, sizeof s->te0));
    s->uploaded = true;
  }
  *te0 = s->d_te0.as<uint32_t>();
  return RG_OK;
}

// the whole-word kernels' tries within the first 8 KiB; the experiments build may cap them
static int fs_tries(int L) {
  const char* kt = knob(Knob::JindoUniTries);
  return std::max(0, std::min(1024 / L, kt ? atoi(kt) : 1024 / L));
}

// Lanes per workgroup: 512 where the items fill the chip's 256 CUs with such workgroups, fewer (down
// to 128) below, so that a small call still spreads its table lookups over every CU's LDS (the 64 KiB
// table fill per workgroup is the price).  The kernels read blockDim.
static unsigned fs_block(unsigned long long n) {
  unsigned b = 512;
  while (b > 128 && n < 256ull * b) b >>= 1;
  return b;
}
// workgroups over n items: the whole-word loops balance lanes only over several items (about 4 per
// lane, at least a workgroup per CU where there is that much work)
static unsigned fs_grid(unsigned long long n, unsigned b) {
  return (unsigned)std::min<unsigned long long>((n + b - 1) / b, 1024);
}
static unsigned fs_grid_whole(unsigned long long n, unsigned b) {
  return (unsigned)std::max<unsigned long long>(std::min<unsigned long long>((n + b * 4 - 1) / (b * 4), 1024),
                                                std::min<unsigned long long>((n + b - 1) / b, 256));
}

static rg_status fs_check(const rg_fsampler* s, unsigned long long first, size_t n, const void* out,
                          const void* scratch, bool dev) {
  if (!s) return fs_invalid("NULL handle");
  if (n == 0) return RG_OK;
  if (!out) return fs_invalid("NULL output");
  if (dev && !scratch) return fs_invalid("NULL scratch");
  if (n > ((size_t)1 << 44) || !instances_ok(first, n))
    return fs_invalid("first_instance + n passes 2^64 - 1 (or n is above 2^44)");
  if (dev && overlap(out, n * s->f.L * 8, scratch, kFsScratchBytes)) return fs_invalid("d_out overlaps d_scratch");
  return RG_OK;
}

template <int L>
static rg_status fs_elems_L(const rg_fsampler* s, const uint32_t* te0, unsigned long long first, size_t n,
                            uint64_t* out, void* scratch, hipStream_t st) {
  FsArgs<L> a;
  a.key = s->key;
  a.te0 = te0;
  a.F = field_params<L>(&s->f);
  a.kbytes = s->kbytes;
  a.top_mask = s->top_mask;
  a.first = first;
  a.n = n;
  a.out = out;
  const unsigned b = fs_block(n);
  if constexpr (L % 2 == 0) {
    if (s->whole) {
      int* flag = reinterpret_cast<int*>(scratch);
      RG_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
      hipLaunchKernelGGL(fs_whole_kernel<L>, dim3(fs_grid_whole(n, b)), dim3(b), 0, st, a, flag, fs_tries(L));
      RG_TRY(check_launch("field sampler (whole words)"));
      hipLaunchKernelGGL(fs_fix_kernel<L>, dim3(fs_grid(n, b)), dim3(b), 0, st, a, (const int*)flag);
      return check_launch("field sampler (long draws)");
    }
  }
  hipLaunchKernelGGL(fs_elems_kernel<L>, dim3(fs_grid(n, b)), dim3(b), 0, st, a);
  return check_launch("field sampler");
}

static rg_status ms_check(const rg_fsampler* s, size_t rank, size_t mask_rank, size_t emb_rank, size_t n_proofs,
                          unsigned long long first, const void* mask, const void* mask_com, const void* mask_sum,
                          const void* scratch, bool dev) {
  if (!s) return ms_invalid("NULL handle");
  if (rank == 0 || mask_rank < rank || mask_rank > emb_rank || emb_rank > ((size_t)1 << 40))
    return ms_invalid("rank <= mask_rank <= emb_rank <= 2^40 does not hold, or rank = 0");
  if (n_proofs > RG_BK_MULTI_MAX_PROOFS)
    return ms_invalid("n_proofs " + std::to_string(n_proofs) + " is over RG_BK_MULTI_MAX_PROOFS");
  if (n_proofs == 0) return RG_OK;
  if (!instances_ok(first, (unsigned __int128)n_proofs * mask_rank))
    return ms_invalid("first_instance + n_proofs * mask_rank passes 2^64 - 1");
  if (!mask || !mask_sum) return ms_invalid("a NULL buffer");
  if (dev && !scratch) return ms_invalid("NULL scratch");
  const size_t e = (size_t)s->f.L * 8;
  const void* bufs[] = {mask, mask_com, mask_sum, dev ? scratch : nullptr};
  const size_t len[] = {n_proofs * emb_rank * e, n_proofs * mask_rank * e, n_proofs * e, kFsScratchBytes};
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j)
      if (overlap(bufs[i], len[i], bufs[j], len[j])) return ms_invalid("two buffers alias");
  return RG_OK;
}

template <int L>
static rg_status ms_L(const rg_fsampler* s, const uint32_t* te0, size_t rank, size_t mask_rank, size_t emb_rank,
                      size_t n_proofs, unsigned long long first, uint64_t* mask, uint64_t* mask_com,
                      uint64_t* mask_sum, void* scratch, hipStream_t st) {
  MsArgs<L> a;
  a.key = s->key;
  a.te0 = te0;
  a.F = field_params<L>(&s->f);
  a.kbytes = s->kbytes;
  a.top_mask = s->top_mask;
  a.first = first;
  a.rank = rank;
  a.mask_rank = mask_rank;
  a.emb = emb_rank;
  a.n_proofs = n_proofs;
  a.mask = mask;
  a.mask_com = mask_com;
  a.mask_sum = mask_sum;
  const unsigned long long chains = (unsigned long long)n_proofs * rank;
  const unsigned b = fs_block(chains);
  if constexpr (L % 2 == 0) {
    if (s->whole) {
      int* flag = reinterpret_cast<int*>(scratch);
      const int tries = fs_tries(L);
      RG_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
      hipLaunchKernelGGL(mask_sampled_whole_kernel<L>, dim3(fs_grid_whole(chains, b)), dim3(b), 0, st, a, flag, tries);
      RG_TRY(check_launch("buckler mask sampled (whole words)"));
      hipLaunchKernelGGL((mask_sampled_chain_kernel<L, true>), dim3(fs_grid(chains, b)), dim3(b), 0, st, a,
                         (const int*)flag, tries);
      return check_launch("buckler mask sampled (long draws)");
    }
  }
  hipLaunchKernelGGL((mask_sampled_chain_kernel<L, false>), dim3(fs_grid(chains, b)), dim3(b), 0, st, a,
                     (const int*)nullptr, 0);
  return check_launch("buckler mask sampled");
}

}  // namespace rg

using namespace rg;

extern "C" {

rg_status rg_field_sampler_create(const rg_field* f, const uint8_t* seed, size_t seed_len, rg_fsampler** out) {
  if (!out) return fs_invalid("NULL out");
  *out = nullptr;
  if (!f) return fs_invalid("NULL field");
  if (!seed && seed_len) return fs_invalid("NULL seed");
  if (!limbs_supported(f->L)) {
    set_last_error("field sampler: no kernel for " + std::to_string(f->L) + " limbs (1, 2, 4, 7, 14)");
    return RG_ERR_UNSUPPORTED;
  }
  AesKey key;
  const uint8_t none = 0;
  RG_TRY(derive_key(seed ? seed : &none, seed_len, key));
  auto s = new rg_fsampler();
  s->f = *f;
  s->key = key;
  set_random_shape(f, s->kbytes, s->top_mask);
  s->whole = f->L % 2 == 0 && s->kbytes == 8 * f->L;
  aes_te0(s->te0);
  *out = s;
  return RG_OK;
}

void rg_field_sampler_destroy(rg_fsampler* s) { delete s; }

size_t rg_field_sampler_scratch_bytes(const rg_fsampler* s) { return s ? kFsScratchBytes : 0; }

rg_status rg_field_sampler_elems_dev(const rg_fsampler* s, unsigned long long first_instance, size_t n,
                                     uint64_t* d_out, void* d_scratch, void* stream) {
  RG_TRY(fs_check(s, first_instance, n, d_out, d_scratch, true));
  if (n == 0) return RG_OK;
  const uint32_t* te0 = nullptr;
  RG_TRY(fs_table(s, &te0));  // first use uploads
  hipStream_t st = as_stream(stream);
  return dispatch_limbs(s->f.L,
                        [&](auto Lc) { return fs_elems_L<Lc()>(s, te0, first_instance, n, d_out, d_scratch, st); });
}

rg_status rg_field_sampler_elems(const rg_fsampler* s, unsigned long long first_instance, size_t n, uint64_t* out) {
  RG_TRY(fs_check(s, first_instance, n, out, nullptr, false));
  if (n == 0) return RG_OK;
  DevBuf d, scr;
  RG_TRY(d.alloc(n * s->f.L * 8));
  RG_TRY(scr.alloc(kFsScratchBytes));
  RG_TRY(rg_field_sampler_elems_dev(s, first_instance, n, d.as<uint64_t>(), scr.p, nullptr));
  return d.download(out, n * s->f.L * 8);
}

rg_status rg_buckler_sumcheck_mask_batch_sampled_dev(const rg_fsampler* s, size_t rank, size_t mask_rank,
                                                     size_t emb_rank, size_t n_proofs,
                                                     unsigned long long first_instance, uint64_t* d_mask,
                                                     uint64_t* d_mask_com, uint64_t* d_mask_sum, void* d_scratch,
                                                     void* stream) {
  RG_TRY(ms_check(s, rank, mask_rank, emb_rank, n_proofs, first_instance, d_mask, d_mask_com, d_mask_sum, d_scratch,
                  true));
  if (n_proofs == 0) return RG_OK;
  const uint32_t* te0 = nullptr;
  RG_TRY(fs_table(s, &te0));  // first use uploads
  hipStream_t st = as_stream(stream);
  return dispatch_limbs(s->f.L, [&](auto Lc) {
    return ms_L<Lc()>(s, te0, rank, mask_rank, emb_rank, n_proofs, first_instance, d_mask, d_mask_com, d_mask_sum,
                      d_scratch, st);
  });
}

rg_status rg_buckler_sumcheck_mask_batch_sampled(const rg_fsampler* s, size_t rank, size_t mask_rank, size_t emb_rank,
                                                 size_t n_proofs, unsigned long long first_instance, uint64_t* mask,
                                                 uint64_t* mask_com, uint64_t* mask_sum) {
  RG_TRY(ms_check(s, rank, mask_rank, emb_rank, n_proofs, first_instance, mask, mask_com, mask_sum, nullptr, false));
  if (n_proofs == 0) return RG_OK;
  const size_t e = (size_t)s->f.L * 8, np = n_proofs;
  DevBuf dm, dc, ds, scr;
  RG_TRY(dm.alloc(np * emb_rank * e));
  if (mask_com) RG_TRY(dc.alloc(np * mask_rank * e));
  RG_TRY(ds.alloc(np * e));
  RG_TRY(scr.alloc(kFsScratchBytes));
  RG_TRY(rg_buckler_sumcheck_mask_batch_sampled_dev(s, rank, mask_rank, emb_rank, np, first_instance, dm.as<uint64_t>(),
                                                    mask_com ? dc.as<uint64_t>() : nullptr, ds.as<uint64_t>(), scr.p,
                                                    nullptr));
  RG_TRY(dm.download(mask, np * emb_rank * e));
  if (mask_com) RG_TRY(dc.download(mask_com, np * mask_rank * e));
  return ds.download(mask_sum, np * e);
}

}  // extern "C"
