// buckler_lin.hip -- the linear-check half of the Buckler prover (buckler/linear.go,
// buckler/prover.go:381-485), for gfx950:
//   * the four LinearCheckers (linear.go:26-180), TransformTo (M v) and TransposeTo (M^T v):
//     the negacyclic NTT (the library's NTT kernels; the transpose is a reverse-and-scale pass
//     in front of the InvNTT), the automorphism (rg_poly_aut_dev with idx or idx^-1 mod 2 rank),
//     the 128 x rank random projection kept bit-packed (16 bytes per column) and the
//     projection-recompose product with the decomposition base;
//   * the power vector of linCheck (prover.go:409-413): a block of exponents per lane, the first
//     by square-and-multiply, the rest by walking;
//   * Prover.sumCheckMask (prover.go:381-397) in its elementwise form;
//   * the tail shared by linCheck / sumCheck / arithCheck (prover.go:399-404, 439-458, 465-484):
//     scale, InvNTT, add mask, QuoRemByVanishing and the quo / remLo / remHi gather;
//   * Prover.linCheck (prover.go:406-459): all transposes of the power vector encoded and
//     transformed in one batch, then ONE pass over the coefficients with eval in registers (the
//     reference runs four full-polynomial passes per constraint, prover.go:431-437).
// Every sum and product is the canonical Montgomery arithmetic of field.hpp, so every output limb
// equals the reference's.  All randomness and all challenges are injected.
#include <algorithm>
#include <vector>

#include "buckler_impl.hpp"
#include "common.hpp"
#include "field.hpp"
#include "host_field.hpp"
#include "ntt_plan.hpp"

namespace rg {

constexpr int kProjRows = 128;   // linear.go:99
constexpr int kProjChunk = 128;  // columns per workgroup of the projection transform
constexpr int kPowBlock = 16;    // exponents per lane of the power vector
constexpr size_t kMaxGridY = 65535;  // the y extent of a grid: the entries with an item per blockIdx.y refuse more

// ---- NTT checker: vOut[i] = v[rank-1-i] * scale (linear.go:39-41) ------------------------------
template <int L>
__global__ __launch_bounds__(256) void revscale_kernel(FieldParams<L> F, Elem<L> scale, uint64_t* out,
                                                       const uint64_t* v, long long rank, long long batch) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= batch * rank) return;
  const long long b = gid / rank, i = gid % rank;
  uint64_t x[L];
  el_copy<L>(x, v + (b * rank + (rank - 1 - i)) * L);
  f_mul<L>(x, x, scale.v, F);
  el_copy<L>(out + gid * L, x);
}

// ---- projection checker ---------------------------------------------------------------------
// bits[j][w] = ~(bytes 4w .. 4w+3 of column j's 32 XOF bytes, little-endian), w < 4: bit i % 32 of
// word i / 32 is bit i % 8 of byte i / 8, set iff the XOF bit is 0 (prover.go:171-176).  Matrix
// blockIdx.y: bits [.][rank][4] from xof [.][rank][32]
__global__ __launch_bounds__(256) void proj_pack_kernel(uint32_t* bits, const uint8_t* xof, long long rank) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= rank * 4) return;
  bits += (long long)blockIdx.y * rank * 4;
  xof += (long long)blockIdx.y * rank * 32;
  const long long j = gid >> 2;
  const int w = (int)(gid & 3);
  const uint8_t* s = xof + j * 32 + 4 * w;
  const uint32_t x = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
  bits[gid] = ~x;
}

// TransformTo, stage 1 (linear.go:113-119): a workgroup per chunk of kProjChunk columns, a lane
// per row.  The chunk of v and its column masks sit in LDS; every lane reads the same v[j] and
// the same mask word (broadcast) and adds v[j] or 0.  partial [batch][chunks][128][L].
template <int L>
__global__ __launch_bounds__(kProjRows) void proj_fwd_kernel(FieldParams<L> F, uint64_t* partial, const uint64_t* v,
                                                              const uint32_t* bits, long long rank) {
  __shared__ uint64_t sv[kProjChunk * L];
  __shared__ uint32_t sm[kProjChunk * 4];
  const int tid = threadIdx.x;
  const long long chunks = gridDim.x, b = blockIdx.y, j0 = (long long)blockIdx.x * kProjChunk;
  const long long j = j0 + tid;
  if (j < rank) {
    el_copy<L>(sv + tid * L, v + (b * rank + j) * L);
#pragma unroll
    for (int w = 0; w < 4; ++w) sm[tid * 4 + w] = bits[j * 4 + w];
  }
  __syncthreads();
  const int cnt = (int)min((long long)kProjChunk, rank - j0);
  const int word = tid >> 5, bit = tid & 31;
  uint64_t acc[L];
  el_zero<L>(acc);
#pragma unroll 1
  for (int jj = 0; jj < cnt; ++jj) {
    const uint64_t m = 0 - (uint64_t)((sm[jj * 4 + word] >> bit) & 1u);
    uint64_t x[L];
#pragma unroll
    for (int l = 0; l < L; ++l) x[l] = sv[jj * L + l] & m;
    f_add<L>(acc, acc, x, F);
  }
  el_copy<L>(partial + ((b * chunks + blockIdx.x) * kProjRows + tid) * L, acc);
}

// stage 2: the chunk partials summed in chunk order; rows 128 .. rank-1 are zero (linear.go:120-122)
template <int L>
__global__ __launch_bounds__(256) void proj_sum_kernel(FieldParams<L> F, uint64_t* out, const uint64_t* partial,
                                                       long long rank, long long chunks, long long batch) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= batch * rank) return;
  const long long b = gid / rank, i = gid % rank;
  uint64_t acc[L];
  el_zero<L>(acc);
  if (i < kProjRows) {
    for (long long c = 0; c < chunks; ++c) {
      uint64_t x[L];
      el_copy<L>(x, partial + ((b * chunks + c) * kProjRows + i) * L);
      f_add<L>(acc, acc, x, F);
    }
  }
  el_copy<L>(out + gid * L, acc);
}

// TransposeTo (linear.go:125-137): a lane per column, v[0..127] in LDS.  Vector b = blockIdx.y reads
// the matrix at bits + b * bits_stride words: 0 for the checker's one matrix, rank * 4 for a matrix
// per vector
template <int L>
__global__ __launch_bounds__(kProjRows) void proj_tr_kernel(FieldParams<L> F, uint64_t* out, const uint64_t* v,
                                                             const uint32_t* bits, long long bits_stride,
                                                             long long rank) {
  __shared__ uint64_t sv[kProjRows * L];
  const int tid = threadIdx.x;
  const long long b = blockIdx.y, j = (long long)blockIdx.x * kProjRows + tid;
  bits += b * bits_stride;
  el_copy<L>(sv + tid * L, v + (b * rank + tid) * L);  // rank >= 128
  __syncthreads();
  if (j >= rank) return;
  uint64_t acc[L];
  el_zero<L>(acc);
#pragma unroll 1
  for (int w = 0; w < 4; ++w) {
    const uint32_t mw = bits[j * 4 + w];
#pragma unroll 1
    for (int k = 0; k < 32; ++k) {
      const uint64_t m = 0 - (uint64_t)((mw >> k) & 1u);
      uint64_t x[L];
#pragma unroll
      for (int l = 0; l < L; ++l) x[l] = sv[(w * 32 + k) * L + l] & m;
      f_add<L>(acc, acc, x, F);
    }
  }
  el_copy<L>(out + (b * rank + j) * L, acc);
}

// ---- recompose checker (linear.go:155-180) ----------------------------------------------------
template <int L>
__global__ __launch_bounds__(256) void recompose_fwd_kernel(FieldParams<L> F, uint64_t* out, const uint64_t* v,
                                                            const uint64_t* base, long long nb, long long rank,
                                                            long long batch) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= batch * rank) return;
  const long long b = gid / rank, i = gid % rank;
  uint64_t acc[L];
  el_zero<L>(acc);
  if (i < rank / nb) {
    for (long long j = 0; j < nb; ++j) {
      uint64_t x[L], y[L];
      el_copy<L>(x, base + j * L);
      el_copy<L>(y, v + (b * rank + i * nb + j) * L);
      f_mul<L>(x, x, y, F);
      f_add<L>(acc, acc, x, F);
    }
  }
  el_copy<L>(out + gid * L, acc);
}

template <int L>
__global__ __launch_bounds__(256) void recompose_tr_kernel(FieldParams<L> F, uint64_t* out, const uint64_t* v,
                                                           const uint64_t* base, long long nb, long long rank,
                                                           long long batch) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= batch * rank) return;
  const long long b = gid / rank, k = gid % rank;
  uint64_t x[L];
  el_zero<L>(x);
  if (k < (rank / nb) * nb) {
    uint64_t y[L];
    el_copy<L>(x, base + (k % nb) * L);
    el_copy<L>(y, v + (b * rank + k / nb) * L);
    f_mul<L>(x, x, y, F);
  }
  el_copy<L>(out + gid * L, x);
}

// ---- power vector (prover.go:409-413) ---------------------------------------------------------
// base blockIdx.y at c + blockIdx.y * c_stride words, its table at out + blockIdx.y * n elements
template <int L>
__global__ __launch_bounds__(256) void powers_kernel(FieldParams<L> F, Elem<L> one, const uint64_t* c,
                                                     long long c_stride, uint64_t* out, long long n) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long e0 = t * kPowBlock;
  if (e0 >= n) return;
  c += (long long)blockIdx.y * c_stride;
  out += (long long)blockIdx.y * n * L;
  uint64_t cv[L], p[L], sq[L];
  el_copy<L>(cv, c);
  el_copy<L>(p, one.v);
  el_copy<L>(sq, cv);
  for (unsigned long long e = (unsigned long long)e0; e; e >>= 1) {  // p = c^e0
    if (e & 1) f_mul<L>(p, p, sq, F);
    f_mul<L>(sq, sq, sq, F);
  }
  const long long e1 = min(n, e0 + kPowBlock);
  for (long long e = e0; e < e1; ++e) {
    el_copy<L>(out + e * L, p);
    f_mul<L>(p, p, cv, F);
  }
}

// ---- sumCheckMask (prover.go:381-397), elementwise: step i of the reference's loop reads
// mask[i] before step i + rank touches it, so every read sees an original draw
template <int L>
__global__ __launch_bounds__(256) void mask_kernel(FieldParams<L> F, uint64_t* mask, uint64_t* mask_sum,
                                                   const uint64_t* r, long long rank, long long mask_rank,
                                                   long long emb) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= emb) return;
  uint64_t x[L];
  el_zero<L>(x);
  if (k < mask_rank) {
    el_copy<L>(x, r + k * L);
    if (k == 0) el_copy<L>(mask_sum, x);  // maskSum := mask.Coeffs[0] before the loop
    if (k + rank < mask_rank) {
      uint64_t y[L];
      el_copy<L>(y, r + (k + rank) * L);
      f_sub<L>(x, x, y, F);
    }
  }
  el_copy<L>(mask + k * L, x);
}

// ---- check tail: quo = quoPoly[:n_quo], remLo[i] = rem[i+1], remHi = zeros | remLo ---------
template <int L>
__global__ __launch_bounds__(256) void tail_kernel(uint64_t* quo, uint64_t* rem_lo, uint64_t* rem_hi,
                                                   const uint64_t* quo_poly, const uint64_t* rem, long long n_quo,
                                                   long long rank, long long jindo_rank) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_quo) el_copy<L>(quo + i * L, quo_poly + i * L);
  if (!rem_lo) return;
  if (i < rank - 1) el_copy<L>(rem_lo + i * L, rem + (i + 1) * L);
  if (i < jindo_rank) {
    const long long z = jindo_rank - (rank - 1);
    uint64_t x[L];
    el_zero<L>(x);
    if (i >= z) el_copy<L>(x, rem + (i - z + 1) * L);
    el_copy<L>(rem_hi + i * L, x);
  }
}

// ---- linCheck's fused pass (prover.go:427-438) -----------------------------------------------
// ecd [1 + n_chk][emb][L]: row 0 = NTT(Encode(linCheckVec)), row 1 + c = NTT(Encode(M_c^T linCheckVec))
template <int L>
struct LinArgs {
  FieldParams<L> F;
  const uint32_t* pair_off;
  const uint32_t* pairs;
  const uint64_t* ecd;
  const uint64_t* w;
  const uint64_t* bc;
  uint64_t* out;
  long long emb;
  int n_chk;
};

template <int L>
__global__ __launch_bounds__(256) void lin_kernel(LinArgs<L> a) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.emb) return;
  uint64_t ev[L], bc[L], e0[L];
  el_zero<L>(ev);  // eval := NewPoly(true)
  el_copy<L>(bc, a.bc);
  el_copy<L>(e0, a.ecd + j * L);
  uint32_t k = a.pair_off[0];
  for (int c = 0; c < a.n_chk; ++c) {
    const uint32_t k1 = a.pair_off[c + 1];
    if (k == k1) continue;
    uint64_t tr[L];
    el_copy<L>(tr, a.ecd + ((size_t)(1 + c) * a.emb + j) * L);
    for (; k < k1; ++k) {
      uint64_t term[L], x[L];
      el_copy<L>(x, a.w + ((size_t)a.pairs[2 * k + 1] * a.emb + j) * L);
      f_mul<L>(term, tr, x, a.F);  // MulTo(term, linCheckEcdTr, wIn)
      el_copy<L>(x, a.w + ((size_t)a.pairs[2 * k] * a.emb + j) * L);
      f_mul<L>(x, e0, x, a.F);
      f_sub<L>(term, term, x, a.F);  // MulSubTo(term, linCheckEcd, wOut)
      f_mul<L>(ev, ev, bc, a.F);     // ScalarMulTo(eval, eval, batchConst)
      f_add<L>(ev, ev, term, a.F);   // AddTo(eval, eval, term)
    }
  }
  el_copy<L>(a.out + j * L, ev);
}

// ---- host side ----------------------------------------------------------------------------------
template <int L>
static rg_status revscale_L(const rg_linchecker* c, uint64_t* out, const uint64_t* v, long long batch, hipStream_t st) {
  hipLaunchKernelGGL(revscale_kernel<L>, dim3(grid256(batch * c->rank)), dim3(256), 0, st, field_params<L>(&c->f),
                     elem<L>(c->scale), out, v, c->rank, batch);
  return check_launch("ntt checker transpose");
}

static long long proj_chunks(long long rank) { return (rank + kProjChunk - 1) / kProjChunk; }

template <int L>
static rg_status proj_fwd_L(const rg_linchecker* c, uint64_t* out, const uint64_t* v, long long batch,
                            uint64_t* scratch, hipStream_t st) {
  const long long chunks = proj_chunks(c->rank);
  hipLaunchKernelGGL(proj_fwd_kernel<L>, dim3((unsigned)chunks, (unsigned)batch), dim3(kProjRows), 0, st,
                     field_params<L>(&c->f), scratch, v, c->bits.as<uint32_t>(), c->rank);
  RG_TRY(check_launch("proj transform"));
  hipLaunchKernelGGL(proj_sum_kernel<L>, dim3(grid256(batch * c->rank)), dim3(256), 0, st, field_params<L>(&c->f), out,
                     scratch, c->rank, chunks, batch);
  return check_launch("proj transform sum");
}

template <int L>
static rg_status proj_tr_L(const rg_linchecker* c, uint64_t* out, const uint64_t* v, long long batch,
                           const uint32_t* bits, long long bits_stride, hipStream_t st) {
  hipLaunchKernelGGL(proj_tr_kernel<L>, dim3((unsigned)proj_chunks(c->rank), (unsigned)batch), dim3(kProjRows), 0, st,
                     field_params<L>(&c->f), out, v, bits, bits_stride, c->rank);
  return check_launch("proj transpose");
}

template <int L>
static rg_status recompose_L(const rg_linchecker* c, bool tr, uint64_t* out, const uint64_t* v, long long batch,
                             hipStream_t st) {
  if (tr)
    hipLaunchKernelGGL(recompose_tr_kernel<L>, dim3(grid256(batch * c->rank)), dim3(256), 0, st, field_params<L>(&c->f),
                       out, v, c->base.as<uint64_t>(), c->nb, c->rank, batch);
  else
    hipLaunchKernelGGL(recompose_fwd_kernel<L>, dim3(grid256(batch * c->rank)), dim3(256), 0, st,
                       field_params<L>(&c->f), out, v, c->base.as<uint64_t>(), c->nb, c->rank, batch);
  return check_launch("recompose checker");
}

template <int L>
static rg_status powers_L(const rg_field* f, const uint64_t* c, long long c_stride, long long n_c, long long n,
                          uint64_t* out, hipStream_t st) {
  const long long lanes = (n + kPowBlock - 1) / kPowBlock;
  hipLaunchKernelGGL(powers_kernel<L>, dim3(grid256(lanes), (unsigned)n_c), dim3(256), 0, st, field_params<L>(f),
                     elem<L>(f->one), c, c_stride * L, out, n);
  return check_launch("powers");
}

template <int L>
static rg_status mask_L(const rg_field* f, long long rank, long long mask_rank, long long emb, const uint64_t* r,
                        uint64_t* mask, uint64_t* mask_sum, hipStream_t st) {
  hipLaunchKernelGGL(mask_kernel<L>, dim3(grid256(emb)), dim3(256), 0, st, field_params<L>(f), mask, mask_sum, r, rank,
                     mask_rank, emb);
  return check_launch("sumcheck mask");
}

template <int L>
static rg_status tail_L(uint64_t* quo, uint64_t* rem_lo, uint64_t* rem_hi, const uint64_t* quo_poly,
                        const uint64_t* rem, long long n_quo, long long rank, long long jindo_rank, hipStream_t st) {
  long long n = n_quo;
  if (rem_lo) n = std::max(n, std::max(rank - 1, jindo_rank));
  if (n == 0) return RG_OK;
  hipLaunchKernelGGL(tail_kernel<L>, dim3(grid256(n)), dim3(256), 0, st, quo, rem_lo, rem_hi, quo_poly, rem, n_quo, rank,
                     jindo_rank);
  return check_launch("check tail");
}

template <int L>
static rg_status lin_L(const rg_lincheck* lc, const uint64_t* ecd, const uint64_t* w, const uint64_t* bc, uint64_t* out,
                       long long emb, hipStream_t st) {
  LinArgs<L> a;
  a.F = field_params<L>(ntt_field(lc->emb));
  const LinProg p = lin_prog(lc);
  a.pair_off = p.pair_off;
  a.pairs = p.pairs;
  a.ecd = ecd;
  a.w = w;
  a.bc = bc;
  a.out = out;
  a.emb = emb;
  a.n_chk = p.n_chk;
  hipLaunchKernelGGL(lin_kernel<L>, dim3(grid256(emb)), dim3(256), 0, st, a);
  return check_launch("linCheck");
}

// modInverse (linear.go:75-91) for an odd x modulo the power of two m
static long long mod_inverse(long long x, long long m) {
  long long a = x % m, b = m, u = 1, v = 0;
  while (b) {
    const long long q = a / b, t = a - q * b, s = u - q * v;
    a = b;
    b = t;
    u = v;
    v = s;
  }
  u %= m;
  return u < 0 ? u + m : u;
}

// the limb-count dispatch of each launcher
static rg_status revscale(const rg_linchecker* c, uint64_t* out, const uint64_t* v, long long batch, hipStream_t st) {
  return dispatch_limbs(c->f.L, [&](auto Lc) { return revscale_L<Lc()>(c, out, v, batch, st); });
}
static rg_status proj_fwd(const rg_linchecker* c, uint64_t* out, const uint64_t* v, long long batch, uint64_t* scratch,
                          hipStream_t st) {
  return dispatch_limbs(c->f.L, [&](auto Lc) { return proj_fwd_L<Lc()>(c, out, v, batch, scratch, st); });
}
static rg_status proj_tr(const rg_linchecker* c, uint64_t* out, const uint64_t* v, long long batch,
                         const uint32_t* bits, long long bits_stride, hipStream_t st) {
  return dispatch_limbs(c->f.L, [&](auto Lc) { return proj_tr_L<Lc()>(c, out, v, batch, bits, bits_stride, st); });
}
static rg_status recompose(const rg_linchecker* c, bool tr, uint64_t* out, const uint64_t* v, long long batch,
                           hipStream_t st) {
  return dispatch_limbs(c->f.L, [&](auto Lc) { return recompose_L<Lc()>(c, tr, out, v, batch, st); });
}
static rg_status lin_pass(const rg_lincheck* lc, const uint64_t* ecd, const uint64_t* w, const uint64_t* bc,
                          uint64_t* out, long long emb, hipStream_t st) {
  return dispatch_limbs(ntt_field(lc->emb)->L, [&](auto Lc) { return lin_L<Lc()>(lc, ecd, w, bc, out, emb, st); });
}

static rg_status checker_apply(const rg_linchecker* c, bool tr, uint64_t* d_out, const uint64_t* d_v, size_t batch,
                               uint64_t* d_scratch, void* stream) {
  if (!c || !d_out || !d_v || d_out == d_v) return RG_ERR_INVALID;
  if (batch == 0) return RG_OK;
  hipStream_t st = as_stream(stream);
  const long long nb = (long long)batch;
  switch (c->kind) {
    case RG_CHK_NTT:
      if (!tr) return rg_ntt_fwd_dev(c->ntt, d_out, d_v, batch, stream);  // linear.go:34-36
      RG_TRY(revscale(c, d_out, d_v, nb, st));                            // linear.go:39-41
      return rg_ntt_inv_dev(c->ntt, d_out, d_out, batch, stream);         // linear.go:42
    case RG_CHK_AUT:
      return rg_poly_aut_dev(&c->f, (size_t)c->rank, tr ? c->idx_inv : c->idx, c->ntt_domain, d_out, d_v, batch,
                             stream);
    case RG_CHK_PROJ:
      if (!c->bits_set || (!tr && !d_scratch)) return RG_ERR_INVALID;
      return tr ? proj_tr(c, d_out, d_v, nb, c->bits.as<uint32_t>(), 0, st)
                : proj_fwd(c, d_out, d_v, nb, d_scratch, st);
    case RG_CHK_RECOMPOSE: return recompose(c, tr, d_out, d_v, nb, st);
    default: return RG_ERR_INVALID;
  }
}

static rg_status checker_host(const rg_linchecker* c, bool tr, uint64_t* out, const uint64_t* v) {
  if (!c || !out || !v) return RG_ERR_INVALID;
  const size_t bytes = (size_t)c->rank * c->f.L * 8;
  DevBuf dv, dout, dscr;
  RG_TRY(dv.upload(v, bytes));
  RG_TRY(dout.alloc(bytes));
  RG_TRY(dscr.alloc(rg_buckler_checker_scratch_bytes(c, 1)));
  RG_TRY(checker_apply(c, tr, dout.as<uint64_t>(), dv.as<uint64_t>(), 1, dscr.as<uint64_t>(), nullptr));
  return dout.download(out, bytes);
}

static rg_linchecker* new_checker(int kind, const rg_field* f, size_t rank) {
  auto c = new rg_linchecker();
  c->kind = kind;
  c->f = *f;
  c->rank = (long long)rank;
  return c;
}

static bool rank_ok(size_t rank) { return rank >= 1 && rank <= (size_t)1 << 30; }

}  // namespace rg

using namespace rg;

extern "C" {

// ---- checkers ----------------------------------------------------------------------------------
rg_status rg_buckler_checker_create_ntt(const rg_field* f, size_t rank, rg_linchecker** out) {
  if (!f || !out) return RG_ERR_INVALID;
  *out = nullptr;
  if (!rank_ok(rank) || !is_pow2((long long)rank)) return RG_ERR_INVALID;
  auto c = new_checker(RG_CHK_NTT, f, rank);
  rg_status s = rg_ntt_create(f, (int)rank, 1, &c->ntt);  // NewCyclotomicTransformer (linear.go:29)
  if (s != RG_OK) {
    delete c;
    return s;
  }
  HostField(f).from_u64(c->scale, (uint64_t)rank);  // SetUint64(rank) (linear.go:30)
  *out = c;
  return RG_OK;
}

rg_status rg_buckler_checker_create_aut(const rg_field* f, size_t rank, long long idx, int ntt_domain,
                                        rg_linchecker** out) {
  if (!f || !out) return RG_ERR_INVALID;
  *out = nullptr;
  if (!rank_ok(rank) || !is_pow2((long long)rank) || (idx & 1) == 0) return RG_ERR_INVALID;
  if (!limbs_supported(f->L)) return RG_ERR_UNSUPPORTED;
  auto c = new_checker(RG_CHK_AUT, f, rank);
  const long long n2 = 2 * (long long)rank;
  c->idx = ((idx % n2) + n2) % n2;
  c->idx_inv = mod_inverse(c->idx, n2);  // linear.go:59
  c->ntt_domain = ntt_domain ? 1 : 0;
  *out = c;
  return RG_OK;
}

rg_status rg_buckler_checker_create_proj(const rg_field* f, size_t rank, rg_linchecker** out) {
  if (!f || !out) return RG_ERR_INVALID;
  *out = nullptr;
  if (!rank_ok(rank) || rank < (size_t)kProjRows) return RG_ERR_INVALID;  // vOut holds the 128 rows
  if (!limbs_supported(f->L)) return RG_ERR_UNSUPPORTED;
  *out = new_checker(RG_CHK_PROJ, f, rank);
  return RG_OK;
}

rg_status rg_buckler_checker_create_recompose(const rg_field* f, size_t rank, const uint64_t* base, size_t nb,
                                              rg_linchecker** out) {
  if (!f || !out) return RG_ERR_INVALID;
  *out = nullptr;
  if (!rank_ok(rank) || nb == 0 || nb > ((size_t)1 << 30) || !base) return RG_ERR_INVALID;
  if (!limbs_supported(f->L)) return RG_ERR_UNSUPPORTED;
  for (size_t j = 0; j < nb; ++j)
    if (HostField::geq(base + j * f->L, f->q, f->L)) return RG_ERR_INVALID;
  auto c = new_checker(RG_CHK_RECOMPOSE, f, rank);
  c->nb = (long long)nb;
  rg_status s = c->base.upload(base, nb * f->L * 8);
  if (s != RG_OK) {
    delete c;
    return s;
  }
  *out = c;
  return RG_OK;
}

void rg_buckler_checker_destroy(rg_linchecker* c) { delete c; }

rg_status rg_buckler_checker_set_xof_dev(rg_linchecker* c, const uint8_t* d_xof, void* stream) {
  if (!c || c->kind != RG_CHK_PROJ || !d_xof) return RG_ERR_INVALID;
  RG_TRY(c->bits.alloc((size_t)c->rank * 16));
  hipLaunchKernelGGL(proj_pack_kernel, dim3(grid256(c->rank * 4)), dim3(256), 0, as_stream(stream),
                     c->bits.as<uint32_t>(), d_xof, c->rank);
  RG_TRY(check_launch("proj set_xof"));
  c->bits_set = true;
  return RG_OK;
}

rg_status rg_buckler_checker_set_xof(rg_linchecker* c, const uint8_t* xof) {
  if (!c || c->kind != RG_CHK_PROJ || !xof) return RG_ERR_INVALID;
  DevBuf dx;
  RG_TRY(dx.upload(xof, (size_t)c->rank * 32));
  RG_TRY(rg_buckler_checker_set_xof_dev(c, dx.as<uint8_t>(), nullptr));
  RG_HIP(hipStreamSynchronize(nullptr));
  return RG_OK;
}

size_t rg_buckler_checker_scratch_bytes(const rg_linchecker* c, size_t batch) {
  if (!c || c->kind != RG_CHK_PROJ) return 0;
  return batch * (size_t)proj_chunks(c->rank) * kProjRows * c->f.L * 8;
}

rg_status rg_buckler_checker_transform_dev(const rg_linchecker* c, uint64_t* d_out, const uint64_t* d_v, size_t batch,
                                           uint64_t* d_scratch, void* stream) {
  return checker_apply(c, false, d_out, d_v, batch, d_scratch, stream);
}

rg_status rg_buckler_checker_transpose_dev(const rg_linchecker* c, uint64_t* d_out, const uint64_t* d_v, size_t batch,
                                           void* stream) {
  return checker_apply(c, true, d_out, d_v, batch, nullptr, stream);
}

rg_status rg_buckler_checker_transform(const rg_linchecker* c, uint64_t* out, const uint64_t* v) {
  return checker_host(c, false, out, v);
}

// ---- projection transpose with a matrix per vector (the verifier's batch of proofs) ---------------
size_t rg_buckler_checker_transpose_xof_scratch_bytes(const rg_linchecker* c, size_t batch) {
  if (!c || c->kind != RG_CHK_PROJ) return 0;
  return batch * (size_t)c->rank * 16;
}

rg_status rg_buckler_checker_transpose_xof_dev(const rg_linchecker* c, uint64_t* d_out, const uint64_t* d_v,
                                               size_t batch, const uint8_t* d_xof, void* d_bits_scratch,
                                               void* stream) {
  if (!c || c->kind != RG_CHK_PROJ || !d_out || !d_v || d_out == d_v) return RG_ERR_INVALID;
  if (batch > kMaxGridY) return RG_ERR_INVALID;  // a vector per blockIdx.y
  if (batch == 0) return RG_OK;
  if (!d_xof || !d_bits_scratch || d_bits_scratch == (const void*)d_out || d_bits_scratch == (const void*)d_v ||
      d_bits_scratch == (const void*)d_xof)
    return RG_ERR_INVALID;
  hipStream_t st = as_stream(stream);
  uint32_t* bits = reinterpret_cast<uint32_t*>(d_bits_scratch);
  hipLaunchKernelGGL(proj_pack_kernel, dim3(grid256(c->rank * 4), (unsigned)batch), dim3(256), 0, st, bits, d_xof,
                     c->rank);
  RG_TRY(check_launch("proj pack"));
  return proj_tr(c, d_out, d_v, (long long)batch, bits, c->rank * 4, st);
}

rg_status rg_buckler_checker_transpose(const rg_linchecker* c, uint64_t* out, const uint64_t* v) {
  return checker_host(c, true, out, v);
}

// ---- power vector ---------------------------------------------------------------------------
rg_status rg_buckler_powers_dev(const rg_field* f, const uint64_t* d_c, size_t n, uint64_t* d_out, void* stream) {
  if (!f || !d_c || (n && !d_out) || d_out == d_c || n > ((size_t)1 << 40)) return RG_ERR_INVALID;
  if (n == 0) return RG_OK;
  hipStream_t st = as_stream(stream);
  return dispatch_limbs(f->L, [&](auto Lc) { return powers_L<Lc()>(f, d_c, 1, 1, (long long)n, d_out, st); });
}

rg_status rg_buckler_powers_batch_dev(const rg_field* f, const uint64_t* d_c, size_t c_stride, size_t n_c, size_t n,
                                      uint64_t* d_out, void* stream) {
  if (!f || n > ((size_t)1 << 40) || n_c > kMaxGridY) return RG_ERR_INVALID;  // a base per blockIdx.y
  if (n_c == 0 || n == 0) return RG_OK;
  if (!d_c || !d_out || d_out == d_c || c_stride == 0 || c_stride > ((size_t)1 << 30)) return RG_ERR_INVALID;
  hipStream_t st = as_stream(stream);
  return dispatch_limbs(f->L, [&](auto Lc) {
    return powers_L<Lc()>(f, d_c, (long long)c_stride, (long long)n_c, (long long)n, d_out, st);
  });
}

rg_status rg_buckler_powers_batch(const rg_field* f, const uint64_t* c, size_t c_stride, size_t n_c, size_t n,
                                  uint64_t* out) {
  if (!f || n > ((size_t)1 << 40) || n_c > kMaxGridY) return RG_ERR_INVALID;
  if (n_c == 0 || n == 0) return RG_OK;
  if (!c || !out || c_stride == 0 || c_stride > ((size_t)1 << 30)) return RG_ERR_INVALID;
  const size_t e = (size_t)f->L * 8;
  DevBuf dc, dout;
  RG_TRY(dc.upload(c, ((n_c - 1) * c_stride + 1) * e));
  RG_TRY(dout.alloc(n_c * n * e));
  RG_TRY(rg_buckler_powers_batch_dev(f, dc.as<uint64_t>(), c_stride, n_c, n, dout.as<uint64_t>(), nullptr));
  return dout.download(out, n_c * n * e);
}

rg_status rg_buckler_powers(const rg_field* f, const uint64_t* c, size_t n, uint64_t* out) {
  if (!f || !c || (n && !out)) return RG_ERR_INVALID;
  if (n == 0) return RG_OK;
  DevBuf dc, dout;
  RG_TRY(dc.upload(c, f->L * 8));
  RG_TRY(dout.alloc(n * f->L * 8));
  RG_TRY(rg_buckler_powers_dev(f, dc.as<uint64_t>(), n, dout.as<uint64_t>(), nullptr));
  return dout.download(out, n * f->L * 8);
}

// ---- sumCheckMask -----------------------------------------------------------------------------
rg_status rg_buckler_sumcheck_mask_dev(const rg_field* f, size_t rank, size_t mask_rank, size_t emb_rank,
                                       const uint64_t* d_rand, uint64_t* d_mask, uint64_t* d_mask_sum, void* stream) {
  if (!f || !d_rand || !d_mask || !d_mask_sum) return RG_ERR_INVALID;
  if (rank == 0 || mask_rank < rank || mask_rank > emb_rank || emb_rank > ((size_t)1 << 40)) return RG_ERR_INVALID;
  if (d_rand == d_mask || d_mask_sum == d_mask || d_mask_sum == d_rand) return RG_ERR_INVALID;
  hipStream_t st = as_stream(stream);
  return dispatch_limbs(f->L, [&](auto Lc) {
    return mask_L<Lc()>(f, (long long)rank, (long long)mask_rank, (long long)emb_rank, d_rand, d_mask, d_mask_sum, st);
  });
}

rg_status rg_buckler_sumcheck_mask(const rg_field* f, size_t rank, size_t mask_rank, size_t emb_rank,
                                   const uint64_t* rand, uint64_t* mask, uint64_t* mask_sum) {
  if (!f || !rand || !mask || !mask_sum) return RG_ERR_INVALID;
  if (rank == 0 || mask_rank < rank || mask_rank > emb_rank || emb_rank > ((size_t)1 << 40)) return RG_ERR_INVALID;
  const size_t e = f->L * 8;
  DevBuf dr, dm, ds;
  RG_TRY(dr.upload(rand, mask_rank * e));
  RG_TRY(dm.alloc(emb_rank * e));
  RG_TRY(ds.alloc(e));
  RG_TRY(rg_buckler_sumcheck_mask_dev(f, rank, mask_rank, emb_rank, dr.as<uint64_t>(), dm.as<uint64_t>(),
                                      ds.as<uint64_t>(), nullptr));
  RG_TRY(dm.download(mask, emb_rank * e));
  return ds.download(mask_sum, e);
}

// ---- check tail ---------------------------------------------------------------------------------
size_t rg_buckler_check_finish_scratch_bytes(const rg_ntt* emb_plan) {
  return emb_plan ? (size_t)rg_ntt_rank(emb_plan) * ntt_field(emb_plan)->L * 8 : 0;
}

rg_status rg_buckler_check_finish_dev(const rg_ntt* emb_plan, size_t rank, uint64_t* d_eval, const uint64_t* d_scale,
                                      const uint64_t* d_mask, size_t n_quo, size_t jindo_rank, uint64_t* d_quo,
                                      uint64_t* d_rem_lo, uint64_t* d_rem_hi, uint64_t* d_scratch, void* stream) {
  if (!emb_plan || ntt_negacyclic(emb_plan) || !d_eval || !d_scratch) return RG_ERR_INVALID;
  const size_t emb = (size_t)rg_ntt_rank(emb_plan);
  if (rank == 0 || rank > emb || n_quo > emb || (n_quo && !d_quo)) return RG_ERR_INVALID;
  if ((d_rem_lo == nullptr) != (d_rem_hi == nullptr)) return RG_ERR_INVALID;
  if (d_rem_lo && jindo_rank + 1 < rank) return RG_ERR_INVALID;  // remHi holds remLo (prover.go:450-456)
  if (d_scratch == d_eval || d_quo == d_eval || d_quo == d_scratch || d_mask == d_eval) return RG_ERR_INVALID;
  if (d_rem_lo && (d_rem_lo == d_eval || d_rem_hi == d_eval || d_rem_lo == d_rem_hi || d_rem_lo == d_scratch ||
                   d_rem_hi == d_scratch || d_rem_lo == d_quo || d_rem_hi == d_quo))
    return RG_ERR_INVALID;
  const rg_field* f = ntt_field(emb_plan);
  if (d_scale) RG_TRY(rg_vec_dev(f, RG_VEC_SMUL, d_eval, d_eval, d_scale, emb, stream));  // ScalarMulTo(eval, eval, bc)
  RG_TRY(rg_ntt_inv_dev(emb_plan, d_eval, d_eval, 1, stream));                            // InvNTTTo(eval, eval)
  if (d_mask) RG_TRY(rg_vec_dev(f, RG_VEC_ADD, d_eval, d_eval, d_mask, emb, stream));     // AddTo(eval, eval, mask)
  // QuoRemByVanishing(eval, rank): quoPoly into scratch, remPoly over eval
  RG_TRY(rg_poly_quorem_vanishing_dev(f, emb, (long long)rank, d_scratch, d_eval, d_eval, 1, stream));
  hipStream_t st = as_stream(stream);
  return dispatch_limbs(f->L, [&](auto Lc) {
    return tail_L<Lc()>(d_quo, d_rem_lo, d_rem_hi, d_scratch, d_eval, (long long)n_quo, (long long)rank,
                        (long long)jindo_rank, st);
  });
}

rg_status rg_buckler_check_finish(const rg_ntt* emb_plan, size_t rank, const uint64_t* eval, const uint64_t* scale,
                                  const uint64_t* mask, size_t n_quo, size_t jindo_rank, uint64_t* quo,
                                  uint64_t* rem_lo, uint64_t* rem_hi) {
  if (!emb_plan || !eval || (n_quo && !quo)) return RG_ERR_INVALID;
  if ((rem_lo == nullptr) != (rem_hi == nullptr)) return RG_ERR_INVALID;
  if (rank == 0 || (rem_lo && jindo_rank + 1 < rank)) return RG_ERR_INVALID;
  const size_t e = ntt_field(emb_plan)->L * 8, emb = (size_t)rg_ntt_rank(emb_plan);
  DevBuf dev, dsc, dmk, dq, dlo, dhi, dscr;
  RG_TRY(dev.upload(eval, emb * e));
  if (scale) RG_TRY(dsc.upload(scale, e));
  if (mask) RG_TRY(dmk.upload(mask, emb * e));
  RG_TRY(dq.alloc(n_quo * e + 8));
  if (rem_lo) {
    RG_TRY(dlo.alloc(rank * e));
    RG_TRY(dhi.alloc(jindo_rank * e + 8));
  }
  RG_TRY(dscr.alloc(emb * e));
  RG_TRY(rg_buckler_check_finish_dev(emb_plan, rank, dev.as<uint64_t>(), scale ? dsc.as<uint64_t>() : nullptr,
                                     mask ? dmk.as<uint64_t>() : nullptr, n_quo, jindo_rank, dq.as<uint64_t>(),
                                     rem_lo ? dlo.as<uint64_t>() : nullptr, rem_lo ? dhi.as<uint64_t>() : nullptr,
                                     dscr.as<uint64_t>(), nullptr));
  if (n_quo) RG_TRY(dq.download(quo, n_quo * e));
  if (rem_lo) {
    if (rank > 1) RG_TRY(dlo.download(rem_lo, (rank - 1) * e));
    if (jindo_rank) RG_TRY(dhi.download(rem_hi, jindo_rank * e));
  }
  return RG_OK;
}

// ---- linCheck -----------------------------------------------------------------------------------
rg_status rg_buckler_lincheck_create(const rg_ntt* enc_plan, const rg_ntt* emb_plan, size_t n_chk,
                                     const rg_linchecker* const* chk, const size_t* pair_off, const uint64_t* pairs,
                                     rg_lincheck** out) {
  if (!out) return RG_ERR_INVALID;
  *out = nullptr;
  if (!enc_plan || !emb_plan || ntt_negacyclic(enc_plan) || ntt_negacyclic(emb_plan)) return RG_ERR_INVALID;
  if (n_chk > (1u << 20) || !pair_off || (n_chk && !chk) || pair_off[0] != 0) return RG_ERR_INVALID;
  const rg_field* f = ntt_field(enc_plan);
  const long long rank = rg_ntt_rank(enc_plan);
  if (!same_field(f, ntt_field(emb_plan)) || rg_ntt_rank(emb_plan) < rank) return RG_ERR_INVALID;
  for (size_t c = 0; c < n_chk; ++c) {
    if (!chk[c] || chk[c]->rank != rank || !same_field(f, &chk[c]->f)) return RG_ERR_INVALID;
    if (pair_off[c + 1] < pair_off[c] || pair_off[c + 1] >= (1u << 30)) return RG_ERR_INVALID;
  }
  const size_t np = pair_off[n_chk];
  if (np && !pairs) return RG_ERR_INVALID;
  auto lc = new rg_lincheck();
  lc->enc = enc_plan;
  lc->emb = emb_plan;
  lc->chk.assign(chk, chk + n_chk);
  lc->n_pairs = (int)np;
  std::vector<uint32_t> h(n_chk + 1 + 2 * np + 2, 0);
  for (size_t c = 0; c <= n_chk; ++c) h[c] = (uint32_t)pair_off[c];
  for (size_t k = 0; k < 2 * np; ++k) {
    if (pairs[k] >= (1u << 31)) {
      delete lc;
      return RG_ERR_INVALID;
    }
    h[n_chk + 1 + k] = (uint32_t)pairs[k];
    lc->max_w = std::max(lc->max_w, (long long)pairs[k]);
  }
  rg_status s = lc->prog.upload(h.data(), h.size() * 4);
  if (s != RG_OK) {
    delete lc;
    return s;
  }
  *out = lc;
  return RG_OK;
}

void rg_buckler_lincheck_destroy(rg_lincheck* lc) { delete lc; }

// scratch (elements of L words): v [1+n_chk][rank] | encode scratch [1+n_chk][rank] |
// ecd [1+n_chk][emb] | eval [emb] | quoPoly [emb]
size_t rg_buckler_lin_check_scratch_bytes(const rg_lincheck* lc) {
  if (!lc) return 0;
  const size_t nv = 1 + lc->chk.size(), rank = (size_t)rg_ntt_rank(lc->enc), emb = (size_t)rg_ntt_rank(lc->emb);
  return (nv * (2 * rank + emb) + 2 * emb) * ntt_field(lc->enc)->L * 8;
}

size_t rg_buckler_lin_check_rem_offset_bytes(const rg_lincheck* lc) {
  if (!lc) return 0;
  const size_t nv = 1 + lc->chk.size(), rank = (size_t)rg_ntt_rank(lc->enc), emb = (size_t)rg_ntt_rank(lc->emb);
  return nv * (2 * rank + emb) * ntt_field(lc->enc)->L * 8;
}

rg_status rg_buckler_lin_check_dev(const rg_lincheck* lc, const uint64_t* d_batch_const, const uint64_t* d_lin_const,
                                   const uint64_t* d_mask, const uint64_t* d_w, size_t n_w, size_t jindo_rank,
                                   uint64_t* d_quo, uint64_t* d_rem_lo, uint64_t* d_rem_hi, uint64_t* d_scratch,
                                   void* stream) {
  if (!lc || !d_batch_const || !d_lin_const || !d_mask || !d_quo || !d_rem_lo || !d_rem_hi || !d_scratch)
    return RG_ERR_INVALID;
  if (lc->max_w >= (long long)n_w || (lc->max_w >= 0 && !d_w)) return RG_ERR_INVALID;  // witness index range
  const rg_field* f = ntt_field(lc->enc);
  const size_t L = f->L, nv = 1 + lc->chk.size(), rank = (size_t)rg_ntt_rank(lc->enc),
               emb = (size_t)rg_ntt_rank(lc->emb);
  if (jindo_rank + 1 < rank) return RG_ERR_INVALID;
  for (const rg_linchecker* c : lc->chk)
    if (c->kind == RG_CHK_PROJ && !c->bits_set) return RG_ERR_INVALID;
  uint64_t* v = d_scratch;
  uint64_t* enc_scr = v + nv * rank * L;
  uint64_t* ecd = enc_scr + nv * rank * L;
  uint64_t* eval = ecd + nv * emb * L;
  uint64_t* quo_poly = eval + emb * L;
  RG_TRY(rg_buckler_powers_dev(f, d_lin_const, rank, v, stream));  // linCheckVec (prover.go:409-413)
  for (size_t c = 0; c < lc->chk.size(); ++c)                      // tr.TransposeTo(linCheckVecTr, linCheckVec)
    RG_TRY(rg_buckler_checker_transpose_dev(lc->chk[c], v + (1 + c) * rank * L, v, 1, stream));
  // Encode + NTT of linCheckVec and of every transpose, one batch each (prover.go:420-421, 429-430)
  RG_TRY(rg_buckler_encode_dev(lc->enc, emb, ecd, v, nv, nullptr, enc_scr, stream));
  RG_TRY(rg_ntt_fwd_dev(lc->emb, ecd, ecd, nv, stream));
  RG_TRY(lin_pass(lc, ecd, d_w, d_batch_const, eval, (long long)emb, as_stream(stream)));
  return rg_buckler_check_finish_dev(lc->emb, rank, eval, d_batch_const, d_mask, rank, jindo_rank, d_quo, d_rem_lo,
                                     d_rem_hi, quo_poly, stream);
}

rg_status rg_buckler_lin_check(const rg_lincheck* lc, const uint64_t* batch_const, const uint64_t* lin_const,
                               const uint64_t* mask, const uint64_t* w, size_t n_w, size_t jindo_rank, uint64_t* quo,
                               uint64_t* rem_lo, uint64_t* rem_hi) {
  if (!lc || !batch_const || !lin_const || !mask || !quo || !rem_lo || !rem_hi || (n_w && !w)) return RG_ERR_INVALID;
  const size_t e = ntt_field(lc->enc)->L * 8, rank = (size_t)rg_ntt_rank(lc->enc), emb = (size_t)rg_ntt_rank(lc->emb);
  if (jindo_rank + 1 < rank) return RG_ERR_INVALID;
  DevBuf dbc, dlc, dmk, dw, dq, dlo, dhi, dscr;
  RG_TRY(dbc.upload(batch_const, e));
  RG_TRY(dlc.upload(lin_const, e));
  RG_TRY(dmk.upload(mask, emb * e));
  if (n_w) RG_TRY(dw.upload(w, n_w * emb * e));
  RG_TRY(dq.alloc(rank * e));
  RG_TRY(dlo.alloc(rank * e));
  RG_TRY(dhi.alloc(jindo_rank * e + 8));
  RG_TRY(dscr.alloc(rg_buckler_lin_check_scratch_bytes(lc)));
  RG_TRY(rg_buckler_lin_check_dev(lc, dbc.as<uint64_t>(), dlc.as<uint64_t>(), dmk.as<uint64_t>(),
                                  n_w ? dw.as<uint64_t>() : nullptr, n_w, jindo_rank, dq.as<uint64_t>(),
                                  dlo.as<uint64_t>(), dhi.as<uint64_t>(), dscr.as<uint64_t>(), nullptr));
  RG_TRY(dq.download(quo, rank * e));
  if (rank > 1) RG_TRY(dlo.download(rem_lo, (rank - 1) * e));
  if (jindo_rank) RG_TRY(dhi.download(rem_hi, jindo_rank * e));
  return RG_OK;
}

}  // extern "C"
