// buckler_proj.hip -- what the Buckler prover does between its first and its last commit round
// (buckler/prover.go:165-240), for a batch of proofs of one compiled circuit and enqueued by calls
// whose launch count has neither n_proofs nor the number of constraints in it, for gfx950:
//   * the projection round (prover.go:165-193): every proof draws its own 128 x rank matrix from
//     its XOF bytes, projChecker.TransformTo of every witness under an approximate infinity-norm
//     constraint (linear.go:108-123) and decomposeBig of the 128 projected values into the digit
//     witness (context.go:206-228), both written into the proof's rows of the witness table.
//       - bproj_mat_kernel: the matrix products of all proofs and constraints in ONE launch.  A
//         workgroup of 512 lanes owns kBprojGroup = 4 chunks of 128 columns of one (proof,
//         constraint): two waves per chunk, a lane per row.  The witness entries and the first 16
//         of each column's 32 XOF bytes go straight into LDS, complemented as proj_pack_kernel
//         (buckler_lin.hip) packs them (bit set <=> XOF bit 0 <=> entry true), so there is no pack
//         launch, no bit-matrix scratch and no checker handle; the four chunks' sums meet in LDS
//         and leave, added in chunk order, as one partial row per workgroup.
//       - bproj_finish_kernel: ONE launch sums the partial rows in workgroup order, stores row
//         `proj` (the 128 sums, zeros above), decomposes each sum (dcmp.hpp) and stores row `dcmp`
//         (128 nb digits, zeros above).  The constraints' bases may differ in length: each
//         constraint brings its own base pointer and nb in the kernel's arguments.
//     No atomics: f_add on canonical residues is exact, and the order is fixed anyway.
//   * the masks (prover.go:210-240, sumCheckMask at 381-397) of all proofs in ONE launch, laid out
//     as the next two calls take them: [n_proofs][emb] for rg_buckler_prove_checks_dev and
//     mask.Coeffs[:maskRank] contiguous, [n_proofs][mask_rank], for rg_jindo_commit_dev.
// Every value is a canonical Montgomery residue (field.hpp) and every step an exact field
// operation, so the limbs equal those of the single entries and of the reference.
#include <algorithm>
#include <string>
#include <vector>

#include "buckler_impl.hpp"
#include "common.hpp"
#include "dcmp.hpp"
#include "field.hpp"

namespace rg {

constexpr int kBprojRows = 128;   // linear.go:99
constexpr int kBprojChunk = 128;  // columns staged in LDS at a time: 4 KiB of XOF bytes
constexpr int kBprojGroup = 4;    // chunks per workgroup, two waves each: one partial row per 512 columns
constexpr int kBprojMaxCons = 32; // constraints of one handle: their table travels as kernel arguments

struct BprojCon {
  const uint64_t* base;  // [nb][L] plain integers, on the device (the rg_dcmp's own copy)
  unsigned src, proj, dcmp, nb;
};

static long long bproj_groups(long long rank) {
  const long long chunks = (rank + kBprojChunk - 1) / kBprojChunk;
  return (chunks + kBprojGroup - 1) / kBprojGroup;
}

// ---- TransformTo (linear.go:113-119) of witness src[blockIdx.y] of proof blockIdx.z ------------
// partial [n_proofs][n_c][groups][128][L]
template <int L>
struct BprojMatArgs {
  FieldParams<L> F;
  const uint64_t* w;   // [n_proofs][n_w][rank][L]
  const uint8_t* xof;  // [n_proofs][rank][32]
  uint64_t* partial;
  unsigned long long rank, n_w;
  unsigned src[kBprojMaxCons];
};

template <int L>
__global__ __launch_bounds__(kBprojGroup * kBprojRows) void bproj_mat_kernel(BprojMatArgs<L> a) {
  __shared__ uint64_t sv[kBprojGroup * kBprojChunk * L];
  __shared__ uint32_t sm[kBprojGroup * kBprojChunk * 4];
  const int tid = threadIdx.x, sub = tid >> 7, row = tid & (kBprojRows - 1);  // two waves per chunk
  const unsigned long long g = blockIdx.x, c = blockIdx.y, p = blockIdx.z;
  const uint64_t* v = a.w + (p * a.n_w + a.src[c]) * a.rank * L;
  const uint8_t* xof = a.xof + p * a.rank * 32;
  const unsigned long long j0 = (g * kBprojGroup + (unsigned)sub) * kBprojChunk;  // may lie past the rank
  const unsigned long long j = j0 + (unsigned)row;
  const uint64_t* svs = sv + sub * kBprojChunk * L;
  const uint32_t* sms = sm + sub * kBprojChunk * 4;
  if (j < a.rank) {
    el_copy<L>(sv + tid * L, v + j * L);
    const uint8_t* s = xof + j * 32;  // bytes 0 .. 15 hold the 128 rows' bits (prover.go:171-176)
#pragma unroll
    for (int wd = 0; wd < 4; ++wd) {
      const uint32_t x = (uint32_t)s[4 * wd] | ((uint32_t)s[4 * wd + 1] << 8) | ((uint32_t)s[4 * wd + 2] << 16) |
                         ((uint32_t)s[4 * wd + 3] << 24);
      sm[tid * 4 + wd] = ~x;
    }
  }
  __syncthreads();
  int cnt = 0;  // the chunk's columns below the rank: the same in both waves of the chunk
  if (j0 < a.rank) cnt = a.rank - j0 < (unsigned long long)kBprojChunk ? (int)(a.rank - j0) : kBprojChunk;
  const int word = row >> 5, bit = row & 31;
  uint64_t acc[L];
  el_zero<L>(acc);
#pragma unroll 1
  for (int jj = 0; jj < cnt; ++jj) {
    const uint64_t m = 0 - (uint64_t)((sms[jj * 4 + word] >> bit) & 1u);
    uint64_t x[L];
#pragma unroll
    for (int l = 0; l < L; ++l) x[l] = svs[jj * L + l] & m;
    f_add<L>(acc, acc, x, a.F);
  }
  __syncthreads();  // every chunk has been read: sv now takes the chunks' sums, [chunk][row][L]
  el_copy<L>(sv + tid * L, acc);
  __syncthreads();
  if (sub) return;
  for (int k = 1; k < kBprojGroup; ++k) {  // in chunk order
    uint64_t x[L];
    el_copy<L>(x, sv + (k * kBprojRows + row) * L);
    f_add<L>(acc, acc, x, a.F);
  }
  el_copy<L>(a.partial + (((p * gridDim.y + c) * gridDim.x + g) * kBprojRows + (unsigned)row) * L, acc);
}

// ---- the partial rows summed in workgroup order, rows `proj` and `dcmp` stored -------------------
// Lane t of constraint blockIdx.y of proof blockIdx.z owns entry t of both rows: proj[t] is the sum
// (t < 128) or zero, dcmp[t nb .. t nb + nb - 1] are the digits of that sum (t < 128) and dcmp[t] is
// zero for t >= 128 nb.  128 nb <= rank, so every entry of both rows has exactly one writer.
template <int L>
struct BprojFinArgs {
  FieldParams<L> F;
  uint64_t one[L], neg_one[L];  // SetInt64(1), SetInt64(-1)
  uint64_t* w;
  const uint64_t* partial;
  unsigned long long rank, n_w, groups;
  BprojCon con[kBprojMaxCons];
};

template <int L>
__global__ __launch_bounds__(256) void bproj_finish_kernel(BprojFinArgs<L> a) {
  const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.rank) return;
  const unsigned long long c = blockIdx.y, p = blockIdx.z;
  const BprojCon con = a.con[c];
  uint64_t* proj = a.w + (p * a.n_w + con.proj) * a.rank * L;
  uint64_t* dcmp = a.w + (p * a.n_w + con.dcmp) * a.rank * L;
  if (t >= (unsigned long long)kBprojRows * con.nb) el_zero<L>(dcmp + t * L);
  if (t >= (unsigned long long)kBprojRows) {
    el_zero<L>(proj + t * L);  // linear.go:120-122
    return;
  }
  const uint64_t* part = a.partial + ((p * gridDim.y + c) * a.groups * kBprojRows + t) * L;
  uint64_t acc[L], unit[L];
  el_zero<L>(acc);
  for (unsigned long long g = 0; g < a.groups; ++g) {
    uint64_t x[L];
    el_copy<L>(x, part + g * kBprojRows * L);
    f_add<L>(acc, acc, x, a.F);
  }
  el_copy<L>(proj + t * L, acc);
  Dcmp<L> d;
  dcmp_init<L>(d, acc, a.F);
  dcmp_unit<L>(unit, d, a.one, a.neg_one);
  uint64_t* o = dcmp + t * con.nb * L;
  for (unsigned j = 0; j < con.nb; ++j) {
    uint64_t b[L];
    el_copy<L>(b, con.base + (unsigned long long)j * L);
    const uint64_t mask = 0 - (uint64_t)dcmp_step<L>(d, b);
#pragma unroll
    for (int l = 0; l < L; ++l) o[(unsigned long long)j * L + l] = unit[l] & mask;
  }
}

// ---- sumCheckMask (prover.go:381-397) of proof blockIdx.y, elementwise as mask_kernel has it ----
template <int L>
__global__ __launch_bounds__(256) void mask_batch_kernel(FieldParams<L> F, uint64_t* mask, uint64_t* mask_com,
                                                         uint64_t* mask_sum, const uint64_t* r,
                                                         unsigned long long rank, unsigned long long mask_rank,
                                                         unsigned long long emb) {
  const unsigned long long k = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= emb) return;
  const unsigned long long p = blockIdx.y;
  r += p * mask_rank * L;
  uint64_t x[L];
  el_zero<L>(x);
  if (k < mask_rank) {
    el_copy<L>(x, r + k * L);
    if (k == 0) el_copy<L>(mask_sum + p * L, x);  // maskSum := mask.Coeffs[0] before the loop
    if (k + rank < mask_rank) {
      uint64_t y[L];
      el_copy<L>(y, r + (k + rank) * L);
      f_sub<L>(x, x, y, F);
    }
    if (mask_com) el_copy<L>(mask_com + (p * mask_rank + k) * L, x);  // mask.Coeffs[:maskRank]
  }
  el_copy<L>(mask + (p * emb + k) * L, x);
}

}  // namespace rg

// What Compile fixes for the projection round; the rg_dcmp handles are borrowed
struct rg_bproj {
  rg_field f;
  long long rank = 0;
  size_t n_w = 0;
  std::vector<rg::BprojCon> con;  // base filled per call
  std::vector<const rg_dcmp*> dcmp;
  uint64_t one[16], neg_one[16];
};

namespace rg {

static rg_status pr_invalid(const std::string& why) {
  set_last_error("buckler proj round: " + why);
  return RG_ERR_INVALID;
}

static rg_status mb_invalid(const std::string& why) {
  set_last_error("buckler mask batch: " + why);
  return RG_ERR_INVALID;
}

// n_proofs the call takes: a proof per grid row, and a witness table of at most 2^44 words
static bool pr_proofs_ok(const rg_bproj* h, size_t n_proofs) {
  if (n_proofs > RG_BK_MULTI_MAX_PROOFS) return false;
  return n_proofs * h->n_w <= (((size_t)1 << 44) / ((size_t)h->rank * h->f.L));
}

static rg_status pr_check(const rg_bproj* h, size_t n_proofs, const void* w, const void* xof) {
  if (!h) return pr_invalid("NULL handle");
  if (!pr_proofs_ok(h, n_proofs))
    return pr_invalid("n_proofs " + std::to_string(n_proofs) + " is over the limit (RG_BK_MULTI_MAX_PROOFS, 2^44 words)");
  if (n_proofs == 0) return RG_OK;
  if (!w) return pr_invalid("NULL witness table");
  if (!xof) return pr_invalid("NULL XOF bytes");
  if (w == xof) return pr_invalid("two buffers alias");
  return RG_OK;
}

template <int L>
static rg_status proj_round_L(const rg_bproj* h, size_t np, uint64_t* w, const uint8_t* xof, uint64_t* scratch,
                              const std::vector<BprojCon>& con, hipStream_t st) {
  const unsigned nc = (unsigned)con.size();
  const long long groups = bproj_groups(h->rank);
  BprojMatArgs<L> m;
  memset(&m, 0, sizeof m);
  m.F = field_params<L>(&h->f);
  m.w = w;
  m.xof = xof;
  m.partial = scratch;
  m.rank = (unsigned long long)h->rank;
  m.n_w = h->n_w;
  for (unsigned c = 0; c < nc; ++c) m.src[c] = con[c].src;
  hipLaunchKernelGGL(bproj_mat_kernel<L>, dim3((unsigned)groups, nc, (unsigned)np), dim3(kBprojGroup * kBprojRows), 0,
                     st, m);
  RG_TRY(check_launch("buckler proj round transform"));
  BprojFinArgs<L> a;
  memset(&a, 0, sizeof a);
  a.F = m.F;
  memcpy(a.one, h->one, 8 * L);
  memcpy(a.neg_one, h->neg_one, 8 * L);
  a.w = w;
  a.partial = scratch;
  a.rank = m.rank;
  a.n_w = m.n_w;
  a.groups = (unsigned long long)groups;
  for (unsigned c = 0; c < nc; ++c) a.con[c] = con[c];
  hipLaunchKernelGGL(bproj_finish_kernel<L>, dim3(grid256(h->rank), nc, (unsigned)np), dim3(256), 0, st, a);
  return check_launch("buckler proj round decompose");
}

static rg_status mb_check(const rg_field* f, size_t rank, size_t mask_rank, size_t emb_rank, size_t n_proofs,
                          const void* rand, const void* mask, const void* mask_com, const void* mask_sum) {
  if (!f) return mb_invalid("NULL field");
  if (!limbs_supported(f->L)) {
    set_last_error("buckler mask batch: no kernel for " + std::to_string(f->L) + " limbs (1, 2, 4, 7, 14)");
    return RG_ERR_UNSUPPORTED;
  }
  if (rank == 0 || mask_rank < rank || mask_rank > emb_rank || emb_rank > ((size_t)1 << 40))
    return mb_invalid("rank <= mask_rank <= emb_rank <= 2^40 does not hold, or rank = 0");
  if (n_proofs > RG_BK_MULTI_MAX_PROOFS)
    return mb_invalid("n_proofs " + std::to_string(n_proofs) + " is over RG_BK_MULTI_MAX_PROOFS");
  if (n_proofs == 0) return RG_OK;
  if (!rand || !mask || !mask_sum) return mb_invalid("a NULL buffer");
  const void* bufs[] = {rand, mask, mask_com, mask_sum};
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j)
      if (bufs[i] && bufs[i] == bufs[j]) return mb_invalid("two buffers alias");
  return RG_OK;
}

}  // namespace rg

using namespace rg;

extern "C" {

rg_status rg_buckler_proj_round_create(const rg_field* f, size_t rank, size_t n_w, size_t n_c, const uint64_t* cons,
                                       const rg_dcmp* const* dcmp, rg_bproj** out) {
  if (!out) return pr_invalid("NULL out");
  *out = nullptr;
  if (!f) return pr_invalid("NULL field");
  if (!limbs_supported(f->L)) {
    set_last_error("buckler proj round: no kernel for " + std::to_string(f->L) + " limbs (1, 2, 4, 7, 14)");
    return RG_ERR_UNSUPPORTED;
  }
  if (rank < (size_t)kBprojRows || rank > ((size_t)1 << 30))
    return pr_invalid("rank " + std::to_string(rank) + " is below 128 (the projected rows) or above 2^30");
  if (n_w == 0 || n_w > ((size_t)1 << 30)) return pr_invalid("n_w out of range");
  if (n_c == 0 || n_c > (size_t)kBprojMaxCons)
    return pr_invalid("n_c " + std::to_string(n_c) + " is not in 1 .. " + std::to_string(kBprojMaxCons));
  if (!cons || !dcmp) return pr_invalid("NULL constraints");
  std::vector<BprojCon> con(n_c);
  for (size_t c = 0; c < n_c; ++c) {
    for (int k = 0; k < 3; ++k)
      if (cons[3 * c + k] >= n_w)
        return pr_invalid("constraint " + std::to_string(c) + ": a witness index >= n_w");
    if (!dcmp[c]) return pr_invalid("constraint " + std::to_string(c) + ": NULL decomposition");
    const DcmpView d = dcmp_view(dcmp[c]);
    if (!same_field(f, d.f)) return pr_invalid("constraint " + std::to_string(c) + ": a decomposition of another field");
    if (d.nb > (long long)(rank / kBprojRows))
      return pr_invalid("constraint " + std::to_string(c) + ": 128 nb > rank");
    con[c] = BprojCon{nullptr, (unsigned)cons[3 * c], (unsigned)cons[3 * c + 1], (unsigned)cons[3 * c + 2],
                      (unsigned)d.nb};
  }
  // an output row is written by one constraint and read by none
  for (size_t c = 0; c < n_c; ++c) {
    if (con[c].proj == con[c].dcmp) return pr_invalid("constraint " + std::to_string(c) + ": proj and dcmp are one row");
    for (size_t e = 0; e < n_c; ++e) {
      if (con[c].proj == con[e].src || con[c].dcmp == con[e].src)
        return pr_invalid("an output row of constraint " + std::to_string(c) + " is the src of constraint " +
                          std::to_string(e));
      if (e != c && (con[c].proj == con[e].proj || con[c].proj == con[e].dcmp || con[c].dcmp == con[e].proj ||
                     con[c].dcmp == con[e].dcmp))
        return pr_invalid("constraints " + std::to_string(c) + " and " + std::to_string(e) + " share an output row");
    }
  }
  auto h = new rg_bproj();
  h->f = *f;
  h->rank = (long long)rank;
  h->n_w = n_w;
  h->con = con;
  h->dcmp.assign(dcmp, dcmp + n_c);
  const DcmpView d0 = dcmp_view(dcmp[0]);
  memset(h->one, 0, sizeof h->one);
  memset(h->neg_one, 0, sizeof h->neg_one);
  memcpy(h->one, d0.one, 8 * f->L);
  memcpy(h->neg_one, d0.neg_one, 8 * f->L);
  *out = h;
  return RG_OK;
}

void rg_buckler_proj_round_destroy(rg_bproj* h) { delete h; }

// scratch: the partial rows [n_proofs][n_c][groups][128][L], groups = ceil(rank / 512)
size_t rg_buckler_prove_proj_round_scratch_bytes(const rg_bproj* h, size_t n_proofs) {
  if (!h || n_proofs == 0 || !pr_proofs_ok(h, n_proofs)) return 0;
  return n_proofs * h->con.size() * (size_t)bproj_groups(h->rank) * kBprojRows * h->f.L * 8;
}

rg_status rg_buckler_prove_proj_round_dev(const rg_bproj* h, size_t n_proofs, uint64_t* d_w, const uint8_t* d_xof,
                                          uint64_t* d_scratch, void* stream) {
  RG_TRY(pr_check(h, n_proofs, d_w, d_xof));
  if (n_proofs == 0) return RG_OK;
  if (!d_scratch) return pr_invalid("NULL scratch");
  if ((const void*)d_scratch == (const void*)d_w || (const void*)d_scratch == (const void*)d_xof)
    return pr_invalid("two buffers alias");
  std::vector<BprojCon> con = h->con;
  for (size_t c = 0; c < con.size(); ++c) RG_TRY(dcmp_base_dev(h->dcmp[c], &con[c].base));  // first use uploads
  hipStream_t st = as_stream(stream);
  return dispatch_limbs(h->f.L, [&](auto Lc) { return proj_round_L<Lc()>(h, n_proofs, d_w, d_xof, d_scratch, con, st); });
}

rg_status rg_buckler_prove_proj_round(const rg_bproj* h, size_t n_proofs, uint64_t* w, const uint8_t* xof) {
  RG_TRY(pr_check(h, n_proofs, w, xof));
  if (n_proofs == 0) return RG_OK;
  const size_t bytes = n_proofs * h->n_w * (size_t)h->rank * h->f.L * 8;
  DevBuf dw, dx, dscr;
  RG_TRY(dw.upload(w, bytes));
  RG_TRY(dx.upload(xof, n_proofs * (size_t)h->rank * 32));
  RG_TRY(dscr.alloc(rg_buckler_prove_proj_round_scratch_bytes(h, n_proofs)));
  RG_TRY(rg_buckler_prove_proj_round_dev(h, n_proofs, dw.as<uint64_t>(), dx.as<uint8_t>(), dscr.as<uint64_t>(),
                                         nullptr));
  return dw.download(w, bytes);
}

rg_status rg_buckler_sumcheck_mask_batch_dev(const rg_field* f, size_t rank, size_t mask_rank, size_t emb_rank,
                                             size_t n_proofs, const uint64_t* d_rand, uint64_t* d_mask,
                                             uint64_t* d_mask_com, uint64_t* d_mask_sum, void* stream) {
  RG_TRY(mb_check(f, rank, mask_rank, emb_rank, n_proofs, d_rand, d_mask, d_mask_com, d_mask_sum));
  if (n_proofs == 0) return RG_OK;
  hipStream_t st = as_stream(stream);
  return dispatch_limbs(f->L, [&](auto Lc) {
    constexpr int L = Lc();
    hipLaunchKernelGGL(mask_batch_kernel<L>, dim3(grid256((long long)emb_rank), (unsigned)n_proofs), dim3(256), 0, st,
                       field_params<L>(f), d_mask, d_mask_com, d_mask_sum, d_rand, (unsigned long long)rank,
                       (unsigned long long)mask_rank, (unsigned long long)emb_rank);
    return check_launch("sumcheck mask batch");
  });
}

rg_status rg_buckler_sumcheck_mask_batch(const rg_field* f, size_t rank, size_t mask_rank, size_t emb_rank,
                                         size_t n_proofs, const uint64_t* rand, uint64_t* mask, uint64_t* mask_com,
                                         uint64_t* mask_sum) {
  RG_TRY(mb_check(f, rank, mask_rank, emb_rank, n_proofs, rand, mask, mask_com, mask_sum));
  if (n_proofs == 0) return RG_OK;
  const size_t e = (size_t)f->L * 8, np = n_proofs;
  DevBuf dr, dm, dc, ds;
  RG_TRY(dr.upload(rand, np * mask_rank * e));
  RG_TRY(dm.alloc(np * emb_rank * e));
  if (mask_com) RG_TRY(dc.alloc(np * mask_rank * e));
  RG_TRY(ds.alloc(np * e));
  RG_TRY(rg_buckler_sumcheck_mask_batch_dev(f, rank, mask_rank, emb_rank, np, dr.as<uint64_t>(), dm.as<uint64_t>(),
                                            mask_com ? dc.as<uint64_t>() : nullptr, ds.as<uint64_t>(), nullptr));
  RG_TRY(dm.download(mask, np * emb_rank * e));
  if (mask_com) RG_TRY(dc.download(mask_com, np * mask_rank * e));
  return ds.download(mask_sum, np * e);
}

}  // extern "C"
