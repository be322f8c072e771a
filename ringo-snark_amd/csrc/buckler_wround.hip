// buckler_wround.hip -- what the Buckler prover does to its witness table before and at its commit
// rounds (buckler/prover.go:77-111, 136-153, 195-201), for a batch of proofs of one compiled circuit
// and enqueued by calls whose launch count has neither n_proofs nor the number of constraints or
// rows in it, for gfx950.  Both rounds work on the proof-major table of rg_buckler_prove_proj_round_dev,
// [n_proofs][n_w][rank][L], whose rows of one witness lie n_w * rank * L words apart:
//   * the decomposition round (prover.go:77-111): the infinity-norm digits and the two-norm witness of
//     every proof and constraint, written into the proof's rows of the table.
//       - bw_inf_kernel: ONE launch for all proofs and infinity-norm constraints, a lane per
//         coefficient as dcmp_inf_kernel (buckler_dcmp.hip) has it.  The base element and the digit
//         row's ID are uniform (scalar loads); consecutive lanes store consecutive elements of one
//         digit row.  The row IDs are a table of the handle on the device: a base has up to several
//         hundred digits.
//       - bw_sq_kernel: ONE launch with the squares of a chunk of 1024 coefficients summed per
//         workgroup, for all proofs and two-norm constraints, into scratch.
//       - bw_two_kernel: ONE launch sums the partials in chunk order, walks the base and stores row
//         `dst` with its zero tail, and sqNm.
//   * the encode round (prover.go:136-153, 195-201): RandEncode of the rows of one commit round of
//     every proof into the embedding-rank table [n_proofs][n_w][emb][L], with the first rank + 1
//     coefficients of each also contiguous, as rg_jindo_commit_dev takes them.
//       - bw_gather_kernel: ONE launch copies the selected plain rows into contiguous scratch; skipped
//         when the rows are 0 .. n_w - 1, for then the table itself is the transform's input.
//       - one batched rg_ntt_inv_dev over the n_proofs * n_sel vectors.
//       - bw_embed_kernel: ONE launch writes the strided rows of the table (embed_kernel's elements,
//         buckler.hip) and the commit rows together.
// The arithmetic is dcmp.hpp's and field.hpp's: every value is a canonical Montgomery residue and
// every step an exact field operation, so the limbs equal those of the single entries and of the
// reference.  Every output word has one writer; there are no atomics.
#include <algorithm>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "buckler_impl.hpp"
#include "common.hpp"
#include "dcmp.hpp"
#include "field.hpp"
#include "ntt_plan.hpp"

namespace rg {

constexpr int kBwMaxCons = 32;    // constraints of one kind in a handle: their table travels as kernel arguments
constexpr int kBwSqBlock = 256;
constexpr int kBwSqChunk = 1024;  // coefficients per workgroup of the sum of squares
constexpr size_t kBwMaxRank = (size_t)1 << 30;
constexpr size_t kBwMaxSel = 65535;  // the selected rows are the grid's y extent

struct BwInfCon {
  const uint64_t* base;  // [nb][L] plain integers, on the device (the rg_dcmp's own copy)
  const uint32_t* rows;  // [nb] digit-row IDs, on the device (the handle's table)
  unsigned src, nb;
};

struct BwTwoCon {
  const uint64_t* base;
  unsigned src, dst, nb;
};

static long long bw_chunks(long long rank) { return (rank + kBwSqChunk - 1) / kBwSqChunk; }

// ---- prover.go:77-86: coefficient i of witness src of constraint blockIdx.y of proof blockIdx.z ----
template <int L>
struct BwInfArgs {
  FieldParams<L> F;
  uint64_t one[L], neg_one[L];  // SetInt64(1), SetInt64(-1)
  uint64_t* w;                  // [n_proofs][n_w][rank][L]
  unsigned long long rank, n_w;
  BwInfCon con[kBwMaxCons];
};

template <int L>
__global__ __launch_bounds__(256) void bw_inf_kernel(BwInfArgs<L> a) {
  const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.rank) return;
  const unsigned long long p = blockIdx.z;
  const BwInfCon con = a.con[blockIdx.y];
  uint64_t* tab = a.w + p * a.n_w * a.rank * L;
  uint64_t x[L], c[L];
  el_copy<L>(x, tab + ((unsigned long long)con.src * a.rank + i) * L);
  Dcmp<L> d;
  dcmp_init<L>(d, x, a.F);
  dcmp_unit<L>(c, d, a.one, a.neg_one);
  for (unsigned j = 0; j < con.nb; ++j) {
    uint64_t b[L], v[L];
    el_copy<L>(b, con.base + (unsigned long long)j * L);
    const uint64_t mask = 0 - (uint64_t)dcmp_step<L>(d, b);
#pragma unroll
    for (int l = 0; l < L; ++l) v[l] = c[l] & mask;
    el_copy<L>(tab + ((unsigned long long)con.rows[j] * a.rank + i) * L, v);
  }
}

// ---- prover.go:99-104, stage 1: the squares of chunk blockIdx.x of witness src of two-norm constraint
// blockIdx.y of proof blockIdx.z, summed as dcmp_two_partial_kernel sums them.
// partial [n_proofs][n_two][chunks][L]
template <int L>
struct BwSqArgs {
  FieldParams<L> F;
  const uint64_t* w;
  uint64_t* partial;
  unsigned long long rank, n_w;
  unsigned src[kBwMaxCons];
};

template <int L>
__global__ __launch_bounds__(kBwSqBlock) void bw_sq_kernel(BwSqArgs<L> a) {
  __shared__ uint64_t red[kBwSqBlock * L];
  const int tid = threadIdx.x;
  const unsigned long long c = blockIdx.y, p = blockIdx.z, i0 = (unsigned long long)blockIdx.x * kBwSqChunk;
  const uint64_t* v = a.w + (p * a.n_w + a.src[c]) * a.rank * L;
  uint64_t acc[L];
  el_zero<L>(acc);
#pragma unroll 1
  for (int r = 0; r < kBwSqChunk / kBwSqBlock; ++r) {
    const unsigned long long i = i0 + (unsigned)(r * kBwSqBlock + tid);
    if (i < a.rank) {
      uint64_t x[L];
      el_copy<L>(x, v + i * L);
      f_mul<L>(x, x, x, a.F);
      f_add<L>(acc, acc, x, a.F);
    }
  }
  el_copy<L>(red + tid * L, acc);
  __syncthreads();
#pragma unroll 1
  for (int h = kBwSqBlock / 2; h > 0; h >>= 1) {
    if (tid < h) {
      uint64_t y[L];
      el_copy<L>(y, red + (tid + h) * L);
      f_add<L>(acc, acc, y, a.F);
      el_copy<L>(red + tid * L, acc);
    }
    __syncthreads();
  }
  if (tid == 0) el_copy<L>(a.partial + ((p * gridDim.y + c) * gridDim.x + blockIdx.x) * L, acc);
}

// ---- stage 2 (prover.go:104-110): a lane per entry of row dst.  A workgroup whose entries reach below
// nb sums the partials in chunk order and walks the base, every lane on the same values (the loads are
// uniform), and lane i keeps the digit of step i; the other workgroups write zeros.
template <int L>
struct BwTwoArgs {
  FieldParams<L> F;
  uint64_t one[L], neg_one[L];
  uint64_t* w;
  uint64_t* sq;  // [n_proofs][n_two][L] or nullptr
  const uint64_t* partial;
  unsigned long long rank, n_w, chunks;
  BwTwoCon con[kBwMaxCons];
};

template <int L>
__global__ __launch_bounds__(256) void bw_two_kernel(BwTwoArgs<L> a) {
  const unsigned long long i0 = (unsigned long long)blockIdx.x * blockDim.x, i = i0 + threadIdx.x;
  const unsigned long long c = blockIdx.y, p = blockIdx.z;
  const BwTwoCon con = a.con[c];
  uint64_t v[L];
  el_zero<L>(v);
  if (i0 < con.nb) {
    const uint64_t* part = a.partial + (p * gridDim.y + c) * a.chunks * L;
    uint64_t acc[L], u[L];
    el_zero<L>(acc);
    for (unsigned long long ch = 0; ch < a.chunks; ++ch) {
      uint64_t y[L];
      el_copy<L>(y, part + ch * L);
      f_add<L>(acc, acc, y, a.F);
    }
    if (a.sq && i == 0) el_copy<L>(a.sq + (p * gridDim.y + c) * L, acc);
    Dcmp<L> d;
    dcmp_init<L>(d, acc, a.F);
    dcmp_unit<L>(u, d, a.one, a.neg_one);
    const unsigned long long j1 = min((unsigned long long)con.nb, i0 + blockDim.x);
    for (unsigned long long j = 0; j < j1; ++j) {
      uint64_t b[L];
      el_copy<L>(b, con.base + j * L);
      const uint64_t mask = 0 - (uint64_t)(dcmp_step<L>(d, b) && j == i);
#pragma unroll
      for (int l = 0; l < L; ++l) v[l] |= u[l] & mask;
    }
  }
  if (i >= a.rank) return;
  el_copy<L>(a.w + ((p * a.n_w + con.dst) * a.rank + i) * L, v);
}

// ---- the plain rows sel[blockIdx.y] of proof blockIdx.z, contiguous: out [n_proofs][n_sel][rank][L] --
template <int L>
__global__ __launch_bounds__(256) void bw_gather_kernel(uint64_t* out, const uint64_t* w, const uint32_t* sel,
                                                        unsigned long long rank, unsigned long long n_w) {
  const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rank) return;
  const unsigned long long s = blockIdx.y, p = blockIdx.z;
  uint64_t x[L];
  el_copy<L>(x, w + ((p * n_w + sel[s]) * rank + i) * L);
  el_copy<L>(out + ((p * gridDim.y + s) * rank + i) * L, x);
}

// ---- encoder.go:32-54: coefficient i of row sel[blockIdx.y] of proof blockIdx.z, as embed_kernel
// (buckler.hip) has it, from the InvNTT output src [n_proofs][n_sel][rank][L]; coefficients 0 .. rank
// also go to com [n_proofs][n_sel][rank + 1][L]
template <int L>
__global__ __launch_bounds__(256) void bw_embed_kernel(FieldParams<L> F, uint64_t* wecd, uint64_t* com,
                                                       const uint64_t* src, const uint64_t* rnd, const uint32_t* sel,
                                                       unsigned long long rank, unsigned long long emb,
                                                       unsigned long long n_w) {
  const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= emb) return;
  const unsigned long long s = blockIdx.y, p = blockIdx.z, v = p * gridDim.y + s;
  uint64_t x[L];
  el_zero<L>(x);  // Coeffs[i].SetUint64(0)
  if (i < rank) {
    el_copy<L>(x, src + (v * rank + i) * L);
    if (i == 0 && rnd) f_sub<L>(x, x, rnd + v * L, F);  // Coeffs[0].Sub(Coeffs[0], Coeffs[rank])
  } else if (i == rank && rnd) {
    el_copy<L>(x, rnd + v * L);  // Coeffs[rank].MustSetRandom()
  }
  el_copy<L>(wecd + ((p * n_w + sel[s]) * emb + i) * L, x);
  if (com && i <= rank) el_copy<L>(com + (v * (rank + 1) + i) * L, x);
}

}  // namespace rg

// What Compile fixes for the decomposition round; the rg_dcmp handles are borrowed
struct rg_bdcmp {
  rg_field f;
  long long rank = 0;
  size_t n_w = 0;
  std::vector<rg::BwInfCon> inf;  // base and rows filled per call
  std::vector<rg::BwTwoCon> two;  // base filled per call
  std::vector<const rg_dcmp*> inf_dc, two_dc;
  std::vector<size_t> row_off;   // constraint c's digit rows: hrows[row_off[c] .. row_off[c] + nb)
  std::vector<uint32_t> hrows;
  uint64_t one[16], neg_one[16];
  // the device copy of the digit-row IDs, made once by the first call that runs a kernel
  mutable std::mutex mu;
  mutable bool uploaded = false;
  mutable rg::DevBuf rows;
};

// What Compile fixes for one commit round's encodings; the plan is borrowed
struct rg_bencode {
  const rg_ntt* enc = nullptr;  // cyclic at the witness rank
  rg_field f;
  long long rank = 0, emb = 0;
  size_t n_w = 0;
  std::vector<uint32_t> hsel;
  bool identity = false;  // sel = 0 .. n_w - 1: no gather
  mutable std::mutex mu;
  mutable bool uploaded = false;
  mutable rg::DevBuf sel;
};

namespace rg {

static rg_status dr_invalid(const std::string& why) {
  set_last_error("buckler dcmp round: " + why);
  return RG_ERR_INVALID;
}

static rg_status er_invalid(const std::string& why) {
  set_last_error("buckler encode round: " + why);
  return RG_ERR_INVALID;
}

// the handle's table on the device; the first caller uploads it and every later one finds it there
static rg_status ensure_table(std::mutex& mu, bool& uploaded, DevBuf& buf, const std::vector<uint32_t>& host) {
  std::lock_guard<std::mutex> lock(mu);
  if (uploaded) return RG_OK;
  RG_TRY(buf.upload(host.data(), host.size() * sizeof(uint32_t)));
  uploaded = true;
  return RG_OK;
}

// n_proofs a call takes: a proof per grid layer, and a table of at most 2^44 words
static bool proofs_ok(size_t n_proofs, size_t n_w, size_t row_words) {
  if (n_proofs > RG_BK_MULTI_MAX_PROOFS) return false;
  return n_proofs * n_w <= (((size_t)1 << 44) / row_words);
}

static bool dr_proofs_ok(const rg_bdcmp* h, size_t n) { return proofs_ok(n, h->n_w, (size_t)h->rank * h->f.L); }
static bool er_proofs_ok(const rg_bencode* h, size_t n) { return proofs_ok(n, h->n_w, (size_t)h->emb * h->f.L); }

static rg_status dr_check(const rg_bdcmp* h, size_t n_proofs, const void* w, const void* sq) {
  if (!h) return dr_invalid("NULL handle");
  if (!dr_proofs_ok(h, n_proofs))
    return dr_invalid("n_proofs " + std::to_string(n_proofs) + " is over the limit (RG_BK_MULTI_MAX_PROOFS, 2^44 words)");
  if (n_proofs == 0) return RG_OK;
  if (!w) return dr_invalid("NULL witness table");
  if (sq && h->two.empty()) return dr_invalid("sq given, but the handle has no two-norm constraint");
  if (sq == w) return dr_invalid("two buffers alias");
  return RG_OK;
}

static rg_status er_check(const rg_bencode* h, size_t n_proofs, const void* w, const void* rand, const void* wecd,
                          const void* com) {
  if (!h) return er_invalid("NULL handle");
  if (!er_proofs_ok(h, n_proofs))
    return er_invalid("n_proofs " + std::to_string(n_proofs) + " is over the limit (RG_BK_MULTI_MAX_PROOFS, 2^44 words)");
  if (n_proofs == 0) return RG_OK;
  if (!w) return er_invalid("NULL witness table");
  if (!wecd) return er_invalid("NULL encoded table");
  if (com && !rand) return er_invalid("com without rand: Encode leaves coefficient `rank` zero, there is nothing to commit to");
  const void* bufs[] = {w, rand, wecd, com};
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j)
      if (bufs[i] && bufs[i] == bufs[j]) return er_invalid("two buffers alias");
  return RG_OK;
}

template <int L>
static rg_status dcmp_round_L(const rg_bdcmp* h, size_t np, uint64_t* w, uint64_t* sq, uint64_t* scratch,
                              const std::vector<BwInfCon>& inf, const std::vector<BwTwoCon>& two, hipStream_t st) {
  const FieldParams<L> F = field_params<L>(&h->f);
  const unsigned long long rank = (unsigned long long)h->rank;
  if (!inf.empty()) {
    BwInfArgs<L> a;
    memset(&a, 0, sizeof a);
    a.F = F;
    memcpy(a.one, h->one, 8 * L);
    memcpy(a.neg_one, h->neg_one, 8 * L);
    a.w = w;
    a.rank = rank;
    a.n_w = h->n_w;
    for (size_t c = 0; c < inf.size(); ++c) a.con[c] = inf[c];
    hipLaunchKernelGGL(bw_inf_kernel<L>, dim3(grid256(h->rank), (unsigned)inf.size(), (unsigned)np), dim3(256), 0, st,
                       a);
    RG_TRY(check_launch("buckler dcmp round infinity-norm digits"));
  }
  if (two.empty()) return RG_OK;
  const long long chunks = bw_chunks(h->rank);
  BwSqArgs<L> s;
  memset(&s, 0, sizeof s);
  s.F = F;
  s.w = w;
  s.partial = scratch;
  s.rank = rank;
  s.n_w = h->n_w;
  for (size_t c = 0; c < two.size(); ++c) s.src[c] = two[c].src;
  hipLaunchKernelGGL(bw_sq_kernel<L>, dim3((unsigned)chunks, (unsigned)two.size(), (unsigned)np), dim3(kBwSqBlock), 0,
                     st, s);
  RG_TRY(check_launch("buckler dcmp round two-norm squares"));
  BwTwoArgs<L> t;
  memset(&t, 0, sizeof t);
  t.F = F;
  memcpy(t.one, h->one, 8 * L);
  memcpy(t.neg_one, h->neg_one, 8 * L);
  t.w = w;
  t.sq = sq;
  t.partial = scratch;
  t.rank = rank;
  t.n_w = h->n_w;
  t.chunks = (unsigned long long)chunks;
  for (size_t c = 0; c < two.size(); ++c) t.con[c] = two[c];
  hipLaunchKernelGGL(bw_two_kernel<L>, dim3(grid256(h->rank), (unsigned)two.size(), (unsigned)np), dim3(256), 0, st,
                     t);
  return check_launch("buckler dcmp round two-norm digits");
}

template <int L>
static rg_status gather_L(const rg_bencode* h, size_t np, uint64_t* out, const uint64_t* w, hipStream_t st) {
  hipLaunchKernelGGL(bw_gather_kernel<L>, dim3(grid256(h->rank), (unsigned)h->hsel.size(), (unsigned)np), dim3(256), 0,
                     st, out, w, h->sel.as<uint32_t>(), (unsigned long long)h->rank, (unsigned long long)h->n_w);
  return check_launch("buckler encode round gather");
}

template <int L>
static rg_status embed_round_L(const rg_bencode* h, size_t np, uint64_t* wecd, uint64_t* com, const uint64_t* src,
                               const uint64_t* rnd, hipStream_t st) {
  hipLaunchKernelGGL(bw_embed_kernel<L>, dim3(grid256(h->emb), (unsigned)h->hsel.size(), (unsigned)np), dim3(256), 0,
                     st, field_params<L>(&h->f), wecd, com, src, rnd, h->sel.as<uint32_t>(),
                     (unsigned long long)h->rank, (unsigned long long)h->emb, (unsigned long long)h->n_w);
  return check_launch("buckler encode round embed");
}

}  // namespace rg

using namespace rg;

extern "C" {

rg_status rg_buckler_dcmp_round_create(const rg_field* f, size_t rank, size_t n_w, size_t n_inf,
                                       const uint64_t* inf_src, const rg_dcmp* const* inf_dcmp,
                                       const uint64_t* inf_rows, size_t n_two, const uint64_t* two_cons,
                                       const rg_dcmp* const* two_dcmp, rg_bdcmp** out) {
  if (!out) return dr_invalid("NULL out");
  *out = nullptr;
  if (!f) return dr_invalid("NULL field");
  if (!limbs_supported(f->L)) {
    set_last_error("buckler dcmp round: no kernel for " + std::to_string(f->L) + " limbs (1, 2, 4, 7, 14)");
    return RG_ERR_UNSUPPORTED;
  }
  if (rank == 0 || rank > kBwMaxRank) return dr_invalid("rank " + std::to_string(rank) + " is 0 or above 2^30");
  if (n_w == 0 || n_w > ((size_t)1 << 30)) return dr_invalid("n_w out of range");
  if (n_inf + n_two == 0) return dr_invalid("no constraint: n_inf + n_two = 0");
  if (n_inf > (size_t)kBwMaxCons || n_two > (size_t)kBwMaxCons)
    return dr_invalid("n_inf " + std::to_string(n_inf) + " or n_two " + std::to_string(n_two) + " is over " +
                      std::to_string(kBwMaxCons));
  if (n_inf && (!inf_src || !inf_dcmp || !inf_rows)) return dr_invalid("NULL infinity-norm constraints");
  if (n_two && (!two_cons || !two_dcmp)) return dr_invalid("NULL two-norm constraints");
  auto h = new rg_bdcmp();
  std::unique_ptr<rg_bdcmp> own(h);
  const DcmpView* first = nullptr;
  DcmpView d0;
  std::vector<unsigned> srcs, outs;
  for (size_t c = 0; c < n_inf; ++c) {
    const std::string who = "infinity-norm constraint " + std::to_string(c);
    if (!inf_dcmp[c]) return dr_invalid(who + ": NULL decomposition");
    const DcmpView d = dcmp_view(inf_dcmp[c]);
    if (!same_field(f, d.f)) return dr_invalid(who + ": a decomposition of another field");
    if (inf_src[c] >= n_w) return dr_invalid(who + ": a witness index >= n_w");
    const size_t off = h->hrows.size();
    for (long long j = 0; j < d.nb; ++j) {
      if (inf_rows[off + j] >= n_w) return dr_invalid(who + ": a witness index >= n_w");
      h->hrows.push_back((uint32_t)inf_rows[off + j]);
      outs.push_back((unsigned)inf_rows[off + j]);
    }
    h->row_off.push_back(off);
    h->inf.push_back(BwInfCon{nullptr, nullptr, (unsigned)inf_src[c], (unsigned)d.nb});
    srcs.push_back((unsigned)inf_src[c]);
    if (!first) first = &(d0 = d);
  }
  for (size_t c = 0; c < n_two; ++c) {
    const std::string who = "two-norm constraint " + std::to_string(c);
    if (!two_dcmp[c]) return dr_invalid(who + ": NULL decomposition");
    const DcmpView d = dcmp_view(two_dcmp[c]);
    if (!same_field(f, d.f)) return dr_invalid(who + ": a decomposition of another field");
    if (two_cons[2 * c] >= n_w || two_cons[2 * c + 1] >= n_w) return dr_invalid(who + ": a witness index >= n_w");
    if ((size_t)d.nb > rank) return dr_invalid(who + ": nb > rank");
    h->two.push_back(BwTwoCon{nullptr, (unsigned)two_cons[2 * c], (unsigned)two_cons[2 * c + 1], (unsigned)d.nb});
    srcs.push_back((unsigned)two_cons[2 * c]);
    outs.push_back((unsigned)two_cons[2 * c + 1]);
    if (!first) first = &(d0 = d);
  }
  // an output row is written by one constraint, once, and read by none
  for (unsigned o : outs)
    if (std::find(srcs.begin(), srcs.end(), o) != srcs.end())
      return dr_invalid("output row " + std::to_string(o) + " is the src of a constraint");
  std::vector<unsigned> sorted = outs;
  std::sort(sorted.begin(), sorted.end());
  const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
  if (dup != sorted.end()) return dr_invalid("output row " + std::to_string(*dup) + " is written twice: constraints share it");
  h->f = *f;
  h->rank = (long long)rank;
  h->n_w = n_w;
  h->inf_dc.assign(inf_dcmp, inf_dcmp + n_inf);
  h->two_dc.assign(two_dcmp, two_dcmp + n_two);
  memset(h->one, 0, sizeof h->one);
  memset(h->neg_one, 0, sizeof h->neg_one);
  memcpy(h->one, first->one, 8 * f->L);
  memcpy(h->neg_one, first->neg_one, 8 * f->L);
  *out = own.release();
  return RG_OK;
}

void rg_buckler_dcmp_round_destroy(rg_bdcmp* h) { delete h; }

// scratch: the partial sums of squares [n_proofs][n_two][chunks][L], chunks = ceil(rank / 1024)
size_t rg_buckler_prove_dcmp_round_scratch_bytes(const rg_bdcmp* h, size_t n_proofs) {
  if (!h || n_proofs == 0 || !dr_proofs_ok(h, n_proofs)) return 0;
  return n_proofs * h->two.size() * (size_t)bw_chunks(h->rank) * h->f.L * 8;
}

rg_status rg_buckler_prove_dcmp_round_dev(const rg_bdcmp* h, size_t n_proofs, uint64_t* d_w, uint64_t* d_sq,
                                          uint64_t* d_scratch, void* stream) {
  RG_TRY(dr_check(h, n_proofs, d_w, d_sq));
  if (n_proofs == 0) return RG_OK;
  if (!h->two.empty() && !d_scratch) return dr_invalid("NULL scratch");
  if (d_scratch && (d_scratch == d_w || d_scratch == d_sq)) return dr_invalid("two buffers alias");
  std::vector<BwInfCon> inf = h->inf;
  std::vector<BwTwoCon> two = h->two;
  if (!inf.empty()) RG_TRY(ensure_table(h->mu, h->uploaded, h->rows, h->hrows));  // first use uploads
  for (size_t c = 0; c < inf.size(); ++c) {
    RG_TRY(dcmp_base_dev(h->inf_dc[c], &inf[c].base));
    inf[c].rows = h->rows.as<uint32_t>() + h->row_off[c];
  }
  for (size_t c = 0; c < two.size(); ++c) RG_TRY(dcmp_base_dev(h->two_dc[c], &two[c].base));
  hipStream_t st = as_stream(stream);
  return dispatch_limbs(h->f.L,
                        [&](auto Lc) { return dcmp_round_L<Lc()>(h, n_proofs, d_w, d_sq, d_scratch, inf, two, st); });
}

rg_status rg_buckler_prove_dcmp_round(const rg_bdcmp* h, size_t n_proofs, uint64_t* w, uint64_t* sq) {
  RG_TRY(dr_check(h, n_proofs, w, sq));
  if (n_proofs == 0) return RG_OK;
  const size_t e = (size_t)h->f.L * 8, bytes = n_proofs * h->n_w * (size_t)h->rank * e;
  DevBuf dw, dsq, dscr;
  RG_TRY(dw.upload(w, bytes));
  if (sq) RG_TRY(dsq.alloc(n_proofs * h->two.size() * e));
  RG_TRY(dscr.alloc(rg_buckler_prove_dcmp_round_scratch_bytes(h, n_proofs)));
  RG_TRY(rg_buckler_prove_dcmp_round_dev(h, n_proofs, dw.as<uint64_t>(), sq ? dsq.as<uint64_t>() : nullptr,
                                         dscr.as<uint64_t>(), nullptr));
  RG_TRY(dw.download(w, bytes));
  if (sq) RG_TRY(dsq.download(sq, n_proofs * h->two.size() * e));
  return RG_OK;
}

rg_status rg_buckler_encode_round_create(const rg_ntt* enc_plan, size_t emb_rank, size_t n_w, size_t n_sel,
                                         const uint64_t* sel, rg_bencode** out) {
  if (!out) return er_invalid("NULL out");
  *out = nullptr;
  if (!enc_plan) return er_invalid("NULL plan");
  const rg_field* f = ntt_field(enc_plan);
  if (!limbs_supported(f->L)) {
    set_last_error("buckler encode round: no kernel for " + std::to_string(f->L) + " limbs (1, 2, 4, 7, 14)");
    return RG_ERR_UNSUPPORTED;
  }
  if (ntt_negacyclic(enc_plan)) return er_invalid("a negacyclic plan: the Encoder's transformer is cyclic");
  const size_t rank = (size_t)rg_ntt_rank(enc_plan);
  if (!is_pow2((long long)emb_rank) || emb_rank <= rank || emb_rank > kBwMaxRank)
    return er_invalid("embedding rank " + std::to_string(emb_rank) + " is no power of two above the rank " +
                      std::to_string(rank) + " (and at most 2^30)");
  if (n_w == 0 || n_w > ((size_t)1 << 30)) return er_invalid("n_w out of range");
  if (n_sel == 0 || n_sel > kBwMaxSel) return er_invalid("n_sel " + std::to_string(n_sel) + " is not in 1 .. 65535");
  if (!sel) return er_invalid("NULL sel");
  std::vector<uint32_t> rows(n_sel);
  bool identity = n_sel == n_w;
  for (size_t s = 0; s < n_sel; ++s) {
    if (sel[s] >= n_w) return er_invalid("sel[" + std::to_string(s) + "]: a witness index >= n_w");
    rows[s] = (uint32_t)sel[s];
    identity = identity && sel[s] == s;
  }
  std::vector<uint32_t> sorted = rows;
  std::sort(sorted.begin(), sorted.end());
  const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
  if (dup != sorted.end()) return er_invalid("row " + std::to_string(*dup) + " is selected twice");
  auto h = new rg_bencode();
  h->enc = enc_plan;
  h->f = *f;
  h->rank = (long long)rank;
  h->emb = (long long)emb_rank;
  h->n_w = n_w;
  h->hsel = rows;
  h->identity = identity;
  *out = h;
  return RG_OK;
}

void rg_buckler_encode_round_destroy(rg_bencode* h) { delete h; }

// scratch: the InvNTT's output (and, with a gather, its input) [n_proofs][n_sel][rank][L]
size_t rg_buckler_prove_encode_round_scratch_bytes(const rg_bencode* h, size_t n_proofs) {
  if (!h || n_proofs == 0 || !er_proofs_ok(h, n_proofs)) return 0;
  return n_proofs * h->hsel.size() * (size_t)h->rank * h->f.L * 8;
}

rg_status rg_buckler_prove_encode_round_dev(const rg_bencode* h, size_t n_proofs, const uint64_t* d_w,
                                            const uint64_t* d_rand, uint64_t* d_wecd, uint64_t* d_com,
                                            uint64_t* d_scratch, void* stream) {
  RG_TRY(er_check(h, n_proofs, d_w, d_rand, d_wecd, d_com));
  if (n_proofs == 0) return RG_OK;
  if (!d_scratch) return er_invalid("NULL scratch");
  if (d_scratch == d_w || d_scratch == d_rand || d_scratch == d_wecd || d_scratch == d_com)
    return er_invalid("two buffers alias");
  RG_TRY(ensure_table(h->mu, h->uploaded, h->sel, h->hsel));  // first use uploads
  hipStream_t st = as_stream(stream);
  const uint64_t* in = d_w;  // sel = 0 .. n_w - 1: the table is [n_proofs * n_w][rank][L] as it stands
  if (!h->identity) {
    RG_TRY(dispatch_limbs(h->f.L, [&](auto Lc) { return gather_L<Lc()>(h, n_proofs, d_scratch, d_w, st); }));
    in = d_scratch;
  }
  RG_TRY(rg_ntt_inv_dev(h->enc, d_scratch, in, n_proofs * h->hsel.size(), stream));
  return dispatch_limbs(
      h->f.L, [&](auto Lc) { return embed_round_L<Lc()>(h, n_proofs, d_wecd, d_com, d_scratch, d_rand, st); });
}

rg_status rg_buckler_prove_encode_round(const rg_bencode* h, size_t n_proofs, const uint64_t* w, const uint64_t* rand,
                                        uint64_t* wecd, uint64_t* com) {
  RG_TRY(er_check(h, n_proofs, w, rand, wecd, com));
  if (n_proofs == 0) return RG_OK;
  const size_t e = (size_t)h->f.L * 8, np = n_proofs, ns = h->hsel.size();
  DevBuf dw, dr, de, dc, dscr;
  RG_TRY(dw.upload(w, np * h->n_w * (size_t)h->rank * e));
  if (rand) RG_TRY(dr.upload(rand, np * ns * e));
  RG_TRY(de.upload(wecd, np * h->n_w * (size_t)h->emb * e));  // the rows outside sel stay as they are
  if (com) RG_TRY(dc.alloc(np * ns * (size_t)(h->rank + 1) * e));
  RG_TRY(dscr.alloc(rg_buckler_prove_encode_round_scratch_bytes(h, np)));
  RG_TRY(rg_buckler_prove_encode_round_dev(h, np, dw.as<uint64_t>(), rand ? dr.as<uint64_t>() : nullptr,
                                           de.as<uint64_t>(), com ? dc.as<uint64_t>() : nullptr, dscr.as<uint64_t>(),
                                           nullptr));
  RG_TRY(de.download(wecd, np * h->n_w * (size_t)h->emb * e));
  if (com) RG_TRY(dc.download(com, np * ns * (size_t)(h->rank + 1) * e));
  return RG_OK;
}

}  // extern "C"
