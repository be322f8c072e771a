// buckler_prove.hip -- Prover.arithCheck, linCheck and sumCheck (buckler/prover.go:399-485) for a
// batch of proofs of one compiled circuit, enqueued by ONE call whose launch count has no n_proofs,
// for gfx950.  All four challenges are fixed before arithCheck runs (prover.go:242-334), so the call
// does the whole round and leaves, per proof, the seven polynomials Prove commits next.
//   * rank-sized stage, all on kernels that exist and laid out [vector][proof][rank] as in
//     buckler_verify.hip: one power table of every proof's linCheckConst, each checker's transpose
//     over all proofs (a projection checker with each proof's own matrix), ONE batched Encode and
//     ONE batched forward NTT at the embedding rank over n_proofs * (1 + n_chk) vectors.
//   * prove_lin_kernel / prove_circuit_kernel: lin_kernel (buckler_lin.hip) and circuit_kernel
//     (buckler.hip) with the proof as grid row y, the proof's constants read from its row of the
//     challenges, 64-bit offsets, and the trailing ScalarMulTo(eval, eval, batchConst) of linCheck
//     and sumCheck (prover.go:439, 465) applied to the value in registers.  One launch per check.
//   * ONE batched InvNTT at the embedding rank over all n_proofs * n_checks evals.
//   * prove_finish_kernel: mask add, QuoRemByVanishing(eval, rank) and the quo / remLo / remHi /
//     rem0 split of every check of every proof in one launch, a lane per residue class mod rank
//     (the suffix sums of poly_ops.hip's quorem_kernel), so quoPoly and remPoly never reach memory.
// Every value is a canonical Montgomery residue (field.hpp) and every step an exact field
// operation, so the limbs equal those of the single-proof entries and of the reference.
#include <algorithm>
#include <string>

#include "buckler_impl.hpp"
#include "common.hpp"
#include "field.hpp"
#include "ntt_plan.hpp"

namespace rg {

// the proof's row of d_chal [n_proofs][4][L]
enum { PC_ARITH_BC = 0, PC_LIN_BC = 1, PC_LIN_CONST = 2, PC_SUM_BC = 3, PC_COUNT = 4 };

// ---- linCheck's pass (prover.go:427-439) over all proofs -------------------------------------
// ecd [1 + n_chk][n_proofs][emb][L]: vector 0 = NTT(Encode(linCheckVec)), vector 1 + c =
// NTT(Encode(M_c^T linCheckVec)), each of proof blockIdx.y; w [n_proofs][n_w][emb][L]
template <int L>
struct ProveLinArgs {
  FieldParams<L> F;
  const uint32_t* pair_off;
  const uint32_t* pairs;
  const uint64_t* ecd;
  const uint64_t* w;
  const uint64_t* chal;
  uint64_t* out;  // [n_proofs][emb][L]
  unsigned long long emb;
  unsigned long long vec_stride;  // elements from one vector's rows to the next vector's: n_proofs * emb
  unsigned long long w_stride;    // elements from one proof's witnesses to the next proof's: n_w * emb
  int n_chk;
};

template <int L>
__global__ __launch_bounds__(256) void prove_lin_kernel(ProveLinArgs<L> a) {
  const unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.emb) return;
  const unsigned long long p = blockIdx.y;
  const uint64_t* ecd = a.ecd + (p * a.emb + j) * L;
  const uint64_t* w = a.w + (p * a.w_stride + j) * L;
  uint64_t ev[L], bc[L], e0[L];
  el_zero<L>(ev);  // eval := NewPoly(true)
  el_copy<L>(bc, a.chal + (p * PC_COUNT + PC_LIN_BC) * L);
  el_copy<L>(e0, ecd);
  uint32_t k = a.pair_off[0];
  for (int c = 0; c < a.n_chk; ++c) {
    const uint32_t k1 = a.pair_off[c + 1];
    if (k == k1) continue;
    uint64_t tr[L];
    el_copy<L>(tr, ecd + (unsigned long long)(1 + c) * a.vec_stride * L);
    for (; k < k1; ++k) {
      uint64_t term[L], x[L];
      el_copy<L>(x, w + (unsigned long long)a.pairs[2 * k + 1] * a.emb * L);
      f_mul<L>(term, tr, x, a.F);  // MulTo(term, linCheckEcdTr, wIn)
      el_copy<L>(x, w + (unsigned long long)a.pairs[2 * k] * a.emb * L);
      f_mul<L>(x, e0, x, a.F);
      f_sub<L>(term, term, x, a.F);  // MulSubTo(term, linCheckEcd, wOut)
      f_mul<L>(ev, ev, bc, a.F);     // ScalarMulTo(eval, eval, batchConst)
      f_add<L>(ev, ev, term, a.F);   // AddTo(eval, eval, term)
    }
  }
  f_mul<L>(ev, ev, bc, a.F);  // ScalarMulTo(eval, eval, batchConst) (prover.go:439)
  el_copy<L>(a.out + (p * a.emb + j) * L, ev);
}

// ---- evalCircuit (prover.go:355-379) over all proofs -----------------------------------------
template <int L>
struct ProveCircArgs {
  FieldParams<L> F;
  const uint32_t* term_off;
  const int* pw_idx;
  const uint32_t* wit_off;
  const uint32_t* wit;
  const uint64_t* coeffs;
  const uint64_t* w;   // [n_proofs][n_w][emb][L]
  const uint64_t* pw;  // [n_proofs][n_pw][emb][L]
  const uint64_t* chal;
  uint64_t* out;  // [n_proofs][emb][L]
  unsigned long long emb, w_stride, pw_stride;  // strides in elements, proof to proof
  int nc;
  int bc_idx;  // the check's batchConst in the proof's row of chal
  int scale;   // sumCheck: ScalarMulTo(eval, eval, batchConst) after evalCircuit (prover.go:465)
};

template <int L>
__global__ __launch_bounds__(256) void prove_circuit_kernel(ProveCircArgs<L> a) {
  const unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.emb) return;
  const unsigned long long p = blockIdx.y;
  const uint64_t* w = a.w + (p * a.w_stride + j) * L;
  const uint64_t* pw = a.pw + (p * a.pw_stride + j) * L;
  uint64_t acc[L], bc[L];
  el_copy<L>(bc, a.chal + (p * PC_COUNT + (unsigned)a.bc_idx) * L);
  el_zero<L>(acc);  // pOut := NewPoly(true)
  uint32_t t = a.term_off[0];
  for (int c = 0; c < a.nc; ++c) {
    uint64_t ev[L];
    el_zero<L>(ev);  // eval.Clear()
    const uint32_t t1 = a.term_off[c + 1];
    for (; t < t1; ++t) {
      uint64_t term[L], x[L];
      el_copy<L>(term, a.coeffs + (size_t)t * L);  // term.Coeffs[j].Set(c.coeffs[i])
      const int pi = a.pw_idx[t];
      if (pi >= 0) {  // MulTo(term, term, pwEcdNTT[...])
        el_copy<L>(x, pw + (unsigned long long)pi * a.emb * L);
        f_mul<L>(term, term, x, a.F);
      }
      for (uint32_t k = a.wit_off[t]; k < a.wit_off[t + 1]; ++k) {  // MulTo(term, term, wEcdNTT[...])
        el_copy<L>(x, w + (unsigned long long)a.wit[k] * a.emb * L);
        f_mul<L>(term, term, x, a.F);
      }
      f_add<L>(ev, ev, term, a.F);  // AddTo(eval, eval, term)
    }
    f_mul<L>(ev, ev, bc, a.F);    // ScalarMulTo(eval, eval, batchConst)
    f_add<L>(acc, acc, ev, a.F);  // AddTo(pOut, pOut, eval)
  }
  if (a.scale) f_mul<L>(acc, acc, bc, a.F);
  el_copy<L>(a.out + (p * a.emb + j) * L, acc);
}

// ---- the tail of all checks of all proofs (prover.go:401-403, 440-458, 466-484) -----------------
// Check blockIdx.z of proof blockIdx.y, residue class k mod rank per lane.  With e = eval + mask
// (coefficient domain) and top the largest t with k + t rank < emb, QuoRemByVanishing(e, rank) is
// quoPoly[k + (t-1) rank] = sum_{s >= t} e[k + s rank] for 1 <= t <= top, quoPoly[k + top rank] = 0
// and remPoly[k] = e[k] + quoPoly[k]; then quo = quoPoly[:n_quo], remLo[i] = remPoly[i + 1], remHi =
// jindo_rank - (rank - 1) zeros | remLo, rem0 = remPoly[0].  Every output word has one writer.
struct ProveFinCheck {
  const uint64_t* mask;  // [n_proofs][emb][L], nullptr: none (arithCheck)
  uint64_t* quo;         // [n_proofs][n_quo][L]
  uint64_t* rem_lo;      // [n_proofs][rank-1][L], nullptr: the remainder is discarded (arithCheck)
  uint64_t* rem_hi;      // [n_proofs][jindo_rank][L]
  unsigned long long n_quo;
  int rem0_slot;  // 0 lin, 1 sum, -1 none
};

template <int L>
struct ProveFinArgs {
  FieldParams<L> F;
  ProveFinCheck chk[3];
  const uint64_t* eval;  // [n_checks][n_proofs][emb][L]
  uint64_t* rem0;        // [n_proofs][2][L] or nullptr
  unsigned long long rank, emb, jindo_rank, n_proofs;
  int rem0_absent;  // bit s: slot s of rem0 belongs to no check and is zeroed
};

template <int L>
__global__ __launch_bounds__(256) void prove_finish_kernel(ProveFinArgs<L> a) {
  const unsigned long long k = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long p = blockIdx.y;
  const ProveFinCheck c = a.chk[blockIdx.z];
  uint64_t zero[L];
  el_zero<L>(zero);
  if (a.rem0 && blockIdx.z == 0 && k < 2 && ((a.rem0_absent >> k) & 1)) el_copy<L>(a.rem0 + (p * 2 + k) * L, zero);
  const unsigned long long z = a.jindo_rank - (a.rank - 1);
  uint64_t* rem_hi = c.rem_hi ? c.rem_hi + p * a.jindo_rank * L : nullptr;
  if (rem_hi && k < z) el_copy<L>(rem_hi + k * L, zero);
  if (k >= a.rank) return;
  const uint64_t* e = a.eval + ((blockIdx.z * a.n_proofs + p) * a.emb) * L;
  const uint64_t* m = c.mask ? c.mask + p * a.emb * L : nullptr;
  uint64_t* quo = c.quo + p * c.n_quo * L;  // never dereferenced when n_quo = 0
  uint64_t s[L], x[L], y[L];
  el_zero<L>(s);
  const unsigned long long top = (a.emb - 1 - k) / a.rank;
  if (k + top * a.rank < c.n_quo) el_copy<L>(quo + (k + top * a.rank) * L, zero);
  for (unsigned long long t = top; t >= 1; --t) {
    const unsigned long long i = k + t * a.rank;
    el_copy<L>(x, e + i * L);
    if (m) {
      el_copy<L>(y, m + i * L);
      f_add<L>(x, x, y, a.F);  // AddTo(eval, eval, mask)
    }
    f_add<L>(s, s, x, a.F);
    if (i - a.rank < c.n_quo) el_copy<L>(quo + (i - a.rank) * L, s);
  }
  if (!c.rem_lo) return;
  el_copy<L>(x, e + k * L);
  if (m) {
    el_copy<L>(y, m + k * L);
    f_add<L>(x, x, y, a.F);
  }
  f_add<L>(x, x, s, a.F);  // remPoly[k]
  if (k == 0) {
    if (a.rem0) el_copy<L>(a.rem0 + (p * 2 + (unsigned)c.rem0_slot) * L, x);
  } else {
    el_copy<L>(c.rem_lo + (p * (a.rank - 1) + k - 1) * L, x);
    el_copy<L>(rem_hi + (z + k - 1) * L, x);
  }
}

static rg_status bp_invalid(const std::string& why) {
  set_last_error("buckler prover: " + why);
  return RG_ERR_INVALID;
}

template <int L>
static rg_status prove_lin_L(const rg_bprover* p, size_t np, const uint64_t* ecd, const uint64_t* w,
                             const uint64_t* chal, uint64_t* out, hipStream_t st) {
  ProveLinArgs<L> a;
  a.F = field_params<L>(ntt_field(p->enc));
  const LinProg lp = lin_prog(p->lin);
  a.pair_off = lp.pair_off;
  a.pairs = lp.pairs;
  a.ecd = ecd;
  a.w = w;
  a.chal = chal;
  a.out = out;
  a.emb = (unsigned long long)p->emb_rank;
  a.vec_stride = (unsigned long long)np * a.emb;
  a.w_stride = (unsigned long long)p->n_w * a.emb;
  a.n_chk = lp.n_chk;
  hipLaunchKernelGGL(prove_lin_kernel<L>, dim3(grid256(p->emb_rank), (unsigned)np), dim3(256), 0, st, a);
  return check_launch("buckler prove linCheck");
}

template <int L>
static rg_status prove_circuit_L(const rg_bprover* p, const rg_circuit* c, int bc_idx, bool scale, size_t np,
                                 const uint64_t* w, const uint64_t* pw, const uint64_t* chal, uint64_t* out,
                                 hipStream_t st) {
  ProveCircArgs<L> a;
  a.F = field_params<L>(&c->f);
  const CircProg cp = circ_prog(c);
  a.term_off = cp.term_off;
  a.pw_idx = cp.pw_idx;
  a.wit_off = cp.wit_off;
  a.wit = cp.wit;
  a.coeffs = cp.coeffs;
  a.w = w;
  a.pw = pw;
  a.chal = chal;
  a.out = out;
  a.emb = (unsigned long long)p->emb_rank;
  a.w_stride = (unsigned long long)p->n_w * a.emb;
  a.pw_stride = (unsigned long long)p->n_pw * a.emb;
  a.nc = cp.nc;
  a.bc_idx = bc_idx;
  a.scale = scale ? 1 : 0;
  hipLaunchKernelGGL(prove_circuit_kernel<L>, dim3(grid256(p->emb_rank), (unsigned)np), dim3(256), 0, st, a);
  return check_launch("buckler prove evalCircuit");
}

struct ProveOut {  // the call's buffers, device or host
  uint64_t *arith_quo, *lin_quo, *lin_rem_lo, *lin_rem_hi, *sum_quo, *sum_rem_lo, *sum_rem_hi, *rem0;
};

template <int L>
static rg_status prove_finish_L(const rg_bprover* p, size_t np, const uint64_t* eval, const uint64_t* lin_mask,
                                const uint64_t* sum_mask, const ProveOut& o, hipStream_t st) {
  ProveFinArgs<L> a;
  memset(&a, 0, sizeof a);
  a.F = field_params<L>(ntt_field(p->enc));
  int n = 0;
  bool any_rem = false;
  if (p->arith) a.chk[n++] = ProveFinCheck{nullptr, o.arith_quo, nullptr, nullptr, p->arith_n_quo, -1};
  if (p->lin) a.chk[n++] = ProveFinCheck{lin_mask, o.lin_quo, o.lin_rem_lo, o.lin_rem_hi, (unsigned long long)p->rank, 0};
  if (p->sum) a.chk[n++] = ProveFinCheck{sum_mask, o.sum_quo, o.sum_rem_lo, o.sum_rem_hi, p->sum_n_quo, 1};
  any_rem = p->lin || p->sum;
  a.eval = eval;
  a.rem0 = o.rem0;
  a.rank = (unsigned long long)p->rank;
  a.emb = (unsigned long long)p->emb_rank;
  a.jindo_rank = (unsigned long long)p->jindo_rank;
  a.n_proofs = np;
  a.rem0_absent = (p->lin ? 0 : 1) | (p->sum ? 0 : 2);
  const long long lanes = std::max(p->rank, any_rem ? p->jindo_rank - (p->rank - 1) : 0LL);
  hipLaunchKernelGGL(prove_finish_kernel<L>, dim3(grid256(lanes), (unsigned)np, (unsigned)n), dim3(256), 0, st, a);
  return check_launch("buckler prove finish");
}

// n_proofs the call takes: RG_BK_MULTI_MAX_PROOFS (a proof per blockIdx.y), and few enough that the
// batched transforms see at most 2^30 polynomials of at most 2^39 words in all, as the verifier's
// batch call has it (there at the witness rank, here at the embedding rank)
static size_t bp_polys(const rg_bprover* p) { return std::max(p->n_lin_vec, p->n_checks); }

static bool bp_proofs_ok(const rg_bprover* p, size_t n_proofs) {
  if (n_proofs > RG_BK_MULTI_MAX_PROOFS) return false;
  const size_t polys = bp_polys(p) * n_proofs;  // < 2^21 * 2^16
  return polys <= ((size_t)1 << 30) && polys * (size_t)p->emb_rank <= (((size_t)1 << 39) / ntt_field(p->enc)->L);
}

// the argument rules both forms share, before any device call
static rg_status bp_check(const rg_bprover* p, size_t n_proofs, const void* w, const void* pw, const void* xof,
                          const void* chal, const void* lin_mask, const void* sum_mask, const ProveOut& o) {
  if (!p) return bp_invalid("NULL handle");
  if (!bp_proofs_ok(p, n_proofs))
    return bp_invalid("n_proofs " + std::to_string(n_proofs) + " is over the limit (RG_BK_MULTI_MAX_PROOFS, 2^39 words)");
  if (n_proofs == 0) return RG_OK;
  if (!chal) return bp_invalid("NULL challenges");
  if ((w == nullptr) != (p->n_w == 0)) return bp_invalid("d_w is NULL iff n_w = 0");
  if ((pw == nullptr) != (p->n_pw == 0)) return bp_invalid("d_pw is NULL iff n_pw = 0");
  if ((xof == nullptr) == p->has_proj)
    return bp_invalid("d_xof is required with a projection checker in the linear check and NULL without one");
  if (p->lin ? (!lin_mask || !o.lin_quo || !o.lin_rem_lo || !o.lin_rem_hi)
             : (lin_mask || o.lin_quo || o.lin_rem_lo || o.lin_rem_hi))
    return bp_invalid(p->lin ? "a NULL buffer of the linear check" : "a buffer of the absent linear check");
  if (p->sum ? (!sum_mask || !o.sum_rem_lo || !o.sum_rem_hi || (p->sum_n_quo && !o.sum_quo))
             : (sum_mask || o.sum_quo || o.sum_rem_lo || o.sum_rem_hi))
    return bp_invalid(p->sum ? "a NULL buffer of the sum check" : "a buffer of the absent sum check");
  if (p->arith ? (p->arith_n_quo && !o.arith_quo) : o.arith_quo != nullptr)
    return bp_invalid(p->arith ? "a NULL quotient of the arithmetic check" : "a buffer of the absent arithmetic check");
  return RG_OK;
}

}  // namespace rg

using namespace rg;

extern "C" {

rg_status rg_buckler_prover_create(const rg_ntt* enc_plan, const rg_ntt* emb_plan, size_t jindo_rank, size_t n_w,
                                   size_t n_pw, const rg_lincheck* lin, const rg_circuit* arith, size_t arith_max_rank,
                                   const rg_circuit* sum, size_t sum_max_rank, rg_bprover** out) {
  if (!out) return bp_invalid("NULL out");
  *out = nullptr;
  if (!enc_plan || !emb_plan) return bp_invalid("NULL encoder or embedding plan");
  if (ntt_negacyclic(enc_plan) || ntt_negacyclic(emb_plan))
    return bp_invalid("the encoder's and the evaluator's plans are cyclic (encoder.go:15-20)");
  if (!lin && !arith && !sum) return bp_invalid("no check: lin, arith and sum are all NULL");
  const rg_field* f = ntt_field(enc_plan);
  const long long rank = rg_ntt_rank(enc_plan), emb = rg_ntt_rank(emb_plan);
  if (!limbs_supported(f->L)) {
    set_last_error("buckler prover: no kernel for " + std::to_string(f->L) + " limbs (1, 2, 4, 7, 14)");
    return RG_ERR_UNSUPPORTED;
  }
  if (!same_field(f, ntt_field(emb_plan)) || emb < rank)
    return bp_invalid("the embedding plan has another field or a rank below the witness rank");
  if (jindo_rank + 1 < (size_t)rank || jindo_rank > ((size_t)1 << 32))
    return bp_invalid("jindo_rank " + std::to_string(jindo_rank) + " < rank - 1 or out of range");
  if (n_w > ((size_t)1 << 30) || n_pw > ((size_t)1 << 20)) return bp_invalid("n_w or n_pw out of range");
  if (lin) {
    if (rg_ntt_rank(lin->enc) != rank || rg_ntt_rank(lin->emb) != emb || !same_field(f, ntt_field(lin->enc)))
      return bp_invalid("the linear check's plans differ from enc_plan / emb_plan");
    if (lin->max_w >= (long long)n_w) return bp_invalid("a pair index >= n_w");
  }
  const rg_circuit* cs[2] = {arith, sum};
  const size_t max_rank[2] = {arith_max_rank, sum_max_rank};
  for (int i = 0; i < 2; ++i) {
    const rg_circuit* c = cs[i];
    if (!c) continue;
    if (!same_field(f, &c->f)) return bp_invalid("a circuit of another field");
    if (c->max_w >= (long long)n_w) return bp_invalid("a circuit's witness index >= n_w");
    if (c->max_pw >= (long long)n_pw) return bp_invalid("a circuit's public-witness index >= n_pw");
    if (max_rank[i] < (size_t)rank || max_rank[i] > (size_t)emb)
      return bp_invalid(std::string(i ? "sum" : "arith") + "_max_rank " + std::to_string(max_rank[i]) +
                        " is below rank or above the embedding rank");
  }
  auto p = new rg_bprover();
  p->enc = enc_plan;
  p->emb = emb_plan;
  p->lin = lin;
  p->arith = arith;
  p->sum = sum;
  p->rank = rank;
  p->emb_rank = emb;
  p->jindo_rank = (long long)jindo_rank;
  p->n_w = n_w;
  p->n_pw = n_pw;
  p->n_lin_vec = lin ? 1 + lin->chk.size() : 0;
  p->n_checks = (arith ? 1 : 0) + (lin ? 1 : 0) + (sum ? 1 : 0);
  p->arith_n_quo = arith ? arith_max_rank - (size_t)rank : 0;
  p->sum_n_quo = sum ? sum_max_rank - (size_t)rank : 0;
  if (lin)
    for (const rg_linchecker* c : lin->chk)
      if (c->kind == RG_CHK_PROJ) p->has_proj = true;
  *out = p;
  return RG_OK;
}

void rg_buckler_prover_destroy(rg_bprover* p) { delete p; }

// scratch (elements of L words): vec [n_lin_vec][n_proofs][rank] | the Encode's scratch, as large |
// ecd [n_lin_vec][n_proofs][emb] | eval [n_checks][n_proofs][emb] | the packed projection matrices
// [n_proofs][rank] x 16 bytes (with a projection checker)
size_t rg_buckler_prove_checks_scratch_bytes(const rg_bprover* p, size_t n_proofs) {
  if (!p || n_proofs == 0 || !bp_proofs_ok(p, n_proofs)) return 0;
  const size_t L = ntt_field(p->enc)->L, rank = (size_t)p->rank, emb = (size_t)p->emb_rank;
  return n_proofs * (p->n_lin_vec * (2 * rank + emb) + p->n_checks * emb) * L * 8 +
         (p->has_proj ? n_proofs * rank * 16 : 0);
}

rg_status rg_buckler_prove_checks_dev(const rg_bprover* p, size_t n_proofs, const uint64_t* d_w, const uint64_t* d_pw,
                                      const uint8_t* d_xof, const uint64_t* d_chal, const uint64_t* d_lin_mask,
                                      const uint64_t* d_sum_mask, uint64_t* d_arith_quo, uint64_t* d_lin_quo,
                                      uint64_t* d_lin_rem_lo, uint64_t* d_lin_rem_hi, uint64_t* d_sum_quo,
                                      uint64_t* d_sum_rem_lo, uint64_t* d_sum_rem_hi, uint64_t* d_rem0,
                                      uint64_t* d_scratch, void* stream) {
  const ProveOut o = {d_arith_quo, d_lin_quo, d_lin_rem_lo, d_lin_rem_hi, d_sum_quo, d_sum_rem_lo, d_sum_rem_hi, d_rem0};
  RG_TRY(bp_check(p, n_proofs, d_w, d_pw, d_xof, d_chal, d_lin_mask, d_sum_mask, o));
  if (n_proofs == 0) return RG_OK;
  if (!d_scratch) return bp_invalid("NULL scratch");
  const void* bufs[] = {d_w,          d_pw,         d_xof,     d_chal,       d_lin_mask,   d_sum_mask,
                        d_arith_quo,  d_lin_quo,    d_lin_rem_lo, d_lin_rem_hi, d_sum_quo, d_sum_rem_lo,
                        d_sum_rem_hi, d_rem0,       d_scratch};
  for (size_t i = 0; i < sizeof bufs / sizeof bufs[0]; ++i)
    for (size_t j = i + 1; j < sizeof bufs / sizeof bufs[0]; ++j)
      if (bufs[i] && bufs[i] == bufs[j]) return bp_invalid("two buffers alias");
  const rg_field* f = ntt_field(p->enc);
  const size_t L = f->L, rank = (size_t)p->rank, emb = (size_t)p->emb_rank, np = n_proofs, nv = p->n_lin_vec;
  hipStream_t st = as_stream(stream);
  uint64_t* vec = d_scratch;  // [nv][n_proofs][rank]
  uint64_t* enc_scr = vec + nv * np * rank * L;
  uint64_t* ecd = enc_scr + nv * np * rank * L;  // [nv][n_proofs][emb]
  uint64_t* eval = ecd + nv * np * emb * L;      // [n_checks][n_proofs][emb]: arith, lin, sum
  void* bits = eval + p->n_checks * np * emb * L;
  uint64_t* ev = eval;
  if (p->arith) {  // evalCircuit(arithBatchConst, ...) (prover.go:400)
    RG_TRY(dispatch_limbs(f->L, [&](auto Lc) {
      return prove_circuit_L<Lc()>(p, p->arith, PC_ARITH_BC, false, np, d_w, d_pw, d_chal, ev, st);
    }));
    ev += np * emb * L;
  }
  if (p->lin) {
    // every proof's linCheckVec (prover.go:409-413): linCheckConst is challenge 2 of 4
    RG_TRY(rg_buckler_powers_batch_dev(f, d_chal + PC_LIN_CONST * L, PC_COUNT, np, rank, vec, stream));
    for (size_t c = 0; c < p->lin->chk.size(); ++c) {  // tr.TransposeTo(linCheckVecTr, linCheckVec), all proofs
      const rg_linchecker* chk = p->lin->chk[c];
      uint64_t* out = vec + (1 + c) * np * rank * L;
      if (chk->kind == RG_CHK_PROJ)  // the proof's own matrix (prover.go:165-176), not the handle's
        RG_TRY(rg_buckler_checker_transpose_xof_dev(chk, out, vec, np, d_xof, bits, stream));
      else
        RG_TRY(rg_buckler_checker_transpose_dev(chk, out, vec, np, stream));
    }
    // Encode + NTT of every vector of every proof, one batch each (prover.go:420-421, 429-430)
    RG_TRY(rg_buckler_encode_dev(p->enc, emb, ecd, vec, nv * np, nullptr, enc_scr, stream));
    RG_TRY(rg_ntt_fwd_dev(p->emb, ecd, ecd, nv * np, stream));
    RG_TRY(dispatch_limbs(f->L, [&](auto Lc) { return prove_lin_L<Lc()>(p, np, ecd, d_w, d_chal, ev, st); }));
    ev += np * emb * L;
  }
  if (p->sum)  // evalCircuit(sumCheckBatchConst, ...) and the scale (prover.go:464-465)
    RG_TRY(dispatch_limbs(f->L, [&](auto Lc) {
      return prove_circuit_L<Lc()>(p, p->sum, PC_SUM_BC, true, np, d_w, d_pw, d_chal, ev, st);
    }));
  RG_TRY(rg_ntt_inv_dev(p->emb, eval, eval, p->n_checks * np, stream));  // InvNTTTo(eval, eval), every check
  return dispatch_limbs(f->L,
                        [&](auto Lc) { return prove_finish_L<Lc()>(p, np, eval, d_lin_mask, d_sum_mask, o, st); });
}

rg_status rg_buckler_prove_checks(const rg_bprover* p, size_t n_proofs, const uint64_t* w, const uint64_t* pw,
                                  const uint8_t* xof, const uint64_t* chal, const uint64_t* lin_mask,
                                  const uint64_t* sum_mask, uint64_t* arith_quo, uint64_t* lin_quo,
                                  uint64_t* lin_rem_lo, uint64_t* lin_rem_hi, uint64_t* sum_quo, uint64_t* sum_rem_lo,
                                  uint64_t* sum_rem_hi, uint64_t* rem0) {
  const ProveOut o = {arith_quo, lin_quo, lin_rem_lo, lin_rem_hi, sum_quo, sum_rem_lo, sum_rem_hi, rem0};
  RG_TRY(bp_check(p, n_proofs, w, pw, xof, chal, lin_mask, sum_mask, o));
  if (n_proofs == 0) return RG_OK;
  const size_t e = (size_t)ntt_field(p->enc)->L * 8, np = n_proofs, rank = (size_t)p->rank,
               emb = (size_t)p->emb_rank, jr = (size_t)p->jindo_rank;
  DevBuf dw, dpw, dxo, dch, dlm, dsm, dscr, dout[8];
  if (p->n_w) RG_TRY(dw.upload(w, np * p->n_w * emb * e));
  if (p->n_pw) RG_TRY(dpw.upload(pw, np * p->n_pw * emb * e));
  if (xof) RG_TRY(dxo.upload(xof, np * rank * 32));
  RG_TRY(dch.upload(chal, np * PC_COUNT * e));
  if (lin_mask) RG_TRY(dlm.upload(lin_mask, np * emb * e));
  if (sum_mask) RG_TRY(dsm.upload(sum_mask, np * emb * e));
  // the outputs in ProveOut's order: host pointer and elements per proof (0 elements: no buffer)
  uint64_t* const host[8] = {arith_quo, lin_quo, lin_rem_lo, lin_rem_hi, sum_quo, sum_rem_lo, sum_rem_hi, rem0};
  const size_t elems[8] = {p->arith_n_quo, rank, rank - 1, jr, p->sum_n_quo, rank - 1, jr, 2};
  uint64_t* dev[8];
  for (int i = 0; i < 8; ++i) {
    dev[i] = nullptr;
    if (!host[i]) continue;
    RG_TRY(dout[i].alloc(np * elems[i] * e + 8));  // + 8: a pointer even for an output of no elements
    dev[i] = dout[i].as<uint64_t>();
  }
  RG_TRY(dscr.alloc(rg_buckler_prove_checks_scratch_bytes(p, np)));
  RG_TRY(rg_buckler_prove_checks_dev(p, np, dw.as<uint64_t>(), dpw.as<uint64_t>(), dxo.as<uint8_t>(),
                                     dch.as<uint64_t>(), dlm.as<uint64_t>(), dsm.as<uint64_t>(), dev[0], dev[1], dev[2],
                                     dev[3], dev[4], dev[5], dev[6], dev[7], dscr.as<uint64_t>(), nullptr));
  for (int i = 0; i < 8; ++i)
    if (host[i] && elems[i]) RG_TRY(dout[i].download(host[i], np * elems[i] * e));
  return RG_OK;
}

}  // extern "C"
