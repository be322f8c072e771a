// buckler_verify.hip -- what buckler.Verifier.Verify computes after the transcript
// (buckler/verifier.go:178-315), for gfx950: the evaluations of the verifier's own vectors and the
// decision of arithCheck, linCheck and sumCheck, enqueued by ONE call that leaves one verdict word.
//   * rank-sized stage, all on kernels that exist: the power vector of linCheckConst
//     (verifier.go:258-262), every checker's TransposeTo of it (verifier.go:273), the public
//     witnesses beside them, ONE batched cyclic InvNTT at the witness rank (Encode: EncodeTo
//     writes zeros above `rank`, encoder.go:32-38, and zeros add nothing to Evaluate, so the
//     embedding rank never appears) and ONE batched Evaluate at evalPoint.
//   * verify_decide_kernel<L>: one workgroup that holds every scalar of verifier.go:178-179,
//     219-315 -- vanishEval, the remLo shift, evalCircuit on scalars for both constraint lists, the
//     linear check's chain, the five comparisons -- so no field element goes to the host between
//     the stages.
//   * a batch of proofs of one handle (rg_buckler_verify_checks_multi_dev): the same stages over
//     scratch laid out [vector][proof][rank] -- one power table of every proof's linCheckConst, each
//     checker's transpose over all proofs (a projection checker with each proof's own matrix), the
//     public witnesses placed by place_pw_kernel, ONE InvNTT, ONE Evaluate with a point per proof and
//     ONE verify_decide_kernel launch with a workgroup per proof: the launch count has no n_proofs.
// Every value is a canonical Montgomery residue (field.hpp), so a sum or product regrouped exactly
// in the field has the reference's limbs.  Three regroupings are used, each an identity of the field:
//   sum_c (bc * ev_c)                    = bc * sum_c ev_c                 (evalCircuit, one bc for all c)
//   Horner  e = e bc + t_k, k < n; e bc + m = sum_k t_k bc^(n-k) + m         (linCheck's chain)
//   (bc * S) * bc                        = S * bc^2                         (sumCheck's second scale)
#include <string>

#include "buckler_impl.hpp"
#include "common.hpp"
#include "field.hpp"
#include "ntt_plan.hpp"

struct rg_bverifier {
  const rg_ntt* enc = nullptr;  // cyclic at the witness rank (borrowed)
  const rg_lincheck* lin = nullptr;
  const rg_circuit* arith = nullptr;
  const rg_circuit* sum = nullptr;
  long long rank = 0, jindo_rank = 0;
  size_t w_cnt = 0, n_pw = 0, n_evals = 0;
  size_t n_lin_vec = 0;  // 1 + n_chk with a linear check, else 0
  // pf.Evals as verifier.go:120-214 walks roundComIdx (-1: absent)
  int i_lin_mask = -1, i_sum_mask = -1, i_arith_quo = -1, i_lin_quo = -1, i_sum_quo = -1;
};

namespace rg {

constexpr int kDecideLanes = 256;
enum { S_VANISH = 0, S_SHIFT, S_BC2, S_CIRC0, S_CIRC1, S_LIN, S_P0, S_COUNT = S_P0 + 9 };

template <int L>
struct DecideArgs {
  FieldParams<L> F;
  Elem<L> one;
  CircProg circ[2];  // arithmetic, sum check (nc < 0: the check is absent)
  const uint32_t* pair_off;  // the rg_lincheck program (nullptr: no linear check)
  const uint32_t* pairs;
  int n_chk, n_pairs;
  const uint64_t* evals;      // pf.Evals [n_evals][L]
  const uint64_t* ev;         // linCheckEval | linCheckTrEval [n_chk] | pwEvals [n_pw]
  const uint64_t* chal;       // evalPoint, arithBatchConst, linCheckBatchConst, linCheckConst, sumCheckBatchConst
  const uint64_t* mask_sums;  // LinCheckMaskSum, SumCheckMaskSum
  uint64_t* verdict;
  uint64_t* sides;   // [8][L] or nullptr
  uint64_t* pw_out;  // [n_pw][L] or nullptr
  unsigned long long rank, shift_exp;
  int n_lin_vec, n_pw;
  int i_lin_mask, i_sum_mask, i_arith_quo, i_lin_quo, i_sum_quo;
  // Workgroup p decides proof p.  Words from one proof's evals, challenges, mask sums, sides and
  // pw_out to the next proof's, and from one vector's evaluation in `ev` to the next vector's of the
  // same proof (`ev` is [vector][proof][L]; proof p's first is at ev + p L).  The verdict stride is 1.
  unsigned long long evals_stride, chal_stride, mask_stride, sides_stride, pw_out_stride, ev_stride;
};

// The sum of every lane's acc, folded through LDS in a fixed tree (lane i takes i + s for s = 128,
// 64, ..., 1; canonical f_add, no atomics), left in dst by lane 0.  Called by all lanes.
template <int L>
__device__ __forceinline__ void block_sum(uint64_t* red, uint64_t* dst, const uint64_t* acc, const FieldParams<L>& F) {
  const int tid = threadIdx.x;
  el_copy<L>(red + tid * L, acc);
  __syncthreads();
#pragma unroll 1
  for (int s = kDecideLanes / 2; s > 0; s >>= 1) {
    if (tid < s) {
      uint64_t a[L], b[L];
      el_copy<L>(a, red + tid * L);
      el_copy<L>(b, red + (tid + s) * L);
      f_add<L>(a, a, b, F);
      el_copy<L>(red + tid * L, a);
    }
    __syncthreads();
  }
  if (tid == 0) el_copy<L>(dst, red);
  __syncthreads();
}

template <int L>
__global__ __launch_bounds__(kDecideLanes) void verify_decide_kernel(DecideArgs<L> a) {
  __shared__ uint64_t red[kDecideLanes * L];
  __shared__ uint64_t slot[S_COUNT * L];
  __shared__ uint32_t bits[3];
  const int tid = threadIdx.x;
  const bool has_a = a.circ[0].nc >= 0, has_l = a.pair_off != nullptr, has_s = a.circ[1].nc >= 0;
  const size_t proof = blockIdx.x;
  a.evals += proof * a.evals_stride;
  a.ev += proof * L;
  a.chal += proof * a.chal_stride;
  a.mask_sums += proof * a.mask_stride;
  a.verdict += proof;
  if (a.sides) a.sides += proof * a.sides_stride;
  if (a.pw_out) a.pw_out += proof * a.pw_out_stride;
  const uint64_t* x = a.chal;
  const uint64_t* pw_ev = a.ev + (size_t)a.n_lin_vec * a.ev_stride;

  // ---- the powers (bignum.Exp).  A lane's tasks: first, on lanes 64, 128 and 192 only,
  // evalPoint^rank - 1, evalPoint^(jindo_rank - (rank - 1)) or sumCheckBatchConst^2 -- one wave
  // each, so the three chains of squarings run on three SIMDs and a wave skips the multiply of a
  // clear exponent bit; then its pairs k = tid, tid + 256, ...: the pair's term (verifier.go:276-283)
  // times bc^(n_pairs - k).  Nothing waits here: wave 0 goes on to the constraints meanwhile.
  uint64_t acc_l[L];
  el_zero<L>(acc_l);
  {
    const int n_pairs = has_l ? a.n_pairs : 0;
    const int special = ((tid & 63) == 0 && tid) ? (tid >> 6) - 1 : -1;  // 0, 1, 2
#pragma unroll 1
    for (int t = tid - kDecideLanes; t < n_pairs; t += kDecideLanes) {
      if (t < 0 && special < 0) continue;
      const uint64_t* base = a.chal + 2 * L;  // linCheckBatchConst
      unsigned long long e = (unsigned long long)(n_pairs - t);
      if (t < 0) {
        base = special == 2 ? a.chal + 4 * L : x;
        e = special == 0 ? a.rank : (special == 1 ? a.shift_exp : 2ull);
      }
      uint64_t r[L], sq[L];
      el_copy<L>(r, a.one.v);  // r = SetUint64(1)
      el_copy<L>(sq, base);
#pragma unroll 1
      for (; e; e >>= 1) {
        if (e & 1) f_mul<L>(r, r, sq, a.F);
        if (e > 1) f_mul<L>(sq, sq, sq, a.F);
      }
      if (t >= 0) {
        int c = 0;
        while (c + 1 < a.n_chk && (uint32_t)t >= a.pair_off[c + 1]) ++c;  // the pair's checker
        uint64_t term[L], u[L], w[L];
        el_copy<L>(u, a.ev + (size_t)(1 + c) * a.ev_stride);
        el_copy<L>(w, a.evals + (size_t)a.pairs[2 * t + 1] * L);
        f_mul<L>(term, u, w, a.F);  // term.Mul(linCheckTrEval, wIn)
        el_copy<L>(u, a.ev);
        el_copy<L>(w, a.evals + (size_t)a.pairs[2 * t] * L);
        f_mul<L>(u, u, w, a.F);       // termMul.Mul(linCheckEval, wOut)
        f_sub<L>(term, term, u, a.F);
        f_mul<L>(term, term, r, a.F);
        f_add<L>(acc_l, acc_l, term, a.F);
      } else {
        if (special == 0) f_sub<L>(r, r, a.one.v, a.F);  // vanishEval.Sub(vanishEval, SetUint64(1))
        el_copy<L>(slot + (S_VANISH + special) * L, r);
      }
    }
  }

  // ---- evalCircuit on scalars (verifier.go:219-240): the constraints of both lists over lanes, one
  // walk; the common batchConst is applied to the folded sums below
  uint64_t acc_a[L], acc_s[L];
  el_zero<L>(acc_a);
  el_zero<L>(acc_s);
  {
    const int nc0 = has_a ? a.circ[0].nc : 0, nc1 = has_s ? a.circ[1].nc : 0;
#pragma unroll 1
    for (int c = tid; c < nc0 + nc1; c += kDecideLanes) {
      const bool second = c >= nc0;
      const uint32_t* term_off = second ? a.circ[1].term_off : a.circ[0].term_off;
      const int* pw_idx = second ? a.circ[1].pw_idx : a.circ[0].pw_idx;
      const uint32_t* wit_off = second ? a.circ[1].wit_off : a.circ[0].wit_off;
      const uint32_t* wit = second ? a.circ[1].wit : a.circ[0].wit;
      const uint64_t* coeffs = second ? a.circ[1].coeffs : a.circ[0].coeffs;
      const int cc = second ? c - nc0 : c;
#pragma unroll 1
      for (uint32_t t = term_off[cc]; t < term_off[cc + 1]; ++t) {
        uint64_t term[L], y[L];
        el_copy<L>(term, coeffs + (size_t)t * L);  // term.Set(c.coeffs[i])
        const int pi = pw_idx[t];
        const uint32_t k0 = wit_off[t], k1 = wit_off[t + 1];
#pragma unroll 1
        for (long long k = (pi >= 0) ? (long long)k0 - 1 : (long long)k0; k < (long long)k1; ++k) {
          const uint64_t* src = (k < (long long)k0) ? pw_ev + (size_t)pi * a.ev_stride : a.evals + (size_t)wit[k] * L;
          el_copy<L>(y, src);
          f_mul<L>(term, term, y, a.F);  // term.Mul(term, pwEvals[...]) / term.Mul(term, evals[...])
        }
        if (second) f_add<L>(acc_s, acc_s, term, a.F);  // eval.Add(eval, term); out.Add(out, eval)
        else f_add<L>(acc_a, acc_a, term, a.F);
      }
    }
  }

  // ---- the folds, for the checks the handle has (uniform branches)
  if (has_a) block_sum<L>(red, slot + S_CIRC0 * L, acc_a, a.F);
  if (has_s) block_sum<L>(red, slot + S_CIRC1 * L, acc_s, a.F);
  if (has_l) block_sum<L>(red, slot + S_LIN * L, acc_l, a.F);
  __syncthreads();

  // ---- the nine products of the three checks, one per lane
  if (tid < 9) {
    const uint64_t *p = nullptr, *q = nullptr;
    const uint64_t* van = slot + S_VANISH * L;
    const uint64_t* sh = slot + S_SHIFT * L;
    switch (tid) {
      case 0: if (has_a) p = a.chal + L, q = slot + S_CIRC0 * L; break;                       // eval of arithCheck
      case 1: if (has_a) p = a.evals + (size_t)a.i_arith_quo * L, q = van; break;             // test.Mul(quoEval, vanishEval)
      case 2: if (has_l) p = sh, q = a.evals + (size_t)(a.i_lin_quo + 1) * L; break;          // remLoShiftEval
      case 3: if (has_l) p = a.evals + (size_t)a.i_lin_quo * L, q = van; break;
      case 4: if (has_l) p = a.evals + (size_t)(a.i_lin_quo + 1) * L, q = x; break;           // rem.Mul(remLoEval, evalPoint)
      case 5: if (has_s) p = sh, q = a.evals + (size_t)(a.i_sum_quo + 1) * L; break;
      case 6: if (has_s) p = a.evals + (size_t)a.i_sum_quo * L, q = van; break;
      case 7: if (has_s) p = a.evals + (size_t)(a.i_sum_quo + 1) * L, q = x; break;
      default: if (has_s) p = slot + S_CIRC1 * L, q = slot + S_BC2 * L; break;                // evalCircuit * bc, * bc
    }
    uint64_t u[L], w[L];
    el_zero<L>(u);
    if (p) {
      el_copy<L>(u, p);
      el_copy<L>(w, q);
      f_mul<L>(u, u, w, a.F);
    }
    el_copy<L>(slot + (S_P0 + tid) * L, u);
  }
  __syncthreads();

  // ---- the comparisons: lane 0 arithCheck, lane 1 linCheck, lane 2 sumCheck; each writes its sides
  if (tid < 3) {
    uint64_t s0[L], ev[L], test[L], y[L];
    uint32_t b = 0;
    el_zero<L>(s0);
    el_zero<L>(ev);
    el_zero<L>(test);
    if (tid == 0 && has_a) {
      el_copy<L>(ev, slot + S_P0 * L);
      el_copy<L>(test, slot + (S_P0 + 1) * L);
      b = el_neq<L>(ev, test) ? 1u : 0u;  // arithCheck: eval.Cmp(test)
    }
    if (tid != 0 && (tid == 1 ? has_l : has_s)) {
      const int quo = tid == 1 ? a.i_lin_quo : a.i_sum_quo;
      const int mask = tid == 1 ? a.i_lin_mask : a.i_sum_mask;
      const int p0 = tid == 1 ? S_P0 + 2 : S_P0 + 5;
      el_copy<L>(s0, slot + p0 * L);
      el_copy<L>(y, a.evals + (size_t)(quo + 2) * L);
      b = el_neq<L>(y, s0) ? (tid == 1 ? 2u : 8u) : 0u;  // remHiEval.Cmp(remLoShiftEval)
      el_copy<L>(ev, tid == 1 ? slot + S_LIN * L : slot + (S_P0 + 8) * L);
      el_copy<L>(y, a.evals + (size_t)mask * L);
      f_add<L>(ev, ev, y, a.F);  // eval.Add(eval, maskEval)
      el_copy<L>(test, slot + (p0 + 1) * L);
      el_copy<L>(y, slot + (p0 + 2) * L);
      f_add<L>(test, test, y, a.F);  // test.Add(test, rem)
      el_copy<L>(y, a.mask_sums + (size_t)(tid - 1) * L);
      f_add<L>(test, test, y, a.F);  // test.Add(test, maskSum)
      b |= el_neq<L>(ev, test) ? (tid == 1 ? 4u : 16u) : 0u;
    }
    bits[tid] = b;
    if (a.sides) {
      uint64_t* o = a.sides + (size_t)(tid == 0 ? 0 : (tid == 1 ? 2 : 5)) * L;
      if (tid != 0) {
        el_copy<L>(o, s0);
        o += L;
      }
      el_copy<L>(o, ev);
      el_copy<L>(o + L, test);
    }
  }
  if (a.pw_out)
    for (int i = tid; i < a.n_pw * L; i += kDecideLanes) a.pw_out[i] = pw_ev[(size_t)(i / L) * a.ev_stride + i % L];
  __syncthreads();
  if (tid == 0) a.verdict[0] = (uint64_t)(bits[0] | bits[1] | bits[2]);
}

static rg_status bv_invalid(const std::string& why) {
  set_last_error("buckler verifier: " + why);
  return RG_ERR_INVALID;
}

template <int L>
static rg_status decide_L(const rg_bverifier* v, size_t n_proofs, const uint64_t* evals, const uint64_t* ev,
                          const uint64_t* chal, const uint64_t* mask_sums, uint64_t* verdict, uint64_t* sides,
                          uint64_t* pw_out, hipStream_t st) {
  const rg_field* f = ntt_field(v->enc);
  DecideArgs<L> a;
  a.F = field_params<L>(f);
  a.one = elem<L>(f->one);
  a.circ[0] = circ_prog(v->arith);
  a.circ[1] = circ_prog(v->sum);
  const LinProg lp = lin_prog(v->lin);
  a.pair_off = lp.pair_off;
  a.pairs = lp.pairs;
  a.n_chk = lp.n_chk;
  a.n_pairs = lp.n_pairs;
  a.evals = evals;
  a.ev = ev;
  a.chal = chal;
  a.mask_sums = mask_sums;
  a.verdict = verdict;
  a.sides = sides;
  a.pw_out = pw_out;
  a.rank = (unsigned long long)v->rank;
  a.shift_exp = (unsigned long long)(v->jindo_rank - (v->rank - 1));
  a.n_lin_vec = (int)v->n_lin_vec;
  a.n_pw = (int)v->n_pw;
  a.i_lin_mask = v->i_lin_mask;
  a.i_sum_mask = v->i_sum_mask;
  a.i_arith_quo = v->i_arith_quo;
  a.i_lin_quo = v->i_lin_quo;
  a.i_sum_quo = v->i_sum_quo;
  a.evals_stride = (unsigned long long)v->n_evals * L;
  a.chal_stride = 5 * L;
  a.mask_stride = 2 * L;
  a.sides_stride = 8 * L;
  a.pw_out_stride = (unsigned long long)v->n_pw * L;
  a.ev_stride = (unsigned long long)n_proofs * L;
  hipLaunchKernelGGL(verify_decide_kernel<L>, dim3((unsigned)n_proofs), dim3(kDecideLanes), 0, st, a);
  return check_launch("buckler verify decide");
}

// scratch (elements of L words): vec [n_vec][rank] | ev [n_vec] | the batched evaluate's scratch
static size_t bv_n_vec(const rg_bverifier* v) { return v->n_lin_vec + v->n_pw; }

// ---- a batch of proofs ---------------------------------------------------------------------------
// The public witnesses of every proof beside the linear check's vectors: pw [proof][j][rank][L] ->
// out [j][proof][rank][L], a word per lane, both sides read and written in runs.
__global__ __launch_bounds__(256) void place_pw_kernel(uint64_t* out, const uint64_t* pw, unsigned long long vec_words,
                                                       unsigned long long n_pw, unsigned long long n_proofs) {
  const unsigned long long gid = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= vec_words * n_pw * n_proofs) return;
  const unsigned long long w = gid % vec_words, pj = gid / vec_words;  // pj = proof * n_pw + j
  const unsigned long long p = pj / n_pw, j = pj % n_pw;
  out[(j * n_proofs + p) * vec_words + w] = pw[gid];
}

static bool bv_has_proj(const rg_bverifier* v) {
  if (v->lin)
    for (const rg_linchecker* c : v->lin->chk)
      if (c->kind == RG_CHK_PROJ) return true;
  return false;
}

// n_proofs the batch entry takes: RG_BK_MULTI_MAX_PROOFS (a proof per blockIdx.y of the power-table
// and projection kernels), and few enough that the n_proofs * n_vec vectors are at most 2^30
// polynomials (the batched evaluate's range) of at most 2^39 words in all: a lane per word fits a
// 1-D grid of 256-lane blocks and every byte offset stays far below 2^63
static bool bv_proofs_ok(const rg_bverifier* v, size_t n_proofs) {
  if (n_proofs > RG_BK_MULTI_MAX_PROOFS) return false;
  const size_t polys = bv_n_vec(v) * n_proofs;  // < 2^22 * 2^16
  return polys <= ((size_t)1 << 30) && polys * (size_t)v->rank <= (((size_t)1 << 39) / ntt_field(v->enc)->L);
}

// scratch of the batch entry (elements of L words): vec [n_vec][n_proofs][rank] | ev [n_vec][n_proofs] |
// the evaluate's scratch | the packed projection matrices [n_proofs][rank] x 16 bytes (with a
// projection checker)
static size_t bv_multi_eval_scratch(const rg_bverifier* v, size_t n_proofs) {
  return rg_poly_evaluate_multi_scratch_bytes(ntt_field(v->enc), (size_t)v->rank, bv_n_vec(v) * n_proofs, n_proofs);
}

}  // namespace rg

using namespace rg;

extern "C" {

rg_status rg_buckler_verifier_create(const rg_ntt* enc_plan, size_t jindo_rank, size_t w_cnt, size_t n_pw,
                                     const rg_lincheck* lin, const rg_circuit* arith, const rg_circuit* sum,
                                     rg_bverifier** out) {
  if (!out) return bv_invalid("NULL out");
  *out = nullptr;
  if (!enc_plan) return bv_invalid("NULL encoder plan");
  if (ntt_negacyclic(enc_plan)) return bv_invalid("the encoder's plan is cyclic (encoder.go:15-20)");
  if (!lin && !arith && !sum) return bv_invalid("no check: lin, arith and sum are all NULL");
  const rg_field* f = ntt_field(enc_plan);
  const long long rank = rg_ntt_rank(enc_plan);
  if (!limbs_supported(f->L)) {
    set_last_error("buckler verifier: no kernel for " + std::to_string(f->L) + " limbs (1, 2, 4, 7, 14)");
    return RG_ERR_UNSUPPORTED;
  }
  if (jindo_rank + 1 < (size_t)rank || jindo_rank > ((size_t)1 << 40))
    return bv_invalid("jindo_rank " + std::to_string(jindo_rank) + " < rank - 1 or out of range");
  if (w_cnt > ((size_t)1 << 30) || n_pw > ((size_t)1 << 20)) return bv_invalid("w_cnt or n_pw out of range");
  if (lin) {
    if (rg_ntt_rank(lin->enc) != rank || !same_field(f, ntt_field(lin->enc)))
      return bv_invalid("the linear check's encoder plan has another rank or field");
    if (lin->max_w >= (long long)w_cnt) return bv_invalid("a pair index >= w_cnt");
  }
  const rg_circuit* cs[2] = {arith, sum};
  for (const rg_circuit* c : cs) {
    if (!c) continue;
    if (!same_field(f, &c->f)) return bv_invalid("a circuit of another field");
    if (c->max_w >= (long long)w_cnt) return bv_invalid("a circuit's witness index >= w_cnt");
    if (c->max_pw >= (long long)n_pw) return bv_invalid("a circuit's public-witness index >= n_pw");
  }
  auto v = new rg_bverifier();
  v->enc = enc_plan;
  v->lin = lin;
  v->arith = arith;
  v->sum = sum;
  v->rank = rank;
  v->jindo_rank = (long long)jindo_rank;
  v->w_cnt = w_cnt;
  v->n_pw = n_pw;
  v->n_lin_vec = lin ? 1 + lin->chk.size() : 0;
  size_t i = w_cnt;  // roundComIdx (verifier.go:120)
  if (lin) v->i_lin_mask = (int)i++;
  if (sum) v->i_sum_mask = (int)i++;
  if (arith) v->i_arith_quo = (int)i++;
  if (lin) v->i_lin_quo = (int)i, i += 3;
  if (sum) v->i_sum_quo = (int)i, i += 3;
  v->n_evals = i;
  *out = v;
  return RG_OK;
}

void rg_buckler_verifier_destroy(rg_bverifier* v) { delete v; }

size_t rg_buckler_verifier_n_evals(const rg_bverifier* v) { return v ? v->n_evals : 0; }

size_t rg_buckler_verify_checks_scratch_bytes(const rg_bverifier* v) {
  if (!v) return 0;
  const size_t nv = bv_n_vec(v);
  const rg_field* f = ntt_field(v->enc);
  return nv * ((size_t)v->rank + 1) * f->L * 8 + rg_poly_evaluate_batch_scratch_bytes(f, (size_t)v->rank, nv);
}

rg_status rg_buckler_verify_checks_dev(const rg_bverifier* v, const uint64_t* d_evals, const uint64_t* d_pw,
                                       const uint64_t* d_chal, const uint64_t* d_mask_sums, uint64_t* d_verdict,
                                       uint64_t* d_sides, uint64_t* d_pw_evals, uint64_t* d_scratch, void* stream) {
  if (!v) return bv_invalid("NULL handle");
  if (!d_evals || !d_chal || !d_verdict) return bv_invalid("NULL evals, challenges or verdict");
  if ((v->lin || v->sum) && !d_mask_sums) return bv_invalid("NULL mask sums");
  if ((d_pw == nullptr) != (v->n_pw == 0)) return bv_invalid("d_pw is NULL iff n_pw = 0");
  const size_t nv = bv_n_vec(v);
  if (nv && !d_scratch) return bv_invalid("NULL scratch");
  const void* bufs[] = {d_evals, d_pw, d_chal, d_mask_sums, d_verdict, d_sides, d_pw_evals, d_scratch};
  for (size_t i = 0; i < sizeof bufs / sizeof bufs[0]; ++i)
    for (size_t j = i + 1; j < sizeof bufs / sizeof bufs[0]; ++j)
      if (bufs[i] && bufs[i] == bufs[j]) return bv_invalid("two buffers alias");
  if (v->lin)
    for (const rg_linchecker* c : v->lin->chk)
      if (c->kind == RG_CHK_PROJ && !c->bits_set) return bv_invalid("a projection checker whose matrix was never set");
  const rg_field* f = ntt_field(v->enc);
  const size_t L = f->L, rank = (size_t)v->rank;
  hipStream_t st = as_stream(stream);
  uint64_t* vec = d_scratch;
  uint64_t* ev = vec + nv * rank * L;
  uint64_t* ev_scr = ev + nv * L;
  if (v->lin) {
    RG_TRY(rg_buckler_powers_dev(f, d_chal + 3 * L, rank, vec, stream));  // linCheckVec (verifier.go:258-262)
    for (size_t c = 0; c < v->lin->chk.size(); ++c)                       // tr.TransposeTo(linCheckVecTr, linCheckVec)
      RG_TRY(rg_buckler_checker_transpose_dev(v->lin->chk[c], vec + (1 + c) * rank * L, vec, 1, stream));
  }
  if (v->n_pw)  // the public witnesses beside them: one batch for the InvNTT
    RG_HIP(hipMemcpyAsync(vec + v->n_lin_vec * rank * L, d_pw, v->n_pw * rank * L * 8, hipMemcpyDeviceToDevice, st));
  if (nv) {
    RG_TRY(rg_ntt_inv_dev(v->enc, vec, vec, nv, stream));  // Encode: InvNTTTo(pOut.Coeffs[:rank], v[:rank])
    RG_TRY(rg_poly_evaluate_batch_dev(f, vec, rank, rank, nv, d_chal, ev, ev_scr, stream));  // Evaluate(evalPoint)
  }
  return dispatch_limbs(f->L, [&](auto Lc) {
    return decide_L<Lc()>(v, 1, d_evals, ev, d_chal, d_mask_sums, d_verdict, d_sides, d_pw_evals, st);
  });
}

rg_status rg_buckler_verify_checks(const rg_bverifier* v, const uint64_t* evals, const uint64_t* pw,
                                   const uint64_t* chal, const uint64_t* mask_sums, uint64_t* verdict,
                                   uint64_t* sides, uint64_t* pw_evals) {
  if (!v) return bv_invalid("NULL handle");
  if (!evals || !chal || !verdict) return bv_invalid("NULL evals, challenges or verdict");
  if ((v->lin || v->sum) && !mask_sums) return bv_invalid("NULL mask sums");
  if ((pw == nullptr) != (v->n_pw == 0)) return bv_invalid("pw is NULL iff n_pw = 0");
  const size_t e = (size_t)ntt_field(v->enc)->L * 8;
  DevBuf dev, dpw, dch, dms, dvd, dsd, dpe, dscr;
  RG_TRY(dev.upload(evals, v->n_evals * e));
  if (v->n_pw) RG_TRY(dpw.upload(pw, v->n_pw * (size_t)v->rank * e));
  RG_TRY(dch.upload(chal, 5 * e));
  if (mask_sums) RG_TRY(dms.upload(mask_sums, 2 * e));
  RG_TRY(dvd.alloc(8));
  if (sides) RG_TRY(dsd.alloc(8 * e));
  if (pw_evals && v->n_pw) RG_TRY(dpe.alloc(v->n_pw * e));
  RG_TRY(dscr.alloc(rg_buckler_verify_checks_scratch_bytes(v)));
  RG_TRY(rg_buckler_verify_checks_dev(v, dev.as<uint64_t>(), dpw.as<uint64_t>(), dch.as<uint64_t>(),
                                      dms.as<uint64_t>(), dvd.as<uint64_t>(), dsd.as<uint64_t>(), dpe.as<uint64_t>(),
                                      dscr.as<uint64_t>(), nullptr));
  RG_TRY(dvd.download(verdict, 8));
  if (sides) RG_TRY(dsd.download(sides, 8 * e));
  if (dpe.p) RG_TRY(dpe.download(pw_evals, v->n_pw * e));
  return RG_OK;
}

// ---- n_proofs proofs of one handle in one call ------------------------------------------------
size_t rg_buckler_verify_checks_multi_scratch_bytes(const rg_bverifier* v, size_t n_proofs) {
  if (!v || n_proofs == 0 || !bv_proofs_ok(v, n_proofs)) return 0;
  const size_t nv = bv_n_vec(v), L = ntt_field(v->enc)->L;
  return nv * n_proofs * ((size_t)v->rank + 1) * L * 8 + bv_multi_eval_scratch(v, n_proofs) +
         (bv_has_proj(v) ? n_proofs * (size_t)v->rank * 16 : 0);
}

// the argument rules both forms share, before any device call
static rg_status bv_multi_check(const rg_bverifier* v, size_t n_proofs, const void* evals, const void* pw,
                                const void* xof, const void* chal, const void* mask_sums, const void* verdict) {
  if (!v) return bv_invalid("NULL handle");
  if (!bv_proofs_ok(v, n_proofs))
    return bv_invalid("n_proofs " + std::to_string(n_proofs) + " is over the limit (RG_BK_MULTI_MAX_PROOFS, 2^39 words)");
  if (n_proofs == 0) return RG_OK;
  if (!evals || !chal || !verdict) return bv_invalid("NULL evals, challenges or verdict");
  if ((v->lin || v->sum) && !mask_sums) return bv_invalid("NULL mask sums");
  if ((pw == nullptr) != (v->n_pw == 0)) return bv_invalid("d_pw is NULL iff n_pw = 0");
  if ((xof == nullptr) == bv_has_proj(v))
    return bv_invalid("d_xof is required with a projection checker in the linear check and NULL without one");
  return RG_OK;
}

rg_status rg_buckler_verify_checks_multi_dev(const rg_bverifier* v, size_t n_proofs, const uint64_t* d_evals,
                                             const uint64_t* d_pw, const uint8_t* d_xof, const uint64_t* d_chal,
                                             const uint64_t* d_mask_sums, uint64_t* d_verdict, uint64_t* d_sides,
                                             uint64_t* d_pw_evals, uint64_t* d_scratch, void* stream) {
  RG_TRY(bv_multi_check(v, n_proofs, d_evals, d_pw, d_xof, d_chal, d_mask_sums, d_verdict));
  if (n_proofs == 0) return RG_OK;
  const size_t nv = bv_n_vec(v);
  if (nv && !d_scratch) return bv_invalid("NULL scratch");
  const void* bufs[] = {d_evals, d_pw, d_xof, d_chal, d_mask_sums, d_verdict, d_sides, d_pw_evals, d_scratch};
  for (size_t i = 0; i < sizeof bufs / sizeof bufs[0]; ++i)
    for (size_t j = i + 1; j < sizeof bufs / sizeof bufs[0]; ++j)
      if (bufs[i] && bufs[i] == bufs[j]) return bv_invalid("two buffers alias");
  const rg_field* f = ntt_field(v->enc);
  const size_t L = f->L, rank = (size_t)v->rank, np = n_proofs;
  hipStream_t st = as_stream(stream);
  uint64_t* vec = d_scratch;  // [n_vec][n_proofs][rank]
  uint64_t* ev = vec + nv * np * rank * L;
  uint64_t* ev_scr = ev + nv * np * L;
  void* bits = reinterpret_cast<char*>(ev_scr) + bv_multi_eval_scratch(v, np);
  if (v->lin) {
    // every proof's linCheckVec (verifier.go:258-262): linCheckConst is challenge 3 of 5
    RG_TRY(rg_buckler_powers_batch_dev(f, d_chal + 3 * L, 5, np, rank, vec, stream));
    for (size_t c = 0; c < v->lin->chk.size(); ++c) {  // tr.TransposeTo(linCheckVecTr, linCheckVec), all proofs
      const rg_linchecker* chk = v->lin->chk[c];
      uint64_t* out = vec + (1 + c) * np * rank * L;
      if (chk->kind == RG_CHK_PROJ)  // the proof's own matrix (prover.go:165-176), not the handle's
        RG_TRY(rg_buckler_checker_transpose_xof_dev(chk, out, vec, np, d_xof, bits, stream));
      else
        RG_TRY(rg_buckler_checker_transpose_dev(chk, out, vec, np, stream));
    }
  }
  if (v->n_pw) {
    const unsigned long long words = (unsigned long long)rank * L;
    hipLaunchKernelGGL(place_pw_kernel, dim3(grid256((long long)(words * v->n_pw * np))), dim3(256), 0, st,
                       vec + v->n_lin_vec * np * rank * L, d_pw, words, (unsigned long long)v->n_pw,
                       (unsigned long long)np);
    RG_TRY(check_launch("buckler verify place pw"));
  }
  if (nv) {
    RG_TRY(rg_ntt_inv_dev(v->enc, vec, vec, nv * np, stream));  // Encode of every vector of every proof
    // vector s of proof p is polynomial s * n_proofs + p: group 1, point p = the proof's evalPoint
    RG_TRY(rg_poly_evaluate_multi_dev(f, vec, rank, rank, nv * np, d_chal, 5, np, 1, ev, ev_scr, stream));
  }
  return dispatch_limbs(f->L, [&](auto Lc) {
    return decide_L<Lc()>(v, np, d_evals, ev, d_chal, d_mask_sums, d_verdict, d_sides, d_pw_evals, st);
  });
}

rg_status rg_buckler_verify_checks_multi(const rg_bverifier* v, size_t n_proofs, const uint64_t* evals,
                                         const uint64_t* pw, const uint8_t* xof, const uint64_t* chal,
                                         const uint64_t* mask_sums, uint64_t* verdict, uint64_t* sides,
                                         uint64_t* pw_evals) {
  RG_TRY(bv_multi_check(v, n_proofs, evals, pw, xof, chal, mask_sums, verdict));
  if (n_proofs == 0) return RG_OK;
  const size_t e = (size_t)ntt_field(v->enc)->L * 8, np = n_proofs;
  DevBuf dev, dpw, dxo, dch, dms, dvd, dsd, dpe, dscr;
  RG_TRY(dev.upload(evals, np * v->n_evals * e));
  if (v->n_pw) RG_TRY(dpw.upload(pw, np * v->n_pw * (size_t)v->rank * e));
  if (xof) RG_TRY(dxo.upload(xof, np * (size_t)v->rank * 32));
  RG_TRY(dch.upload(chal, np * 5 * e));
  if (mask_sums) RG_TRY(dms.upload(mask_sums, np * 2 * e));
  RG_TRY(dvd.alloc(np * 8));
  if (sides) RG_TRY(dsd.alloc(np * 8 * e));
  if (pw_evals && v->n_pw) RG_TRY(dpe.alloc(np * v->n_pw * e));
  RG_TRY(dscr.alloc(rg_buckler_verify_checks_multi_scratch_bytes(v, np)));
  RG_TRY(rg_buckler_verify_checks_multi_dev(v, np, dev.as<uint64_t>(), dpw.as<uint64_t>(), dxo.as<uint8_t>(),
                                            dch.as<uint64_t>(), dms.as<uint64_t>(), dvd.as<uint64_t>(),
                                            dsd.as<uint64_t>(), dpe.as<uint64_t>(), dscr.as<uint64_t>(), nullptr));
  RG_TRY(dvd.download(verdict, np * 8));
  if (sides) RG_TRY(dsd.download(sides, np * 8 * e));
  if (dpe.p) RG_TRY(dpe.download(pw_evals, np * v->n_pw * e));
  return RG_OK;
}

}  // extern "C"
