// buckler_impl.hpp -- what the Buckler units share: the handle definitions of the constraint
// program (buckler.hip), the checkers and the linear check (buckler_lin.hip), and the one decode of
// each handle's device program into pointers (circ_prog, lin_prog), read by the prover's passes and
// by the verifier's checks (buckler_verify.hip), and the handle of the prover's batch call
// (buckler_prove.hip).  Every kernel and launcher stays in its unit, and the verifier and the batch
// prover reach them through the `_dev` entries of include/ringo.h.
#pragma once
#include <string.h>

#include <vector>

#include "common.hpp"

struct rg_circuit {
  rg_field f;
  int nc = 0;        // constraints
  long long nt = 0;  // terms
  long long max_w = -1, max_pw = -1;
  rg::DevBuf prog;   // term_off [nc+1] u32 | pw [nt] i32 | wit_off [nt+1] u32 | wit [nwit] u32 | coeffs [nt][L] u64
  size_t off_pw = 0, off_wo = 0, off_wi = 0, off_cf = 0;  // byte offsets into prog
};

enum { RG_CHK_NTT = 0, RG_CHK_AUT = 1, RG_CHK_PROJ = 2, RG_CHK_RECOMPOSE = 3 };

struct rg_linchecker {
  int kind = 0;
  rg_field f;
  long long rank = 0;
  rg_ntt* ntt = nullptr;  // NTT: the negacyclic plan (owned)
  uint64_t scale[16];     //      SetUint64(rank)
  long long idx = 0, idx_inv = 0;  // aut
  int ntt_domain = 0;
  rg::DevBuf bits;  // proj: [rank][4] u32, bit i of column j set <=> proj[i][j] (allocated by set_xof)
  bool bits_set = false;
  long long nb = 0;  // recompose
  rg::DevBuf base;   //            [nb][L]
  ~rg_linchecker() {
    if (ntt) rg_ntt_destroy(ntt);
  }
};

struct rg_lincheck {
  const rg_ntt* enc = nullptr;  // cyclic at rank (borrowed)
  const rg_ntt* emb = nullptr;  // cyclic at emb (borrowed)
  std::vector<const rg_linchecker*> chk;
  int n_pairs = 0;
  long long max_w = -1;
  rg::DevBuf prog;  // pair_off [n_chk+1] u32 | pairs [n_pairs][2] u32 (wOut, wIn)
};

// What Compile fixes for the prover's three checks (buckler_prove.hip); every handle is borrowed
struct rg_bprover {
  const rg_ntt* enc = nullptr;  // cyclic at the witness rank
  const rg_ntt* emb = nullptr;  // cyclic at the embedding rank
  const rg_lincheck* lin = nullptr;
  const rg_circuit* arith = nullptr;
  const rg_circuit* sum = nullptr;
  long long rank = 0, emb_rank = 0, jindo_rank = 0;
  size_t n_w = 0, n_pw = 0;
  size_t n_lin_vec = 0;  // 1 + n_chk with a linear check, else 0
  size_t n_checks = 0;   // the checks present; their evals stand in the order arith, lin, sum
  size_t arith_n_quo = 0, sum_n_quo = 0;  // max_rank - rank (lin's is rank)
  bool has_proj = false;
};

namespace rg {

struct CircProg {  // rg_circuit::prog as device pointers; nc < 0: no circuit (c == nullptr)
  const uint32_t* term_off;
  const int* pw_idx;
  const uint32_t* wit_off;
  const uint32_t* wit;
  const uint64_t* coeffs;
  int nc;
};

inline CircProg circ_prog(const rg_circuit* c) {
  CircProg p;
  memset(&p, 0, sizeof p);
  p.nc = -1;
  if (!c) return p;
  const char* base = c->prog.as<char>();
  p.term_off = reinterpret_cast<const uint32_t*>(base);
  p.pw_idx = reinterpret_cast<const int*>(base + c->off_pw);
  p.wit_off = reinterpret_cast<const uint32_t*>(base + c->off_wo);
  p.wit = reinterpret_cast<const uint32_t*>(base + c->off_wi);
  p.coeffs = reinterpret_cast<const uint64_t*>(base + c->off_cf);
  p.nc = c->nc;
  return p;
}

struct LinProg {  // rg_lincheck::prog as device pointers; all zero: no linear check (lc == nullptr)
  const uint32_t* pair_off;
  const uint32_t* pairs;
  int n_chk, n_pairs;
};

inline LinProg lin_prog(const rg_lincheck* lc) {
  LinProg p = {nullptr, nullptr, 0, 0};
  if (!lc) return p;
  p.n_chk = (int)lc->chk.size();
  p.pair_off = lc->prog.as<uint32_t>();
  p.pairs = p.pair_off + p.n_chk + 1;
  p.n_pairs = lc->n_pairs;
  return p;
}

// What the projection round (buckler_proj.hip) reads of a decomposition handle, whose definition
// stays in buckler_dcmp.hip.  dcmp_view touches no device; dcmp_base_dev gives the base's device
// copy [nb][L] under the handle's first-use rule (the first caller uploads it and waits for the copy).
struct DcmpView {
  const rg_field* f;
  long long nb;
  const uint64_t* one;      // SetInt64(1)
  const uint64_t* neg_one;  // SetInt64(-1)
};
DcmpView dcmp_view(const rg_dcmp* h);
rg_status dcmp_base_dev(const rg_dcmp* h, const uint64_t** d_base);

}  // namespace rg
