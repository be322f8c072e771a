// buckler_impl.hpp -- the handle definitions the Buckler units share: the constraint program
// (buckler.hip), the checkers and the linear check (buckler_lin.hip), read by the verifier's checks
// (buckler_verify.hip).  Declarations only: every kernel and launcher stays in its unit, and the
// verifier reaches them through the `_dev` entries of include/ringo.h.
#pragma once
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
