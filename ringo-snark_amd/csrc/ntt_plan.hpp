// ntt_plan.hpp -- what ntt.hip hands to the runners of the per-limb-count kernel translation units:
// one NttLaunch per direction, filled when the plan is created (route, passes, tables, constants,
// chunk size; ntt.hip finalize()), and the runners that ntt.hip's run() picks among by route.
#pragma once
#include <mutex>

#include "common.hpp"
#include "ntt_route.hpp"

namespace rg {

struct NttLaunch : NttRouting {  // the direction's route, table format and passes (ntt_route.hpp)
  // set by every call
  const uint64_t* in;
  uint64_t* out;
  size_t batch;
  // fixed for the plan and the direction
  bool inv;
  const uint64_t* tw;  // the direction's table in the route's format
  const uint64_t* q;
  uint64_t qinv;
  const uint64_t* nsc;  // N^-1 (rank_inv) and twInv[1] N^-1 in the table's form; *_sh their Shoup quotients
  uint64_t nsc_sh;
  const uint64_t* w1n;
  uint64_t w1n_sh;
  int logN;
  size_t chunk_polys;  // Tiled (two passes), Lazy64: polynomials per pass pair
  bool tile16;         // Lazy64: ROW forward (RP) / COL inverse on 16 points per thread (ntt_route.hpp)
  WidePasses wide;     // Wide: the passes ntt_wide_pass runs, up to three (ntt_route()'s one or two, or
                       // ntt_wide_long()'s: then NttRouting's own list, which holds two, stays empty)
  struct Aux* aux;  // Fast256: the plan's helper stream for the two-half split; else null
};

// a helper stream and the two events that fork it from and join it back to the caller's stream;
// the mutex serialises the fork/join enqueue of concurrent callers, which share the events
struct Aux {
  hipStream_t s = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  std::mutex mu;
  ~Aux() {
    if (s) (void)hipStreamDestroy(s);
    if (fork) (void)hipEventDestroy(fork);
    if (join) (void)hipEventDestroy(join);
  }
};

// the field and kind of a plan (for the operators built on it: buckler.hip)
const rg_field* ntt_field(const rg_ntt* t);
bool ntt_negacyclic(const rg_ntt* t);

// Tiled or Stages (L7, L14: Wide or Stages) by p.route, one unit per limb count
rg_status ntt_run_L1(const NttLaunch& p, hipStream_t st);
rg_status ntt_run_L2(const NttLaunch& p, hipStream_t st);
rg_status ntt_run_L4(const NttLaunch& p, hipStream_t st);
rg_status ntt_run_L7(const NttLaunch& p, hipStream_t st);
rg_status ntt_run_L14(const NttLaunch& p, hipStream_t st);
// Lazy64 (ntt_l1_lazy.hip) and Fast256 (ntt_l4_fast.hip)
rg_status ntt64_run(const NttLaunch& p, hipStream_t st);
rg_status ntt256_run(const NttLaunch& p, hipStream_t st);

}  // namespace rg
