// ntt.hip -- host side of the bigpoly transformers: table construction (the reference's
// generator search and layouts, math/bigpoly/ntt.go:26-95,153-203), plan creation and the C ABI
// (include/ringo.h).  A plan picks its kernels when it is created: finalize() asks ntt_route.hpp
// for each direction's route and passes, reads the experiments build's NttKernel / NttChunkMb
// switches (here and nowhere else), uploads the table format those routes read and creates the
// helper stream if they use one; run() switches on the stored route.  Runners: ntt_plan.hpp.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "common.hpp"
#include "field.hpp"
#include "host_field.hpp"
#include "ntt_plan.hpp"
#include "ntt_tile.hpp"

struct rg_ntt {
  rg_field f;
  int N, logN, negacyclic;
  std::vector<uint64_t> h_tw, h_twinv, h_ninv;  // Montgomery reps, [N][L]
  rg::DevBuf d_tw, d_twinv;                     // the format the plan's routes read (finalize)
  uint64_t nsc[16], nsc_sh, w1n[16], w1n_sh;    // rank_inv and twInv[1] rank_inv in that format
  rg::NttLaunch dir[2];          // forward, inverse: all of a launch but in, out and batch
  std::unique_ptr<rg::Aux> aux;  // Fast256 (either direction): helper stream of ntt256_run's split (ntt_l4_fast.hip)
  int device = 0;                // the tables and the helper stream live on this device
};

namespace rg {

// 2-adicity check shared by both constructors (ntt.go:27-37, 154-164)
static rg_status check_rank(const rg_field* f, int rank) {
  if (rank <= 0 || (rank & (rank - 1))) return RG_ERR_NOT_POW2;
  int logn = 0;
  while ((1 << logn) < rank) ++logn;
  uint64_t pm1[16];
  memcpy(pm1, f->q, 8 * f->L);
  pm1[0] -= 1;  // q odd
  int tz = 0;
  for (int i = 0; i < f->L; ++i) {
    if (pm1[i] == 0) {
      tz += 64;
      continue;
    }
    tz += __builtin_ctzll(pm1[i]);
    break;
  }
  if (tz < logn + 1) return RG_ERR_UNSUPPORTED;  // 2N | q-1
  return RG_OK;
}

// reference generator search: first x = 2, 3, ... with (x^((q-1)/2^lo))^(2^(lo-1)) != 1
static bool find_root(const HostField& H, int log_order, uint64_t* g) {
  const int L = H.L;
  uint64_t e[16];
  memcpy(e, H.q, 8 * L);
  e[0] -= 1;
  for (int s = log_order; s > 0;) {
    int k = s > 63 ? 63 : s;
    for (int i = 0; i < L; ++i) e[i] = (e[i] >> k) | (i + 1 < L ? e[i + 1] << (64 - k) : 0);
    s -= k;
  }
  const uint64_t half[1] = {(uint64_t)1 << (log_order - 1)};
  for (uint64_t xv = 2; xv < (1u << 24); ++xv) {
    uint64_t x[16], gp[16];
    H.from_u64(x, xv);
    H.pow(g, x, e, L);
    H.pow(gp, g, half, 1);
    if (!H.eq(gp, H.one)) return true;
  }
  return false;
}

static void bitrev_perm(std::vector<uint64_t>& v, int n, int L) {  // vec.go:123-137
  for (int i = 1, j = 0; i < n; ++i) {
    int bit = n >> 1;
    for (; j >= bit; bit >>= 1) j -= bit;
    j += bit;
    if (i < j)
      for (int l = 0; l < L; ++l) std::swap(v[(size_t)i * L + l], v[(size_t)j * L + l]);
  }
}

static rg_status build_tables(rg_ntt* t) {
  const int N = t->N, L = t->f.L;
  HostField H(&t->f);
  t->h_tw.assign((size_t)N * L, 0);
  t->h_twinv.assign((size_t)N * L, 0);
  t->h_ninv.assign(L, 0);
  uint64_t g[16], gi[16];
  if (t->negacyclic) {  // ntt.go:167-192: tw[k] = psi^brv(k)
    if (!find_root(H, t->logN + 1, g)) return RG_ERR_UNSUPPORTED;
    H.inverse(gi, g);
    memcpy(&t->h_tw[0], H.one, 8 * L);
    memcpy(&t->h_twinv[0], H.one, 8 * L);
    for (int i = 1; i < N; ++i) {
      H.mul(&t->h_tw[(size_t)i * L], &t->h_tw[(size_t)(i - 1) * L], g);
      H.mul(&t->h_twinv[(size_t)i * L], &t->h_twinv[(size_t)(i - 1) * L], gi);
    }
    bitrev_perm(t->h_tw, N, L);
    bitrev_perm(t->h_twinv, N, L);
  } else if (N >= 2) {  // ntt.go:40-84: tw[m+i] = brv_{N/2}(w^j)[i]
    if (!find_root(H, t->logN, g)) return RG_ERR_UNSUPPORTED;
    H.inverse(gi, g);
    const int h = N / 2;
    std::vector<uint64_t> ref((size_t)h * L), refi((size_t)h * L);
    memcpy(&ref[0], H.one, 8 * L);
    memcpy(&refi[0], H.one, 8 * L);
    for (int i = 1; i < h; ++i) {
      H.mul(&ref[(size_t)i * L], &ref[(size_t)(i - 1) * L], g);
      H.mul(&refi[(size_t)i * L], &refi[(size_t)(i - 1) * L], gi);
    }
    bitrev_perm(ref, h, L);
    bitrev_perm(refi, h, L);
    for (int m = 1; m <= N / 2; m <<= 1)
      for (int i = 0; i < m; ++i) {
        memcpy(&t->h_tw[(size_t)(m + i) * L], &ref[(size_t)i * L], 8 * L);
        memcpy(&t->h_twinv[(size_t)(m + i) * L], &refi[(size_t)i * L], 8 * L);
      }
  }
  uint64_t n[16];
  H.from_u64(n, (uint64_t)N);
  H.inverse(&t->h_ninv[0], n);  // rankInv (ntt.go:86-87, 194-195)
  return RG_OK;
}

// Lazy64: append the lane-ordered ROW last-round copy for ntt16_pass (ntt64.hpp), W words per entry
static void add_row_copy(std::vector<uint64_t>& v, size_t W) {
  const size_t base = v.size();
  v.resize(base + W * 256 * 192);
  for (int r = 0; r < 256; ++r)
    for (int tt = 0; tt < 32; ++tt) {
      for (int g = 0; g < 2; ++g) {
        const size_t src = (size_t)(1 << 14) + 64 * r + 2 * tt + g, dst = (size_t)r * 192 + 32 * g + tt;
        for (size_t c = 0; c < W; ++c) v[base + W * dst + c] = v[W * src + c];
      }
      for (int j = 0; j < 4; ++j) {
        const size_t src = (size_t)(1 << 15) + 128 * r + 4 * tt + j, dst = (size_t)r * 192 + 64 + 32 * j + tt;
        for (size_t c = 0; c < W; ++c) v[base + W * dst + c] = v[W * src + c];
      }
    }
}

// The four table formats, each for both directions.  finalize() has left rank_inv and
// twInv[1] rank_inv in t->nsc / t->w1n as Montgomery reps, the form of every format but Shoup's.

// L = 1, q < 2^63: the plain twiddle (Montgomery rep * R^-1) and its Shoup quotient,
// shoup(v, w) == v * w mod q == mont(v, w*R); the two constants likewise
static rg_status upload_shoup(rg_ntt* t, bool row_copy) {
  const int N = t->N;
  const uint64_t q = t->f.q[0];
  HostField H(&t->f);
  std::vector<uint64_t> a((size_t)2 * N), b((size_t)2 * N);
  for (int i = 0; i < N; ++i) {
    uint64_t w, wi;
    H.from_mont(&w, &t->h_tw[i]);
    H.from_mont(&wi, &t->h_twinv[i]);
    a[2 * i] = w;
    a[2 * i + 1] = h_shoup(w, q);
    b[2 * i] = wi;
    b[2 * i + 1] = h_shoup(wi, q);
  }
  if (row_copy) {
    add_row_copy(a, 2);
    add_row_copy(b, 2);
  }
  RG_TRY(t->d_tw.upload(a.data(), a.size() * 8));
  RG_TRY(t->d_twinv.upload(b.data(), b.size() * 8));
  const uint64_t w1n = t->w1n[0];
  H.from_mont(&t->nsc[0], &t->h_ninv[0]);
  H.from_mont(&t->w1n[0], &w1n);
  t->nsc_sh = h_shoup(t->nsc[0], q);
  t->w1n_sh = h_shoup(t->w1n[0], q);
  return RG_OK;
}

// Lazy64 with the Montgomery product (ntt64.hpp MONT): one word per twiddle, then the ROW copy,
// then (inverse table) the plan's rank_inv and rank_inv twInv[1 .. 16) for the fold of the last
// inverse round (ntt_tile.hpp): the plan's own rank_inv, whatever a table-built plan was given
static rg_status upload_mont64(rg_ntt* t) {
  std::vector<uint64_t> a(t->h_tw), b(t->h_twinv);
  add_row_copy(a, 1);
  add_row_copy(b, 1);
  HostField H(&t->f);
  uint64_t fold[kNttFoldLen];
  ntt_fold_consts(t->h_twinv.data(), t->h_ninv[0], [&](uint64_t* z, const uint64_t* x, const uint64_t* y) { H.mul(z, x, y); },
                  fold);
  if (b.size() != kNttFoldBase) return RG_ERR_INVALID;  // the kernels' compile-time offset
  b.insert(b.end(), fold, fold + kNttFoldLen);
  RG_TRY(t->d_tw.upload(a.data(), a.size() * 8));
  return t->d_twinv.upload(b.data(), b.size() * 8);
}

// wide fields whose inverse runs on ntt_wide_pass: the inverse table is twInv[i] / 2 (that kernel
// halves every stage instead of scaling by N^-1 at the end)
static rg_status upload_wide(rg_ntt* t) {
  const int N = t->N, L = t->f.L;
  RG_TRY(t->d_tw.upload(t->h_tw.data(), t->h_tw.size() * 8));
  std::vector<uint64_t> b(t->h_twinv.size());
  for (int i = 0; i < N; ++i) {
    const uint64_t* x = &t->h_twinv[(size_t)i * L];
    uint64_t* z = &b[(size_t)i * L];
    uint64_t c = 0;
    if (x[0] & 1) c = HostField::add_n(z, x, t->f.q, L);
    else memcpy(z, x, 8 * L);
    for (int l = 0; l < L; ++l) z[l] = (z[l] >> 1) | ((l + 1 < L ? z[l + 1] : c) << 63);
  }
  return t->d_twinv.upload(b.data(), b.size() * 8);
}

static rg_status upload_plain(rg_ntt* t) {
  RG_TRY(t->d_tw.upload(t->h_tw.data(), t->h_tw.size() * 8));
  return t->d_twinv.upload(t->h_twinv.data(), t->h_twinv.size() * 8);
}

// the helper stream of ntt256_run's two-half split (ntt_l4_fast.hip)
static rg_status create_helper_stream(rg_ntt* t) {
  t->aux.reset(new Aux());
  RG_HIP(hipStreamCreateWithFlags(&t->aux->s, hipStreamNonBlocking));
  RG_HIP(hipEventCreateWithFlags(&t->aux->fork, hipEventDisableTiming));
  RG_HIP(hipEventCreateWithFlags(&t->aux->join, hipEventDisableTiming));
  return RG_OK;
}

// Polynomials per pass pair.  Tiled in two passes: chunks of 192 MiB, so the pass-to-pass
// intermediate stays in the 256 MiB Infinity Cache; Lazy64: the whole batch.  The NttChunkMb
// switch (experiments build) sets the size for both; nothing else chunks.
static size_t chunk_polys(const NttRouting& r, size_t poly_bytes) {
  const bool tiled2 = r.route == NttRoute::Tiled && r.npasses == 2;
  const char* e = knob(Knob::NttChunkMb);
  if (!(tiled2 || (e && r.route == NttRoute::Lazy64))) return ~(size_t)0 >> 1;
  return std::max<size_t>(1, ((size_t)(e ? atoi(e) : 192) << 20) / poly_bytes);
}

// Everything a plan decides, once: the route per direction (ntt_route.hpp), then only the tables
// and the helper stream those routes use, then the two launch descriptions run() starts from.
static rg_status finalize(rg_ntt* t) {
  const int N = t->N, L = t->f.L;
  RG_HIP(hipGetDevice(&t->device));
  HostField H(&t->f);
  // log N halvings give exactly N^-1: a table-built plan whose rank_inv is anything else keeps
  // the per-stage inverse, which multiplies by the caller's rank_inv (ntt.go:242-243)
  uint64_t n[16], ninv[16];
  H.from_u64(n, (uint64_t)N);
  H.inverse(ninv, n);
  const bool halving = H.eq(ninv, &t->h_ninv[0]);
  const char* sw = knob(Knob::NttKernel);
  NttRouting r[2] = {ntt_route(L, t->f.q, t->logN, false, halving, sw),
                     ntt_route(L, t->f.q, t->logN, true, halving, sw)};
  // the wide fields' passes: ntt_route()'s one or two, or above 2^16 (where it answers Stages; and
  // under the experiments build's w3 switch) the up to three of the long route
  WidePasses wp[2];
  for (int d = 0; d < 2; ++d) {
    wp[d] = ntt_wide_long(L, t->f.q, t->logN, d == 1, halving, sw);
    if (wp[d].npasses) {
      r[d].route = NttRoute::Wide;
      r[d].npasses = 0;
    } else if (r[d].route == NttRoute::Wide) {
      wp[d] = {r[d].npasses, {r[d].passes[0], r[d].passes[1], {0, 0}}};
    }
  }
  // the 4-limb q = 1 mod 2^64 plans at 2^17 .. 2^19 (where ntt_route() answers Tiled): Fast256 in
  // three passes, which ntt256_run derives from logN; NttRouting's own list, which holds two, is unused
  for (int d = 0; d < 2; ++d)
    if (ntt_fast256_long(L, t->f.q, t->logN, d == 1, halving, sw)) {
      r[d].route = NttRoute::Fast256;
      r[d].npasses = 3;
      r[d].passes[0] = r[d].passes[1] = {0, 0};
    }
  const uint64_t* twi1 = N >= 2 ? &t->h_twinv[(size_t)1 * L] : H.one;
  memcpy(t->nsc, &t->h_ninv[0], 8 * L);
  H.mul(t->w1n, twi1, &t->h_ninv[0]);  // twInv[1] * N^-1 for the fused last inverse stage
  t->nsc_sh = t->w1n_sh = 0;
  if (r[0].mont) RG_TRY(upload_mont64(t));
  else if (r[0].shoup) RG_TRY(upload_shoup(t, r[0].route == NttRoute::Lazy64));
  else if (r[1].route == NttRoute::Wide) RG_TRY(upload_wide(t));
  else RG_TRY(upload_plain(t));
  // (a plan with one direction long and the other Tiled: both read upload_plain's tables)
  if (r[0].route == NttRoute::Fast256 || r[1].route == NttRoute::Fast256) RG_TRY(create_helper_stream(t));
  for (int d = 0; d < 2; ++d) {
    NttLaunch& p = t->dir[d];  // in, out, batch: run()
    static_cast<NttRouting&>(p) = r[d];
    p.inv = d == 1;
    p.tw = (d ? t->d_twinv : t->d_tw).as<uint64_t>();
    p.q = t->f.q;
    p.qinv = t->f.qinv;
    p.nsc = t->nsc;
    p.nsc_sh = t->nsc_sh;
    p.w1n = t->w1n;
    p.w1n_sh = t->w1n_sh;
    p.logN = t->logN;
    p.chunk_polys = chunk_polys(r[d], (size_t)N * L * 8);
    p.tile16 = ntt64_tile16(r[d].mont, sw);
    p.wide = wp[d];
    p.aux = t->aux.get();
  }
  return RG_OK;
}

static rg_status run(const rg_ntt* t, uint64_t* out, const uint64_t* in, size_t batch, bool inv, hipStream_t st) {
  if (batch == 0) return RG_OK;
  int cur = -1;
  RG_HIP(hipGetDevice(&cur));
  if (cur != t->device) {
    set_last_error("rg_ntt plan used on device " + std::to_string(cur) + ", created on " + std::to_string(t->device));
    return RG_ERR_INVALID;
  }
  NttLaunch p = t->dir[inv];
  p.in = in;
  p.out = out;
  p.batch = batch;
  switch (p.route) {
    case NttRoute::Lazy64: return ntt64_run(p, st);
    case NttRoute::Fast256: return ntt256_run(p, st);
    default: break;  // Tiled, Stages, Wide: the limb count's own unit
  }
  switch (t->f.L) {
    case 1: return ntt_run_L1(p, st);
    case 2: return ntt_run_L2(p, st);
    case 4: return ntt_run_L4(p, st);
    case 7: return ntt_run_L7(p, st);
    case 14: return ntt_run_L14(p, st);
    default: return RG_ERR_UNSUPPORTED;
  }
}

static rg_ntt* new_plan(const rg_field* f, int rank, int negacyclic) {
  rg_ntt* t = new rg_ntt();
  t->f = *f;
  t->N = rank;
  t->logN = 0;
  while ((1 << t->logN) < rank) ++t->logN;
  t->negacyclic = negacyclic ? 1 : 0;
  return t;
}

const rg_field* ntt_field(const rg_ntt* t) { return &t->f; }
bool ntt_negacyclic(const rg_ntt* t) { return t->negacyclic != 0; }

}  // namespace rg

using namespace rg;

extern "C" {

rg_status rg_ntt_create(const rg_field* f, int rank, int negacyclic, rg_ntt** out) {
  if (!f || !out) return RG_ERR_INVALID;
  *out = nullptr;
  RG_TRY(check_rank(f, rank));
  if (!limbs_supported(f->L)) return RG_ERR_UNSUPPORTED;
  rg_ntt* t = new_plan(f, rank, negacyclic);
  rg_status s = build_tables(t);
  if (s == RG_OK) s = finalize(t);
  if (s != RG_OK) {
    delete t;
    return s;
  }
  *out = t;
  return RG_OK;
}

rg_status rg_ntt_create_from_tables(const rg_field* f, int rank, int negacyclic, const uint64_t* tw,
                                    const uint64_t* tw_inv, const uint64_t* rank_inv, rg_ntt** out) {
  if (!f || !out || !tw || !tw_inv || !rank_inv) return RG_ERR_INVALID;
  *out = nullptr;
  RG_TRY(check_rank(f, rank));
  if (!limbs_supported(f->L)) return RG_ERR_UNSUPPORTED;
  const int L = f->L;
  rg_ntt* t = new_plan(f, rank, negacyclic);
  t->h_tw.assign(tw, tw + (size_t)rank * L);
  t->h_twinv.assign(tw_inv, tw_inv + (size_t)rank * L);
  t->h_ninv.assign(rank_inv, rank_inv + L);
  HostField H(&t->f);
  bool ok = !HostField::geq(rank_inv, f->q, L);
  for (size_t i = 0; i < (size_t)rank && ok; ++i)
    ok = !HostField::geq(&t->h_tw[i * L], f->q, L) && !HostField::geq(&t->h_twinv[i * L], f->q, L);
  if (ok && negacyclic) ok = H.eq(&t->h_tw[0], H.one) && H.eq(&t->h_twinv[0], H.one);
  rg_status s = ok ? finalize(t) : RG_ERR_INVALID;
  if (s != RG_OK) {
    delete t;
    return s;
  }
  *out = t;
  return RG_OK;
}

void rg_ntt_destroy(rg_ntt* t) { delete t; }
int rg_ntt_rank(const rg_ntt* t) { return t ? t->N : 0; }

const char* rg_ntt_route_name(const rg_ntt* t, int inverse) {
  if (!t) return nullptr;
  switch (t->dir[inverse != 0].route) {
    case NttRoute::Tiled: return "tiled";
    case NttRoute::Lazy64: return "lazy64";
    case NttRoute::Fast256: return "fast256";
    case NttRoute::Wide: return "wide";
    default: return "stages";
  }
}

int rg_ntt_passes(const rg_ntt* t, int inverse) {
  if (!t) return -1;
  const NttLaunch& p = t->dir[inverse != 0];
  return p.route == NttRoute::Wide ? p.wide.npasses : p.npasses;
}

rg_status rg_ntt_tables(const rg_ntt* t, uint64_t* tw, uint64_t* tw_inv, uint64_t* rank_inv) {
  if (!t) return RG_ERR_INVALID;
  if (tw) memcpy(tw, t->h_tw.data(), t->h_tw.size() * 8);
  if (tw_inv) memcpy(tw_inv, t->h_twinv.data(), t->h_twinv.size() * 8);
  if (rank_inv) memcpy(rank_inv, t->h_ninv.data(), t->h_ninv.size() * 8);
  return RG_OK;
}

static rg_status dev_call(const rg_ntt* t, uint64_t* d_out, const uint64_t* d_in, size_t batch, void* stream,
                          bool inv) {
  if (!t || (batch && (!d_out || !d_in))) return RG_ERR_INVALID;
  if (batch == 0) return RG_OK;
  if (t->N == 1) {  // rank 1: identity (1^-1 = 1)
    if (d_out != d_in)
      RG_HIP(hipMemcpyAsync(d_out, d_in, batch * t->f.L * 8, hipMemcpyDeviceToDevice, as_stream(stream)));
    return RG_OK;
  }
  return run(t, d_out, d_in, batch, inv, as_stream(stream));
}

rg_status rg_ntt_fwd_dev(const rg_ntt* t, uint64_t* d_out, const uint64_t* d_in, size_t batch, void* stream) {
  return dev_call(t, d_out, d_in, batch, stream, false);
}
rg_status rg_ntt_inv_dev(const rg_ntt* t, uint64_t* d_out, const uint64_t* d_in, size_t batch, void* stream) {
  return dev_call(t, d_out, d_in, batch, stream, true);
}

static rg_status host_call(const rg_ntt* t, uint64_t* out, const uint64_t* in, size_t batch, bool inv) {
  if (!t || (batch && (!out || !in))) return RG_ERR_INVALID;
  if (batch == 0) return RG_OK;
  const size_t bytes = batch * (size_t)t->N * t->f.L * 8;
  DevBuf buf;
  RG_TRY(buf.upload(in, bytes));
  RG_TRY(dev_call(t, buf.as<uint64_t>(), buf.as<uint64_t>(), batch, nullptr, inv));
  return buf.download(out, bytes);
}

rg_status rg_ntt_fwd(const rg_ntt* t, uint64_t* out, const uint64_t* in, size_t batch) {
  return host_call(t, out, in, batch, false);
}
rg_status rg_ntt_inv(const rg_ntt* t, uint64_t* out, const uint64_t* in, size_t batch) {
  return host_call(t, out, in, batch, true);
}

}  // extern "C"
