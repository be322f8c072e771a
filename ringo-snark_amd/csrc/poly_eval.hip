// poly_eval.hip -- Poly.Evaluate (math/bigpoly/poly.go:64-76) of a batch of polynomials at one
// point, for gfx950: evals[i] = Poly(v[i]).Evaluate(x) of Prover.Evaluate (jindo/prover.go:318-321)
// on the committed polynomials where they already lie.
//
// The polynomial is cut into tiles of T = kEvalTile = 256 K consecutive coefficients; a workgroup
// owns one tile of one polynomial.  Lane t reads coefficients tile + 256 k + t for k = K-1 .. 0, so
// across the workgroup every load is one contiguous run of 256 * 8 L bytes, and runs Horner in
// y = x^256 over them; it multiplies once by x^t and the 256 lane values are summed by an f_add
// tree in LDS:
//   tile sum = sum_t x^t sum_k p[tile + 256 k + t] y^k = sum_{i < T} p[tile + i] x^i.
// A second, small kernel folds each polynomial's tile sums by Horner in x^T.  x^t (t < 256),
// x^256 and x^T depend on the point alone: rg_buckler_powers_dev writes them into the scratch once
// per call.  One f_mul per coefficient plus 1/K.
// With a point per group of polynomials (rg_poly_evaluate_multi_dev: polynomial b at point
// (b / group) % n_points) the same two kernels read the tables of their polynomial's point, and the
// tables of all points come from two rg_buckler_powers_batch_dev launches; one point is the case
// n_points = 1 of the same code.
// Every sum is the canonical arithmetic of field.hpp and the value of a polynomial at a point is
// one residue, so every output limb equals the reference's single Horner pass.  No atomics: a
// tile sum has one writer (lane 0 of its workgroup), an output element one lane.
#include "common.hpp"
#include "field.hpp"

namespace rg {

constexpr int kEvalLanes = 256;
constexpr int kEvalK = 16;                        // Horner steps per lane
constexpr int kEvalTile = kEvalLanes * kEvalK;    // T: coefficients per workgroup
// loads in flight per lane ahead of their Horner steps (their registers: U L words)
template <int L>
constexpr int kEvalUnroll = L <= 4 ? 4 : (L <= 7 ? 2 : 1);

// Polynomial b is evaluated at point (b / group) % n_points (one point: group = batch, n_points = 1)
struct EvalPoints {
  uint32_t group, n_points;
};

// pw: x^t for t <= 256 of every point ([n_points][257][L]); tiles [batch][ntiles][L]
template <int L>
__global__ __launch_bounds__(kEvalLanes) void eval_tile_kernel(FieldParams<L> F, const uint64_t* p, long long n,
                                                              long long stride, long long ntiles, const uint64_t* pw,
                                                              EvalPoints pts, uint64_t* tiles) {
  __shared__ uint64_t red[kEvalLanes * L];
  constexpr int U = kEvalUnroll<L>;
  const int t = threadIdx.x;
  const long long b = blockIdx.x / ntiles, tile = blockIdx.x % ntiles;
  pw += (long long)(((uint32_t)b / pts.group) % pts.n_points) * ((kEvalLanes + 1) * L);  // uniform: scalar
  const long long lo = tile * kEvalTile;
  const long long left = n - lo;  // >= 1: coefficients of this tile and after
  const uint64_t* src = p + (b * stride + lo) * L;
  uint64_t y[L], z[L];
  el_copy<L>(y, pw + (long long)kEvalLanes * L);
#pragma unroll
  for (int l = 0; l < L; ++l) z[l] = 0;
  // rows 256 k .. 256 k + 255 that hold a coefficient below n (uniform over the workgroup)
  const int rows = (int)min((long long)kEvalK, (left + kEvalLanes - 1) / kEvalLanes);
  int k = rows - 1;
  for (; k >= U - 1; k -= U) {
    uint64_t c[U][L];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long i = (long long)(k - u) * kEvalLanes + t;
      const bool in = i < left;  // the last row of the last tile is partial: never read past n
#pragma unroll
      for (int l = 0; l < L; ++l) c[u][l] = in ? src[i * L + l] : 0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      f_mul<L>(z, z, y, F);
      f_add<L>(z, z, c[u], F);
    }
  }
  for (; k >= 0; --k) {
    const long long i = (long long)k * kEvalLanes + t;
    const bool in = i < left;
    uint64_t c[L];
#pragma unroll
    for (int l = 0; l < L; ++l) c[l] = in ? src[i * L + l] : 0;
    f_mul<L>(z, z, y, F);
    f_add<L>(z, z, c, F);
  }
  {
    uint64_t xt[L];
    el_copy<L>(xt, pw + (long long)t * L);
    f_mul<L>(z, z, xt, F);
  }
  el_copy<L>(red + t * L, z);
  __syncthreads();
  for (int s = kEvalLanes >> 1; s > 0; s >>= 1) {
    if (t < s) f_add<L>(red + t * L, red + t * L, red + (t + s) * L, F);
    __syncthreads();
  }
  if (t < L) tiles[blockIdx.x * (long long)L + t] = red[t];
}

// out[b] = sum_j tiles[b][j] (x^T)^j by Horner from the top; ntiles = 0 (n = 0) leaves z = 0.
// pt: (x^256)^k for k <= K of every point ([n_points][K + 1][L]); the last of a table is x^T
template <int L>
__global__ __launch_bounds__(256) void eval_fold_kernel(FieldParams<L> F, const uint64_t* tiles, long long ntiles,
                                                        long long batch, const uint64_t* pt, EvalPoints pts,
                                                        uint64_t* out) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  uint64_t y[L], z[L];
#pragma unroll
  for (int l = 0; l < L; ++l) y[l] = z[l] = 0;
  if (ntiles) el_copy<L>(y, pt + ((long long)(((uint32_t)b / pts.group) % pts.n_points) * (kEvalK + 1) + kEvalK) * L);
  for (long long j = ntiles - 1; j >= 0; --j) {
    uint64_t c[L];
    el_copy<L>(c, tiles + (b * ntiles + j) * L);
    f_mul<L>(z, z, y, F);
    f_add<L>(z, z, c, F);
  }
  el_copy<L>(out + b * L, z);
}

static long long eval_tiles(size_t n) { return (long long)((n + kEvalTile - 1) / kEvalTile); }

// the points a call reads: polynomial b < batch takes point (b / group) % n_points, so a group
// beyond the batch is the batch and the points beyond the last group are never reached
static EvalPoints eval_points(size_t batch, size_t n_points, size_t group) {
  EvalPoints pts;
  pts.group = (uint32_t)(group < batch ? group : batch);
  const size_t groups = (batch + pts.group - 1) / pts.group;
  pts.n_points = (uint32_t)(n_points < groups ? n_points : groups);
  return pts;
}

template <int L>
static rg_status eval_batch_L(const rg_field* f, const uint64_t* p, long long n, long long stride, long long batch,
                              const uint64_t* x, long long x_stride, EvalPoints pts, uint64_t* out, uint64_t* scratch,
                              hipStream_t st) {
  const FieldParams<L> F = field_params<L>(f);
  const long long ntiles = eval_tiles((size_t)n);
  uint64_t* pw = scratch;                                          // per point: x^0 .. x^256
  uint64_t* pt = pw + (size_t)pts.n_points * (kEvalLanes + 1) * L;  // (x^256)^0 .. (x^256)^K: the last is x^T
  uint64_t* tiles = pt + (size_t)pts.n_points * (kEvalK + 1) * L;
  if (ntiles) {
    RG_TRY(rg_buckler_powers_batch_dev(f, x, (size_t)x_stride, pts.n_points, kEvalLanes + 1, pw, st));
    RG_TRY(rg_buckler_powers_batch_dev(f, pw + kEvalLanes * L, kEvalLanes + 1, pts.n_points, kEvalK + 1, pt, st));
    hipLaunchKernelGGL(eval_tile_kernel<L>, dim3((unsigned)(ntiles * batch)), dim3(kEvalLanes), 0, st, F, p, n, stride,
                       ntiles, pw, pts, tiles);
    RG_TRY(check_launch("evaluate batch tiles"));
  }
  hipLaunchKernelGGL(eval_fold_kernel<L>, dim3(grid256(batch)), dim3(256), 0, st, F, tiles, ntiles, batch, pt, pts,
                     out);
  return check_launch("evaluate batch fold");
}

// the checks both forms share, before any device call; *done: nothing to launch
static rg_status eval_batch_check(const rg_field* f, const void* p, size_t n, size_t stride, size_t batch,
                                  const void* x, const void* out, bool* done) {
  *done = false;
  if (!f) {
    set_last_error("evaluate batch: NULL field handle");
    return RG_ERR_INVALID;
  }
  if (!limbs_supported(f->L)) {
    set_last_error("evaluate batch: no kernel for " + std::to_string(f->L) + " limbs (1, 2, 4, 7, 14)");
    return RG_ERR_UNSUPPORTED;
  }
  if (stride < n) {
    set_last_error("evaluate batch: stride " + std::to_string(stride) + " < n " + std::to_string(n));
    return RG_ERR_INVALID;
  }
  if (batch == 0) {
    *done = true;
    return RG_OK;
  }
  if (!x || !out || (n && !p)) {
    set_last_error("evaluate batch: NULL buffer");
    return RG_ERR_INVALID;
  }
  // one workgroup per tile in a 1-D grid; batch * stride <= 2^50 elements keeps every byte offset below 2^63
  if (stride > ((size_t)1 << 40) || batch > ((size_t)1 << 30) || batch * stride > ((size_t)1 << 50) ||
      (unsigned long long)eval_tiles(n) * batch > 0x7fffffffull) {
    set_last_error("evaluate batch: n, stride or batch out of range");
    return RG_ERR_INVALID;
  }
  return RG_OK;
}

// what the several-point forms add to eval_batch_check; a table per point goes through one
// rg_buckler_powers_batch_dev, which takes at most 65535 bases
static rg_status eval_multi_check(size_t batch, size_t x_stride, size_t n_points, size_t group) {
  if (group == 0 || n_points == 0 || x_stride == 0) {
    set_last_error("evaluate multi: group, n_points or x_stride is 0");
    return RG_ERR_INVALID;
  }
  if (x_stride > ((size_t)1 << 30) || (batch && eval_points(batch, n_points, group).n_points > 65535)) {
    set_last_error("evaluate multi: x_stride out of range or more than 65535 points in use");
    return RG_ERR_INVALID;
  }
  return RG_OK;
}

static size_t eval_scratch_bytes(const rg_field* f, size_t n, size_t batch, size_t n_points) {
  return (n_points * ((size_t)(kEvalLanes + 1) + (kEvalK + 1)) + batch * (size_t)eval_tiles(n)) * f->L * 8;
}

static rg_status eval_launch(const rg_field* f, const uint64_t* d_p, size_t n, size_t stride, size_t batch,
                             const uint64_t* d_x, size_t x_stride, EvalPoints pts, uint64_t* d_out, void* d_scratch,
                             void* stream) {
  if (!d_scratch) {
    set_last_error("evaluate batch: NULL scratch");
    return RG_ERR_INVALID;
  }
  hipStream_t st = as_stream(stream);
  return dispatch_limbs(f->L, [&](auto Lc) {
    return eval_batch_L<Lc()>(f, d_p, (long long)n, (long long)stride, (long long)batch, d_x, (long long)x_stride, pts,
                              d_out, (uint64_t*)d_scratch, st);
  });
}

}  // namespace rg

using namespace rg;

extern "C" {

size_t rg_poly_evaluate_batch_scratch_bytes(const rg_field* f, size_t n, size_t batch) {
  return f ? eval_scratch_bytes(f, n, batch, 1) : 0;
}

rg_status rg_poly_evaluate_batch_dev(const rg_field* f, const uint64_t* d_p, size_t n, size_t stride, size_t batch,
                                     const uint64_t* d_x, uint64_t* d_out, void* d_scratch, void* stream) {
  bool done;
  RG_TRY(eval_batch_check(f, d_p, n, stride, batch, d_x, d_out, &done));
  if (done) return RG_OK;
  return eval_launch(f, d_p, n, stride, batch, d_x, 1, eval_points(batch, 1, batch), d_out, d_scratch, stream);
}

// host-pointer form: p holds (batch - 1) stride + n elements
rg_status rg_poly_evaluate_batch(const rg_field* f, const uint64_t* p, size_t n, size_t stride, size_t batch,
                                 const uint64_t* x, uint64_t* out) {
  bool done;
  RG_TRY(eval_batch_check(f, p, n, stride, batch, x, out, &done));
  if (done) return RG_OK;
  const size_t e = (size_t)f->L * 8;
  DevBuf dp, dx, dout, ds;
  if (n) RG_TRY(dp.upload(p, ((batch - 1) * stride + n) * e));
  RG_TRY(dx.upload(x, e));
  RG_TRY(dout.alloc(batch * e));
  RG_TRY(ds.alloc(rg_poly_evaluate_batch_scratch_bytes(f, n, batch)));
  RG_TRY(rg_poly_evaluate_batch_dev(f, n ? dp.as<uint64_t>() : nullptr, n, stride, batch, dx.as<uint64_t>(),
                                    dout.as<uint64_t>(), ds.p, nullptr));
  return dout.download(out, batch * e);
}

// ---- a point per group of polynomials ---------------------------------------------------------
size_t rg_poly_evaluate_multi_scratch_bytes(const rg_field* f, size_t n, size_t batch, size_t n_points) {
  if (!f) return 0;
  return eval_scratch_bytes(f, n, batch, n_points < batch ? n_points : batch);
}

rg_status rg_poly_evaluate_multi_dev(const rg_field* f, const uint64_t* d_p, size_t n, size_t stride, size_t batch,
                                     const uint64_t* d_x, size_t x_stride, size_t n_points, size_t group,
                                     uint64_t* d_out, void* d_scratch, void* stream) {
  bool done;
  RG_TRY(eval_batch_check(f, d_p, n, stride, batch, d_x, d_out, &done));
  RG_TRY(eval_multi_check(batch, x_stride, n_points, group));
  if (done) return RG_OK;
  return eval_launch(f, d_p, n, stride, batch, d_x, x_stride, eval_points(batch, n_points, group), d_out, d_scratch,
                     stream);
}

// host-pointer form: x holds (n_points - 1) x_stride + 1 elements
rg_status rg_poly_evaluate_multi(const rg_field* f, const uint64_t* p, size_t n, size_t stride, size_t batch,
                                 const uint64_t* x, size_t x_stride, size_t n_points, size_t group, uint64_t* out) {
  bool done;
  RG_TRY(eval_batch_check(f, p, n, stride, batch, x, out, &done));
  RG_TRY(eval_multi_check(batch, x_stride, n_points, group));
  if (done) return RG_OK;
  const size_t e = (size_t)f->L * 8;
  DevBuf dp, dx, dout, ds;
  if (n) RG_TRY(dp.upload(p, ((batch - 1) * stride + n) * e));
  RG_TRY(dx.upload(x, ((n_points - 1) * x_stride + 1) * e));
  RG_TRY(dout.alloc(batch * e));
  RG_TRY(ds.alloc(rg_poly_evaluate_multi_scratch_bytes(f, n, batch, n_points)));
  RG_TRY(rg_poly_evaluate_multi_dev(f, n ? dp.as<uint64_t>() : nullptr, n, stride, batch, dx.as<uint64_t>(), x_stride,
                                    n_points, group, dout.as<uint64_t>(), ds.p, nullptr));
  return dout.download(out, batch * e);
}

}  // extern "C"
