// jindo_setup.hip -- the Jindo handle (jindo_impl.hpp): its ring, CRT and rounding tables, the
// device-resident commit key with the MFMA MAC's key image, and the per-stream scratch.  Host
// code only; the kernels are jindo_commit.hip (the pipeline overview), jindo_sample.hip and
// jindo_verify.hip.
#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "ck_crs.hpp"
#include "host_field.hpp"
#include "jindo_impl.hpp"
#include "mac_mfma.hpp"

namespace rg {

// ring.PrimitiveRoot: smallest g >= 3 that generates Z_q^* (factors by trial division +
// Pollard rho; q < 2^62)
static bool is_prime_u64(uint64_t n) {
  if (n < 2) return false;
  static const uint64_t sp[] = {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37};
  for (uint64_t p : sp)
    if (n % p == 0) return n == p;
  uint64_t d = n - 1;
  int r = 0;
  while (!(d & 1)) d >>= 1, ++r;
  for (uint64_t a : sp) {
    uint64_t x = h_powmod(a, d, n);
    if (x == 1 || x == n - 1) continue;
    bool ok = false;
    for (int k = 1; k < r && !ok; ++k) {
      x = h_mulmod(x, x, n);
      ok = x == n - 1;
    }
    if (!ok) return false;
  }
  return true;
}
static uint64_t gcd_u64(uint64_t a, uint64_t b) {
  while (b) {
    uint64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}
static uint64_t rho(uint64_t n) {
  if (!(n & 1)) return 2;
  for (uint64_t c = 1;; ++c) {
    uint64_t x = 2, y = 2, g = 1;
    while (g == 1) {
      x = (h_mulmod(x, x, n) + c) % n;
      y = (h_mulmod(y, y, n) + c) % n;
      y = (h_mulmod(y, y, n) + c) % n;
      g = gcd_u64(x > y ? x - y : y - x, n);
    }
    if (g != n) return g;
  }
}
static void factor(uint64_t n, std::vector<uint64_t>& f) {
  if (n == 1) return;
  if (is_prime_u64(n)) {
    if (std::find(f.begin(), f.end(), n) == f.end()) f.push_back(n);
    return;
  }
  uint64_t dv = rho(n);
  factor(dv, f);
  factor(n / dv, f);
}
static uint64_t primitive_root(uint64_t q) {
  std::vector<uint64_t> f;
  factor(q - 1, f);
  for (uint64_t g = 3;; ++g) {
    bool ok = true;
    for (uint64_t p : f) ok = ok && h_powmod(g, (q - 1) / p, q) != 1;
    if (ok) return g;
  }
}
static uint64_t brv(uint64_t x, int logn) {
  uint64_t r = 0;
  for (int i = 0; i < logn; ++i) r = (r << 1) | ((x >> i) & 1);
  return r;
}

static rg_status make_ring(int d, const uint64_t* primes, int n, uint64_t base, RnsPrime* P, DevBuf& fwd, DevBuf& bwd) {
  int logd = 0;
  while ((1 << logd) < d) ++logd;
  std::vector<ulonglong2> f((size_t)n * d), b((size_t)n * d);
  for (int l = 0; l < n; ++l) {
    const uint64_t q = primes[l];
    if (!is_prime_u64(q) || (q - 1) % (2 * (uint64_t)d) || (q >> 62)) return RG_ERR_INVALID;
    RnsPrime& R = P[l];
    R.q = q;
    R.r64 = (uint64_t)(((unsigned __int128)1 << 64) % q);
    R.r64_sh = h_shoup(R.r64, q);
    R.rinv = h_powmod(R.r64, q - 2, q);
    R.rinv_sh = h_shoup(R.rinv, q);
    R.one_sh = h_shoup(1, q);
    R.ninv = h_powmod((uint64_t)d, q - 2, q);
    R.ninv_sh = h_shoup(R.ninv, q);
    R.bmod = base % q;
    R.bmod_sh = h_shoup(R.bmod, q);
    const uint64_t g = primitive_root(q);
    const uint64_t psi = h_powmod(g, (q - 1) / (2 * (uint64_t)d), q), psii = h_powmod(psi, q - 2, q);
    uint64_t x = 1, y = 1;
    for (int j = 0; j < d; ++j) {
      const size_t k = (size_t)l * d + brv((uint64_t)j, logd);
      f[k].x = x;
      f[k].y = h_shoup(x, q);
      b[k].x = y;
      b[k].y = h_shoup(y, q);
      x = h_mulmod(x, psi, q);
      y = h_mulmod(y, psii, q);
    }
    R.rw1 = h_mulmod(R.r64, f[(size_t)l * d + 1].x, q);
    R.rw1_sh = h_shoup(R.rw1, q);
  }
  RG_TRY(fwd.upload(f.data(), f.size() * sizeof(ulonglong2)));
  RG_TRY(bwd.upload(b.data(), b.size() * sizeof(ulonglong2)));
  return RG_OK;
}

static void make_crt(const uint64_t* primes, int n, CrtDev& C) {
  memset(&C, 0, sizeof(C));
  C.n = n;
  for (int j = 0; j < n; ++j) {
    C.q[j] = primes[j];
    for (int k = 0; k < j; ++k) {
      C.inv[j][k] = h_powmod(primes[k] % primes[j], primes[j] - 2, primes[j]);
      C.inv_sh[j][k] = h_shoup(C.inv[j][k], primes[j]);
    }
  }
  unsigned __int128 acc;
  uint64_t Q[5] = {1, 0, 0, 0, 0};
  for (int j = 0; j < n; ++j) {
    uint64_t carry = 0;
    for (int i = 0; i < 4; ++i) {
      acc = (unsigned __int128)Q[i] * primes[j] + carry;
      Q[i] = (uint64_t)acc;
      carry = (uint64_t)(acc >> 64);
    }
  }
  for (int i = 0; i < 4; ++i) {
    C.Q[i] = Q[i];
    C.Qhalf[i] = (Q[i] >> 1) | (i + 1 < 4 ? Q[i + 1] << 63 : 0);
  }
}

static void make_dst(const uint64_t* primes, int n, DstDev& D) {
  memset(&D, 0, sizeof(D));
  D.n = n;
  for (int l = 0; l < n; ++l) {
    const uint64_t q = primes[l];
    uint64_t p = 1 % q;
    const uint64_t r64 = (uint64_t)(((unsigned __int128)1 << 64) % q);
    for (int i = 0; i < 4; ++i) {
      D.pw[l][i] = p;
      D.pw_sh[l][i] = h_shoup(p, q);
      p = h_mulmod(p, r64, q);
    }
  }
}

RingDev ring_dev(const RnsPrime* P, int n, const DevBuf& f, const DevBuf& b) {
  RingDev R;
  memset(&R, 0, sizeof(R));
  R.n = n;
  for (int l = 0; l < n; ++l) R.p[l] = P[l];
  R.fwd = f.as<const ulonglong2>();
  R.bwd = b.as<const ulonglong2>();
  return R;
}

static rg_status validate(const rg_jindo_params* p) {
  if (!p) return RG_ERR_INVALID;
  if (p->nq < 1 || p->nq > kMaxQ || p->nqo < 1 || p->nqo > kMaxQ || p->nqo > p->nq) return RG_ERR_INVALID;
  if (p->d < 2 || p->d > kMaxD || (p->d & (p->d - 1))) return RG_ERR_INVALID;
  if (p->rows < 2 || p->cols < 1 || p->slots < 1 || p->exp < 1 || p->slots * p->exp > p->d) return RG_ERR_INVALID;
  if (p->in_msis < 1 || p->in_msis > kMaxJ || p->out_msis < 1 || p->out_msis > kMaxJ || p->mlwe < 0) return RG_ERR_INVALID;
  if (p->dcmp != (p->cols + 1) * p->in_msis) return RG_ERR_INVALID;
  if (p->base < 2 || (p->base >> 32)) return RG_ERR_INVALID;
  for (int l = 0; l < p->nq; ++l)
    if (p->q[l] <= p->base) return RG_ERR_INVALID;  // digits (<= b) are used as residues directly
  for (int l = 0; l < p->nqo; ++l)
    if (p->qo[l] <= p->base) return RG_ERR_INVALID;
  if (!(p->field_limbs == 1 || p->field_limbs == 2 || p->field_limbs == 4 || p->field_limbs == 7 ||
        p->field_limbs == 14))
    return RG_ERR_UNSUPPORTED;
  return RG_OK;
}

static rg_status build(rg_jindo* J) {
  const rg_jindo_params& p = J->p;
  if (!init_field(&J->field, p.field_limbs, p.field_q)) return RG_ERR_INVALID;
  RG_TRY(make_ring(p.d, p.q, p.nq, p.base, J->rq, J->rootsq_f, J->rootsq_b));
  RG_TRY(make_ring(p.d, p.qo, p.nqo, p.base, J->ro, J->rootso_f, J->rootso_b));
  make_crt(p.q, p.nq, J->crt_q);
  make_crt(p.qo, p.nqo, J->crt_o);
  make_dst(p.qo, p.nqo, J->dst_o);
  make_dst(p.q, p.nq, J->dst_q);
  J->base_inv = (uint64_t)(((unsigned __int128)1 << 64) / p.base);
  return RG_OK;
}

static size_t ck_sizes(const rg_jindo_params& p, size_t* in, size_t* ml, size_t* out) {
  *in = (size_t)p.in_msis * p.rows * p.nq * p.d;
  *ml = (size_t)p.in_msis * p.mlwe * p.nq * p.d;
  *out = (size_t)p.out_msis * p.dcmp * p.nqo * p.d;
  return *in + *ml + *out;
}

// The calling stream's scratch, grown to `batch` commits.  Growing first drains the stream (its
// earlier commits may still read the old buffers); other streams are untouched.
// These three buffers are JSizes::scratch(), which rg_jindo_scratch_bytes reports.
rg_status stream_scratch(rg_jindo* J, size_t batch, hipStream_t st, rg_jindo_scratch** out) {
  const JSizes z = sizes_of(J->p, batch);
  std::lock_guard<std::mutex> lk(J->mu);
  std::unique_ptr<rg_jindo_scratch>& S = J->scratch[st];
  if (!S) S.reset(new rg_jindo_scratch());
  if (S->digits.bytes < z.digits || S->com.bytes < z.inner || S->ocom.bytes < z.outer)
    RG_HIP(hipStreamSynchronize(st));
  RG_TRY(S->digits.alloc(z.digits));
  RG_TRY(S->com.alloc(z.inner));
  RG_TRY(S->ocom.alloc(z.outer));
  *out = S.get();
  return RG_OK;
}

// a ring prime as the MFMA MAC takes it (the key image here, the launches in jindo_commit.hip)
MfmaPrime mfma_prime(const RnsPrime& P) { return MfmaPrime{P.q, P.rinv, P.rinv_sh, P.one_sh}; }

// A handle's buffers belong to the device it was created on
rg_status on_device(const rg_jindo* J) {
  int cur = -1;
  RG_HIP(hipGetDevice(&cur));
  if (cur != J->device) {
    set_last_error("rg_jindo handle used on device " + std::to_string(cur) + ", created on " +
                   std::to_string(J->device));
    return RG_ERR_INVALID;
  }
  return RG_OK;
}

}  // namespace rg

using namespace rg;

extern "C" {

// A validated handle with its ring tables, owned by the caller until it hands it out
static rg_status jindo_new(const rg_jindo_params* p, rg_jindo** out, std::unique_ptr<rg_jindo>& J) {
  if (!out) return RG_ERR_INVALID;
  *out = nullptr;
  RG_TRY(validate(p));
  J.reset(new rg_jindo());
  J->p = *p;
  if (hipGetDevice(&J->device) != hipSuccess) J->device = 0;
  return build(J.get());
}

// The commit key is device-resident from here on: ck_in/ck_mlwe/ck_out hold it in the
// entities.go layouts; the MAC kernels' key images (the MFMA MAC's digits
// words) are built from them on the device, only for the MAC each product runs on.
static rg_status finish_ck(rg_jindo* J, hipStream_t st) {
  const rg_jindo_params& p = J->p;
  // RINGO_JINDO_MAC (experiments build): l = mac_kernel; default = the MFMA MAC where it applies,
  // else mac_kernel
  const char* mk = knob(Knob::JindoMac);
  const bool legacy = mk && mk[0] == 'l';
  const bool no_mfma = legacy;
  const size_t pcq = (size_t)p.nq * p.d, pco = (size_t)p.nqo * p.d;
  {
    uint64_t pq[kMaxQ], po[kMaxQ];
    MfmaPrime mq[kMaxQ], mo[kMaxQ];
    for (int l = 0; l < p.nq; ++l) pq[l] = J->rq[l].q, mq[l] = mfma_prime(J->rq[l]);
    for (int l = 0; l < p.nqo; ++l) po[l] = J->ro[l].q, mo[l] = mfma_prime(J->ro[l]);
    J->mfma_q = no_mfma ? 0 : mac_mfma_nb(pq, p.nq, p.in_msis, p.rows + p.mlwe, p.d);
    J->mfma_o = no_mfma ? 0 : mac_mfma_nb(po, p.nqo, p.out_msis, p.dcmp, p.d);
    if (J->mfma_q)
      RG_TRY(mac_mfma_key_dev(J->ck_in.as<uint64_t>(), p.rows, J->ck_mlwe.as<uint64_t>(), p.mlwe, p.in_msis,
                              (long long)pcq, p.d, J->mfma_q, mq, p.nq, J->ckm_in, st));
    if (J->mfma_o)
      RG_TRY(mac_mfma_key_dev(J->ck_out.as<uint64_t>(), p.dcmp, nullptr, 0, p.out_msis, (long long)pco, p.d,
                              J->mfma_o, mo, p.nqo, J->ckm_out, st));
  }
  RG_HIP(hipStreamSynchronize(st));
  return RG_OK;
}

// ck_* host (kind = H2D) or device (kind = D2D) arrays -> the handle's device buffers
static rg_status take_ck(rg_jindo* J, const uint64_t* ck_in, const uint64_t* ck_mlwe, const uint64_t* ck_out,
                         hipMemcpyKind kind, hipStream_t st) {
  size_t a, b, c;
  ck_sizes(J->p, &a, &b, &c);
  RG_TRY(J->ck_in.alloc(a * 8));
  RG_TRY(J->ck_mlwe.alloc(b * 8));
  RG_TRY(J->ck_out.alloc(c * 8));
  RG_HIP(hipMemcpyAsync(J->ck_in.p, ck_in, a * 8, kind, st));
  if (b) RG_HIP(hipMemcpyAsync(J->ck_mlwe.p, ck_mlwe, b * 8, kind, st));
  RG_HIP(hipMemcpyAsync(J->ck_out.p, ck_out, c * 8, kind, st));
  return finish_ck(J, st);
}

rg_status rg_jindo_create(const rg_jindo_params* p, const uint64_t* ck_in, const uint64_t* ck_mlwe,
                          const uint64_t* ck_out, rg_jindo** out) {
  if (!ck_in || !ck_out || (!ck_mlwe && p && p->mlwe)) return RG_ERR_INVALID;
  std::unique_ptr<rg_jindo> J;
  RG_TRY(jindo_new(p, out, J));
  RG_TRY(take_ck(J.get(), ck_in, ck_mlwe, ck_out, hipMemcpyHostToDevice, nullptr));
  *out = J.release();
  return RG_OK;
}

rg_status rg_jindo_create_dev(const rg_jindo_params* p, const uint64_t* d_ck_in, const uint64_t* d_ck_mlwe,
                              const uint64_t* d_ck_out, void* stream, rg_jindo** out) {
  if (!d_ck_in || !d_ck_out || (!d_ck_mlwe && p && p->mlwe)) return RG_ERR_INVALID;
  std::unique_ptr<rg_jindo> J;
  RG_TRY(jindo_new(p, out, J));
  RG_TRY(take_ck(J.get(), d_ck_in, d_ck_mlwe, d_ck_out, hipMemcpyDeviceToDevice, as_stream(stream)));
  *out = J.release();
  return RG_OK;
}

rg_status rg_jindo_create_from_crs(const rg_jindo_params* p, const uint8_t* crs, size_t crs_len, rg_jindo** out) {
  if (!crs && crs_len) return RG_ERR_INVALID;
  std::unique_ptr<rg_jindo> J;
  RG_TRY(jindo_new(p, out, J));
  const rg_jindo_params& P = J->p;
  CtrStream u(crs, crs_len);
  if (!u.ok) {
    set_last_error("libcrypto (SHA384/AES-256-CTR) unavailable");
    return RG_ERR_UNSUPPORTED;
  }
  size_t a, b, c;
  ck_sizes(P, &a, &b, &c);
  std::vector<uint64_t> h_in(a), h_ml(b), h_out(c);
  const size_t d = P.d;
  // entities.go:24-61: In, then MLWE, then Out; coefficient-major, limb-minor draws
  for (int i = 0; i < P.in_msis; ++i)
    for (int j = 0; j < P.rows; ++j)
      for (size_t k = 0; k < d; ++k)
        for (int l = 0; l < P.nq; ++l) h_in[(((size_t)i * P.rows + j) * P.nq + l) * d + k] = u.sample_n(P.q[l]);
  for (int i = 0; i < P.in_msis; ++i)
    for (int j = 0; j < P.mlwe; ++j)
      for (size_t k = 0; k < d; ++k)
        for (int l = 0; l < P.nq; ++l) h_ml[(((size_t)i * P.mlwe + j) * P.nq + l) * d + k] = u.sample_n(P.q[l]);
  for (int i = 0; i < P.out_msis; ++i)
    for (int j = 0; j < P.dcmp; ++j)
      for (size_t k = 0; k < d; ++k)
        for (int l = 0; l < P.nqo; ++l) h_out[(((size_t)i * P.dcmp + j) * P.nqo + l) * d + k] = u.sample_n(P.qo[l]);
  RG_TRY(take_ck(J.get(), h_in.data(), h_ml.data(), h_out.data(), hipMemcpyHostToDevice, nullptr));
  *out = J.release();
  return RG_OK;
}

void rg_jindo_destroy(rg_jindo* j) {
  if (j) (void)hipDeviceSynchronize();  // scratch may still be in use by queued commits
  delete j;
}

rg_status rg_jindo_commit_key(const rg_jindo* J, uint64_t* ck_in, uint64_t* ck_mlwe, uint64_t* ck_out) {
  if (!J) return RG_ERR_INVALID;
  size_t a, b, c;
  ck_sizes(J->p, &a, &b, &c);
  if (ck_in) RG_HIP(hipMemcpy(ck_in, J->ck_in.p, a * 8, hipMemcpyDeviceToHost));
  if (ck_mlwe && b) RG_HIP(hipMemcpy(ck_mlwe, J->ck_mlwe.p, b * 8, hipMemcpyDeviceToHost));
  if (ck_out) RG_HIP(hipMemcpy(ck_out, J->ck_out.p, c * 8, hipMemcpyDeviceToHost));
  return RG_OK;
}

rg_status rg_jindo_commit_key_dev(const rg_jindo* J, const uint64_t** d_ck_in, const uint64_t** d_ck_mlwe,
                                  const uint64_t** d_ck_out) {
  if (!J) return RG_ERR_INVALID;
  if (d_ck_in) *d_ck_in = J->ck_in.as<const uint64_t>();
  if (d_ck_mlwe) *d_ck_mlwe = J->ck_mlwe.as<const uint64_t>();
  if (d_ck_out) *d_ck_out = J->ck_out.as<const uint64_t>();
  return RG_OK;
}

size_t rg_jindo_scratch_bytes(const rg_jindo* J, size_t batch) {
  return J ? sizes_of(J->p, batch).scratch() : 0;
}

rg_status rg_jindo_release_stream(rg_jindo* J, void* stream) {
  if (!J) return RG_ERR_INVALID;
  RG_TRY(on_device(J));
  hipStream_t st = as_stream(stream);
  std::lock_guard<std::mutex> lk(J->mu);
  RG_HIP(hipStreamSynchronize(st));
  auto a = J->aux.find(st);
  if (a != J->aux.end()) {
    for (hipStream_t x : a->second.s)
      if (x) {
        RG_HIP(hipStreamSynchronize(x));
        J->scratch.erase(x);
        (void)hipStreamDestroy(x);
      }
    for (hipEvent_t x : a->second.e)
      if (x) (void)hipEventDestroy(x);
    J->aux.erase(a);
  }
  J->scratch.erase(st);
  return RG_OK;
}

rg_status rg_jindo_mac_kinds(const rg_jindo* J, int* inner, int* outer) {
  if (!J || !inner || !outer) return RG_ERR_INVALID;
  *inner = J->mfma_q ? RG_MAC_MFMA : RG_MAC_GENERIC;
  *outer = J->mfma_o ? RG_MAC_MFMA : RG_MAC_GENERIC;
  return RG_OK;
}

}  // extern "C"
