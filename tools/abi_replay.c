/* abi_replay.c -- a C11 caller of include/ringo.h: the call sequences of INTEGRATION.md, compiled.
 *
 * The product is a C ABI that Go binds through cgo; this program is the same caller without Go: it
 * includes ringo.h and the C standard library only, takes every device buffer from rg_malloc, moves
 * data with rg_memcpy_h2d / rg_memcpy_d2h + rg_stream_sync, and runs on the null stream.  It decides
 * nothing about values: it reads raw little-endian arrays (DIR/NAME.bin) and integers (DIR/params.txt,
 * one `key value` per line; doubles travel as their IEEE-754 bit patterns), writes what the library
 * returned as DIR/NAME.bin, and tests/test_capi_c.py and tests/test_gpu_capi_c.py compare those
 * files bit for bit with the ctypes mirror and the C oracle.
 *
 *   abi_replay layout            sizes, offsets and enumerators as the C compiler sees them (no GPU)
 *   abi_replay refuse            host-side refusals: the documented status codes (no GPU)
 *   abi_replay bigpoly DIR       INTEGRATION.md section 1
 *   abi_replay jindo DIR         INTEGRATION.md section 2 (Commit, Evaluate, Verify, sampled Commit)
 *   abi_replay buckler DIR       INTEGRATION.md section 3 (linear check, decomposition, encode)
 *   abi_replay bverify DIR       INTEGRATION.md section 3, Verifier.Verify's checks (one verdict word)
 *
 * Exit status: 0; 2 when a call returned a status other than the expected one (the call,
 * rg_status_string and rg_last_error go to stderr); 3 for a usage or file error.
 * Built by ringo-snark_amd/Makefile into ringo-snark_amd/lib/abi_replay. */
#include <inttypes.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ringo.h"

/* What the header's prose and the ctypes mirror rely on. */
_Static_assert(sizeof(rg_status) == sizeof(int), "rg_status is returned as int");
_Static_assert(sizeof(size_t) == 8 && sizeof(void*) == 8, "64-bit caller");
_Static_assert(sizeof(long long) == 8 && sizeof(unsigned long long) == 8, "first_commit / idx are 64-bit");
_Static_assert(sizeof(double) == 8, "IEEE-754 binary64");
_Static_assert(sizeof(rg_jindo_seeds) == 192, "six 32-byte seeds, no padding");
_Static_assert(offsetof(rg_jindo_seeds, uniform) == 160, "seeds are consecutive");
_Static_assert(sizeof(rg_jindo_stddevs) == 48, "six doubles, no padding");
_Static_assert(offsetof(rg_jindo_params, q) + sizeof(((rg_jindo_params*)0)->q) == offsetof(rg_jindo_params, qo),
               "q[4] and qo[4] are adjacent");
_Static_assert(sizeof(((rg_jindo_params*)0)->field_q) == 16 * 8, "field modulus: up to 16 limbs");
_Static_assert(sizeof(((rg_jindo_verify_result*)0)->outer_norm_sq) == 80, "norm sums: 10 words");
_Static_assert(sizeof(((rg_jindo_verify_result*)0)->eval_lhs) == 128, "evaluation sides: 16 limbs");
_Static_assert(RG_OK == 0 && RG_ERR_RANK == -6, "status codes");
_Static_assert(RG_VEC_ADD == 0 && RG_VEC_SMUL_SUB == 8, "vec ops are 0..8");

/* ---- files ------------------------------------------------------------------------------------- */
static const char* g_dir = ".";

static void die(const char* what, const char* name) {
  fprintf(stderr, "abi_replay: %s %s\n", what, name);
  exit(3);
}

static void* xmalloc(size_t bytes) {
  void* p = malloc(bytes ? bytes : 1);
  if (!p) die("out of memory", "");
  return p;
}

static void path_of(char* buf, size_t cap, const char* name, const char* ext) {
  int n = snprintf(buf, cap, "%s/%s%s", g_dir, name, ext);
  if (n < 0 || (size_t)n >= cap) die("path too long:", name);
}

/* NAME_I, for the per-case files (a small ring of buffers: several may be live in one call) */
static const char* idx(const char* base, size_t i) {
  static char ring[8][64];
  static unsigned at;
  char* b = ring[at++ % 8];
  snprintf(b, sizeof ring[0], "%s_%zu", base, i);
  return b;
}

/* DIR/NAME.bin, which must hold exactly `bytes` bytes */
static void* read_bin(const char* name, size_t bytes) {
  char path[1024];
  path_of(path, sizeof path, name, ".bin");
  FILE* fp = fopen(path, "rb");
  if (!fp) die("cannot open", path);
  void* p = xmalloc(bytes);
  if (fread(p, 1, bytes, fp) != bytes || fgetc(fp) != EOF) die("unexpected size of", path);
  fclose(fp);
  return p;
}

static void write_bin(const char* name, const void* p, size_t bytes) {
  char path[1024];
  path_of(path, sizeof path, name, ".bin");
  FILE* fp = fopen(path, "wb");
  if (!fp) die("cannot create", path);
  if (fwrite(p, 1, bytes, fp) != bytes || fclose(fp) != 0) die("cannot write", path);
}

/* DIR/params.txt */
enum { KV_MAX = 256 };
static char g_key[KV_MAX][48];
static uint64_t g_val[KV_MAX];
static int g_nkv;

static void kv_load(void) {
  char path[1024];
  path_of(path, sizeof path, "params", ".txt");
  FILE* fp = fopen(path, "r");
  if (!fp) die("cannot open", path);
  char val[64];
  while (g_nkv < KV_MAX && fscanf(fp, "%47s %63s", g_key[g_nkv], val) == 2) {
    char* end;
    g_val[g_nkv] = strtoull(val, &end, 10);
    if (*end) die("not an integer:", val);
    g_nkv++;
  }
  fclose(fp);
}

static uint64_t kv(const char* key) {
  for (int i = 0; i < g_nkv; i++)
    if (strcmp(g_key[i], key) == 0) return g_val[i];
  die("params.txt lacks", key);
  return 0;
}

static double kv_double(const char* key) {
  uint64_t bits = kv(key);
  double x;
  memcpy(&x, &bits, sizeof x);
  return x;
}

/* ---- status ------------------------------------------------------------------------------------ */
static void fail(const char* call, int st, int want) {
  fprintf(stderr, "abi_replay: %s\n  returned %d (%s), expected %d\n  rg_last_error: %s\n", call, st,
          rg_status_string(st), want, rg_last_error());
  exit(2);
}

#define CK(call)                              \
  do {                                        \
    int st_ = (int)(call);                    \
    if (st_ != RG_OK) fail(#call, st_, RG_OK); \
  } while (0)

/* ---- device memory: rg_malloc / rg_memcpy_* / rg_stream_sync only ------------------------------ */
enum { DEV_MAX = 128 };
static void* g_dev[DEV_MAX];
static int g_ndev;

static void* dalloc(size_t bytes) {
  void* d = NULL;
  if (g_ndev == DEV_MAX) die("too many device buffers", "");
  CK(rg_malloc(&d, bytes ? bytes : 8));
  g_dev[g_ndev++] = d;
  return d;
}

static void dfree_all(void) {
  while (g_ndev) CK(rg_free(g_dev[--g_ndev]));
}

static void h2d(void* d, const void* h, size_t bytes) {
  CK(rg_memcpy_h2d(d, h, bytes, NULL));
  CK(rg_stream_sync(NULL)); /* the host buffer may be reused only after the sync (ringo.h) */
}

static void d2h(void* h, const void* d, size_t bytes) {
  CK(rg_memcpy_d2h(h, d, bytes, NULL));
  CK(rg_stream_sync(NULL)); /* and read only after it */
}

/* an output buffer, pre-filled so a word the library leaves unwritten shows in the comparison */
static void* dout(size_t bytes) {
  void* h = xmalloc(bytes);
  memset(h, 0x5a, bytes);
  void* d = dalloc(bytes);
  h2d(d, h, bytes);
  free(h);
  return d;
}

static void* dput_file(const char* name, size_t bytes) {
  void* h = read_bin(name, bytes);
  void* d = dalloc(bytes);
  h2d(d, h, bytes);
  free(h);
  return d;
}

static void dsave(const char* name, const void* d, size_t bytes) {
  void* h = xmalloc(bytes);
  d2h(h, d, bytes);
  write_bin(name, h, bytes);
  free(h);
}

/* ---- layout ------------------------------------------------------------------------------------ */
#define P_SIZE(T) printf("sizeof." #T " %zu\n", sizeof(T))
#define P_FIELD(T, f) \
  printf(#T "." #f ".offset %zu\n" #T "." #f ".size %zu\n", offsetof(T, f), sizeof(((T*)0)->f))
#define P_ENUM(e) printf(#e " %d\n", (int)(e))

static int mode_layout(void) {
  P_SIZE(rg_jindo_params);
  P_FIELD(rg_jindo_params, rank);
  P_FIELD(rg_jindo_params, rows);
  P_FIELD(rg_jindo_params, cols);
  P_FIELD(rg_jindo_params, slots);
  P_FIELD(rg_jindo_params, exp);
  P_FIELD(rg_jindo_params, d);
  P_FIELD(rg_jindo_params, in_msis);
  P_FIELD(rg_jindo_params, out_msis);
  P_FIELD(rg_jindo_params, mlwe);
  P_FIELD(rg_jindo_params, dcmp);
  P_FIELD(rg_jindo_params, log_in_cut);
  P_FIELD(rg_jindo_params, log_out_cut);
  P_FIELD(rg_jindo_params, base);
  P_FIELD(rg_jindo_params, nq);
  P_FIELD(rg_jindo_params, nqo);
  P_FIELD(rg_jindo_params, q);
  P_FIELD(rg_jindo_params, qo);
  P_FIELD(rg_jindo_params, field_limbs);
  P_FIELD(rg_jindo_params, field_q);
  P_SIZE(rg_jindo_stddevs);
  P_FIELD(rg_jindo_stddevs, ecd);
  P_FIELD(rg_jindo_stddevs, ecd_blind);
  P_FIELD(rg_jindo_stddevs, mask);
  P_FIELD(rg_jindo_stddevs, mask_blind);
  P_FIELD(rg_jindo_stddevs, mlwe);
  P_FIELD(rg_jindo_stddevs, mask_mlwe);
  P_SIZE(rg_jindo_seeds);
  P_FIELD(rg_jindo_seeds, enc_cdt);
  P_FIELD(rg_jindo_seeds, enc_cosac);
  P_FIELD(rg_jindo_seeds, enc_cosac_round);
  P_FIELD(rg_jindo_seeds, mlwe_cdt);
  P_FIELD(rg_jindo_seeds, mlwe_round);
  P_FIELD(rg_jindo_seeds, uniform);
  P_SIZE(rg_jindo_verify_result);
  P_FIELD(rg_jindo_verify_result, outer_norm_sq);
  P_FIELD(rg_jindo_verify_result, inner_norm_sq);
  P_FIELD(rg_jindo_verify_result, outer_ok);
  P_FIELD(rg_jindo_verify_result, inner_ok);
  P_FIELD(rg_jindo_verify_result, consistency_ok);
  P_FIELD(rg_jindo_verify_result, eval_ok);
  P_FIELD(rg_jindo_verify_result, eval_lhs);
  P_FIELD(rg_jindo_verify_result, eval_rhs);
  P_FIELD(rg_jindo_verify_result, ok);
  P_SIZE(rg_status);
  P_ENUM(RG_OK);
  P_ENUM(RG_ERR_INVALID);
  P_ENUM(RG_ERR_NOT_POW2);
  P_ENUM(RG_ERR_UNSUPPORTED);
  P_ENUM(RG_ERR_DEVICE);
  P_ENUM(RG_ERR_NOMEM);
  P_ENUM(RG_ERR_RANK);
  P_ENUM(RG_VEC_ADD);
  P_ENUM(RG_VEC_SUB);
  P_ENUM(RG_VEC_NEG);
  P_ENUM(RG_VEC_MUL);
  P_ENUM(RG_VEC_SMUL);
  P_ENUM(RG_VEC_MUL_ADD);
  P_ENUM(RG_VEC_MUL_SUB);
  P_ENUM(RG_VEC_SMUL_ADD);
  P_ENUM(RG_VEC_SMUL_SUB);
  P_ENUM(RG_MAC_GENERIC);
  P_ENUM(RG_MAC_VALU3);
  P_ENUM(RG_MAC_MFMA);
  P_ENUM(RG_SAMPLER_LAYOUT);
  return 0;
}

/* ---- refusals: rejected on the host, before anything reaches a device --------------------------- */
#define EXPECT(want, call)                    \
  do {                                        \
    int st_ = (int)(call);                    \
    if (st_ != (want)) fail(#call, st_, want); \
    printf("%d %s\n", st_, #call);            \
  } while (0)

/* the same without the line of output */
#define QUIET(want, call)                     \
  do {                                        \
    int st_ = (int)(call);                    \
    if (st_ != (want)) fail(#call, st_, want); \
  } while (0)

static int mode_refuse(void) {
  const uint64_t q63[1] = {UINT64_C(0x4452100000000001)}; /* 47104^4 + 1 */
  const uint64_t even[1] = {4};
  uint64_t one[1] = {1}, out[1] = {0};
  int a = 0, b = 0;
  rg_field *f = NULL, *g = NULL;
  rg_ntt* t = NULL;
  CK(rg_field_create(1, q63, &f));
  EXPECT(RG_ERR_INVALID, rg_field_create(1, even, &g));
  EXPECT(RG_ERR_INVALID, rg_ntt_fwd(NULL, out, one, 1));
  EXPECT(RG_ERR_INVALID, rg_vec(NULL, RG_VEC_ADD, out, one, one, 1));
  EXPECT(RG_ERR_INVALID, rg_jindo_commit(NULL, one, 1, one, one, NULL, NULL, out, out, out, out));
  EXPECT(RG_ERR_INVALID, rg_jindo_mac_kinds(NULL, &a, &b));
  /* stride < n: refused by the argument check shared by the host and the device form */
  EXPECT(RG_ERR_INVALID, rg_poly_evaluate_batch(f, one, 8, 4, 2, one, out));
  EXPECT(RG_ERR_INVALID, rg_poly_evaluate_batch_dev(f, one, 8, 4, 2, one, out, out, NULL));
  EXPECT(RG_ERR_NOT_POW2, rg_ntt_create(f, 12, 1, &t));
  EXPECT(RG_ERR_INVALID, rg_set_probe(1)); /* the product library has no measurement switch */
  EXPECT(RG_OK, rg_set_probe(0));
  if (rg_jindo_scratch_bytes(NULL, 3) != 0) fail("rg_jindo_scratch_bytes(NULL, 3) != 0", 1, 0);
  /* the plan's route report: no plan, no route (checked, not printed) */
  if (rg_ntt_route_name(NULL, 0) != NULL || rg_ntt_route_name(NULL, 1) != NULL) fail("rg_ntt_route_name(NULL) != NULL", 1, 0);
  if (rg_ntt_passes(NULL, 0) != -1 || rg_ntt_passes(NULL, 1) != -1) fail("rg_ntt_passes(NULL) != -1", 1, 0);
  /* the Buckler verifier's entries: checked, not printed (the lines above are read as a fixed set) */
  {
    rg_bverifier* v = NULL;
    uint64_t word[1] = {0};
    QUIET(RG_ERR_INVALID, rg_buckler_verifier_create(NULL, 128, 4, 0, NULL, NULL, NULL, &v));
    QUIET(RG_ERR_INVALID, rg_buckler_verifier_create(NULL, 128, 4, 0, NULL, NULL, NULL, NULL));
    QUIET(RG_ERR_INVALID, rg_buckler_verify_checks_dev(NULL, one, NULL, one, one, word, NULL, NULL, out, NULL));
    QUIET(RG_ERR_INVALID, rg_buckler_verify_checks(NULL, one, NULL, one, one, word, NULL, NULL));
    if (v != NULL) fail("rg_buckler_verifier_create left a handle behind", 1, 0);
    if (rg_buckler_verifier_n_evals(NULL) != 0) fail("rg_buckler_verifier_n_evals(NULL) != 0", 1, 0);
    if (rg_buckler_verify_checks_scratch_bytes(NULL) != 0) fail("rg_buckler_verify_checks_scratch_bytes(NULL) != 0", 1, 0);
    rg_buckler_verifier_destroy(NULL);
  }
  rg_field_destroy(f);
  return 0;
}

/* ---- bigpoly -------------------------------------------------------- */
static int mode_bigpoly(void) {
  kv_load();
  const int L = (int)kv("limbs"), N = (int)kv("rank"), neg = (int)kv("negacyclic");
  const size_t batch = kv("batch"), eval_n = kv("eval_n"), stride = kv("stride");
  const long long n_vanish = (long long)kv("n_vanish"), aut_idx = (long long)kv("aut_idx");
  const size_t e = (size_t)L * 8, poly = (size_t)N * e, all = batch * poly;

  uint64_t* q = read_bin("q", e);
  rg_field* f = NULL;
  CK(rg_field_create(L, q, &f));
  uint64_t* consts = xmalloc((1 + 2 * (size_t)L) * 8); /* qinv_neg, r2[L], one[L] */
  CK(rg_field_constants(f, consts, consts + 1, consts + 1 + L));
  write_bin("consts", consts, (1 + 2 * (size_t)L) * 8);

  /* the Go transformer's tables, verbatim, and read back */
  uint64_t *tw = read_bin("tw", poly), *twi = read_bin("tw_inv", poly), *ri = read_bin("rank_inv", e);
  rg_ntt* t = NULL;
  CK(rg_ntt_create_from_tables(f, N, neg, tw, twi, ri, &t));
  memset(tw, 0, poly);
  memset(twi, 0, poly);
  memset(ri, 0, e);
  CK(rg_ntt_tables(t, tw, twi, ri));
  write_bin("tw_out", tw, poly);
  write_bin("tw_inv_out", twi, poly);
  write_bin("rank_inv_out", ri, e);
  const uint64_t info[2] = {(uint64_t)rg_field_limbs(f), (uint64_t)rg_ntt_rank(t)};
  write_bin("info", info, sizeof info);

  /* host forms, in place as the shim calls them */
  uint64_t *a = read_bin("a", all), *b = read_bin("b", all), *x = read_bin("x", e);
  uint64_t* buf = xmalloc(all);
  memcpy(buf, a, all);
  CK(rg_ntt_fwd(t, buf, buf, batch));
  write_bin("fwd", buf, all);
  CK(rg_ntt_inv(t, buf, buf, batch));
  write_bin("inv", buf, all);
  CK(rg_vec(f, RG_VEC_MUL, buf, a, b, batch * (size_t)N));
  write_bin("mul", buf, all);
  uint64_t* rem = xmalloc(poly);
  CK(rg_poly_quorem_vanishing(f, (size_t)N, n_vanish, buf, rem, a));
  write_bin("quo", buf, poly);
  write_bin("rem", rem, poly);
  CK(rg_poly_aut(f, (size_t)N, aut_idx, 0, buf, a));
  write_bin("aut", buf, poly);
  CK(rg_poly_evaluate(f, a, (size_t)N, x, buf));
  write_bin("eval", buf, e);

  /* the same data on rg_malloc'd buffers */
  uint64_t *d_a = dalloc(all), *d_b = dalloc(all), *d_x = dalloc(e);
  h2d(d_a, a, all);
  h2d(d_b, b, all);
  h2d(d_x, x, e);
  uint64_t *d_fwd = dout(all), *d_mul = dout(all);
  CK(rg_ntt_fwd_dev(t, d_fwd, d_a, batch, NULL)); /* out of place */
  dsave("fwd_dev", d_fwd, all);
  CK(rg_vec_dev(f, RG_VEC_MUL, d_mul, d_fwd, d_b, batch * (size_t)N, NULL));
  dsave("mul_dev", d_mul, all);
  CK(rg_ntt_inv_dev(t, d_mul, d_mul, batch, NULL)); /* in place */
  dsave("inv_dev", d_mul, all);
  const size_t scr = rg_poly_evaluate_batch_scratch_bytes(f, eval_n, batch);
  void* d_scr = dalloc(scr);
  uint64_t* d_ev = dout(batch * e);
  CK(rg_poly_evaluate_batch_dev(f, d_a, eval_n, stride, batch, d_x, d_ev, d_scr, NULL));
  dsave("eval_batch_dev", d_ev, batch * e);

  dfree_all();
  rg_ntt_destroy(t);
  rg_field_destroy(f);
  free(q), free(consts), free(tw), free(twi), free(ri), free(a), free(b), free(x), free(buf), free(rem);
  return 0;
}

/* ---- jindo ---------------------------------------------------------- */
static int mode_jindo(void) {
  kv_load();
  rg_jindo_params p;
  memset(&p, 0, sizeof p);
  p.rank = (int)kv("rank"), p.rows = (int)kv("rows"), p.cols = (int)kv("cols"), p.slots = (int)kv("slots");
  p.exp = (int)kv("exp"), p.d = (int)kv("d");
  p.in_msis = (int)kv("in_msis"), p.out_msis = (int)kv("out_msis"), p.mlwe = (int)kv("mlwe");
  p.dcmp = (int)kv("dcmp");
  p.log_in_cut = (int)kv("log_in_cut"), p.log_out_cut = (int)kv("log_out_cut");
  p.base = kv("base");
  p.nq = (int)kv("nq"), p.nqo = (int)kv("nqo");
  for (int i = 0; i < p.nq; i++) p.q[i] = kv(idx("q", (size_t)i));
  for (int i = 0; i < p.nqo; i++) p.qo[i] = kv(idx("qo", (size_t)i));
  p.field_limbs = (int)kv("field_limbs");
  for (int i = 0; i < p.field_limbs; i++) p.field_q[i] = kv(idx("field_q", (size_t)i));

  const size_t L = (size_t)p.field_limbs, d = (size_t)p.d, nq = (size_t)p.nq, nqo = (size_t)p.nqo;
  const size_t cols = (size_t)p.cols, rows = (size_t)p.rows, slots = (size_t)p.slots, c1 = cols + 1;
  const size_t nm = (size_t)(p.in_msis + p.mlwe), in_msis = (size_t)p.in_msis, out_msis = (size_t)p.out_msis;
  const size_t dcmp = (size_t)p.dcmp, e = L * 8;
  /* sizes in bytes, as include/ringo.h lays the arrays out */
  const size_t z_ck_in = in_msis * rows * nq * d * 8, z_ck_mlwe = in_msis * (size_t)p.mlwe * nq * d * 8;
  const size_t z_ck_out = out_msis * dcmp * nqo * d * 8;
  const size_t z_last = cols * slots * e, z_mask = rows * slots * e, z_en = c1 * rows * d * 8, z_mn = c1 * nm * d * 8;
  const size_t z_incom = dcmp * nqo * d * 8, z_enc = c1 * rows * nq * d * 8, z_mlwe = c1 * nm * nq * d * 8;
  const size_t z_com = out_msis * nq * d * 8;
  const size_t z_partial = c1 * nq * d * 8, z_pf_enc = rows * nq * d * 8, z_pf_mlwe = nm * nq * d * 8;

  /* 1. NewProver from the CRS; the derived key; which kernels the handle chose */
  static const uint8_t crs[6] = {'J', 'i', 'n', 'd', 'o', '!'};
  rg_jindo* j = NULL;
  CK(rg_jindo_create_from_crs(&p, crs, sizeof crs, &j));
  {
    uint64_t *a = xmalloc(z_ck_in), *b = xmalloc(z_ck_mlwe), *c = xmalloc(z_ck_out);
    CK(rg_jindo_commit_key(j, a, b, c));
    write_bin("ck_in", a, z_ck_in);
    write_bin("ck_mlwe", b, z_ck_mlwe);
    write_bin("ck_out", c, z_ck_out);
    free(a), free(b), free(c);
    int32_t kinds[2];
    int inner = -1, outer = -1;
    CK(rg_jindo_mac_kinds(j, &inner, &outer));
    kinds[0] = inner, kinds[1] = outer;
    write_bin("mac_kinds", kinds, sizeof kinds);
  }

  /* 2. Prover.Commit on host arrays, randomness injected */
  const size_t ncases = kv("ncases");
  for (size_t i = 0; i < ncases; i++) {
    const size_t nv = kv(idx("case_nv", i));
    uint64_t *v = read_bin(idx("case_v", i), nv * e), *last = read_bin(idx("case_last_row", i), z_last);
    uint64_t* mask = read_bin(idx("case_mask", i), z_mask);
    int64_t *en = read_bin(idx("case_enc_noise", i), z_en), *mn = read_bin(idx("case_mlwe_noise", i), z_mn);
    uint64_t *o_incom = xmalloc(z_incom), *o_enc = xmalloc(z_enc), *o_mlwe = xmalloc(z_mlwe), *o_com = xmalloc(z_com);
    CK(rg_jindo_commit(j, v, nv, last, mask, en, mn, o_incom, o_enc, o_mlwe, o_com));
    write_bin(idx("case_incom", i), o_incom, z_incom);
    write_bin(idx("case_enc", i), o_enc, z_enc);
    write_bin(idx("case_mlwe", i), o_mlwe, z_mlwe);
    write_bin(idx("case_com", i), o_com, z_com);
    free(v), free(last), free(mask), free(en), free(mn), free(o_incom), free(o_enc), free(o_mlwe), free(o_com);
  }

  /* 3. the batch on the device: Commit, Evaluate, Verify */
  const size_t B = kv("batch"), nv = kv("nv");
  uint64_t* d_v = dput_file("v", B * nv * e);
  {
    uint64_t *d_last = dput_file("last_row", B * z_last), *d_mask = dput_file("mask", B * z_mask);
    int64_t *d_en = dput_file("enc_noise", B * z_en), *d_mn = dput_file("mlwe_noise", B * z_mn);
    uint64_t *d_incom = dout(B * z_incom), *d_enc = dout(B * z_enc), *d_mlwe = dout(B * z_mlwe);
    uint64_t* d_com = dout(B * z_com);
    CK(rg_jindo_commit_dev(j, B, d_v, nv, d_last, d_mask, d_en, d_mn, d_incom, d_enc, d_mlwe, d_com, NULL));
    dsave("incom", d_incom, B * z_incom);
    dsave("enc", d_enc, B * z_enc);
    dsave("mlwe", d_mlwe, B * z_mlwe);
    dsave("com", d_com, B * z_com);

    /* the challenges from the transcript's bytes: both rings for the batch, ringQ for the columns */
    uint64_t *d_bq = NULL, *d_bo = NULL;
    if (B > 1) {
      uint8_t* d_bb = dput_file("bbytes", 16 * B);
      d_bq = dout(B * nq * d * 8), d_bo = dout(B * nqo * d * 8);
      CK(rg_jindo_encode_challenges_dev(j, 0, d_bb, B, d_bq, NULL));
      CK(rg_jindo_encode_challenges_dev(j, 1, d_bb, B, d_bo, NULL));
      dsave("bq", d_bq, B * nq * d * 8);
      dsave("bo", d_bo, B * nqo * d * 8);
    }
    uint8_t* d_cb = dput_file("cbytes", 16 * cols);
    uint64_t* d_chals = dout(cols * nq * d * 8);
    CK(rg_jindo_encode_challenges_dev(j, 0, d_cb, cols, d_chals, NULL));
    dsave("chals", d_chals, cols * nq * d * 8);

    /* the point's vectors: the verifier's call (left and right) and the prover's (left only) */
    uint64_t* d_x = dput_file("x", e);
    uint64_t *d_left = dout(z_pf_enc), *d_right = dout(z_last), *d_left_only = dout(z_pf_enc);
    CK(rg_jindo_eval_point_dev(j, d_x, d_left, d_right, NULL));
    CK(rg_jindo_eval_point_dev(j, d_x, d_left_only, NULL, NULL));
    dsave("left", d_left, z_pf_enc);
    dsave("right", d_right, z_last);
    dsave("left_only", d_left_only, z_pf_enc);

    /* evals[i] = Poly(v[i]).Evaluate(x) on the device copies of v that Commit read */
    rg_field* f = NULL;
    CK(rg_field_create(p.field_limbs, p.field_q, &f));
    void* d_scr = dalloc(rg_poly_evaluate_batch_scratch_bytes(f, nv, B));
    uint64_t* d_y = dout(B * e);
    CK(rg_poly_evaluate_batch_dev(f, d_v, nv, nv, B, d_x, d_y, d_scr, NULL));
    dsave("y", d_y, B * e);

    uint64_t *d_ob_incom = dout(z_incom), *d_ob_enc = dout(z_enc), *d_ob_mlwe = dout(z_mlwe);
    CK(rg_jindo_eval_batch_dev(j, B, d_incom, d_enc, d_mlwe, d_bq, d_bo, d_ob_incom, d_ob_enc, d_ob_mlwe, NULL));
    dsave("ob_incom", d_ob_incom, z_incom);
    dsave("ob_enc", d_ob_enc, z_enc);
    dsave("ob_mlwe", d_ob_mlwe, z_mlwe);
    uint64_t* d_partial = dout(z_partial);
    CK(rg_jindo_eval_partial_dev(j, d_ob_enc, d_left, d_partial, NULL));
    dsave("partial", d_partial, z_partial);
    uint64_t *d_pf_enc = dout(z_pf_enc), *d_pf_mlwe = dout(z_pf_mlwe);
    CK(rg_jindo_eval_respond_dev(j, d_ob_enc, d_ob_mlwe, d_chals, d_pf_enc, d_pf_mlwe, NULL));
    dsave("pf_enc", d_pf_enc, z_pf_enc);
    dsave("pf_mlwe", d_pf_mlwe, z_pf_mlwe);

    const double in_nm = kv_double("in_com_dcmp_two_nm"), res_nm = kv_double("res_two_nm");
    rg_jindo_verify_result res;
    memset(&res, 0, sizeof res); /* padding included: the struct is written out raw */
    CK(rg_jindo_verify_dev(j, B, d_com, d_bq, d_bo, d_chals, d_left, d_right, d_y, d_ob_incom, d_partial, d_pf_enc,
                           d_pf_mlwe, in_nm, res_nm, &res, NULL));
    write_bin("verify", &res, sizeof res);
    /* the same proof with one word of the last y changed */
    uint64_t* y = xmalloc(B * e);
    d2h(y, d_y, B * e);
    y[(B - 1) * L] ^= 1;
    h2d(d_y, y, B * e);
    free(y);
    memset(&res, 0, sizeof res);
    CK(rg_jindo_verify_dev(j, B, d_com, d_bq, d_bo, d_chals, d_left, d_right, d_y, d_ob_incom, d_partial, d_pf_enc,
                           d_pf_mlwe, in_nm, res_nm, &res, NULL));
    write_bin("verify_bad_y", &res, sizeof res);
    rg_field_destroy(f);
  }

  /* 4. the randomness drawn on the device */
  {
    rg_jindo_stddevs sd;
    sd.ecd = kv_double("ecd_sd"), sd.ecd_blind = kv_double("ecd_blind_sd");
    sd.mask = kv_double("mask_sd"), sd.mask_blind = kv_double("mask_blind_sd");
    sd.mlwe = kv_double("mlwe_sd"), sd.mask_mlwe = kv_double("mask_mlwe_sd");
    CK(rg_jindo_set_stddevs(j, &sd));
    double* delta = xmalloc((size_t)p.exp * sizeof *delta);
    CK(rg_jindo_delta_inv(j, delta));
    write_bin("delta_inv", delta, (size_t)p.exp * sizeof *delta);
    free(delta);
    uint8_t* raw = read_bin("seeds", 6 * 32);
    rg_jindo_seeds seeds;
    memcpy(seeds.enc_cdt, raw, 32);
    memcpy(seeds.enc_cosac, raw + 32, 32);
    memcpy(seeds.enc_cosac_round, raw + 64, 32);
    memcpy(seeds.mlwe_cdt, raw + 96, 32);
    memcpy(seeds.mlwe_round, raw + 128, 32);
    memcpy(seeds.uniform, raw + 160, 32);
    free(raw);
    const unsigned long long first_commit = kv("first_commit");
    uint64_t *d_incom = dout(B * z_incom), *d_enc = dout(B * z_enc), *d_mlwe = dout(B * z_mlwe);
    uint64_t* d_com = dout(B * z_com);
    CK(rg_jindo_commit_sampled_dev(j, B, d_v, nv, &seeds, first_commit, d_incom, d_enc, d_mlwe, d_com, NULL));
    dsave("sampled_incom", d_incom, B * z_incom);
    dsave("sampled_enc", d_enc, B * z_enc);
    dsave("sampled_mlwe", d_mlwe, B * z_mlwe);
    dsave("sampled_com", d_com, B * z_com);
  }

  dfree_all();
  rg_jindo_destroy(j);
  return 0;
}

/* ---- buckler -------------------------------------------------------- */
static int mode_buckler(void) {
  kv_load();
  const int L = (int)kv("limbs");
  const size_t rank = kv("rank"), emb = kv("emb"), jindo_rank = kv("jindo_rank"), n_w = kv("n_w");
  const size_t nb = kv("recompose_nb"), n_pairs = kv("n_pairs");
  const long long aut_idx = (long long)kv("aut_idx");
  const size_t e = (size_t)L * 8;
  enum { N_CHK = 4 };

  uint64_t* q = read_bin("q", e);
  rg_field* f = NULL;
  CK(rg_field_create(L, q, &f));
  rg_ntt *enc_plan = NULL, *emb_plan = NULL; /* the encoder's and the evaluator's cyclic transformers */
  CK(rg_ntt_create(f, (int)rank, 0, &enc_plan));
  CK(rg_ntt_create(f, (int)emb, 0, &emb_plan));

  /* ctx.linCheckers: one checker of each kind, the projection matrix from the XOF bytes */
  rg_linchecker* chk[N_CHK] = {NULL, NULL, NULL, NULL};
  uint64_t* rbase = read_bin("recompose_base", nb * e);
  uint8_t* xof = read_bin("xof", rank * 32);
  CK(rg_buckler_checker_create_ntt(f, rank, &chk[0]));
  CK(rg_buckler_checker_create_aut(f, rank, aut_idx, 0, &chk[1]));
  CK(rg_buckler_checker_create_proj(f, rank, &chk[2]));
  CK(rg_buckler_checker_create_recompose(f, rank, rbase, nb, &chk[3]));
  CK(rg_buckler_checker_set_xof(chk[2], xof));

  /* ctx.linCheckConstraints: the handle array and the size_t offsets, as cgo passes them */
  uint64_t* off64 = read_bin("pair_off", (N_CHK + 1) * 8);
  size_t pair_off[N_CHK + 1];
  for (int i = 0; i <= N_CHK; i++) pair_off[i] = (size_t)off64[i];
  uint64_t* pairs = read_bin("pairs", n_pairs * 2 * 8);
  const rg_linchecker* const chks[N_CHK] = {chk[0], chk[1], chk[2], chk[3]};
  rg_lincheck* lc = NULL;
  CK(rg_buckler_lincheck_create(enc_plan, emb_plan, N_CHK, chks, pair_off, pairs, &lc));

  /* linCheckMask from 2 rank uploaded draws, then linCheck on wEcdNTT */
  uint64_t* d_rand = dput_file("rand", 2 * rank * e);
  uint64_t *d_mask = dout(emb * e), *d_sum = dout(e);
  CK(rg_buckler_sumcheck_mask_dev(f, rank, 2 * rank, emb, d_rand, d_mask, d_sum, NULL));
  dsave("mask", d_mask, emb * e);
  dsave("mask_sum", d_sum, e);
  uint64_t *d_bc = dput_file("bc", e), *d_lc = dput_file("lc", e), *d_w = dput_file("w", n_w * emb * e);
  uint64_t *d_quo = dout(rank * e), *d_lo = dout((rank - 1) * e), *d_hi = dout(jindo_rank * e);
  const size_t scr = rg_buckler_lin_check_scratch_bytes(lc), rem_off = rg_buckler_lin_check_rem_offset_bytes(lc);
  if (rem_off + e > scr) fail("rg_buckler_lin_check_rem_offset_bytes(lc) + element > scratch", 1, 0);
  unsigned char* d_scr = dalloc(scr);
  CK(rg_buckler_lin_check_dev(lc, d_bc, d_lc, d_mask, d_w, n_w, jindo_rank, d_quo, d_lo, d_hi, (uint64_t*)(void*)d_scr,
                              NULL));
  dsave("quo", d_quo, rank * e);
  dsave("rem_lo", d_lo, (rank - 1) * e);
  dsave("rem_hi", d_hi, jindo_rank * e);
  dsave("rem0", d_scr + rem_off, e);

  /* the infinity-norm digits of dcmp_batch witnesses, straight into RandEncode */
  const size_t dnb = kv("dcmp_nb"), dbatch = kv("dcmp_batch");
  uint64_t* dbase = read_bin("dcmp_base", dnb * e);
  rg_dcmp* dc = NULL;
  CK(rg_buckler_dcmp_create(f, dbase, dnb, &dc));
  uint64_t* d_dw = dput_file("dcmp_w", dbatch * rank * e);
  uint64_t* d_dig = dout(dbatch * dnb * rank * e);
  CK(rg_buckler_dcmp_inf_dev(dc, d_dw, dbatch, rank, d_dig, NULL));
  dsave("digits", d_dig, dbatch * dnb * rank * e);
  uint64_t* d_blind = dput_file("blind", dbatch * dnb * e);
  uint64_t* d_escr = dalloc(rg_buckler_encode_scratch_bytes(enc_plan, dbatch * dnb));
  uint64_t* d_ecd = dout(dbatch * dnb * emb * e);
  CK(rg_buckler_encode_dev(enc_plan, emb, d_ecd, d_dig, dbatch * dnb, d_blind, d_escr, NULL));
  dsave("ecd", d_ecd, dbatch * dnb * emb * e);

  dfree_all();
  rg_buckler_dcmp_destroy(dc);
  rg_buckler_lincheck_destroy(lc);
  for (int i = 0; i < N_CHK; i++) rg_buckler_checker_destroy(chk[i]);
  rg_ntt_destroy(emb_plan);
  rg_ntt_destroy(enc_plan);
  rg_field_destroy(f);
  free(q), free(rbase), free(xof), free(off64), free(pairs), free(dbase);
  return 0;
}

/* ---- Verifier.Verify's checks --------------------------------------- */
/* One constraint list as rg_buckler_circuit_create takes it: PREFIX_term_off [nc + 1], PREFIX_coeffs
 * [nt][L], PREFIX_pw_idx [nt] (int64, < 0: none), PREFIX_wit_off [nt + 1], PREFIX_wit [nwit]. */
static rg_circuit* circuit_from_files(const rg_field* f, const char* prefix, size_t e) {
  char key[64], name[64];
  snprintf(key, sizeof key, "%s_nc", prefix);
  const size_t nc = kv(key);
  snprintf(key, sizeof key, "%s_nt", prefix);
  const size_t nt = kv(key);
  snprintf(key, sizeof key, "%s_nwit", prefix);
  const size_t nwit = kv(key);
  snprintf(name, sizeof name, "%s_term_off", prefix);
  uint64_t* to64 = read_bin(name, (nc + 1) * 8);
  snprintf(name, sizeof name, "%s_coeffs", prefix);
  uint64_t* coeffs = read_bin(name, nt * e);
  snprintf(name, sizeof name, "%s_pw_idx", prefix);
  long long* pw_idx = read_bin(name, nt * 8);
  snprintf(name, sizeof name, "%s_wit_off", prefix);
  uint64_t* wo64 = read_bin(name, (nt + 1) * 8);
  snprintf(name, sizeof name, "%s_wit", prefix);
  uint64_t* wit = read_bin(name, nwit * 8);
  size_t* term_off = xmalloc((nc + 1) * sizeof *term_off);
  size_t* wit_off = xmalloc((nt + 1) * sizeof *wit_off);
  for (size_t i = 0; i <= nc; i++) term_off[i] = (size_t)to64[i];
  for (size_t i = 0; i <= nt; i++) wit_off[i] = (size_t)wo64[i];
  rg_circuit* c = NULL;
  CK(rg_buckler_circuit_create(f, nc, term_off, coeffs, pw_idx, wit_off, wit, &c));
  free(to64), free(coeffs), free(pw_idx), free(wo64), free(wit), free(term_off), free(wit_off);
  return c;
}

static int mode_bverify(void) {
  kv_load();
  const int L = (int)kv("limbs");
  const size_t rank = kv("rank"), jindo_rank = kv("jindo_rank"), w_cnt = kv("w_cnt"), n_pw = kv("n_pw");
  const size_t nb = kv("recompose_nb"), n_pairs = kv("n_pairs"), ncases = kv("ncases");
  const long long aut_idx = (long long)kv("aut_idx");
  const size_t e = (size_t)L * 8;
  enum { N_CHK = 4 };

  /* what Compile fixes: the encoder's plan, the checkers, the three constraint sets */
  uint64_t* q = read_bin("q", e);
  rg_field* f = NULL;
  CK(rg_field_create(L, q, &f));
  rg_ntt* enc_plan = NULL;
  CK(rg_ntt_create(f, (int)rank, 0, &enc_plan));
  rg_linchecker* chk[N_CHK] = {NULL, NULL, NULL, NULL};
  uint64_t* rbase = read_bin("recompose_base", nb * e);
  uint8_t* xof = read_bin("xof", rank * 32);
  CK(rg_buckler_checker_create_ntt(f, rank, &chk[0]));
  CK(rg_buckler_checker_create_aut(f, rank, aut_idx, 0, &chk[1]));
  CK(rg_buckler_checker_create_proj(f, rank, &chk[2]));
  CK(rg_buckler_checker_create_recompose(f, rank, rbase, nb, &chk[3]));
  uint64_t* off64 = read_bin("pair_off", (N_CHK + 1) * 8);
  size_t pair_off[N_CHK + 1];
  for (int i = 0; i <= N_CHK; i++) pair_off[i] = (size_t)off64[i];
  uint64_t* pairs = read_bin("pairs", n_pairs * 2 * 8);
  const rg_linchecker* const chks[N_CHK] = {chk[0], chk[1], chk[2], chk[3]};
  rg_lincheck* lc = NULL; /* the verifier never reads the embedding plan: the encoder's stands in */
  CK(rg_buckler_lincheck_create(enc_plan, enc_plan, N_CHK, chks, pair_off, pairs, &lc));
  rg_circuit *arith = circuit_from_files(f, "arith", e), *sum = circuit_from_files(f, "sum", e);
  rg_bverifier* v = NULL;
  CK(rg_buckler_verifier_create(enc_plan, jindo_rank, w_cnt, n_pw, lc, arith, sum, &v));
  const size_t n_evals = rg_buckler_verifier_n_evals(v);
  const uint64_t info[2] = {(uint64_t)n_evals, (uint64_t)rg_buckler_verify_checks_scratch_bytes(v)};
  write_bin("info", info, sizeof info);

  /* per proof: the projection matrix from the transcript's XOF bytes, then one call and one word */
  CK(rg_buckler_checker_set_xof(chk[2], xof));
  uint64_t* d_pw = dput_file("pw", n_pw * rank * e);
  uint64_t* d_scr = dalloc(rg_buckler_verify_checks_scratch_bytes(v));
  for (size_t i = 0; i < ncases; i++) {
    uint64_t* d_evals = dput_file(idx("evals", i), n_evals * e);
    uint64_t *d_chal = dput_file(idx("chal", i), 5 * e), *d_ms = dput_file(idx("mask_sums", i), 2 * e);
    uint64_t *d_verdict = dout(8), *d_sides = dout(8 * e), *d_pwe = dout(n_pw * e);
    CK(rg_buckler_verify_checks_dev(v, d_evals, d_pw, d_chal, d_ms, d_verdict, d_sides, d_pwe, d_scr, NULL));
    uint64_t verdict = 0;
    d2h(&verdict, d_verdict, 8); /* the one word */
    printf("case %zu verdict %" PRIu64 "\n", i, verdict);
    write_bin(idx("verdict", i), &verdict, 8);
    dsave(idx("sides", i), d_sides, 8 * e);
    dsave(idx("pw_evals", i), d_pwe, n_pw * e);
  }
  /* the host-pointer form on the first case */
  {
    uint64_t *evals = read_bin(idx("evals", 0), n_evals * e), *pw = read_bin("pw", n_pw * rank * e);
    uint64_t *chal = read_bin(idx("chal", 0), 5 * e), *ms = read_bin(idx("mask_sums", 0), 2 * e);
    uint64_t verdict = ~UINT64_C(0), *sides = xmalloc(8 * e), *pwe = xmalloc(n_pw * e);
    CK(rg_buckler_verify_checks(v, evals, pw, chal, ms, &verdict, sides, pwe));
    write_bin("host_verdict", &verdict, 8);
    write_bin("host_sides", sides, 8 * e);
    write_bin("host_pw_evals", pwe, n_pw * e);
    free(evals), free(pw), free(chal), free(ms), free(sides), free(pwe);
  }

  dfree_all();
  rg_buckler_verifier_destroy(v);
  rg_buckler_circuit_destroy(arith);
  rg_buckler_circuit_destroy(sum);
  rg_buckler_lincheck_destroy(lc);
  for (int i = 0; i < N_CHK; i++) rg_buckler_checker_destroy(chk[i]);
  rg_ntt_destroy(enc_plan);
  rg_field_destroy(f);
  free(q), free(rbase), free(xof), free(off64), free(pairs);
  return 0;
}

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  if (argc > 2) g_dir = argv[2];
  if (strcmp(mode, "layout") == 0) return mode_layout();
  if (strcmp(mode, "refuse") == 0) return mode_refuse();
  if (argc > 2 && strcmp(mode, "bigpoly") == 0) return mode_bigpoly();
  if (argc > 2 && strcmp(mode, "jindo") == 0) return mode_jindo();
  if (argc > 2 && strcmp(mode, "buckler") == 0) return mode_buckler();
  if (argc > 2 && strcmp(mode, "bverify") == 0) return mode_bverify();
  fprintf(stderr, "usage: abi_replay layout|refuse [DIR] | bigpoly|jindo|buckler|bverify DIR\n");
  return 3;
}
