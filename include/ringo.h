/* ringo.h -- C ABI of libringo, the MI355X (gfx950) implementation of ringo-snark's
 * NTT / Jindo-commit hot path.
 *
 * Every entry point is what the reference's Go side would bind through cgo (see
 * INTEGRATION.md for the binding).  The reference interface each one replaces is cited as
 * path:line into sp301415/ringo-snark.  Plain pointers and sizes only; no torch types.
 *
 * Conventions
 *  - Field elements are gnark `Uint [L]uint64` values in Montgomery form (R = 2^(64L)),
 *    little-endian limbs, fully reduced (jindo/internal/zp/element.go:37-51).  A polynomial
 *    of rank N is N consecutive elements: layout [N][L] (what a contiguous []zp.Uint holds).
 *  - Batched calls take [batch][N][L] with polys back to back.
 *  - Jindo ring polynomials use Lattigo's limb-major layout Coeffs[limb][coeff]
 *    (ring.Poly, lattigo/v6 v6.1.0).
 *  - `*_dev` entry points take DEVICE pointers and a hipStream_t (passed as void*; NULL =
 *    the null stream) and are asynchronous.  Entry points without `_dev` take HOST pointers
 *    and are synchronous (they stage through library-owned device buffers).
 *  - Outputs may alias inputs exactly (out == in); partial overlap is invalid.
 *  - Return value: RG_OK or a negative rg_status; the library never aborts.  The Go shim
 *    maps the codes to the reference's panics (messages in rg_status_string).
 *  - Handles are immutable after creation and may be shared by threads; each call is
 *    thread-safe (host staging is per call).  A Jindo handle keeps device scratch per HIP
 *    stream, so concurrent `_dev` calls on different streams never share scratch; calls on
 *    one stream are ordered by the stream.  A handle belongs to the device that was current
 *    when it was created (RG_ERR_INVALID elsewhere); one handle per GPU.
 */
#ifndef RINGO_H
#define RINGO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  RG_OK = 0,
  RG_ERR_INVALID = -1,     /* shape/argument error  -> Go panic "inconsistent input(s)" */
  RG_ERR_NOT_POW2 = -2,    /* ntt.go:27-29,154-156  "rank must be a power of two" */
  RG_ERR_UNSUPPORTED = -3, /* ntt.go:35-37,162-164  "NTT not supported" */
  RG_ERR_DEVICE = -4,      /* HIP runtime error (message via rg_last_error) */
  RG_ERR_NOMEM = -5,
  RG_ERR_RANK = -6         /* jindo/prover.go:46-49 "len(v) > params.rank" */
} rg_status;

const char* rg_status_string(int status);
/* Thread-local text of the last device error (hipGetErrorString + call site). */
const char* rg_last_error(void);
/* Library build id (kernel set + gfx target + sampler layout), for logs.  The string ends in
 * "sampler-layout N" with N = RG_SAMPLER_LAYOUT of the build: the partition of the device
 * samplers' draws into UniformSampler instances (rg_jindo_seeds).  The same seeds and
 * first_commit give the same sampled commitments only between builds of one layout.
 *   1: rounds 3-4 (COSAC instances per group of 16 coefficients)
 *   2: round 5 on (COSAC instances per group of 8 coefficients) */
#define RG_SAMPLER_LAYOUT 2
const char* rg_version(void);

/* ------------------------------------------------------------------------------------ */
/* Field (math/bignum.Uint[E], gnark-generated zp.Uint)                                   */
/* ------------------------------------------------------------------------------------ */
typedef struct rg_field rg_field;

/* Replaces the compile-time field type E.  q_le: the modulus as `limbs` little-endian
 * words (zp.q0..q{L-1}, element.go:47-50).  The library derives qInvNeg (element.go:72) and
 * R^2 (element.go:784) itself; rg_field_constants exposes them for cross-checks.
 * limbs in 1..16. */
rg_status rg_field_create(int limbs, const uint64_t* q_le, rg_field** out);
void rg_field_destroy(rg_field* f);
int rg_field_limbs(const rg_field* f);
/* qinv_neg: -q^-1 mod 2^64; r2_le, one_le: R^2 mod q and R mod q (limbs words each). */
rg_status rg_field_constants(const rg_field* f, uint64_t* qinv_neg, uint64_t* r2_le, uint64_t* one_le);

/* ------------------------------------------------------------------------------------ */
/* bigpoly transformers (math/bigpoly/ntt.go)                                             */
/* ------------------------------------------------------------------------------------ */
typedef struct rg_ntt rg_ntt;

/* Replaces NewCyclotomicTransformer (negacyclic=1, ntt.go:153-203) and
 * NewCyclicTransformer (negacyclic=0, ntt.go:26-95).  The library derives psi/omega by the
 * reference's generator search (first x = 2,3,... ; ntt.go:46-53,173-180) and builds the
 * twiddle tables itself. */
rg_status rg_ntt_create(const rg_field* f, int rank, int negacyclic, rg_ntt** out);
/* Same, but with the tables taken verbatim from the Go transformer (tw, twInv: rank
 * elements each in Montgomery form, laid out [rank][L]; rank_inv: one element), so twiddle
 * parity holds by construction.  Tables are validated (tw[0] == twInv[0] == 1). */
rg_status rg_ntt_create_from_tables(const rg_field* f, int rank, int negacyclic, const uint64_t* tw,
                                    const uint64_t* tw_inv, const uint64_t* rank_inv, rg_ntt** out);
void rg_ntt_destroy(rg_ntt* t);
int rg_ntt_rank(const rg_ntt* t); /* Rank() (ntt.go:139,469) */
/* Which kernel family serves this plan in one direction, and in how many passes.  name is "stages" (0
 * passes: one launch per stage), "tiled" (1 or 2), "lazy64" (2), "fast256" (2 at rank 2^15 / 2^16, 3 at
 * 2^17 .. 2^19), "wide" (1 or 2 up to rank 2^16, 3 at 2^17 .. 2^24).  Reads the plan only. */
const char* rg_ntt_route_name(const rg_ntt* t, int inverse);
int rg_ntt_passes(const rg_ntt* t, int inverse);
/* Copy the tables out (Montgomery, [rank][L] each + one element). */
rg_status rg_ntt_tables(const rg_ntt* t, uint64_t* tw, uint64_t* tw_inv, uint64_t* rank_inv);

/* FwdNTTTo(vOut, v) (ntt.go:98-115,206-223) on `batch` polys: natural -> bit-reversed.
 * The _dev forms order all their work on `stream`; a "fast256" plan (4 limbs, q = 1 mod 2^64, q < 2^255)
 * runs half of its work on a helper stream of its own, forked from and joined back into `stream`: at
 * rank 2^15 / 2^16 from a batch of 8 up, at rank 2^17 .. 2^19 from 8 blocks of 2^16 points up (batch
 * 4, 2, 1). */
rg_status rg_ntt_fwd(const rg_ntt* t, uint64_t* out, const uint64_t* in, size_t batch);
rg_status rg_ntt_fwd_dev(const rg_ntt* t, uint64_t* d_out, const uint64_t* d_in, size_t batch, void* stream);
/* InvNTTTo(vOut, v) (ntt.go:118-136,226-244): bit-reversed -> natural, times rank^-1. */
rg_status rg_ntt_inv(const rg_ntt* t, uint64_t* out, const uint64_t* in, size_t batch);
rg_status rg_ntt_inv_dev(const rg_ntt* t, uint64_t* d_out, const uint64_t* d_in, size_t batch, void* stream);

/* ------------------------------------------------------------------------------------ */
/* Pointwise ops (math/bigpoly/vec.go:9-121 via baseOperator, base_op.go:49-171)         */
/* ------------------------------------------------------------------------------------ */
typedef enum {
  RG_VEC_ADD = 0,      /* out = a + b        AddTo        base_op.go:49-55   */
  RG_VEC_SUB = 1,      /* out = a - b        SubTo        base_op.go:64-70   */
  RG_VEC_NEG = 2,      /* out = -a           NegTo        base_op.go:79-85   */
  RG_VEC_MUL = 3,      /* out = a * b        MulTo        base_op.go:133-142 */
  RG_VEC_SMUL = 4,     /* out = a * c        ScalarMulTo  base_op.go:94-100 */
  RG_VEC_MUL_ADD = 5,  /* out += a * b       MulAddTo     base_op.go:144-157 */
  RG_VEC_MUL_SUB = 6,  /* out -= a * b       MulSubTo     base_op.go:159-172 */
  RG_VEC_SMUL_ADD = 7, /* out += a * c       ScalarMulAddTo base_op.go:102-112 */
  RG_VEC_SMUL_SUB = 8  /* out -= a * c       ScalarMulSubTo base_op.go:114-124 */
} rg_vec_op;

/* n elements ([n][L]).  For the SMUL* ops `b` points to ONE element (the scalar c);
 * for NEG `b` is ignored.  Domain checks (IsNTT flags) stay in the caller, as in Go. */
rg_status rg_vec(const rg_field* f, int op, uint64_t* out, const uint64_t* a, const uint64_t* b, size_t n);
rg_status rg_vec_dev(const rg_field* f, int op, uint64_t* d_out, const uint64_t* d_a, const uint64_t* d_b, size_t n,
                     void* stream);

/* Uint.Marshal() (element.go) of n elements: each taken out of Montgomery form and written as 8 * L
 * big-endian bytes.  Element k is read at d_x + k * x_stride * L words (the strided read of
 * rg_jindo_eval_point_multi_dev's d_x) and written at d_out + k * out_stride; the bytes between 8 * L
 * and out_stride are not touched.  Any built field, one launch, asynchronous on `stream`; it exists so
 * that an evaluation point reaches a device transcript (rg_xof_absorb_plan_dev) without a host copy.
 * RG_ERR_INVALID: a NULL argument, x_stride of 0, or out_stride < 8 * L with n > 1; n == 0 does nothing. */
rg_status rg_field_marshal_dev(const rg_field* f, const uint64_t* d_x, size_t n, size_t x_stride, uint8_t* d_out,
                               size_t out_stride, void* stream);

/* ---- remaining bigpoly operators used by Buckler ------------- */
/* CyclicEvaluator.QuoRemByVanishing(p, N) (math/bigpoly/cyclic.go:18-37): quotient and
 * remainder of each of `batch` rank-coefficient polynomials by X^n_vanish - 1 (coefficient
 * domain; the IsNTT / rank panics stay with the caller).  d_rem may alias d_p, d_quo may not. */
rg_status rg_poly_quorem_vanishing_dev(const rg_field* f, size_t rank, long long n_vanish, uint64_t* d_quo,
                                       uint64_t* d_rem, const uint64_t* d_p, size_t batch, void* stream);
rg_status rg_poly_quorem_vanishing(const rg_field* f, size_t rank, long long n_vanish, uint64_t* quo, uint64_t* rem,
                                   const uint64_t* p);
/* CyclotomicEvaluator.AutTo(pOut, p, idx) (cyclotomic.go:29-86): X -> X^idx on each of `batch`
 * polynomials, coefficient domain (ntt_domain = 0, autTo) or NTT domain (autNTTTo).  idx must
 * be odd (RG_ERR_INVALID = the reference's "AutTo: idx must be odd" panic); d_out != d_p. */
rg_status rg_poly_aut_dev(const rg_field* f, size_t rank, long long idx, int ntt_domain, uint64_t* d_out,
                          const uint64_t* d_p, size_t batch, void* stream);
rg_status rg_poly_aut(const rg_field* f, size_t rank, long long idx, int ntt_domain, uint64_t* out, const uint64_t* p);
/* Poly.Evaluate(x) (poly.go:64-76): sum p_i x^i of n coefficients into ONE element d_out;
 * d_scratch holds rg_poly_evaluate_scratch_bytes(f, n) bytes. */
rg_status rg_poly_evaluate_dev(const rg_field* f, const uint64_t* d_p, size_t n, const uint64_t* d_x, uint64_t* d_out,
                               uint64_t* d_scratch, void* stream);
size_t rg_poly_evaluate_scratch_bytes(const rg_field* f, size_t n);
rg_status rg_poly_evaluate(const rg_field* f, const uint64_t* p, size_t n, const uint64_t* x, uint64_t* out);
/* Poly.Evaluate(x) of `batch` polynomials at ONE point (evals[i] = Poly(v[i]).Evaluate(x),
 * jindo/prover.go:318-321): polynomial b starts at element b * stride of d_p and its first n
 * coefficients are evaluated (stride >= n; elements [n, stride) are never read, so a prefix of
 * a longer polynomial, such as Buckler's comPolys inside their embedRank buffers, is evaluated
 * in place).  d_out [batch][L]; n = 0 gives 0.  d_scratch holds
 * rg_poly_evaluate_batch_scratch_bytes(f, n, batch) bytes.  A workgroup per tile of 4096
 * coefficients reads them coalesced and the tile sums fold per polynomial; no atomics, so the
 * result does not depend on scheduling.  RG_ERR_UNSUPPORTED for a limb count other than
 * 1, 2, 4, 7, 14; RG_ERR_INVALID for stride < n or a NULL buffer; batch = 0 does nothing.
 * The host form reads (batch - 1) * stride + n elements of p. */
size_t rg_poly_evaluate_batch_scratch_bytes(const rg_field* f, size_t n, size_t batch);
rg_status rg_poly_evaluate_batch_dev(const rg_field* f, const uint64_t* d_p, size_t n, size_t stride, size_t batch,
                                     const uint64_t* d_x, uint64_t* d_out, void* d_scratch, void* stream);
rg_status rg_poly_evaluate_batch(const rg_field* f, const uint64_t* p, size_t n, size_t stride, size_t batch,
                                 const uint64_t* x, uint64_t* out);
/* The same with a point per group of polynomials: polynomial b is evaluated at point
 * (b / group) % n_points, and point p is the element at d_x + p * x_stride * L words.  A buffer
 * laid out [proof][slot] takes group = slots per proof; one laid out [slot][proof] takes group = 1
 * and n_points = proofs (the index wraps).  The kernels are those of rg_poly_evaluate_batch_dev, each
 * reading the power tables of its polynomial's point; the tables of all points come from two
 * rg_buckler_powers_batch_dev calls, so the launch count (4) does not depend on n_points, and
 * n_points = 1 gives the limbs of rg_poly_evaluate_batch_dev.  d_scratch holds
 * rg_poly_evaluate_multi_scratch_bytes(f, n, batch, n_points) bytes.  RG_ERR_INVALID for group = 0,
 * n_points = 0 or x_stride = 0, for more than 65535 points in use (points beyond the last group are
 * never read) and for what rg_poly_evaluate_batch_dev refuses.  The host form reads
 * (n_points - 1) * x_stride + 1 elements of x. */
size_t rg_poly_evaluate_multi_scratch_bytes(const rg_field* f, size_t n, size_t batch, size_t n_points);
rg_status rg_poly_evaluate_multi_dev(const rg_field* f, const uint64_t* d_p, size_t n, size_t stride, size_t batch,
                                     const uint64_t* d_x, size_t x_stride, size_t n_points, size_t group,
                                     uint64_t* d_out, void* d_scratch, void* stream);
rg_status rg_poly_evaluate_multi(const rg_field* f, const uint64_t* p, size_t n, size_t stride, size_t batch,
                                 const uint64_t* x, size_t x_stride, size_t n_points, size_t group, uint64_t* out);
/* CyclotomicEvaluator.ModSwitchTo(pOut, pBig, qBig) (cyclotomic.go:97-124) on n coefficients:
 * pBig[i] as w little-endian words of a two's-complement integer ([n][w], |pBig[i]| < 2^(64w-1);
 * Go's big.Int values, e.g. PolyToBigintCentered output), qBig as w words (host, 0 < qBig <
 * 2^(64w-1)); out[i] = the reference's round(pBig[i] q / qBig) mod q (remainders above
 * floor(qBig/2) round up) in Montgomery form ([n][L]).  w <= 8.  The rank check ("input size
 * not consistent") and IsNTT = false stay with the caller. */
rg_status rg_poly_modswitch_dev(const rg_field* f, size_t n, const uint64_t* d_pbig, size_t w, const uint64_t* qbig,
                                uint64_t* d_out, void* stream);
rg_status rg_poly_modswitch(const rg_field* f, size_t n, const uint64_t* pbig, size_t w, const uint64_t* qbig,
                            uint64_t* out);

/* ---- Buckler prover device work -------------------------------- */
/* Encoder.EncodeTo / RandEncodeTo (buckler/encoder.go:32-54) of `batch` witness vectors:
 * t is the encoder's CyclicTransformer at the witness rank (newEncoder, encoder.go:15-20; a
 * negacyclic plan is RG_ERR_INVALID).  d_v [batch][rank][L] -> d_out [batch][embed_rank][L]:
 * InvNTT into coefficients 0..rank-1, zeros above.  d_rand [batch][L] (NULL = EncodeTo) holds
 * RandEncodeTo's MustSetRandom draws (Montgomery, injected): coeff[rank] = r, coeff[0] -= r.
 * batch > 1 needs d_scratch of rg_buckler_encode_scratch_bytes(t, batch) bytes. */
rg_status rg_buckler_encode_dev(const rg_ntt* t, size_t embed_rank, uint64_t* d_out, const uint64_t* d_v,
                                size_t batch, const uint64_t* d_rand, uint64_t* d_scratch, void* stream);
size_t rg_buckler_encode_scratch_bytes(const rg_ntt* t, size_t batch);
rg_status rg_buckler_encode(const rg_ntt* t, size_t embed_rank, uint64_t* out, const uint64_t* v,
                            const uint64_t* rand);
/* The arithmetic constraints Prover.evalCircuit walks (buckler/constraint.go:6-12, built by
 * AddTerm / SubTerm / AddTermWithConst): constraint c owns terms term_off[c] .. term_off[c+1]-1;
 * term t = coeffs[t] ([L], Montgomery, < q) * public witness pw_idx[t] (< 0: none, the
 * hasCoeffPublicWitness flag) * witnesses wit_idx[wit_off[t] .. wit_off[t+1]-1] (witnessToID
 * numbering).  Uploaded once (Compile time); immutable. */
typedef struct rg_circuit rg_circuit;
rg_status rg_buckler_circuit_create(const rg_field* f, size_t n_constraints, const size_t* term_off,
                                    const uint64_t* coeffs, const long long* pw_idx, const size_t* wit_off,
                                    const uint64_t* wit_idx, rg_circuit** out);
void rg_buckler_circuit_destroy(rg_circuit* c);
/* Prover.evalCircuit(batchConst, constraints, wData) (buckler/prover.go:355-379): d_out [rank][L]
 * = sum_c batchConst * sum_t coeff_t * pwEcdNTT[pw_t] * prod wEcdNTT[w], NTT domain, fused in one
 * pass.  d_w [n_w][rank][L] = wEcdNTT, d_pw [n_pw][rank][L] = pwEcdNTT, d_batch_const one element;
 * a witness index >= n_w (n_pw) is RG_ERR_INVALID. */
rg_status rg_buckler_eval_circuit_dev(const rg_circuit* c, size_t rank, const uint64_t* d_batch_const,
                                      const uint64_t* d_w, size_t n_w, const uint64_t* d_pw, size_t n_pw,
                                      uint64_t* d_out, void* stream);
rg_status rg_buckler_eval_circuit(const rg_circuit* c, size_t rank, const uint64_t* batch_const, const uint64_t* w,
                                  size_t n_w, const uint64_t* pw, size_t n_pw, uint64_t* out);

/* ---- Buckler linear check and sum check (buckler/linear.go, buckler/prover.go:381-485) ---- */
/* All results are canonical Montgomery elements, bit-identical to the reference.  Challenges and
 * MustSetRandom draws are injected.  Every `_dev` entry validates its arguments before touching
 * the device (RG_ERR_INVALID) and is asynchronous on `stream`; the forms without `_dev` take host
 * pointers and are synchronous.
 *
 * LinearChecker (linear.go:12-17): a matrix M applied as TransformTo (M v) and TransposeTo (M^T v)
 * on vectors [rank][L].  A checker is immutable after creation, except a projection checker's
 * matrix (rg_buckler_checker_set_xof*; not concurrent with calls that use the checker).
 *  - NewNTTChecker (linear.go:26-43): the negacyclic FwdNTT at rank; the transpose is
 *    vOut[i] = v[rank-1-i] * SetUint64(rank), then InvNTT.  rank not a power of two is
 *    RG_ERR_INVALID.
 *  - NewAutChecker (linear.go:54-73): AutTo with idx (transform) or idx^-1 mod 2 rank (transpose,
 *    modInverse linear.go:75-91), coefficient (ntt_domain = 0) or NTT domain.  An even idx or a
 *    rank that is not a power of two is RG_ERR_INVALID.
 *  - newProjChecker (linear.go:98-137): the 128 x rank boolean matrix, kept bit-packed on the
 *    device (16 bytes per column).  rank < 128 is RG_ERR_INVALID.  The matrix is set from the raw
 *    XOF bytes [rank][32] as the prover reads them (prover.go:168-176): entry (i, j) is true iff
 *    bit i % 8 of byte i / 8 of column j's 32 bytes is 0.  A checker may be re-set; it is
 *    RG_ERR_INVALID to apply one that was never set.
 *  - newProjRecomposeChecker (linear.go:144-180): base [nb][L] = decomposeBase(bound)
 *    (utils.go:7-32) as Montgomery elements < q, computed by the caller.  With g = rank / nb:
 *    transform out[i] = sum_j base[j] v[i nb + j] (i < g), zero above; transpose
 *    out[i nb + j] = base[j] v[i] (i < g), zero from g nb.  nb = 0 is RG_ERR_INVALID. */
typedef struct rg_linchecker rg_linchecker;
rg_status rg_buckler_checker_create_ntt(const rg_field* f, size_t rank, rg_linchecker** out);
rg_status rg_buckler_checker_create_aut(const rg_field* f, size_t rank, long long idx, int ntt_domain,
                                        rg_linchecker** out);
rg_status rg_buckler_checker_create_proj(const rg_field* f, size_t rank, rg_linchecker** out);
rg_status rg_buckler_checker_create_recompose(const rg_field* f, size_t rank, const uint64_t* base, size_t nb,
                                              rg_linchecker** out);
void rg_buckler_checker_destroy(rg_linchecker* c);
rg_status rg_buckler_checker_set_xof_dev(rg_linchecker* c, const uint8_t* d_xof, void* stream);
rg_status rg_buckler_checker_set_xof(rg_linchecker* c, const uint8_t* xof);
/* TransformTo / TransposeTo on `batch` vectors, d_v [batch][rank][L] -> d_out [batch][rank][L];
 * d_out == d_v is RG_ERR_INVALID.  The projection transform sums per-chunk partial rows in a fixed
 * order (no atomics) and needs d_scratch of rg_buckler_checker_scratch_bytes(c, batch) bytes; the
 * other kinds ignore d_scratch (0 bytes). */
size_t rg_buckler_checker_scratch_bytes(const rg_linchecker* c, size_t batch);
rg_status rg_buckler_checker_transform_dev(const rg_linchecker* c, uint64_t* d_out, const uint64_t* d_v, size_t batch,
                                           uint64_t* d_scratch, void* stream);
rg_status rg_buckler_checker_transpose_dev(const rg_linchecker* c, uint64_t* d_out, const uint64_t* d_v, size_t batch,
                                           void* stream);
rg_status rg_buckler_checker_transform(const rg_linchecker* c, uint64_t* out, const uint64_t* v);
rg_status rg_buckler_checker_transpose(const rg_linchecker* c, uint64_t* out, const uint64_t* v);
/* TransposeTo of a projection checker with a matrix per vector: vector i of d_v [batch][rank][L] is
 * transposed by the matrix packed from the 32 * rank XOF bytes at d_xof + i * 32 * rank (each proof
 * draws its own from projConst, prover.go:165-176).  The checker's own matrix is neither read nor
 * changed, so a checker that was never set is accepted and calls on several streams are independent.
 * d_bits_scratch holds rg_buckler_checker_transpose_xof_scratch_bytes(c, batch) bytes (16 per column
 * and vector).  RG_ERR_INVALID for a checker of another kind, a NULL or aliased buffer, or batch >
 * 65535. */
size_t rg_buckler_checker_transpose_xof_scratch_bytes(const rg_linchecker* c, size_t batch);
rg_status rg_buckler_checker_transpose_xof_dev(const rg_linchecker* c, uint64_t* d_out, const uint64_t* d_v,
                                               size_t batch, const uint8_t* d_xof, void* d_bits_scratch,
                                               void* stream);
/* linCheckVec (prover.go:409-413): out[0] = SetUint64(1), out[i] = out[i-1] * c, n elements. */
rg_status rg_buckler_powers_dev(const rg_field* f, const uint64_t* d_c, size_t n, uint64_t* d_out, void* stream);
rg_status rg_buckler_powers(const rg_field* f, const uint64_t* c, size_t n, uint64_t* out);
/* The power tables of n_c bases in one launch: out[k][i] = c_k^i for k < n_c, i < n, with base k at
 * d_c + k * c_stride * L words and d_out [n_c][n][L].  n_c = 0 or n = 0 does nothing; c_stride = 0
 * or n_c > 65535 (a base per grid row) is RG_ERR_INVALID.  The host form reads
 * (n_c - 1) * c_stride + 1 elements of c. */
rg_status rg_buckler_powers_batch_dev(const rg_field* f, const uint64_t* d_c, size_t c_stride, size_t n_c, size_t n,
                                      uint64_t* d_out, void* stream);
rg_status rg_buckler_powers_batch(const rg_field* f, const uint64_t* c, size_t c_stride, size_t n_c, size_t n,
                                  uint64_t* out);
/* Prover.sumCheckMask(maskRank) (prover.go:381-397) from the mask_rank injected draws d_rand, in
 * the order the reference draws them: mask[k] = r[k] - r[k+rank] while k + rank < mask_rank, r[k]
 * up to mask_rank, zero up to emb_rank; maskSum = r[0].  rank <= mask_rank <= emb_rank, and d_rand
 * and d_mask may not alias (RG_ERR_INVALID). */
rg_status rg_buckler_sumcheck_mask_dev(const rg_field* f, size_t rank, size_t mask_rank, size_t emb_rank,
                                       const uint64_t* d_rand, uint64_t* d_mask, uint64_t* d_mask_sum, void* stream);
rg_status rg_buckler_sumcheck_mask(const rg_field* f, size_t rank, size_t mask_rank, size_t emb_rank,
                                   const uint64_t* rand, uint64_t* mask, uint64_t* mask_sum);
/* The tail of linCheck / sumCheck / arithCheck (prover.go:439-458, 465-484, 401-403) on the NTT-domain
 * d_eval [emb][L] (emb = the rank of the cyclic emb_plan; clobbered): eval *= scale (NULL: skipped,
 * arithCheck), InvNTT, eval += mask [emb][L] (NULL: skipped), QuoRemByVanishing(eval, rank), then
 * d_quo [n_quo][L] = quoPoly[:n_quo], d_rem_lo [rank-1][L] = rem[1..rank-1], d_rem_hi
 * [jindo_rank][L] = jindo_rank - (rank-1) zeros, then remLo.  n_quo = rank (lin), sumCheckMaxRank -
 * rank (sum), arithCheckMaxRank - rank (arith).  d_rem_lo and d_rem_hi may be NULL together
 * (arithCheck discards the remainder); jindo_rank < rank - 1 is RG_ERR_INVALID.  d_scratch holds
 * rg_buckler_check_finish_scratch_bytes(emb_plan) bytes; no two buffers may alias. */
size_t rg_buckler_check_finish_scratch_bytes(const rg_ntt* emb_plan);
rg_status rg_buckler_check_finish_dev(const rg_ntt* emb_plan, size_t rank, uint64_t* d_eval, const uint64_t* d_scale,
                                      const uint64_t* d_mask, size_t n_quo, size_t jindo_rank, uint64_t* d_quo,
                                      uint64_t* d_rem_lo, uint64_t* d_rem_hi, uint64_t* d_scratch, void* stream);
rg_status rg_buckler_check_finish(const rg_ntt* emb_plan, size_t rank, const uint64_t* eval, const uint64_t* scale,
                                  const uint64_t* mask, size_t n_quo, size_t jindo_rank, uint64_t* quo,
                                  uint64_t* rem_lo, uint64_t* rem_hi);
/* Prover.linCheck (prover.go:406-459).  The handle holds what Compile fixes: the encoder's cyclic
 * plan at the witness rank, the cyclic plan at the embedding rank, the ordered checkers
 * (ctx.linCheckers) and, for checker c, its ordered witness-ID pairs pairs[pair_off[c] ..
 * pair_off[c+1]-1] = (wOut, wIn) (ctx.linCheckConstraints).  Plans and checkers are borrowed: they
 * outlive the handle.  Every checker has the encoder plan's rank and field (RG_ERR_INVALID). */
typedef struct rg_lincheck rg_lincheck;
rg_status rg_buckler_lincheck_create(const rg_ntt* enc_plan, const rg_ntt* emb_plan, size_t n_chk,
                                     const rg_linchecker* const* chk, const size_t* pair_off, const uint64_t* pairs,
                                     rg_lincheck** out);
void rg_buckler_lincheck_destroy(rg_lincheck* lc);
/* d_batch_const, d_lin_const: one element each; d_mask [emb][L] (linCheckMask); d_w [n_w][emb][L] =
 * wEcdNTT (a pair index >= n_w is RG_ERR_INVALID).  The power vector, every checker's transpose
 * of it, one batched Encode and one batched NTT, one fused pass over the coefficients (eval =
 * eval bc + ecdTr w[wIn] - ecd w[wOut] per pair, eval in registers), then the check tail with
 * scale = bc and n_quo = rank: d_quo [rank][L], d_rem_lo [rank-1][L], d_rem_hi [jindo_rank][L].
 * d_scratch holds rg_buckler_lin_check_scratch_bytes(lc) bytes; calls on different streams use
 * different scratch.  When the call has completed, remPoly [emb][L] stands in d_scratch at byte
 * offset rg_buckler_lin_check_rem_offset_bytes(lc): its element 0 is the sum the verifier compares
 * with LinCheckMaskSum (verifier.go:288-293), which linCheck itself does not return. */
size_t rg_buckler_lin_check_scratch_bytes(const rg_lincheck* lc);
size_t rg_buckler_lin_check_rem_offset_bytes(const rg_lincheck* lc);
rg_status rg_buckler_lin_check_dev(const rg_lincheck* lc, const uint64_t* d_batch_const, const uint64_t* d_lin_const,
                                   const uint64_t* d_mask, const uint64_t* d_w, size_t n_w, size_t jindo_rank,
                                   uint64_t* d_quo, uint64_t* d_rem_lo, uint64_t* d_rem_hi, uint64_t* d_scratch,
                                   void* stream);
rg_status rg_buckler_lin_check(const rg_lincheck* lc, const uint64_t* batch_const, const uint64_t* lin_const,
                               const uint64_t* mask, const uint64_t* w, size_t n_w, size_t jindo_rank, uint64_t* quo,
                               uint64_t* rem_lo, uint64_t* rem_hi);

/* ---- Buckler verifier's checks (buckler/verifier.go:178-315) ------------------------------ */
/* What Verifier.Verify computes after the transcript: pwEvals, vanishEval, arithCheck, linCheck and
 * sumCheck, decided on the device.  One call enqueues the whole decision on `stream` -- the power
 * vector of linCheckConst, every checker's transpose of it, ONE batched cyclic InvNTT at the witness
 * rank over those and the public witnesses (Encode; the zeros EncodeTo writes above `rank` add
 * nothing to Evaluate, so the embedding rank never appears), ONE batched Evaluate at evalPoint and
 * ONE one-workgroup kernel with all the scalar algebra -- and leaves one verdict word; nothing is
 * copied back and nothing is waited for inside.  Everything is Montgomery, canonical and injected.
 * The rest of Verify stays where it is: the transcript with the caller, polyVerifier.Verify =
 * rg_jindo_verify_dev (before or after), the public witnesses pwBase / pwMask on the host, the
 * projection matrix by rg_buckler_checker_set_xof* on the shared checker before the call.
 *
 * The handle holds what Compile fixes.  enc_plan: the encoder's cyclic plan at the witness rank (a
 * negacyclic plan is RG_ERR_INVALID).  lin / arith / sum: HasLinearCheck / HasArithmeticCheck /
 * HasSumCheck; each may be NULL, all three NULL is RG_ERR_INVALID.  Handles are borrowed and outlive
 * the verifier.  RG_ERR_INVALID also for: a `lin` whose encoder plan has another rank or field, a
 * circuit of another field, a circuit or pair index >= w_cnt (the reference indexes pf.Evals with
 * witness IDs < wCnt), a public-witness index >= n_pw, jindo_rank < rank - 1.  RG_ERR_UNSUPPORTED for
 * a limb count other than 1, 2, 4, 7, 14.  rg_last_error has the reason.  Creating a verifier
 * touches no device.
 *
 * pf.Evals is laid out as verifier.go:120-214 walks roundComIdx: w_cnt witnesses, the lin mask (if
 * lin), the sum mask (if sum), the arith quo (if arith), lin quo / remLo / remHi, sum quo / remLo /
 * remHi; rg_buckler_verifier_n_evals is its length.
 *
 * d_evals [n_evals][L]; d_pw [n_pw][rank][L], the public-witness vectors (NULL iff n_pw = 0);
 * d_chal [5][L]: evalPoint, arithBatchConst, linCheckBatchConst, linCheckConst, sumCheckBatchConst;
 * d_mask_sums [2][L]: LinCheckMaskSum, SumCheckMaskSum (those of absent checks are ignored; NULL is
 * allowed with arith alone); d_verdict: one word, 0 iff the reference's three checks all return true
 * -- the reference returns at the first failure, the device reports every one (bits below; a check
 * the handle lacks never sets its bits).  Optional d_sides [8][L]: arith (eval, test), lin (shift *
 * remLo, eval, test), sum (shift * remLo, eval, test), zeros for absent checks.  Optional d_pw_evals
 * [n_pw][L].  d_scratch holds rg_buckler_verify_checks_scratch_bytes(v) bytes; calls on different
 * streams use different scratch.  Every argument is validated before the device is touched
 * (RG_ERR_INVALID); no buffer may alias another.  The form without `_dev` takes host pointers and is
 * synchronous.
 *
 * The reference is mirrored where it is odd: ctx.sumCheckSums is not read by the verifier's sumCheck
 * (verifier.go:296-315), and evalCircuit multiplies every constraint by the same batchConst, not by
 * its powers (verifier.go:235). */
#define RG_BK_VERIFY_ARITH 1    /* arithCheck: eval != quoEval * vanishEval */
#define RG_BK_VERIFY_LIN_REM 2  /* linCheck: remHiEval != evalPoint^(jindoRank - (rank - 1)) * remLoEval */
#define RG_BK_VERIFY_LIN 4      /* linCheck: the main identity fails */
#define RG_BK_VERIFY_SUM_REM 8  /* sumCheck: the remHi identity fails */
#define RG_BK_VERIFY_SUM 16     /* sumCheck: the main identity fails */
typedef struct rg_bverifier rg_bverifier;
rg_status rg_buckler_verifier_create(const rg_ntt* enc_plan, size_t jindo_rank, size_t w_cnt, size_t n_pw,
                                     const rg_lincheck* lin, const rg_circuit* arith, const rg_circuit* sum,
                                     rg_bverifier** out);
void rg_buckler_verifier_destroy(rg_bverifier* v);
size_t rg_buckler_verifier_n_evals(const rg_bverifier* v);
size_t rg_buckler_verify_checks_scratch_bytes(const rg_bverifier* v);
rg_status rg_buckler_verify_checks_dev(const rg_bverifier* v, const uint64_t* d_evals, const uint64_t* d_pw,
                                       const uint64_t* d_chal, const uint64_t* d_mask_sums, uint64_t* d_verdict,
                                       uint64_t* d_sides, uint64_t* d_pw_evals, uint64_t* d_scratch, void* stream);
rg_status rg_buckler_verify_checks(const rg_bverifier* v, const uint64_t* evals, const uint64_t* pw,
                                   const uint64_t* chal, const uint64_t* mask_sums, uint64_t* verdict,
                                   uint64_t* sides, uint64_t* pw_evals);
/* n_proofs proofs of one compiled circuit (one handle) decided by one call whose launch count does
 * not depend on n_proofs.  Every per-proof argument is proof-major and has the single entry's
 * meaning per proof: d_evals [n_proofs][n_evals][L], d_pw [n_proofs][n_pw][rank][L] (NULL iff n_pw =
 * 0), d_chal [n_proofs][5][L], d_mask_sums [n_proofs][2][L], d_verdict [n_proofs] words (the bits
 * above, per proof), optional d_sides [n_proofs][8][L] and d_pw_evals [n_proofs][n_pw][L].
 * d_xof [n_proofs][32 * rank] bytes: the XOF bytes of each proof's projection matrix (prover.go:165-176).
 * Every projection checker of the handle uses the proof's one matrix, as the reference's single
 * ctx.projChecker does; the checkers' own matrices are neither read nor changed.  d_xof is required
 * iff the handle's linear check holds a projection checker and must be NULL otherwise.
 *
 * The pipeline: one rg_buckler_powers_batch_dev of every proof's linCheckConst, each checker's
 * transpose over all proofs in one call (rg_buckler_checker_transpose_xof_dev for a projection
 * checker), one kernel placing the public witnesses beside them, ONE batched InvNTT over all
 * n_proofs * (1 + n_chk + n_pw) vectors, ONE rg_poly_evaluate_multi_dev at the proofs' evalPoints
 * and ONE launch of the decision kernel with a workgroup per proof.  Each output word has one
 * writer; nothing is copied back and nothing is waited for inside.
 *
 * n_proofs = 0 does nothing.  RG_ERR_INVALID for n_proofs > RG_BK_MULTI_MAX_PROOFS (a proof per grid
 * row of the power-table and projection kernels), for n_proofs * (1 + n_chk + n_pw) > 2^30 vectors or
 * more than 2^39 words in them (grid extents and byte offsets), and for what the single entry refuses;
 * every argument is validated before the device is touched and no buffer may alias another.
 * d_scratch holds rg_buckler_verify_checks_multi_scratch_bytes(v, n_proofs) bytes (0 for an n_proofs
 * that is refused); calls on different streams use different scratch.  The form without `_dev`
 * takes host pointers and is synchronous. */
#define RG_BK_MULTI_MAX_PROOFS 65535
size_t rg_buckler_verify_checks_multi_scratch_bytes(const rg_bverifier* v, size_t n_proofs);
rg_status rg_buckler_verify_checks_multi_dev(const rg_bverifier* v, size_t n_proofs, const uint64_t* d_evals,
                                             const uint64_t* d_pw, const uint8_t* d_xof, const uint64_t* d_chal,
                                             const uint64_t* d_mask_sums, uint64_t* d_verdict, uint64_t* d_sides,
                                             uint64_t* d_pw_evals, uint64_t* d_scratch, void* stream);
rg_status rg_buckler_verify_checks_multi(const rg_bverifier* v, size_t n_proofs, const uint64_t* evals,
                                         const uint64_t* pw, const uint8_t* xof, const uint64_t* chal,
                                         const uint64_t* mask_sums, uint64_t* verdict, uint64_t* sides,
                                         uint64_t* pw_evals);

/* ---- Buckler prover's checks for a batch of proofs (buckler/prover.go:399-485) ------------- */
/* Prover.arithCheck, linCheck and sumCheck of n_proofs proofs of one compiled circuit, enqueued by
 * one call whose launch count does not depend on n_proofs: the prover's counterpart of
 * rg_buckler_verify_checks_multi_dev, with its vocabulary, layouts and limits.  All four challenges
 * are fixed before arithCheck runs (prover.go:242-334), so one call does the whole round and leaves,
 * for every proof, the seven polynomials Prove commits next; each output, being proof-major, goes
 * straight into rg_jindo_commit_dev with batch = n_proofs.  Everything is Montgomery, canonical and
 * injected; the transcript, the masks (rg_buckler_sumcheck_mask_dev, one round earlier) and the
 * commits stay with the caller.
 *
 * The handle holds what Compile fixes.  enc_plan / emb_plan: the encoder's cyclic plan at the witness
 * rank and the evaluator's cyclic plan at the embedding rank (a negacyclic plan is RG_ERR_INVALID).
 * lin / arith / sum: HasLinearCheck / HasArithmeticCheck / HasSumCheck; each may be NULL, all three
 * NULL is RG_ERR_INVALID.  arith_max_rank / sum_max_rank: ctx.arithCheckMaxRank / sumCheckMaxRank,
 * read for a present check only.  Handles are borrowed and outlive the prover.  RG_ERR_INVALID also
 * for: a `lin` whose plans differ in rank or field from enc_plan / emb_plan, a circuit of another
 * field, a circuit or pair index >= n_w, a public-witness index >= n_pw, jindo_rank < rank - 1 (or
 * above 2^32), a present check with max_rank < rank or max_rank > the embedding rank.
 * RG_ERR_UNSUPPORTED for a limb count other than 1, 2, 4, 7, 14.  rg_last_error has the reason.
 * Creating a prover touches no device.
 *
 * Every array is proof-major.  Inputs: d_w [n_proofs][n_w][emb][L] = wEcdNTT (NULL iff n_w = 0);
 * d_pw [n_proofs][n_pw][emb][L] = pwEcdNTT (NULL iff n_pw = 0); d_xof [n_proofs][32 * rank] bytes,
 * each proof's projection matrix (prover.go:165-176), required iff `lin` holds a projection checker
 * and NULL otherwise -- the checkers' own matrices are neither read nor changed; d_chal
 * [n_proofs][4][L]: arithBatchConst, linCheckBatchConst, linCheckConst, sumCheckBatchConst; d_lin_mask,
 * d_sum_mask [n_proofs][emb][L] (linCheckMask, sumCheckMask).  Outputs, with n_quo = arith_max_rank -
 * rank, rank, sum_max_rank - rank for arith, lin, sum: quo [n_proofs][n_quo][L]; remLo
 * [n_proofs][rank-1][L]; remHi [n_proofs][jindo_rank][L] = jindo_rank - (rank-1) zeros, then remLo
 * (arithCheck discards its remainder).  Optional d_rem0 [n_proofs][2][L]: element 0 of linCheck's
 * and of sumCheck's remPoly, the sums the verifier compares with LinCheckMaskSum / SumCheckMaskSum
 * (verifier.go:288-293; the single entry leaves lin's at rg_buckler_lin_check_rem_offset_bytes);
 * zeros for an absent check.  The pointers of an absent check must be NULL; a quo with n_quo = 0 may
 * be NULL and nothing is written.
 *
 * The pipeline: one rg_buckler_powers_batch_dev of every proof's linCheckConst, each checker's
 * transpose over all proofs in one call (rg_buckler_checker_transpose_xof_dev for a projection
 * checker), ONE batched Encode and ONE batched NTT at the embedding rank over the n_proofs * (1 +
 * n_chk) vectors, one kernel per check for the NTT-domain evaluation (linCheck's pass and evalCircuit
 * with a proof per grid row, the trailing ScalarMulTo of linCheck and sumCheck folded in), ONE batched
 * InvNTT over all n_proofs * n_checks evals and ONE kernel with the mask add, QuoRemByVanishing and
 * the quo / remLo / remHi / rem0 split of every check.  Each output word has one writer; nothing is
 * allocated, copied back or waited for inside.
 *
 * n_proofs = 0 does nothing.  RG_ERR_INVALID for n_proofs > RG_BK_MULTI_MAX_PROOFS, for n_proofs *
 * max(1 + n_chk, n_checks) > 2^30 polynomials or more than 2^39 words in them, and for any two
 * aliased buffers; every argument is validated before the device is touched.  d_scratch holds
 * rg_buckler_prove_checks_scratch_bytes(p, n_proofs) bytes (0 for an n_proofs that is refused); calls
 * on different streams use different scratch.  The form without `_dev` takes host pointers and is
 * synchronous. */
typedef struct rg_bprover rg_bprover;
rg_status rg_buckler_prover_create(const rg_ntt* enc_plan, const rg_ntt* emb_plan, size_t jindo_rank, size_t n_w,
                                   size_t n_pw, const rg_lincheck* lin, const rg_circuit* arith, size_t arith_max_rank,
                                   const rg_circuit* sum, size_t sum_max_rank, rg_bprover** out);
void rg_buckler_prover_destroy(rg_bprover* p);
size_t rg_buckler_prove_checks_scratch_bytes(const rg_bprover* p, size_t n_proofs);
rg_status rg_buckler_prove_checks_dev(const rg_bprover* p, size_t n_proofs, const uint64_t* d_w, const uint64_t* d_pw,
                                      const uint8_t* d_xof, const uint64_t* d_chal, const uint64_t* d_lin_mask,
                                      const uint64_t* d_sum_mask, uint64_t* d_arith_quo, uint64_t* d_lin_quo,
                                      uint64_t* d_lin_rem_lo, uint64_t* d_lin_rem_hi, uint64_t* d_sum_quo,
                                      uint64_t* d_sum_rem_lo, uint64_t* d_sum_rem_hi, uint64_t* d_rem0,
                                      uint64_t* d_scratch, void* stream);
rg_status rg_buckler_prove_checks(const rg_bprover* p, size_t n_proofs, const uint64_t* w, const uint64_t* pw,
                                  const uint8_t* xof, const uint64_t* chal, const uint64_t* lin_mask,
                                  const uint64_t* sum_mask, uint64_t* arith_quo, uint64_t* lin_quo,
                                  uint64_t* lin_rem_lo, uint64_t* lin_rem_hi, uint64_t* sum_quo, uint64_t* sum_rem_lo,
                                  uint64_t* sum_rem_hi, uint64_t* rem0);

/* ---- Buckler norm decomposition (buckler/utils.go:34-56, buckler/prover.go:77-111, 182-192) ---- */
/* decomposeBig on the device: a Montgomery element w is taken out of Montgomery form, centred
 * (x > q >> 1 stands for x - q) and walked down the base b_0, b_1, ...: digit +1 and x -= b_j while
 * x >= b_j, digit -1 and x += b_j while x <= -b_j, else 0.  The digits come out as the field
 * elements SetInt64 makes: 0, R mod q, q - (R mod q).  A value beyond the sum of the base leaves a
 * residual, as in the reference; it is no error.
 *
 * The handle holds the base [nb][L] as PLAIN little-endian integers (not Montgomery; the caller
 * computes decomposeBase(bound), utils.go:7-32) with R mod q and its negation.  An element that
 * does not fit L limbs is given as 2^(64L) - 1: no |x| <= q / 2 reaches either.  nb = 0 or a zero
 * base element is RG_ERR_INVALID.  Creating a handle touches no device: the base is uploaded once,
 * by the first call that runs a kernel, to the device current then (that one call waits for the
 * copy; capture a graph only after it).  Every `_dev` entry validates its arguments before it
 * touches the device, writes every word of its output, and is asynchronous on `stream`; d_out ==
 * d_w is RG_ERR_INVALID, as is any other aliasing.  rank <= 2^30, batch <= 65535. */
typedef struct rg_dcmp rg_dcmp;
rg_status rg_buckler_dcmp_create(const rg_field* f, const uint64_t* base, size_t nb, rg_dcmp** out);
void rg_buckler_dcmp_destroy(rg_dcmp* h);
/* The infinity-norm expansion (prover.go:77-86): d_w [batch][rank][L] -> d_out [batch][nb][rank][L],
 * digit-major: d_out + (k nb + j) rank L is digit witness j of input k, so d_out is a batch of
 * batch * nb witnesses as rg_buckler_encode_dev takes them. */
rg_status rg_buckler_dcmp_inf_dev(const rg_dcmp* h, const uint64_t* d_w, size_t batch, size_t rank, uint64_t* d_out,
                                  void* stream);
/* The projection decomposition (prover.go:182-192): d_out[i nb + j] = digit j of d_w[i], i < 128;
 * entries 128 nb .. rank - 1 are zero.  d_w holds at least 128 elements, d_out [rank][L];
 * rank < 128 or 128 nb > rank is RG_ERR_INVALID. */
rg_status rg_buckler_dcmp_proj_dev(const rg_dcmp* h, const uint64_t* d_w, size_t rank, uint64_t* d_out, void* stream);
/* The two-norm witness (prover.go:99-110) of each of `batch` vectors d_w [batch][rank][L]: sqNm =
 * sum_i plain(w_i)^2 mod q of that vector alone, then decomposeBig(sqNm) through the centring (a sum
 * above q / 2 gives -1 digits).  d_out [batch][rank][L]: the digits in entries 0 .. nb - 1, zero
 * above; nb > rank is RG_ERR_INVALID.  d_sq (optional) [batch][L]: sqNm in Montgomery form.  The
 * squares are summed per workgroup into d_scratch (rg_buckler_dcmp_two_scratch_bytes bytes) and
 * those sums in a fixed order: no atomics, and the result is exact either way. */
size_t rg_buckler_dcmp_two_scratch_bytes(const rg_dcmp* h, size_t batch, size_t rank);
rg_status rg_buckler_dcmp_two_dev(const rg_dcmp* h, const uint64_t* d_w, size_t batch, size_t rank, uint64_t* d_out,
                                  uint64_t* d_sq, uint64_t* d_scratch, void* stream);
rg_status rg_buckler_dcmp_inf(const rg_dcmp* h, const uint64_t* w, size_t batch, size_t rank, uint64_t* out);
rg_status rg_buckler_dcmp_proj(const rg_dcmp* h, const uint64_t* w, size_t rank, uint64_t* out);
rg_status rg_buckler_dcmp_two(const rg_dcmp* h, const uint64_t* w, size_t batch, size_t rank, uint64_t* out,
                              uint64_t* sq);

/* ---- Buckler prover's projection round and masks for a batch of proofs (prover.go:165-240) ---- */
/* What Prove does between two batched commit rounds, for n_proofs proofs of one compiled circuit and
 * in the vocabulary of rg_buckler_prove_checks_dev: every array proof-major, Montgomery and canonical,
 * every argument validated before the device is touched (rg_last_error has the reason), everything
 * asynchronous on `stream`, nothing allocated, copied back or waited for inside (one exception below),
 * every output word written by exactly one writer, a launch count without n_proofs in it.  n_proofs =
 * 0 does nothing; n_proofs > RG_BK_MULTI_MAX_PROOFS and any two aliased buffers are RG_ERR_INVALID; a
 * limb count other than 1, 2, 4, 7, 14 is RG_ERR_UNSUPPORTED.  The XOF, the transcript, SetBytes and
 * decomposeBase stay with the caller.
 *
 * The projection round (prover.go:165-193).  The handle holds what Compile fixes: the field, the
 * witness rank, the number of witnesses n_w of the table and the n_c approximate infinity-norm
 * constraints, cons [n_c][3] = the witness IDs (src, proj, dcmp) of each, with dcmp[c] the borrowed
 * rg_dcmp of decomposeBase(rank * bound) of constraint c (context.go:206-228); the bases may differ in
 * length.  Creating it touches no device.  RG_ERR_INVALID for rank < 128 (or above 2^30), n_c = 0 or
 * n_c > 32 (the constraint table travels as kernel arguments), an index >= n_w, 128 nb > rank for any
 * constraint, an rg_dcmp of another field, and an output row (proj or dcmp) that is another output row
 * or any constraint's src: the reference ranges over a map there, so no order is defined that a result
 * could depend on.  Several constraints may share one src.
 *
 * d_w [n_proofs][n_w][rank][L]: the plain witness table as wData.w holds it, read and written in
 * place.  d_xof [n_proofs][32 * rank] bytes: each proof's projection matrix (prover.go:168-176), the
 * bytes rg_buckler_prove_checks_dev takes later; entry (i, j) is true iff bit i % 8 of byte i / 8 of
 * column j's 32 bytes is 0.  For every proof and constraint, row proj becomes TransformTo(w[src])
 * under the proof's matrix (the 128 sums in entries 0 .. 127, zeros above, linear.go:108-123) and row
 * dcmp becomes out[i nb + j] = digit j of proj[i] for i < 128, zeros from 128 nb (prover.go:182-192),
 * the digits as rg_buckler_dcmp_proj_dev writes them.  Every other row of d_w is left untouched.
 *
 * Two launches: one with the matrix products of all proofs and constraints, a workgroup per 512
 * columns that reads its XOF bytes straight into LDS (no pack launch, no bit-matrix scratch, no
 * checker handle) and leaves one partial row; one that sums the partial rows in column order,
 * decomposes and stores both rows with their zero tails.  No atomics.  d_scratch holds
 * rg_buckler_prove_proj_round_scratch_bytes(h, n_proofs) = n_proofs * n_c * ceil(rank / 512) * 128 * L * 8
 * bytes (0 for an n_proofs that is refused); calls on different streams use different scratch and may
 * share the handle.  The bases reach the device by the rg_dcmp handles' own first-use rule: the first
 * call that uses a handle nobody has used yet uploads its base and waits for that copy (capture a
 * graph only after it).  The form without `_dev` takes host pointers and is synchronous. */
typedef struct rg_bproj rg_bproj;
rg_status rg_buckler_proj_round_create(const rg_field* f, size_t rank, size_t n_w, size_t n_c, const uint64_t* cons,
                                       const rg_dcmp* const* dcmp, rg_bproj** out);
void rg_buckler_proj_round_destroy(rg_bproj* h);
size_t rg_buckler_prove_proj_round_scratch_bytes(const rg_bproj* h, size_t n_proofs);
rg_status rg_buckler_prove_proj_round_dev(const rg_bproj* h, size_t n_proofs, uint64_t* d_w, const uint8_t* d_xof,
                                          uint64_t* d_scratch, void* stream);
rg_status rg_buckler_prove_proj_round(const rg_bproj* h, size_t n_proofs, uint64_t* w, const uint8_t* xof);
/* Prover.sumCheckMask(maskRank) (prover.go:381-397) of n_proofs proofs in one launch, with the
 * constraints and refusals of rg_buckler_sumcheck_mask_dev.  d_rand [n_proofs][mask_rank][L]: the draws
 * in the reference's order.  d_mask [n_proofs][emb_rank][L]: what rg_buckler_prove_checks_dev takes as
 * d_lin_mask / d_sum_mask.  d_mask_com (optional) [n_proofs][mask_rank][L]: mask.Coeffs[:maskRank] of
 * every proof, contiguous, as rg_jindo_commit_dev takes it with batch = n_proofs and nv = mask_rank.
 * d_mask_sum [n_proofs][L].  The call needs no scratch. */
rg_status rg_buckler_sumcheck_mask_batch_dev(const rg_field* f, size_t rank, size_t mask_rank, size_t emb_rank,
                                             size_t n_proofs, const uint64_t* d_rand, uint64_t* d_mask,
                                             uint64_t* d_mask_com, uint64_t* d_mask_sum, void* stream);
rg_status rg_buckler_sumcheck_mask_batch(const rg_field* f, size_t rank, size_t mask_rank, size_t emb_rank,
                                         size_t n_proofs, const uint64_t* rand, uint64_t* mask, uint64_t* mask_com,
                                         uint64_t* mask_sum);

/* ---- Buckler prover's MustSetRandom draws on the device (element.go:299-343) ---- */
/* A field-element sampler on any built field: NewUniformSamplerWithSeed(seed) in place of crypto/rand,
 * as rg_jindo_seeds.uniform is for a Jindo handle.  Element i of d_out [n][L] is Uint.SetRandom reading
 * from instance first_instance + i of that sampler (the instance windows of rg_jindo_sample_dev: IV +
 * instance * 2^24): k = ceil(bitLen(q - 1) / 8) bytes, the top byte's unused bits cleared, rejected
 * while >= q; the stored limbs are the accepted candidate's little-endian words, no domain conversion,
 * as in the reference.  One element is one instance, so every value is a pure function of (seed,
 * instance, q) and the partition of draws among instances is the caller's.
 *
 * Creating the handle touches no device; RG_ERR_UNSUPPORTED where libcrypto's SHA-384 is missing and
 * for a limb count other than 1, 2, 4, 7, 14.  The handle's AES table reaches the device by the
 * first-use rule of rg_dcmp: the first call that runs a kernel uploads it, to the device current then,
 * and waits for that copy (capture a graph only after it).  Apart from that the `_dev` entry is
 * asynchronous on `stream`: nothing is allocated, freed, copied to the host or waited for inside, and
 * the handle is only read, so calls on different streams with different scratch are independent.
 * Stream items, whatever n: 3 on the whole-word route (even L with k = 8 L, e.g. q255: a 4-byte memset
 * of the long-draw flag in d_scratch, the draws, the long draws' fix-up), 1 on the byte-serial route
 * (every other field).  d_scratch holds rg_field_sampler_scratch_bytes(s) = 256 bytes.
 *
 * n = 0 returns RG_OK and touches nothing.  RG_ERR_INVALID, before the device is touched and with a
 * reason in rg_last_error that starts "field sampler": a NULL handle, output or scratch; first_instance
 * + n passing 2^64 - 1 (or n above 2^44); d_out overlapping d_scratch.  The form without `_dev` takes
 * a host pointer and is synchronous. */
typedef struct rg_fsampler rg_fsampler;
rg_status rg_field_sampler_create(const rg_field* f, const uint8_t* seed, size_t seed_len, rg_fsampler** out);
void rg_field_sampler_destroy(rg_fsampler* s);
size_t rg_field_sampler_scratch_bytes(const rg_fsampler* s);
rg_status rg_field_sampler_elems_dev(const rg_fsampler* s, unsigned long long first_instance, size_t n,
                                     uint64_t* d_out, void* d_scratch, void* stream);
rg_status rg_field_sampler_elems(const rg_fsampler* s, unsigned long long first_instance, size_t n, uint64_t* out);
/* Prover.sumCheckMask(maskRank) (prover.go:381-397) of n_proofs proofs with its draws made inside the
 * mask kernel: draw k of proof p is the element of instance first_instance + p * mask_rank + k, and
 * the outputs equal, word for word, rg_field_sampler_elems_dev(s, first_instance, n_proofs * mask_rank,
 * d_rand) followed by rg_buckler_sumcheck_mask_batch_dev on that d_rand -- which never exists here.
 * d_mask [n_proofs][emb_rank][L], d_mask_com (optional) [n_proofs][mask_rank][L], d_mask_sum
 * [n_proofs][L] (draw 0, before the subtraction).  Every draw is made once (a lane walks k, k + rank,
 * k + 2 rank, ... of one proof; mask_rank is not bounded by 2 rank), every output word, the zeros up
 * to emb_rank included, has exactly one writer, no atomics.  Stream items, whatever n_proofs: 3 on the
 * whole-word route, 1 on the byte-serial route.  d_scratch holds rg_field_sampler_scratch_bytes(s)
 * bytes.  The constraints and refusals of rg_buckler_sumcheck_mask_batch_dev (rank <= mask_rank <=
 * emb_rank, n_proofs <= RG_BK_MULTI_MAX_PROOFS, overlapping buffers), a NULL handle or scratch, and
 * first_instance + n_proofs * mask_rank passing 2^64 - 1: RG_ERR_INVALID before the device is touched,
 * the reason starting "buckler mask sampled".  n_proofs = 0 does nothing.  The first-use rule of the
 * handle applies.  The form without `_dev` takes host pointers and is synchronous. */
rg_status rg_buckler_sumcheck_mask_batch_sampled_dev(const rg_fsampler* s, size_t rank, size_t mask_rank,
                                                     size_t emb_rank, size_t n_proofs,
                                                     unsigned long long first_instance, uint64_t* d_mask,
                                                     uint64_t* d_mask_com, uint64_t* d_mask_sum, void* d_scratch,
                                                     void* stream);
rg_status rg_buckler_sumcheck_mask_batch_sampled(const rg_fsampler* s, size_t rank, size_t mask_rank, size_t emb_rank,
                                                 size_t n_proofs, unsigned long long first_instance, uint64_t* mask,
                                                 uint64_t* mask_com, uint64_t* mask_sum);

/* ---- Buckler prover's witness rounds for a batch of proofs (prover.go:77-111, 136-153, 195-201) ---- */
/* What Prove does to its witness table before its first commit and at each commit round, for n_proofs
 * proofs of one compiled circuit and in the vocabulary of rg_buckler_prove_proj_round_dev: every array
 * proof-major, Montgomery and canonical, every argument validated before the device is touched
 * (rg_last_error has the reason), everything asynchronous on `stream`, nothing allocated, copied back or
 * waited for inside (one exception below), every output word written by exactly one writer, no atomics,
 * a launch count without n_proofs in it.  n_proofs = 0 does nothing; n_proofs > RG_BK_MULTI_MAX_PROOFS
 * (or a table above 2^44 words) and any two aliased buffers are RG_ERR_INVALID; a limb count other than
 * 1, 2, 4, 7, 14 is RG_ERR_UNSUPPORTED.  The transcript, the XOF, SetBytes, decomposeBase and pwBase /
 * pwMask stay with the caller.  With both rounds a witness table stays on the device, in one layout,
 * from the assignment to the d_w of rg_buckler_prove_checks_dev.
 *
 * Creating either handle touches no device.  A handle's own small table (the digit-row IDs, the
 * selected rows) reaches the device by the first-use rule of rg_dcmp: the first call that runs a kernel
 * uploads it, to the device current then, and waits for that copy; the borrowed rg_dcmp handles upload
 * their bases under their own rule in the same call (capture a graph only after it).  Calls on different
 * streams use different scratch and may share a handle.  The forms without `_dev` take host pointers
 * and are synchronous.
 *
 * The decomposition round (prover.go:77-111).  The handle holds what Compile fixes: the field, the
 * witness rank, the number of witnesses n_w of the table,
 *   - n_inf infinity-norm constraints (context.go:136-145): inf_src [n_inf] the witness IDs,
 *     inf_dcmp [n_inf] the borrowed rg_dcmp of decomposeBase(bound) of each, and inf_rows, the digit-row
 *     IDs wDcmp[j] of all constraints one after the other, nb(c) of constraint c in base order (nb(c) is
 *     inf_dcmp[c]'s).  Compile makes the rows of a constraint consecutive; any distinct rows are taken.
 *   - n_two two-norm constraints (context.go:171-185): two_cons [n_two][2] = (src, dst) and two_dcmp
 *     [n_two] the borrowed rg_dcmp of each.
 * RG_ERR_INVALID for n_inf + n_two = 0, n_inf > 32 or n_two > 32 (the constraint tables travel as kernel
 * arguments; the digit-row IDs, up to several hundred a constraint, live on the device), an index >=
 * n_w, an rg_dcmp of another field, nb > rank for a two-norm constraint, rank 0 or above 2^30, and an
 * output row (a digit row or a dst) that is another output row or any constraint's src: the reference
 * ranges over maps there (prover.go:77, 89), so no order is defined that a result could depend on.
 * Several constraints may share one src.
 *
 * d_w [n_proofs][n_w][rank][L]: the plain witness table as wData.w holds it, read and written in place.
 * For every proof and infinity-norm constraint, digit row j becomes digit j of every coefficient of
 * w[src], the elements rg_buckler_dcmp_inf_dev writes.  For every proof and two-norm constraint, row dst
 * gets the digits of sqNm = sum_i plain(w[src]_i)^2 mod q in entries 0 .. nb - 1 and zeros above, as
 * rg_buckler_dcmp_two_dev writes them.  d_sq (optional, NULL for a handle with n_two = 0)
 * [n_proofs][n_two][L]: sqNm in Montgomery form.  Every other row of d_w is left untouched.
 *
 * Three launches (one with n_two = 0, two with n_inf = 0): the digits of all proofs and infinity-norm
 * constraints, a lane per coefficient; the squares of all proofs and two-norm constraints summed per
 * workgroup of 1024 coefficients into scratch; those sums added in chunk order, decomposed and stored
 * with the zero tail.  d_scratch holds rg_buckler_prove_dcmp_round_scratch_bytes(h, n_proofs) =
 * n_proofs * n_two * ceil(rank / 1024) * L * 8 bytes (0 for an n_proofs that is refused; d_scratch may be
 * NULL when n_two = 0). */
typedef struct rg_bdcmp rg_bdcmp;
rg_status rg_buckler_dcmp_round_create(const rg_field* f, size_t rank, size_t n_w, size_t n_inf,
                                       const uint64_t* inf_src, const rg_dcmp* const* inf_dcmp,
                                       const uint64_t* inf_rows, size_t n_two, const uint64_t* two_cons,
                                       const rg_dcmp* const* two_dcmp, rg_bdcmp** out);
void rg_buckler_dcmp_round_destroy(rg_bdcmp* h);
size_t rg_buckler_prove_dcmp_round_scratch_bytes(const rg_bdcmp* h, size_t n_proofs);
rg_status rg_buckler_prove_dcmp_round_dev(const rg_bdcmp* h, size_t n_proofs, uint64_t* d_w, uint64_t* d_sq,
                                          uint64_t* d_scratch, void* stream);
rg_status rg_buckler_prove_dcmp_round(const rg_bdcmp* h, size_t n_proofs, uint64_t* w, uint64_t* sq);
/* The encode round (prover.go:136-153, 195-201): wEcd[i] = RandEncode(w[i]) for the rows of one commit
 * round, the first-round rows or ctx.wSecond after the projection round; a prover makes one handle per
 * round.  The handle holds the encoder's cyclic plan at the witness rank (borrowed; a negacyclic plan is
 * RG_ERR_INVALID), the embedding rank (a power of two above the rank, at most 2^30), n_w and sel
 * [n_sel], the rows of this round: distinct, each < n_w, in any order, 1 <= n_sel <= 65535.
 *
 * d_w [n_proofs][n_w][rank][L]: the plain table.  d_rand [n_proofs][n_sel][L]: the MustSetRandom draws
 * in sel order; NULL means EncodeTo, so the public witnesses' table can use the same entry.  d_wecd
 * [n_proofs][n_w][emb][L].  d_com (optional) [n_proofs][n_sel][rank + 1][L]; d_com with d_rand NULL is
 * RG_ERR_INVALID.  For every proof and s < n_sel, row sel[s] of d_wecd becomes RandEncode(w[sel[s]]):
 * the cyclic InvNTT in coefficients 0 .. rank - 1, coeff[rank] = r, coeff[0] -= r, zeros above, the
 * elements rg_buckler_encode_dev writes; d_com[proof][s] gets its first rank + 1 coefficients,
 * contiguous, which is the input of rg_jindo_commit_dev with batch = n_proofs * n_sel and nv = rank + 1.
 * Rows of d_wecd outside sel are left untouched.
 *
 * Two launches plus the plan's own: one gather of the selected rows into scratch (skipped when sel is
 * 0 .. n_w - 1, and then the table itself is the transform's input), one batched rg_ntt_inv_dev over
 * the n_proofs * n_sel vectors, one kernel that writes the strided d_wecd rows and the d_com rows
 * together.  d_scratch holds rg_buckler_prove_encode_round_scratch_bytes(h, n_proofs) =
 * n_proofs * n_sel * rank * L * 8 bytes (0 for an n_proofs that is refused).
 *
 * The forward transform is deliberately not in this call: wEcdNTT is first read by the checks, after
 * the last commit round (prover.go:242-334).  So once both rounds have written d_wecd the caller runs
 * ONE in-place rg_ntt_fwd_dev(emb_plan, d_wecd, d_wecd, n_proofs * n_w) over the whole contiguous
 * table; the result is the d_w of rg_buckler_prove_checks_dev. */
typedef struct rg_bencode rg_bencode;
rg_status rg_buckler_encode_round_create(const rg_ntt* enc_plan, size_t emb_rank, size_t n_w, size_t n_sel,
                                         const uint64_t* sel, rg_bencode** out);
void rg_buckler_encode_round_destroy(rg_bencode* h);
size_t rg_buckler_prove_encode_round_scratch_bytes(const rg_bencode* h, size_t n_proofs);
rg_status rg_buckler_prove_encode_round_dev(const rg_bencode* h, size_t n_proofs, const uint64_t* d_w,
                                            const uint64_t* d_rand, uint64_t* d_wecd, uint64_t* d_com,
                                            uint64_t* d_scratch, void* stream);
rg_status rg_buckler_prove_encode_round(const rg_bencode* h, size_t n_proofs, const uint64_t* w, const uint64_t* rand,
                                        uint64_t* wecd, uint64_t* com);

/* ------------------------------------------------------------------------------------ */
/* Jindo commitment (jindo/params.go, encoder.go, rns.go, prover.go, entities.go)         */
/* ------------------------------------------------------------------------------------ */
/* Shapes exactly as jindo.Parameters holds them (params.go:64-123); taken from Go
 * (NewParameters' float search is not re-derived here).
 * Accepted beyond NewParameters' own shapes (tests/golden/jindo_synth_params.json runs them): any
 * power-of-two d in 2..1024, 1..4 distinct primes q = 1 mod 2d below 2^62 per ring, of any sizes
 * and in any order, 2 <= base < 2^32 below every ring prime, slots * exp <= d (coefficients
 * [slots * exp, d) of an encode carry no digit), MSIS ranks up to 32.  The device samplers
 * (rg_jindo_sample_dev, rg_jindo_commit_sampled_dev) cover d = 256 only: RG_ERR_UNSUPPORTED. */
typedef struct {
  int rank, rows, cols, slots; /* Rank() Rows() Cols() Slots()                      */
  int exp;                     /* Exp(): digits per element (k)                      */
  int d;                       /* ring degree = max(k, 256)                          */
  int in_msis, out_msis, mlwe; /* InMSISRank() OutMSISRank() MLWERank()              */
  int dcmp;                    /* InCommitDecomposeLen()                             */
  int log_in_cut, log_out_cut; /* LogInCutOff() OutCutOff()                          */
  uint64_t base;               /* Base(): b with p = b^k + 1                          */
  int nq, nqo;                 /* limbs of RingQ() / RingQOut() (1..4, nqo <= nq)    */
  uint64_t q[4], qo[4];        /* RingQ().ModuliChain(), RingQOut().ModuliChain()   */
  int field_limbs;             /* L of E                                             */
  uint64_t field_q[16];        /* modulus of E, little-endian                        */
} rg_jindo_params;

typedef struct rg_jindo rg_jindo;

/* NewProver's deterministic part (prover.go:28-40): builds RNS NTT tables (Lattigo
 * convention: smallest primitive root >= 3) and uploads the commit key.
 * ck_in   [in_msis][rows][nq][d]   CommitKey.In   (entities.go:24-35)
 * ck_mlwe [in_msis][mlwe][nq][d]   CommitKey.MLWE (entities.go:37-48)
 * ck_out  [out_msis][dcmp][nqo][d] CommitKey.Out  (entities.go:50-61)                 */
rg_status rg_jindo_create(const rg_jindo_params* p, const uint64_t* ck_in, const uint64_t* ck_mlwe,
                          const uint64_t* ck_out, rg_jindo** out);
/* Same, with the commit key in DEVICE memory on the current device (e.g. the buffer an RCCL
 * broadcast of the key landed in): copied device-to-device on `stream`, never
 * through the host.  Returns after the copy and the key transposition have completed. */
rg_status rg_jindo_create_dev(const rg_jindo_params* p, const uint64_t* d_ck_in, const uint64_t* d_ck_mlwe,
                              const uint64_t* d_ck_out, void* stream, rg_jindo** out);
/* Same, deriving the commit key from the CRS exactly as NewCommitKey does
 * (SHA-384 -> AES-256-CTR -> SampleN, entities.go:21-73, uniform.go:38-95). */
rg_status rg_jindo_create_from_crs(const rg_jindo_params* p, const uint8_t* crs, size_t crs_len, rg_jindo** out);
void rg_jindo_destroy(rg_jindo* j);
/* Copy the commit key out (same layouts as rg_jindo_create). */
rg_status rg_jindo_commit_key(const rg_jindo* j, uint64_t* ck_in, uint64_t* ck_mlwe, uint64_t* ck_out);
/* The handle's device-resident commit key (same layouts; valid until rg_jindo_destroy), e.g. as
 * the source of a cross-GPU broadcast. */
rg_status rg_jindo_commit_key_dev(const rg_jindo* j, const uint64_t** d_ck_in, const uint64_t** d_ck_mlwe,
                                  const uint64_t** d_ck_out);

/* Prover.Commit (prover.go:45-62) with the randomness INJECTED so the result is
 * bit-exact against Go given the same draws:
 *  v          [nv][L]  the committed vector, Montgomery (1 <= nv <= rank)
 *  last_row   [cols*slots][L]  genFirstLastRow's MustSetRandom draws, last entry 0 (:68-72)
 *  mask       [rows][slots][L] the mask column's MustSetRandom draws, one row per
 *                              randEncodeTo (:95-115; rows the reference skips are ignored)
 *  enc_noise  [cols+1][rows][d] int64  the Gaussian samples c of each randEncodeTo
 *                              (encoder.go:166-183, TwinCDT or COSAC)
 *  mlwe_noise [cols+1][in_msis+mlwe][d] int64  the MLWE samples (prover.go:130-139)
 * Outputs (Lattigo limb-major residues, NTT + Montgomery domain, as Go holds them):
 *  o_incom  [dcmp][nqo][d]              Opening.InCommit
 *  o_enc    [cols+1][rows][nq][d]       Opening.Encode   (skipped rows = 0, as in Go)
 *  o_mlwe   [cols+1][in_msis+mlwe][nq][d]  Opening.MLWE
 *  o_com    [out_msis][nq][d]           Commitment.Value (rows >= nqo are 0: the reference
 *                                       allocates ringQ polys, entities.go:85-94)       */
rg_status rg_jindo_commit(const rg_jindo* j, const uint64_t* v, size_t nv, const uint64_t* last_row,
                          const uint64_t* mask, const int64_t* enc_noise, const int64_t* mlwe_noise,
                          uint64_t* o_incom, uint64_t* o_enc, uint64_t* o_mlwe, uint64_t* o_com);
/* Device-resident batch: `batch` independent commits of equal length nv; every array above
 * gains a leading [batch] dimension.  Asynchronous on `stream`. */
rg_status rg_jindo_commit_dev(const rg_jindo* j, size_t batch, const uint64_t* d_v, size_t nv,
                              const uint64_t* d_last_row, const uint64_t* d_mask, const int64_t* d_enc_noise,
                              const int64_t* d_mlwe_noise, uint64_t* d_incom, uint64_t* d_enc, uint64_t* d_mlwe,
                              uint64_t* d_com, void* stream);
/* The deterministic Ajtai core of Commit (prover.go:144-202) for a Go caller that keeps its own
 * encoder: from the NTT-domain Opening.Encode [cols+1][rows][nq][d] and Opening.MLWE
 * [cols+1][in_msis+mlwe][nq][d] (as Go holds them after commitColTo's encode and MLWE loops),
 * the inner Ajtai MACs, CRT rounding into Opening.InCommit [dcmp][nqo][d] (:144-176) and
 * outerCommitTo into Commitment.Value [out_msis][nq][d] (:180-202).  `_dev`: `batch` openings
 * back to back, asynchronous on `stream`.
 * Precondition (as in Lattigo, whose ring elements are always reduced): every word of `enc`,
 * `mlwe` and of the commit key given to rg_jindo_create* is a canonical residue (< its prime).
 * The MFMA MAC splits words into base-256 digits under that bound; a non-canonical word gives a
 * wrong commitment, not an error. */
rg_status rg_jindo_commit_core(const rg_jindo* j, const uint64_t* enc, const uint64_t* mlwe, uint64_t* o_incom,
                               uint64_t* o_com);
rg_status rg_jindo_commit_core_dev(const rg_jindo* j, size_t batch, const uint64_t* d_enc, const uint64_t* d_mlwe,
                                   uint64_t* d_incom, uint64_t* d_com, void* stream);
/* Bytes of device scratch rg_jindo_commit_dev needs for `batch` commits (allocated on first
 * use and cached inside the handle, one set per stream; exposed for capacity planning). */
size_t rg_jindo_scratch_bytes(const rg_jindo* j, size_t batch);
/* Drop the scratch cached for `stream` (and for the library-owned stream that splits a sampled
 * commit issued on it), after draining both.  Scratch sets are kept per stream for the handle's
 * lifetime otherwise; a caller that creates streams per request calls this before destroying one
 * (a destroyed stream's handle value may be reused by a new stream).  Not concurrent with calls
 * on that stream. */
rg_status rg_jindo_release_stream(rg_jindo* j, void* stream);
/* Which kernel runs the inner (prover.go:149-157) and outer (:180-191) Ajtai products of this
 * handle: RG_MAC_MFMA (mac_mfma.hip, the matrix cores; needs canonical inputs, see
 * rg_jindo_commit_core_dev) or RG_MAC_GENERIC (mac_kernel).  RG_MAC_VALU3 is never returned by this
 * build (the VALU mac3h kernel was removed in round 6; tools/experiments/jindo_knob_kernels.patch).
 * Introspection only; no reference counterpart. */
enum { RG_MAC_GENERIC = 0, RG_MAC_VALU3 = 1, RG_MAC_MFMA = 2 };
rg_status rg_jindo_mac_kinds(const rg_jindo* j, int* inner, int* outer);

/* ---- the prover's randomness on the device --------------------- */
/* The standard deviations jindo.Parameters holds (params.go:99-111): ecdStdDev,
 * ecdBlindStdDev, maskStdDev, maskBlindStdDev, mlweStdDev, maskMLWEStdDev.  Go takes them from
 * NewParameters' float search; the library builds the TwinCDT tables (gaussian_twin_cdt.go:13-70),
 * the ziggurat tables (gaussian_rounded.go:22-52) and the encoder's deltaInv (encoder.go:50-67)
 * from them.  Setup: call once per handle before the sampled entry points (not concurrently
 * with them).  All must be > 0 (RoundedGaussianSampler panics otherwise). */
typedef struct {
  double ecd, ecd_blind, mask, mask_blind, mlwe, mask_mlwe;
} rg_jindo_stddevs;
rg_status rg_jindo_set_stddevs(rg_jindo* j, const rg_jindo_stddevs* sd);
/* The encoder's deltaInv[exp] (-b^i / p as Go's big.Float computes it, zeroed below
 * 2^-50 / (b exp); encoder.go:50-67). */
rg_status rg_jindo_delta_inv(const rg_jindo* j, double* out);

/* One 32-byte seed per sampler the reference's Commit draws from (each is
 * NewUniformSamplerWithSeed(seed): key = SHA-384(seed)[:32], IV = [32:48], AES-256-CTR,
 * uniform.go:38-54): Encoder.twinCDT, Encoder.cosac and the RoundedGaussianSampler inside it,
 * Prover.mlweSampler, Prover.roundedSampler, and `uniform` in place of crypto/rand for
 * MustSetRandom (prover.go:65-139, encoder.go:149-183).  A Go caller draws them from crypto/rand.
 * On the device each sampler instance is a window of its domain's counter space (instance n =
 * the UniformSampler with IV + n 2^24, a 128-bit sum, so the 2^64 instance numbers have disjoint
 * windows): one per encode polynomial (twinCDT), per group of 8 consecutive coefficients of a
 * COSAC-encoded polynomial (COSAC and its RoundedGaussianSampler, instance poly (d/8) + group),
 * per MLWE polynomial (mlweSampler), per mask-column MLWE sample (rounded) and per field element
 * (uniform), numbered from `first_commit`, the index of
 * the batch's first commit among all commits made with these seeds (so batches and GPUs never
 * share keystream).  The sampled entry points return RG_ERR_INVALID when an instance number of
 * commits [first_commit, first_commit + batch) would pass 2^64 - 1, i.e. when
 * (first_commit + batch) * max((cols+1) rows d, (cols+1)(in_msis+mlwe) d, (cols+rows) slots) > 2^64.
 * Each instance is exactly the reference's sampler; the partition of draws among instances is
 * this library's.  Two provers (e.g. Go's SafeCopy, prover.go:327-339, which gives the copy new
 * crypto/rand samplers) either hold their own seeds or disjoint first_commit ranges. */
typedef struct {
  uint8_t enc_cdt[32], enc_cosac[32], enc_cosac_round[32], mlwe_cdt[32], mlwe_round[32], uniform[32];
} rg_jindo_seeds;
/* The randomness of `batch` commits of v (the layouts rg_jindo_commit_dev takes): lastRow (last
 * entry 0) and mask elements, the Gaussian samples of every randEncodeTo (centres from deltaInv
 * and the digits of the encoded elements) and of every MLWE polynomial.  Skipped encodes get 0. */
rg_status rg_jindo_sample_dev(const rg_jindo* j, size_t batch, const uint64_t* d_v, size_t nv,
                              const rg_jindo_seeds* seeds, unsigned long long first_commit, uint64_t* d_last_row,
                              uint64_t* d_mask, int64_t* d_enc_noise, int64_t* d_mlwe_noise, void* stream);
/* Prover.Commit end to end on the device (prover.go:45-202): rg_jindo_sample_dev, then
 * rg_jindo_commit_dev on that randomness (kept in the stream's scratch).  The batch runs as a DAG
 * over `stream` and two library-owned streams of that caller stream joined to it by events (the
 * COSAC sampler and the MLWE samplers beside TwinCDT, so each fills the others' tails); the
 * outputs are complete, as usual, when `stream` has passed the call. */
rg_status rg_jindo_commit_sampled_dev(const rg_jindo* j, size_t batch, const uint64_t* d_v, size_t nv,
                                      const rg_jindo_seeds* seeds, unsigned long long first_commit, uint64_t* d_incom,
                                      uint64_t* d_enc, uint64_t* d_mlwe, uint64_t* d_com, void* stream);
/* UniformSampler.Sample() words [first_word, first_word + n) of instance `instance` of
 * NewUniformSamplerWithSeed(seed) (instance 0 is that sampler itself; uniform.go:56-82, including
 * the XOR-accumulating 8192-byte buffer). */
rg_status rg_uniform_words_dev(const uint8_t* seed, size_t seed_len, unsigned long long instance,
                               unsigned long long first_word, size_t n, uint64_t* d_out, void* stream);

/* Prover.Evaluate (prover.go:205-324), device-resident, with the Fiat-Shamir challenges
 * INJECTED: the transcript (SHAKE128 over CommitKey/Commitment/Proof serializations) stays in
 * the Go caller, which also keeps the shape panics (:206-216).  What it derives from the
 * transcript's bytes is built on the device: the challenge polynomials by
 * rg_jindo_encode_challenges_dev, encode(leftVec(x)) by rg_jindo_eval_point_dev and the
 * evaluations by rg_poly_evaluate_batch_dev (below).  Challenge polynomials are ringQ / ringQOut
 * residues in the NTT + Montgomery domain, as Go holds them; every product is
 * MulCoeffsMontgomeryThenAdd.
 * 1. openBatch = sum_i open[i] * batch[i] (:228-266); with d_bq = d_bo = NULL (params.batch == 1,
 *    batch must be 1) openBatch = open[0] (:267-269).  A GPU holding a shard of a batch passes its
 *    openings and their challenges; the shards' openBatches sum across GPUs (RCCL all-reduce of
 *    the words, exact while n_gpus * q < 2^64) and rg_jindo_eval_reduce_dev folds them mod q.
 *      d_incom [batch][dcmp][nqo][d], d_enc [batch][cols+1][rows][nq][d],
 *      d_mlwe [batch][cols+1][in_msis+mlwe][nq][d]  the openings (rg_jindo_commit_dev layout)
 *      d_bq [batch][nq][d], d_bo [batch][nqo][d]     batch[i] in ringQ and batchOut[i] in ringQOut
 *      d_ob_*  openBatch in the single-opening layouts; openBatch.InCommit = Proof.InCommit */
rg_status rg_jindo_eval_batch_dev(const rg_jindo* j, size_t batch, const uint64_t* d_incom, const uint64_t* d_enc,
                                  const uint64_t* d_mlwe, const uint64_t* d_bq, const uint64_t* d_bo,
                                  uint64_t* d_ob_incom, uint64_t* d_ob_enc, uint64_t* d_ob_mlwe, void* stream);
/* words mod q, in place, over an openBatch (after a cross-GPU sum of partial openBatches) */
rg_status rg_jindo_eval_reduce_dev(const rg_jindo* j, uint64_t* d_ob_incom, uint64_t* d_ob_enc, uint64_t* d_ob_mlwe,
                                   void* stream);
/* 2. Proof.Partial[i] = sum_j left[j] * openBatch.Encode[i][j] (:274-278) and
 *    Proof.PartialMask over column cols (:280-282):
 *      d_left [rows][nq][d] (encode(leftVec(x)[j]))   d_partial [cols+1][nq][d], last = PartialMask */
rg_status rg_jindo_eval_partial_dev(const rg_jindo* j, const uint64_t* d_ob_enc, const uint64_t* d_left,
                                    uint64_t* d_partial, void* stream);
/* 3. Proof.Encode[i] = openBatch.Encode[cols][i] + sum_j chals[j] * openBatch.Encode[j][i] and
 *    Proof.MLWE[i] likewise (:300-314):
 *      d_chals [cols][nq][d]   d_pf_enc [rows][nq][d]   d_pf_mlwe [in_msis+mlwe][nq][d]          */
rg_status rg_jindo_eval_respond_dev(const rg_jindo* j, const uint64_t* d_ob_enc, const uint64_t* d_ob_mlwe,
                                    const uint64_t* d_chals, uint64_t* d_pf_enc, uint64_t* d_pf_mlwe, void* stream);
/* The evaluation point's vectors (utils.go:63-82), from x (one Montgomery element on the device):
 *   d_left  [rows][nq][d]  Encoder.encode([leftVec(x)[j]]) (encoder.go:105-146) for every row j:
 *           leftVec[j] = (x^(cols slots))^j, then leftVec[rows-1] = x; digit i of the plain value at
 *           coefficient i * slots, every other coefficient zero, MFormLazy and NTT per prime -- word
 *           for word what Commit produces for that element in slot 0 of an otherwise empty row
 *   d_right [cols*slots][L]  rightVec(x)[i] = x^i; NULL: not written (Evaluate needs d_left only)
 * Any shape rg_jindo_create accepts.  Asynchronous on `stream`. */
rg_status rg_jindo_eval_point_dev(const rg_jindo* j, const uint64_t* d_x, uint64_t* d_left, uint64_t* d_right,
                                  void* stream);
/* encodeChallengeTo (utils.go:20-46) of n challenges into ringQ (ring = 0) or ringQOut (ring = 1):
 * d_bytes [n][16], the transcript's bytes of each challenge (two big-endian words, the first the
 * low word); exp successive remainders by ChallengeBound, a remainder r > bound / 2 stored as
 * q_l - (bound - r), at coefficients i * slots; MForm and NTT.  d_out [n][nq or nqo][d].
 * ChallengeBound = 1 gives zero polynomials, as in the reference.  RG_ERR_INVALID for another
 * `ring`, and where ChallengeBound is 0 (exp > 120), the reference's division by zero. */
rg_status rg_jindo_encode_challenges_dev(const rg_jindo* j, int ring, const uint8_t* d_bytes, size_t n,
                                         uint64_t* d_out, void* stream);
/* Parameters.ChallengeBound() (params.go:357-360): min(base, 1 << (120 / exp)) / 2.  RG_ERR_INVALID
 * (with the reason in rg_last_error) where it is 0. */
rg_status rg_jindo_challenge_bound(const rg_jindo_params* p, uint64_t* bound);

/* Verifier.Verify (verifier.go:50-282), device-resident, with the Fiat-Shamir challenges
 * INJECTED as in Evaluate: the caller replays the transcript (SHAKE128 over the commit key,
 * commitments, x, Proof.Partial; :56-96) and keeps the shape panics (:51-54); the challenge
 * polynomials, encode(leftVec(x)) and rightVec(x) (utils.go:20-82) come from
 * rg_jindo_encode_challenges_dev and rg_jindo_eval_point_dev on the transcript's bytes.
 *   d_com   [batch][out_msis][nq][d]  the commitments (rg_jindo_commit_dev layout)
 *   d_bq, d_bo [batch][nq][d], [batch][nqo][d]  batch[i] / batchOut[i]; NULL when batch == 1
 *   d_chals [cols][nq][d]   d_left [rows][nq][d] (encode(leftVec(x)[j]))
 *   d_right [cols*slots][L] rightVec(x)   d_y [batch][L]  the claimed evaluations (Montgomery)
 *   the Proof: d_pf_incom [dcmp][nqo][d], d_pf_partial [cols+1][nq][d] (Partial, then
 *   PartialMask), d_pf_enc [rows][nq][d], d_pf_mlwe [in_msis+mlwe][nq][d]  (as Evaluate wrote)
 *   in_com_dcmp_two_nm, res_two_nm: Parameters.InComDcmpTwoNm() / ResTwoNm() (params.go:432-440)
 * All four checks run (the reference stops at the first failure; `ok` is the same verdict).
 * ModUpQtoP (:173) is taken as the centred lift of the ringQOut coefficients (the reading under
 * which the reference's own TestJindo completes; Lattigo's source is absent: parity unpinned).
 * Synchronous: returns after the result is on the host. */
typedef struct {
  uint64_t outer_norm_sq[10]; /* verifyNorm's nmSq before Sqrt (:263-276), little-endian words */
  uint64_t inner_norm_sq[10];
  int outer_ok, inner_ok;     /* Float64(isqrt(nmSq)) < bound (:278-281), decided exactly  */
  int consistency_ok;         /* verifyConsistency (:203-221)                              */
  int eval_ok;                /* verifyEval (:224-259)                                     */
  uint64_t eval_lhs[16];      /* sum right * Decode(Partial) (Montgomery)                  */
  uint64_t eval_rhs[16];      /* yBatch                                                    */
  int ok;                     /* Verify's return value                                     */
} rg_jindo_verify_result;
rg_status rg_jindo_verify_dev(const rg_jindo* j, size_t batch, const uint64_t* d_com, const uint64_t* d_bq,
                              const uint64_t* d_bo, const uint64_t* d_chals, const uint64_t* d_left,
                              const uint64_t* d_right, const uint64_t* d_y, const uint64_t* d_pf_incom,
                              const uint64_t* d_pf_partial, const uint64_t* d_pf_enc, const uint64_t* d_pf_mlwe,
                              double in_com_dcmp_two_nm, double res_two_nm, rg_jindo_verify_result* res,
                              void* stream);
/* n_proofs proofs against one handle verified by one enqueue: the Jindo counterpart of
 * rg_buckler_verify_checks_multi_dev, to be queued behind it on the same stream.  Every array
 * argument of rg_jindo_verify_dev gains a leading [n_proofs] dimension, proof-major and contiguous
 * (d_com [n_proofs][batch][out_msis][nq][d], d_chals [n_proofs][cols][nq][d], d_left
 * [n_proofs][rows][nq][d], d_right [n_proofs][cols*slots][L], d_y [n_proofs][batch][L], ...): each
 * proof has its own transcript, hence its own challenges and evaluation point.  `batch` and the two
 * bounds hold for all proofs; d_bq and d_bo are both NULL iff batch == 1.
 *
 * d_out [n_proofs][RG_JINDO_VERIFY_WORDS] receives one record per proof, every word written:
 *   word 0      ok (1 or 0)
 *   word 1      bit 0 outer_ok, bit 1 inner_ok, bit 2 consistency_ok, bit 3 eval_ok
 *   words 2-11  outer_norm_sq        words 12-21  inner_norm_sq
 *   words 22-37 eval_lhs: L words, the rest 0
 *   words 38-53 eval_rhs: L words, the rest 0 (batch == 1: y[0], as the single entry reports it)
 * with the single entry's values, the norm decisions included (made on the device against K^2 of each
 * bound).  rg_jindo_verify_unpack (host only) turns one record into an rg_jindo_verify_result;
 * RG_ERR_INVALID for a NULL argument or a field_limbs no kernel is built for.
 *
 * Asynchronous on `stream`: nothing is allocated, freed, copied to the host or waited for inside, and
 * the number of launches does not depend on n_proofs.  The handle is only read, so calls on different
 * streams with different scratch are independent.  d_scratch holds
 * rg_jindo_verify_multi_scratch_bytes(j, n_proofs, batch) bytes (0 for a NULL handle, an n_proofs of 0
 * or above RG_JINDO_VERIFY_MAX_PROOFS -- a proof per grid row -- or batch < 1).
 * RG_ERR_INVALID, with the reason in rg_last_error and before the device is touched: a NULL handle,
 * input, output or scratch; n_proofs of 0 or above the limit; batch < 1; the d_bq / d_bo rule; d_out
 * or d_scratch overlapping an input or each other. */
#define RG_JINDO_VERIFY_MAX_PROOFS 65535
#define RG_JINDO_VERIFY_WORDS 54 /* uint64 words per proof record */
size_t rg_jindo_verify_multi_scratch_bytes(const rg_jindo* j, size_t n_proofs, size_t batch);
rg_status rg_jindo_verify_multi_dev(const rg_jindo* j, size_t n_proofs, size_t batch, const uint64_t* d_com,
                                    const uint64_t* d_bq, const uint64_t* d_bo, const uint64_t* d_chals,
                                    const uint64_t* d_left, const uint64_t* d_right, const uint64_t* d_y,
                                    const uint64_t* d_pf_incom, const uint64_t* d_pf_partial,
                                    const uint64_t* d_pf_enc, const uint64_t* d_pf_mlwe, double in_com_dcmp_two_nm,
                                    double res_two_nm, uint64_t* d_out, void* d_scratch, void* stream);
rg_status rg_jindo_verify_unpack(const uint64_t* words, int field_limbs, rg_jindo_verify_result* res);
/* rg_jindo_eval_point_dev for n_points points in one enqueue: what a batch verification derives from
 * its proofs' evaluation points, in the layouts rg_jindo_verify_multi_dev takes.
 *   d_x     point k is the Montgomery element at d_x + k * x_stride * L words; x_stride = 5 reads the
 *           points in place from the Buckler batch's d_chal [n_proofs][5][L] (evalPoint is element 0)
 *   d_left  [n_points][rows][nq][d]     d_right [n_points][cols*slots][L]; NULL: not written
 * Each point gives, word for word, what rg_jindo_eval_point_dev gives for it, left[rows-1] = x
 * written last included (also when rows == 1).  Any shape rg_jindo_create accepts, any built limb
 * count.
 *
 * Asynchronous on `stream`: nothing is allocated, freed, copied to the host or waited for inside; the
 * handle is only read (no per-stream state, no lock), so calls on different streams with different
 * d_scratch are independent; two launches whatever n_points (every point's leftVec and rightVec by
 * square and multiply, a lane per element; then the encoding, a workgroup per row and point).
 * d_scratch holds rg_jindo_eval_point_multi_scratch_bytes(j, n_points) bytes, every point's leftVec
 * [n_points][rows][L] (0 for a NULL handle, n_points of 0 or above RG_JINDO_POINT_MAX_POINTS -- a
 * point per grid row).  n_points == 0 returns RG_OK and touches nothing.  RG_ERR_INVALID, with the reason in rg_last_error
 * and before the device is touched: a NULL handle, d_x, d_left or d_scratch; x_stride of 0 or above
 * 2^30; n_points above the limit; d_left, d_right or d_scratch overlapping each other or the strided
 * extent of d_x. */
#define RG_JINDO_POINT_MAX_POINTS 65535
size_t rg_jindo_eval_point_multi_scratch_bytes(const rg_jindo* j, size_t n_points);
rg_status rg_jindo_eval_point_multi_dev(const rg_jindo* j, size_t n_points, const uint64_t* d_x, size_t x_stride,
                                        uint64_t* d_left, uint64_t* d_right, void* d_scratch, void* stream);
/* The whole front end of rg_jindo_verify_multi_dev, from the bytes of n_proofs replayed transcripts:
 * the three encodeChallengeTo passes of rg_jindo_encode_challenges_dev (batch[i] into ringQ and
 * ringQOut, chals into ringQ), then the point pass above, queued on `stream` with a launch count
 * (5, or 3 when batch == 1) that does not depend on n_proofs.
 *   d_x, x_stride  as above, a point per proof
 *   d_batch_bytes  [n_proofs][batch][16]; NULL iff batch == 1     d_chal_bytes [n_proofs][cols][16]
 *   d_bq, d_bo     [n_proofs][batch][nq | nqo][d]; both NULL iff batch == 1
 *   d_chals [n_proofs][cols][nq][d]   d_left, d_right, d_scratch  as above
 * The outputs are the d_bq, d_bo, d_chals, d_left and d_right arguments of rg_jindo_verify_multi_dev;
 * a batch verification is: the bytes, this call, rg_buckler_verify_checks_multi_dev,
 * rg_jindo_verify_multi_dev, on one stream.  The bytes are either uploaded from a host transcript or
 * squeezed in place by a device one (rg_xof_squeeze_dev writes d_batch_bytes and d_chal_bytes in
 * exactly this layout), in which case nothing of the batch passes through the host.  Asynchrony, scratch (the same size:
 * rg_jindo_verify_inputs_multi_scratch_bytes) and refusals as above, over every output and input; also
 * refused: batch < 1 or above 32768, the NULL rule of d_batch_bytes / d_bq / d_bo, a NULL d_chal_bytes
 * or d_chals, and a ChallengeBound of 0 (rg_jindo_challenge_bound: exp > 120). */
size_t rg_jindo_verify_inputs_multi_scratch_bytes(const rg_jindo* j, size_t n_proofs);
rg_status rg_jindo_verify_inputs_multi_dev(const rg_jindo* j, size_t n_proofs, size_t batch, const uint64_t* d_x,
                                           size_t x_stride, const uint8_t* d_batch_bytes, const uint8_t* d_chal_bytes,
                                           uint64_t* d_bq, uint64_t* d_bo, uint64_t* d_chals, uint64_t* d_left,
                                           uint64_t* d_right, void* d_scratch, void* stream);

/* Prover.Evaluate (prover.go:205-324) for n_proofs proofs of one handle, in two enqueues around the
 * transcript, which Evaluate reads twice: the batch bytes before openBatch, the challenge bytes
 * after Partial / PartialMask have been absorbed.  With a host transcript a batch is: upload the
 * points and batch bytes, call 1, download d_pf_partial, absorb and squeeze on the host, upload the
 * challenge bytes, call 2 (and rg_poly_evaluate_multi_dev for the evaluations), all on one stream.
 * With a device transcript (rg_xof_*, above) there is no host step: rg_xof_squeeze_dev writes
 * d_batch_bytes before call 1, rg_xof_absorb_plan_dev reads d_pf_partial after it and a second
 * squeeze writes d_chal_bytes before call 2, one uninterrupted queue.
 *
 * 1. rg_jindo_eval_open_multi_dev (:227-289): the batch challenges' encodings, encode(leftVec(x)),
 *    openBatch and the partials of every proof.
 *      d_incom, d_enc, d_mlwe  the openings: opening t of proof p starts p * open_proof_stride +
 *          t * open_commit_stride openings in, one opening being one [dcmp][nqo][d],
 *          [cols+1][rows][nq][d] or [cols+1][in_msis+mlwe][nq][d] block of the respective array.
 *          Strides (batch, 1) read a [proof][commit] buffer; (1, n_proofs) read the [commit][proof]
 *          buffers that one rg_jindo_commit_dev per round with batch = n_proofs leaves behind.
 *      d_x, x_stride   as rg_jindo_eval_point_multi_dev, a point per proof, read in place
 *      d_batch_bytes   [n_proofs][batch][16]
 *      d_ob_enc  [n_proofs][cols+1][rows][nq][d]   d_ob_mlwe [n_proofs][cols+1][in_msis+mlwe][nq][d]
 *      d_pf_incom   [n_proofs][dcmp][nqo][d]  openBatch.InCommit = Proof.InCommit
 *      d_pf_partial [n_proofs][cols+1][nq][d]  Partial, then PartialMask
 *    batch == 1: openBatch = open[0] (:267-269); d_batch_bytes, d_ob_enc and d_ob_mlwe are all NULL
 *    (with batch > 1 none of them is), d_pf_incom receives a copy of each proof's InCommit, the
 *    partials come straight from d_enc, and the caller hands d_enc and d_mlwe themselves to call 2
 *    with ob_proof_stride = open_proof_stride.
 *    Stream items: 7 for batch > 1 (two challenge encodings, two for the point pass, the InCommit and
 *    MLWE combinations, and one kernel that forms openBatch.Encode and the partials together: every
 *    opening word of Encode read once, openBatch.Encode written once and never read back), 4 for
 *    batch == 1 (the point pass, the InCommit copy, the partials).
 * 2. rg_jindo_eval_respond_multi_dev (:296-316): the response challenges' encodings, Proof.Encode and
 *    Proof.MLWE of every proof.
 *      d_ob_enc, d_ob_mlwe  the openBatch of proof p starts p * ob_proof_stride openings in: 1 after
 *                           call 1, open_proof_stride when batch == 1 and the openings are passed
 *      d_chal_bytes [n_proofs][cols][16]
 *      d_pf_enc [n_proofs][rows][nq][d]   d_pf_mlwe [n_proofs][in_msis+mlwe][nq][d]
 *    Stream items: 3 (the encoding, the two response products), whatever batch was.
 * Every output word is the canonical residue the single entries (rg_jindo_encode_challenges_dev,
 * rg_jindo_eval_point_dev, rg_jindo_eval_batch_dev, rg_jindo_eval_partial_dev,
 * rg_jindo_eval_respond_dev) give for that proof.
 *
 * Both are asynchronous on `stream`: nothing is allocated, freed, copied to the host or waited for
 * inside, the handle is only read, and the counts above do not depend on n_proofs.  d_scratch holds
 * rg_jindo_eval_open_multi_scratch_bytes(j, n_proofs, batch) resp.
 * rg_jindo_eval_respond_multi_scratch_bytes(j, n_proofs) bytes; both return 0 for the arguments the
 * call refuses (a NULL handle, n_proofs of 0 or above RG_JINDO_EVAL_MAX_PROOFS -- a proof per grid
 * row --, batch < 1 or above 32768).  RG_ERR_INVALID, with a reason in rg_last_error that starts
 * "jindo eval multi" and before the device is touched: a NULL handle, required buffer or scratch;
 * n_proofs or batch out of range; a stride of 0 (or above 2^31; x_stride above 2^30); the NULL rule
 * broken either way; a ChallengeBound of 0 (rg_jindo_challenge_bound); an output or the scratch
 * overlapping an input or another output, the extent of a strided input being its last opening's end. */
#define RG_JINDO_EVAL_MAX_PROOFS 65535
size_t rg_jindo_eval_open_multi_scratch_bytes(const rg_jindo* j, size_t n_proofs, size_t batch);
rg_status rg_jindo_eval_open_multi_dev(const rg_jindo* j, size_t n_proofs, size_t batch, const uint64_t* d_incom,
                                       const uint64_t* d_enc, const uint64_t* d_mlwe, size_t open_proof_stride,
                                       size_t open_commit_stride, const uint64_t* d_x, size_t x_stride,
                                       const uint8_t* d_batch_bytes, uint64_t* d_ob_enc, uint64_t* d_ob_mlwe,
                                       uint64_t* d_pf_incom, uint64_t* d_pf_partial, void* d_scratch, void* stream);
size_t rg_jindo_eval_respond_multi_scratch_bytes(const rg_jindo* j, size_t n_proofs);
rg_status rg_jindo_eval_respond_multi_dev(const rg_jindo* j, size_t n_proofs, const uint64_t* d_ob_enc,
                                          const uint64_t* d_ob_mlwe, size_t ob_proof_stride,
                                          const uint8_t* d_chal_bytes, uint64_t* d_pf_enc, uint64_t* d_pf_mlwe,
                                          void* d_scratch, void* stream);

/* ------------------------------------------------------------------------------------ */
/* SHAKE128 sponges on the device (the Jindo transcript, the projection XOF)              */
/* ------------------------------------------------------------------------------------ */
/* n_states independent SHAKE128 sponges (golang.org/x/crypto/sha3 NewShake128) that move in
 * lockstep: every state absorbs, and squeezes, the same number of bytes in every call, each state its
 * own bytes.  The position in the block and the phase (absorbing or squeezing) are therefore facts
 * of the handle on the host; only the [n_states][25] words live on the device.
 *
 *   rg_xof_create        n_states zeroed sponges, absorbing, at position 0
 *   rg_xof_reset_dev     sha3's Reset(): zeroed and absorbing again
 *   rg_xof_copy_dev      Clone(): dst takes src's words, position and phase
 *   rg_xof_absorb_dev    state s absorbs the len bytes at d_bytes + s * state_stride; stride 0 gives
 *                        every state the same bytes.  Any pointer alignment, stride and len (0 too).
 *   rg_xof_absorb_plan_dev  every state absorbs the message a plan describes (below)
 *   rg_xof_squeeze_dev   state s writes the next len bytes of its output at d_out + s * out_stride;
 *                        the bytes between len and out_stride are not touched.  The first squeeze
 *                        pads and permutes; later ones continue the same stream (Go's Read of 16
 *                        bytes, cols times over, is one stream).  Absorbing after a squeeze is
 *                        RG_ERR_INVALID (the reference panics); reset returns the handle to absorbing.
 *
 * A plan is the serialisation of one message as a flat list of segments, absorbed in order:
 *   base == RG_XOF_LITERAL   len bytes at `offset` of the plan's literal blob, which is copied to the
 *                            device once, at creation, and is the same for every state
 *   any other base           for state s, len bytes at d_bases[base] + offset + s * state_stride
 * Lattigo's Poly.WriteTo framing is not pinned by this library: the caller states the framing bytes
 * as literals, and the residue rows are segments into the buffers rg_jindo_commit_dev and
 * rg_jindo_eval_open_multi_dev leave behind (a coefficient is a little-endian uint64 there as in
 * Lattigo's serialisation).  Up to 65,536 segments and RG_XOF_MAX_BASES bases; the base pointers
 * travel as kernel arguments, so one plan serves every batch.  rg_xof_plan_bytes: the bytes each
 * state absorbs (0 for NULL).
 *
 * Every _dev call is asynchronous on `stream`: nothing is allocated, freed, copied to the host or
 * waited for inside, and each is one stream item whatever n_states, len and the segment count.
 * RG_ERR_INVALID, with the reason in rg_last_error (it starts "xof:") and before the device is
 * touched or the handle changed: a NULL argument (d_bytes / d_out may be NULL when len is 0);
 * n_states of 0; a segment whose base is outside [-1, n_bases) or whose base pointer is NULL; a
 * literal run past the blob; n_bases above RG_XOF_MAX_BASES; out_stride < len with more than one
 * state; a copy between handles of different n_states; absorbing after a squeeze.
 * A handle is NOT safe for concurrent calls: its position and phase change with every call, so one
 * thread at a time, and calls on one handle take effect in the order they are issued on one stream. */
typedef struct rg_xof rg_xof;
typedef struct rg_xof_plan rg_xof_plan;
#define RG_XOF_LITERAL (-1)
#define RG_XOF_MAX_BASES 8
typedef struct
{
  int base;
  size_t offset, state_stride, len;
} rg_xof_seg;

rg_status rg_xof_create(size_t n_states, rg_xof** out);
void rg_xof_destroy(rg_xof* x);
rg_status rg_xof_reset_dev(rg_xof* x, void* stream);
rg_status rg_xof_copy_dev(rg_xof* dst, const rg_xof* src, void* stream);
rg_status rg_xof_absorb_dev(rg_xof* x, const uint8_t* d_bytes, size_t len, size_t state_stride, void* stream);
rg_status rg_xof_plan_create(const rg_xof_seg* segs, size_t n_segs, const uint8_t* literals, size_t literal_len,
                             rg_xof_plan** out);
void rg_xof_plan_destroy(rg_xof_plan* p);
size_t rg_xof_plan_bytes(const rg_xof_plan* p);
rg_status rg_xof_absorb_plan_dev(rg_xof* x, const rg_xof_plan* p, const void* const* d_bases, size_t n_bases,
                                 void* stream);
rg_status rg_xof_squeeze_dev(rg_xof* x, uint8_t* d_out, size_t len, size_t out_stride, void* stream);

/* ------------------------------------------------------------------------------------ */
/* Device memory helpers (so a cgo caller needs no HIP headers)                           */
/* ------------------------------------------------------------------------------------ */
/* rg_malloc: `bytes` of memory on the current device (RG_ERR_NOMEM when it has none left).
 * rg_memcpy_*: asynchronous copies ordered on `stream` (NULL = the null stream) with the `_dev`
 * calls issued on it, so a kernel launched after rg_memcpy_h2d on the same stream reads the
 * copied data.  The host side may be ordinary pageable memory (a Go slice, malloc), and for such
 * memory the call may return before the copy has happened: the caller may overwrite or free the
 * source of rg_memcpy_h2d, and may read the destination of rg_memcpy_d2h, only after
 * rg_stream_sync(stream) has returned.  rg_stream_sync returns when everything issued on `stream`
 * so far has completed.  tools/abi_replay.c is a caller written to this contract. */
rg_status rg_malloc(void** d_ptr, size_t bytes);
rg_status rg_free(void* d_ptr);
rg_status rg_memcpy_h2d(void* d_dst, const void* src, size_t bytes, void* stream);
rg_status rg_memcpy_d2h(void* dst, const void* d_src, size_t bytes, void* stream);
rg_status rg_memcpy_d2d(void* d_dst, const void* d_src, size_t bytes, void* stream);
rg_status rg_stream_sync(void* stream);
rg_status rg_set_device(int device);
/* Measurement hook.  libringo.so refuses every probe but 0 (RG_ERR_INVALID): no production call
 * can switch a kernel.  Only the experiments build (libringo_exp.so, bench.py's compute-floor
 * legs and tools/) honours it: probe 4 makes the single-word 2^16 NTT launches (ntt16_pass), probe
 * 5 the q255 2^16 launches (ntt256_pass), skip their HBM data loads and stores, so the same
 * launches time the kernel's compute floor; their outputs are then meaningless.  0 restores the
 * production kernels.  Per calling thread. */
rg_status rg_set_probe(int probe);
/* the calling thread's current device (one rank per GPU: LOCAL_RANK -> rg_set_device) */
rg_status rg_get_device(int* device);
rg_status rg_device_count(int* n);

#ifdef __cplusplus
}
#endif
#endif /* RINGO_H */
