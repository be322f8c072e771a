"""buckler mirror: the Buckler prover's per-witness device work over
libringo -- the Encoder (buckler/encoder.go) and ArithmeticConstraint / Prover.evalCircuit
(buckler/constraint.go, buckler/prover.go:355-379).  Same names and argument meaning as the
reference; MustSetRandom draws are injected (`rand=`), as everywhere in this library.

    enc = NewEncoder(F, rank, embRank)                 # newEncoder (encoder.go:15-20)
    p = enc.RandEncode(w, rand=r)                      # RandEncode (encoder.go:42-54)
    c = ArithmeticConstraint(F); c.AddTerm(None, a, b) # constraint.go:15-53
    out = EvalCircuit(F, batchConst, [c], wEcdNTT, pwEcdNTT)   # prover.go:355-379

and the linear-check half (buckler/linear.go, buckler/prover.go:381-485): the four LinearCheckers,
sumCheckMask, and linCheck / sumCheck / arithCheck with their challenges injected.

    chk = NewNTTChecker(F, rank); chk.TransformTo(vOut, v); chk.TransposeTo(vOut, v)
    proj = ProjChecker(F, rank); proj.SetXOF(xof_bytes)        # prover.go:168-176
    mask, maskSum = SumCheckMask(F, rank, maskRank, embRank, rand)
    quo, remLo, remHi = LinCheck(F, rank, embRank, jindoRank, bc, lc, mask, checkers, pairs, wEcdNTT)

and the norm decomposition of the witness assignment (buckler/utils.go:34-56, prover.go:77-111,
182-192):

    dc = Decomposer(F, bound)                                  # decomposeBase(bound) uploaded once
    digits = dc.DecomposeInf(w)                                # [nb][rank][L], one witness per digit
    wDcmp = dc.DecomposeProj(wProj)                            # second round, prover.go:182-192
    wDcmp, sqNm = dc.DecomposeTwoNorm(w); pwBase, pwMask = TwoNormPublic(F, rank, bound)

and the verifier's checks (buckler/verifier.go:178-315), one proof or a batch of proofs of one circuit:

    plan = VerifyPlan(F, rank, jindoRank, wCnt, nPw, lin, arith, sum)
    verdict, sides, pwEvals = plan.checks(evals, pw, chal, maskSums)
    verdicts, sides, pwEvals = plan.checks_multi(evals, pw, xof, chal, maskSums)   # [n] in front of each

and the prover's three checks (buckler/prover.go:399-485) for a batch of proofs of one circuit in one call:

    plan = ProvePlan(F, rank, embRank, jindoRank, nW, nPw, lin, arith, arithMaxRank, sum, sumMaxRank)
    arithQuo, linQuo, linRemLo, linRemHi, sumQuo, sumRemLo, sumRemHi, rem0 = plan.checks(w, pw, xof, chal, linMask, sumMask)

and what stands between the commit rounds before them (buckler/prover.go:165-240), for the same batch:

    proj = ProjRoundPlan(F, rank, nW, [(src, projID, dcmpID, Decomposer(F, rank * bound))])
    w = proj.round(w, xof)                                     # the proj and dcmp rows of every proof
    masks, maskComs, maskSums = SumCheckMaskBatch(F, rank, maskRank, embRank, rand)

and what stands before the first commit and at each commit round (buckler/prover.go:77-111, 136-153,
195-201), on the same proof-major table:

    dcmp = DcmpRoundPlan(F, rank, nW, inf=[(src, bound, [digit rows])], two=[(src, bound, dst)])
    w, sqNm = dcmp.round(w)                                    # the digit and dst rows of every proof
    enc = EncodeRoundPlan(F, rank, embRank, nW, sel)           # sel: the rows of this commit round
    wEcd, comPolys = enc.round(w, rand, wEcd)                  # RandEncode of rows sel, Coeffs[:rank+1] contiguous

and the MustSetRandom draws all of these take, made on the device (element.go:299-343):

    smp = FieldSampler(F, seed)                                # NewUniformSamplerWithSeed(seed) for crypto/rand
    rand = smp.elems(first, n)                                 # element i: SetRandom from instance first + i
    masks, maskComs, maskSums = SumCheckMaskBatchSampled(smp, rank, maskRank, embRank, nProofs, first)
"""
import ctypes

import numpy as np

from ._lib import check, lib, ptr, vp
from .bigpoly import NewCyclicTransformer, Poly, RingoPanic, _addr, _stream


class Encoder:
    """Encoder[E] (buckler/encoder.go:9-12): a CyclicTransformer at the witness rank and the
    embedding rank of the output polynomials."""

    def __init__(self, field, rank, embed_rank):
        self.field = field
        self.ntt = NewCyclicTransformer(field, rank)
        self.embedRank = embed_rank

    def Encode(self, v):  # encoder.go:24-28
        pOut = Poly(self.field, self.embedRank, False)
        self.EncodeTo(pOut, v)
        return pOut

    def EncodeTo(self, pOut, v):  # encoder.go:32-38
        self._encode(pOut, v, None)

    def RandEncode(self, v, rand):  # encoder.go:42-46
        pOut = Poly(self.field, self.embedRank, False)
        self.RandEncodeTo(pOut, v, rand)
        return pOut

    def RandEncodeTo(self, pOut, v, rand):  # encoder.go:50-54; rand = the MustSetRandom draw
        self._encode(pOut, v, rand)

    def _encode(self, pOut, v, rand):
        L, rank = self.field.L, self.ntt.Rank()
        v = np.ascontiguousarray(np.asarray(v, np.uint64).reshape(-1, L)[:rank])  # v[:e.ntt.Rank()]
        if v.shape[0] < rank:
            raise RingoPanic("index out of range")  # Go slices past len(v)
        if pOut.Rank() < rank + (1 if rand is not None else 0):
            raise RingoPanic("index out of range")
        r = None if rand is None else np.ascontiguousarray(np.asarray(rand, np.uint64).reshape(L))
        out = np.zeros((pOut.Rank(), L), np.uint64)
        check(lib().rg_buckler_encode(self.ntt.h, pOut.Rank(), ptr(out), ptr(v), ptr(r)))
        pOut.Coeffs[...] = out
        pOut.IsNTT = False

    def encode_dev(self, d_out, d_v, batch, d_rand=None, d_scratch=None, stream=None):
        """rg_buckler_encode_dev: `batch` witnesses [batch][rank][L] -> [batch][embedRank][L]."""
        L, rank = self.field.L, self.ntt.Rank()
        sw = self.scratch_bytes(batch) // 8
        check(lib().rg_buckler_encode_dev(self.ntt.h, self.embedRank, _addr(d_out, batch * self.embedRank * L),
                                          _addr(d_v, batch * rank * L), batch,
                                          _addr(d_rand, batch * L) if d_rand is not None else None,
                                          _addr(d_scratch, sw) if d_scratch is not None else None, _stream(stream)))

    def scratch_bytes(self, batch):
        return lib().rg_buckler_encode_scratch_bytes(self.ntt.h, batch)


def NewEncoder(field, rank, embed_rank):
    return Encoder(field, rank, embed_rank)


class ArithmeticConstraint:
    """ArithmeticConstraint[E] (constraint.go:6-12).  Witnesses and public witnesses are given by
    their witnessToID numbers; coefficients are Montgomery elements ([L] words)."""

    def __init__(self, field):
        self.field = field
        self.coeffs, self.hasCoeffPublicWitness, self.coeffsPublicWitness, self.witness = [], [], [], []
        self.wRank = 0

    def _const(self, v):
        return np.asarray(self.field.mont([v % self.field.q]), np.uint64).reshape(self.field.L)

    def AddTerm(self, coeffPublicWitness, *witness):  # constraint.go:15-21
        self.AddTermWithConst(self._const(1), coeffPublicWitness, *witness)

    def SubTerm(self, coeffPublicWitness, *witness):  # constraint.go:23-29
        self.AddTermWithConst(self._const(-1), coeffPublicWitness, *witness)

    def AddTermWithConst(self, coeff, coeffPublicWitness, *witness):  # constraint.go:31-53
        self.coeffs.append(np.asarray(coeff, np.uint64).reshape(self.field.L))
        self.hasCoeffPublicWitness.append(coeffPublicWitness is not None)
        self.coeffsPublicWitness.append(0 if coeffPublicWitness is None else int(coeffPublicWitness))
        self.witness.append([int(w) for w in witness])
        self.wRank = max(self.wRank, len(witness))

    def maxRank(self, rank):  # constraint.go:56-70
        maxDeg = 0
        for i, ws in enumerate(self.witness):
            deg = (rank - 1 if self.hasCoeffPublicWitness[i] else 0) + len(ws) * rank
            maxDeg = max(maxDeg, deg)
        return maxDeg + 1


class Circuit:
    """A set of constraints uploaded once (rg_buckler_circuit_create): the program evalCircuit walks."""

    def __init__(self, field, constraints):
        self.field = field
        L = field.L
        term_off, coeffs, pw, wit_off, wit = [0], [], [], [0], []
        for c in constraints:
            for i in range(len(c.coeffs)):
                coeffs.append(c.coeffs[i])
                pw.append(c.coeffsPublicWitness[i] if c.hasCoeffPublicWitness[i] else -1)
                wit.extend(c.witness[i])
                wit_off.append(len(wit))
            term_off.append(len(pw))
        self.n_w = 1 + max(wit, default=-1)
        self.n_pw = 1 + max(pw, default=-1)
        sz = ctypes.c_size_t
        to = (sz * len(term_off))(*term_off)
        wo = (sz * len(wit_off))(*wit_off)
        wi = (ctypes.c_uint64 * max(1, len(wit)))(*wit)
        pi = (ctypes.c_longlong * max(1, len(pw)))(*pw)
        cf = np.ascontiguousarray(np.array(coeffs, np.uint64).reshape(-1, L) if coeffs else np.zeros((1, L), np.uint64))
        h = vp()
        st = lib().rg_buckler_circuit_create(field.h, len(constraints), to, ptr(cf), pi, wo, wi, ctypes.byref(h))
        if st == -1:
            raise RingoPanic("inconsistent input(s)")
        check(st)
        self.h = h
        self._L = lib()

    def __del__(self):
        if getattr(self, "h", None) and getattr(self, "_L", None):  # the CDLL bound at creation
            self._L.rg_buckler_circuit_destroy(self.h)  # (module globals may already be gone at interpreter exit)
            self.h = None

    def eval_dev(self, rank, d_batch_const, d_w, n_w, d_pw, n_pw, d_out, stream=None):
        """rg_buckler_eval_circuit_dev (device-resident wEcdNTT [n_w][rank][L], pwEcdNTT [n_pw][rank][L])."""
        L = self.field.L
        check(lib().rg_buckler_eval_circuit_dev(self.h, rank, _addr(d_batch_const, L),
                                                _addr(d_w, n_w * rank * L) if n_w else None, n_w,
                                                _addr(d_pw, n_pw * rank * L) if n_pw else None, n_pw,
                                                _addr(d_out, rank * L), _stream(stream)))


def EvalCircuit(field, batchConst, constraints, wEcdNTT, pwEcdNTT):
    """Prover.evalCircuit (prover.go:355-379): wEcdNTT / pwEcdNTT are lists of NTT-domain Polys
    (or [n][rank][L] arrays); returns the NTT-domain Poly."""
    L = field.L
    circ = Circuit(field, constraints)

    def stack(ps):
        if ps is None or len(ps) == 0:
            return None, 0
        if isinstance(ps, np.ndarray):
            return np.ascontiguousarray(ps, np.uint64), ps.shape[0]
        for p in ps:
            if not p.IsNTT:
                raise RingoPanic("input not in NTT domain")  # base_op.go:133-142 MulTo
        return np.ascontiguousarray(np.stack([p.Coeffs for p in ps]), np.uint64), len(ps)

    w, n_w = stack(wEcdNTT)
    pw, n_pw = stack(pwEcdNTT)
    rank = (w if w is not None else pw).shape[-2] if (w is not None or pw is not None) else 0
    if n_w < circ.n_w or n_pw < circ.n_pw:
        raise RingoPanic("index out of range")
    out = Poly(field, rank, True)
    bc = np.ascontiguousarray(np.asarray(batchConst, np.uint64).reshape(L))
    res = np.zeros((rank, L), np.uint64)
    check(lib().rg_buckler_eval_circuit(circ.h, rank, ptr(bc), ptr(w), n_w, ptr(pw), n_pw, ptr(res)))
    out.Coeffs[...] = res
    return out


# ---- linear checkers (buckler/linear.go) ----------------------------------------------------------
def _status(st):
    if st == -1:
        raise RingoPanic("inconsistent input(s)")
    check(st)


def _elem(field, x):
    return np.ascontiguousarray(np.asarray(x, np.uint64).reshape(field.L))


def decomposeBase(x):
    """decomposeBase (utils.go:7-32) on a Python int."""
    x = int(x)
    dcmpLen = x.bit_length()
    tz = (x & -x).bit_length() - 1 if x else 0  # TrailingZeroBits
    if (1 << tz) == x:
        dcmpLen -= 1
    if dcmpLen <= 0:
        raise RingoPanic("index out of range")  # base[dcmpLen-1] on an empty slice
    base = []
    for _ in range(dcmpLen - 1):
        b = x - sum(base)
        base.append((b >> 1) + (b & 1))
    base.append(1)
    return base


class LinearChecker:
    """LinearChecker[E] (linear.go:12-17) over an rg_linchecker: TransformTo computes vOut = M v,
    TransposeTo vOut = M^T v, on [rank][L] arrays."""

    def __init__(self, field, rank, h):
        self.field, self.rank, self.h = field, rank, h
        self._L = lib()

    def __del__(self):
        if getattr(self, "h", None) and getattr(self, "_L", None):
            self._L.rg_buckler_checker_destroy(self.h)
            self.h = None

    def _host(self, fn, vOut, v):
        L = self.field.L
        v = np.asarray(v, np.uint64).reshape(-1, L)
        if v.shape[0] < self.rank or np.asarray(vOut).reshape(-1, L).shape[0] < self.rank:
            raise RingoPanic("index out of range")
        v = np.ascontiguousarray(v[:self.rank])
        out = np.zeros((self.rank, L), np.uint64)
        _status(fn(self.h, ptr(out), ptr(v)))
        np.asarray(vOut).reshape(-1, L)[:self.rank] = out
        return vOut

    def TransformTo(self, vOut, v):
        return self._host(lib().rg_buckler_checker_transform, vOut, v)

    def TransposeTo(self, vOut, v):
        return self._host(lib().rg_buckler_checker_transpose, vOut, v)

    def scratch_bytes(self, batch):
        return lib().rg_buckler_checker_scratch_bytes(self.h, batch)

    def transform_dev(self, d_out, d_v, batch, d_scratch=None, stream=None):
        """rg_buckler_checker_transform_dev: [batch][rank][L] -> [batch][rank][L]."""
        w = batch * self.rank * self.field.L
        sw = self.scratch_bytes(batch) // 8
        _status(lib().rg_buckler_checker_transform_dev(self.h, _addr(d_out, w), _addr(d_v, w), batch,
                                                       _addr(d_scratch, sw) if d_scratch is not None else None,
                                                       _stream(stream)))

    def transpose_dev(self, d_out, d_v, batch, stream=None):
        w = batch * self.rank * self.field.L
        _status(lib().rg_buckler_checker_transpose_dev(self.h, _addr(d_out, w), _addr(d_v, w), batch, _stream(stream)))


def NewNTTChecker(field, rank):
    """NewNTTChecker (linear.go:26-32)."""
    if rank <= 0 or rank & (rank - 1):
        raise RingoPanic("rank must be a power of two")  # NewCyclotomicTransformer, ntt.go:154-156
    h = vp()
    st = lib().rg_buckler_checker_create_ntt(field.h, rank, ctypes.byref(h))
    if st == -3:
        raise RingoPanic("NTT not supported")
    _status(st)
    return LinearChecker(field, rank, h)


def NewAutChecker(field, rank, idx, isNTT):
    """NewAutChecker (linear.go:54-61); `rank` stands for the evaluator's."""
    if idx % 2 == 0:
        raise RingoPanic("modular inverse does not exist")  # linear.go:86-88
    h = vp()
    _status(lib().rg_buckler_checker_create_aut(field.h, rank, idx, 1 if isNTT else 0, ctypes.byref(h)))
    return LinearChecker(field, rank, h)


class ProjChecker(LinearChecker):
    """newProjChecker (linear.go:98-106); SetXOF fills the matrix as Prove does (prover.go:168-176)."""

    def __init__(self, field, rank):
        if rank < 128:
            raise RingoPanic("index out of range")  # TransformTo writes vOut[0..127]
        h = vp()
        _status(lib().rg_buckler_checker_create_proj(field.h, rank, ctypes.byref(h)))
        super().__init__(field, rank, h)

    def SetXOF(self, xof):
        """xof: rank * 32 bytes, the SHAKE128 output column by column."""
        xof = bytes(xof)
        if len(xof) < self.rank * 32:
            raise RingoPanic("index out of range")
        _status(lib().rg_buckler_checker_set_xof(self.h, xof))
        return self

    def set_xof_dev(self, d_xof, stream=None):
        """rg_buckler_checker_set_xof_dev: d_xof a contiguous uint8 tensor of rank * 32 bytes (or an address)."""
        if not isinstance(d_xof, int):
            if str(d_xof.dtype) != "torch.uint8" or not d_xof.is_contiguous() or d_xof.device.type != "cuda" \
                    or d_xof.numel() < self.rank * 32:
                raise RingoPanic("XOF buffer: need rank * 32 contiguous bytes on the GPU")
            d_xof = d_xof.data_ptr()
        _status(lib().rg_buckler_checker_set_xof_dev(self.h, d_xof, _stream(stream)))
        return self

    def transpose_xof_scratch_bytes(self, batch):
        return lib().rg_buckler_checker_transpose_xof_scratch_bytes(self.h, batch)

    def transpose_xof_dev(self, d_out, d_v, batch, d_xof, d_bits_scratch, stream=None):
        """rg_buckler_checker_transpose_xof_dev: vector i of [batch][rank][L] transposed by the matrix
        of the XOF bytes d_xof[i] ([batch][rank * 32] uint8); the checker's own matrix is not used."""
        w = batch * self.rank * self.field.L
        _status(lib().rg_buckler_checker_transpose_xof_dev(
            self.h, _addr(d_out, w), _addr(d_v, w), batch, _xof_addr(d_xof, batch * self.rank * 32),
            _addr(d_bits_scratch, self.transpose_xof_scratch_bytes(batch) // 8), _stream(stream)))


def _xof_addr(d_xof, nbytes):
    """Device address of a contiguous uint8 tensor of at least nbytes (or an address)."""
    if d_xof is None or isinstance(d_xof, int):
        return d_xof
    if str(d_xof.dtype) != "torch.uint8" or not d_xof.is_contiguous() or d_xof.device.type != "cuda" \
            or d_xof.numel() < nbytes:
        raise RingoPanic(f"XOF buffer: need {nbytes} contiguous bytes on the GPU")
    return d_xof.data_ptr()


class ProjRecomposeChecker(LinearChecker):
    """newProjRecomposeChecker (linear.go:144-153): dcmpBase = decomposeBase(bound) as field elements."""

    def __init__(self, field, rank, bound):
        self.dcmpBase = decomposeBase(bound)
        base = np.ascontiguousarray(field.mont(self.dcmpBase))
        h = vp()
        _status(lib().rg_buckler_checker_create_recompose(field.h, rank, ptr(base), len(self.dcmpBase),
                                                          ctypes.byref(h)))
        super().__init__(field, rank, h)


# ---- sumCheckMask, the check tail, linCheck / sumCheck / arithCheck (prover.go:381-485) -----------
def Powers(field, c, n):
    """linCheckVec (prover.go:409-413): [n][L] with out[0] = 1, out[i] = out[i-1] * c."""
    out = np.zeros((n, field.L), np.uint64)
    _status(lib().rg_buckler_powers(field.h, ptr(_elem(field, c)), n, ptr(out)))
    return out


def powers_dev(field, d_c, n, d_out, stream=None):
    _status(lib().rg_buckler_powers_dev(field.h, _addr(d_c, field.L), n, _addr(d_out, n * field.L), _stream(stream)))


def PowersBatch(field, cs, n, c_stride=1):
    """rg_buckler_powers_batch: out[k][i] = c_k^i, [n_c][n][L]; cs holds base k at element k * c_stride."""
    cs = np.ascontiguousarray(np.asarray(cs, np.uint64).reshape(-1, field.L))
    if c_stride <= 0 or cs.shape[0] == 0:
        raise RingoPanic("inconsistent input(s)")
    n_c = (cs.shape[0] - 1) // c_stride + 1
    out = np.zeros((n_c, n, field.L), np.uint64)
    _status(lib().rg_buckler_powers_batch(field.h, ptr(cs), c_stride, n_c, n, ptr(out)))
    return out


def powers_batch_dev(field, d_c, c_stride, n_c, n, d_out, stream=None):
    """rg_buckler_powers_batch_dev: base k at d_c + k * c_stride * L words, d_out [n_c][n][L]."""
    L = field.L
    _status(lib().rg_buckler_powers_batch_dev(field.h, _addr(d_c, ((n_c - 1) * c_stride + 1) * L if n_c else None),
                                              c_stride, n_c, n, _addr(d_out, n_c * n * L), _stream(stream)))


def SumCheckMask(field, rank, maskRank, embRank, rand):
    """Prover.sumCheckMask(maskRank) (prover.go:381-397); rand [maskRank][L] = the MustSetRandom
    draws in the reference's order.  Returns (mask Poly of embRank, maskSum [L])."""
    L = field.L
    r = np.ascontiguousarray(np.asarray(rand, np.uint64).reshape(-1, L))
    if r.shape[0] < maskRank or maskRank > embRank:
        raise RingoPanic("index out of range")
    mask = Poly(field, embRank, False)
    res = np.zeros((embRank, L), np.uint64)
    msum = np.zeros(L, np.uint64)
    _status(lib().rg_buckler_sumcheck_mask(field.h, rank, maskRank, embRank, ptr(r), ptr(res), ptr(msum)))
    mask.Coeffs[...] = res
    return mask, msum


def sumcheck_mask_dev(field, rank, maskRank, embRank, d_rand, d_mask, d_mask_sum, stream=None):
    L = field.L
    _status(lib().rg_buckler_sumcheck_mask_dev(field.h, rank, maskRank, embRank, _addr(d_rand, maskRank * L),
                                               _addr(d_mask, embRank * L), _addr(d_mask_sum, L), _stream(stream)))


def check_finish_dev(embT, rank, d_eval, d_scale, d_mask, n_quo, jindo_rank, d_quo, d_rem_lo, d_rem_hi, d_scratch,
                     stream=None):
    """rg_buckler_check_finish_dev; embT = the CyclicTransformer at the embedding rank."""
    L, emb = embT.field.L, embT.Rank()
    _status(lib().rg_buckler_check_finish_dev(
        embT.h, rank, _addr(d_eval, emb * L), _addr(d_scale, L) if d_scale is not None else None,
        _addr(d_mask, emb * L) if d_mask is not None else None, n_quo, jindo_rank, _addr(d_quo, n_quo * L),
        _addr(d_rem_lo, (rank - 1) * L) if d_rem_lo is not None else None,
        _addr(d_rem_hi, jindo_rank * L) if d_rem_hi is not None else None,
        _addr(d_scratch, check_finish_scratch_bytes(embT) // 8), _stream(stream)))


def check_finish_scratch_bytes(embT):
    return lib().rg_buckler_check_finish_scratch_bytes(embT.h)


def _coeffs(p):
    return np.ascontiguousarray(p.Coeffs if isinstance(p, Poly) else p, np.uint64)


def _finish(field, embT, rank, evalNTT, scale, mask, n_quo, jindoRank, want_rem):
    L = field.L
    if n_quo < 0 or n_quo > embT.Rank():
        raise RingoPanic("slice bounds out of range")
    quo = np.zeros((n_quo, L), np.uint64)
    lo = np.zeros((rank - 1, L), np.uint64) if want_rem else None
    hi = np.zeros((jindoRank, L), np.uint64) if want_rem else None
    if want_rem and jindoRank < rank - 1:
        raise RingoPanic("index out of range")
    _status(lib().rg_buckler_check_finish(embT.h, rank, ptr(_coeffs(evalNTT)),
                                          ptr(_elem(field, scale)) if scale is not None else None,
                                          ptr(_coeffs(mask)) if mask is not None else None, n_quo, jindoRank,
                                          ptr(quo), ptr(lo), ptr(hi)))
    return quo, lo, hi


class LinCheckPlan:
    """What linCheck takes from the compiled context (rg_lincheck): the encoder at `rank`, the
    evaluator's transformer at `embRank`, ctx.linCheckers and ctx.linCheckConstraints as one list
    of (wOut, wIn) witness-ID pairs per checker."""

    def __init__(self, field, rank, embRank, checkers, constraints):
        if len(checkers) != len(constraints):
            raise RingoPanic("inconsistent input(s)")
        self.field, self.rank, self.embRank = field, rank, embRank
        self.enc = NewCyclicTransformer(field, rank)
        self.emb = NewCyclicTransformer(field, embRank)
        self.checkers = list(checkers)  # kept alive: the handle borrows them
        off, flat = [0], []
        for ps in constraints:
            for wOut, wIn in ps:
                flat += [int(wOut), int(wIn)]
            off.append(len(flat) // 2)
        self.n_w = 1 + max(flat, default=-1)
        hs = (vp * max(1, len(checkers)))(*[c.h.value for c in self.checkers])
        po = (ctypes.c_size_t * len(off))(*off)
        pa = (ctypes.c_uint64 * max(1, len(flat)))(*flat)
        h = vp()
        _status(lib().rg_buckler_lincheck_create(self.enc.h, self.emb.h, len(checkers), hs, po, pa, ctypes.byref(h)))
        self.h = h
        self._L = lib()

    def __del__(self):
        if getattr(self, "h", None) and getattr(self, "_L", None):
            self._L.rg_buckler_lincheck_destroy(self.h)
            self.h = None

    def scratch_bytes(self):
        return lib().rg_buckler_lin_check_scratch_bytes(self.h)

    def rem_offset_words(self):
        """Word offset of remPoly [embRank][L] in the scratch of a completed lin_check_dev."""
        return lib().rg_buckler_lin_check_rem_offset_bytes(self.h) // 8

    def lin_check_dev(self, d_batch_const, d_lin_const, d_mask, d_w, n_w, jindo_rank, d_quo, d_rem_lo, d_rem_hi,
                      d_scratch, stream=None):
        """rg_buckler_lin_check_dev (device-resident wEcdNTT [n_w][embRank][L])."""
        L, rank, emb = self.field.L, self.rank, self.embRank
        _status(lib().rg_buckler_lin_check_dev(
            self.h, _addr(d_batch_const, L), _addr(d_lin_const, L), _addr(d_mask, emb * L),
            _addr(d_w, n_w * emb * L) if n_w else None, n_w, jindo_rank, _addr(d_quo, rank * L),
            _addr(d_rem_lo, (rank - 1) * L), _addr(d_rem_hi, jindo_rank * L),
            _addr(d_scratch, self.scratch_bytes() // 8), _stream(stream)))


def _stack_ntt(ps):
    if ps is None or len(ps) == 0:
        return None, 0
    if isinstance(ps, np.ndarray):
        return np.ascontiguousarray(ps, np.uint64), ps.shape[0]
    for p in ps:
        if not p.IsNTT:
            raise RingoPanic("input not in NTT domain")
    return np.ascontiguousarray(np.stack([p.Coeffs for p in ps]), np.uint64), len(ps)


def LinCheck(field, rank, embRank, jindoRank, batchConst, linCheckConst, linCheckMask, checkers, constraints, wEcdNTT):
    """Prover.linCheck (prover.go:406-459) -> (quo [rank][L], remLo [rank-1][L], remHi [jindoRank][L])."""
    L = field.L
    plan = constraints if isinstance(constraints, LinCheckPlan) else LinCheckPlan(field, rank, embRank, checkers,
                                                                                  constraints)
    w, n_w = _stack_ntt(wEcdNTT)
    if n_w < plan.n_w or jindoRank < rank - 1:
        raise RingoPanic("index out of range")
    quo = np.zeros((rank, L), np.uint64)
    lo = np.zeros((max(rank - 1, 1), L), np.uint64)
    hi = np.zeros((max(jindoRank, 1), L), np.uint64)
    _status(lib().rg_buckler_lin_check(plan.h, ptr(_elem(field, batchConst)), ptr(_elem(field, linCheckConst)),
                                       ptr(_coeffs(linCheckMask)), ptr(w), n_w, jindoRank, ptr(quo), ptr(lo),
                                       ptr(hi)))
    return quo, lo[:rank - 1], hi[:jindoRank]


def SumCheck(field, rank, embRank, jindoRank, sumCheckMaxRank, batchConst, sumCheckMask, constraints, wEcdNTT,
             pwEcdNTT):
    """Prover.sumCheck (prover.go:461-485) -> (quo [sumCheckMaxRank - rank][L], remLo, remHi)."""
    ev = EvalCircuit(field, batchConst, constraints, wEcdNTT, pwEcdNTT)
    if ev.Rank() != embRank:
        raise RingoPanic("inconsistent input(s)")
    return _finish(field, NewCyclicTransformer(field, embRank), rank, ev, batchConst, sumCheckMask,
                   sumCheckMaxRank - rank, jindoRank, True)


def ArithCheck(field, rank, embRank, arithCheckMaxRank, batchConst, constraints, wEcdNTT, pwEcdNTT):
    """Prover.arithCheck (prover.go:399-404) -> (quo [arithCheckMaxRank - rank][L], None, None): the
    reference discards the remainder."""
    ev = EvalCircuit(field, batchConst, constraints, wEcdNTT, pwEcdNTT)
    if ev.Rank() != embRank:
        raise RingoPanic("inconsistent input(s)")
    return _finish(field, NewCyclicTransformer(field, embRank), rank, ev, None, None, arithCheckMaxRank - rank, 0,
                   False)


# ---- the verifier's checks (buckler/verifier.go:178-315) -------------------------------------------
# verdict bits of rg_buckler_verify_checks* (include/ringo.h RG_BK_VERIFY_*)
VERIFY_ARITH, VERIFY_LIN_REM, VERIFY_LIN, VERIFY_SUM_REM, VERIFY_SUM = 1, 2, 4, 8, 16


class VerifyPlan:
    """What Verifier.Verify's checks take from the compiled context (rg_bverifier): the encoder's
    plan at `rank`, jindoRank, wCnt, the number of public witnesses, and the linear check (a
    LinCheckPlan), the arithmetic and the sum-check constraints (Circuit objects or constraint
    lists), each optional.  `n_evals` is the length of pf.Evals in the reference's order: wCnt
    witnesses, lin mask, sum mask, arith quo, lin quo / remLo / remHi, sum quo / remLo / remHi."""

    def __init__(self, field, rank, jindoRank, wCnt, nPw, lin=None, arith=None, sum=None, enc=None):
        self.field, self.rank, self.jindoRank, self.wCnt, self.nPw = field, rank, jindoRank, wCnt, nPw
        self.enc = enc if enc is not None else (lin.enc if lin is not None else NewCyclicTransformer(field, rank))
        as_circ = lambda c: c if c is None or isinstance(c, Circuit) else Circuit(field, c)  # noqa: E731
        self.lin, self.arith, self.sum = lin, as_circ(arith), as_circ(sum)  # kept alive: the handle borrows them
        h = vp()
        _status(lib().rg_buckler_verifier_create(self.enc.h, jindoRank, wCnt, nPw, lin.h if lin is not None else None,
                                                 self.arith.h if self.arith is not None else None,
                                                 self.sum.h if self.sum is not None else None, ctypes.byref(h)))
        self.h = h
        self._L = lib()
        self.n_evals = lib().rg_buckler_verifier_n_evals(h)

    def __del__(self):
        if getattr(self, "h", None) and getattr(self, "_L", None):
            self._L.rg_buckler_verifier_destroy(self.h)
            self.h = None

    def scratch_bytes(self):
        return lib().rg_buckler_verify_checks_scratch_bytes(self.h)

    def checks_dev(self, d_evals, d_pw, d_chal, d_mask_sums, d_verdict, d_sides=None, d_pw_evals=None, d_scratch=None,
                   stream=None):
        """rg_buckler_verify_checks_dev: d_evals [n_evals][L], d_pw [nPw][rank][L] (None iff nPw = 0),
        d_chal [5][L] (evalPoint, arithBatchConst, linCheckBatchConst, linCheckConst,
        sumCheckBatchConst), d_mask_sums [2][L], d_verdict one word; optional d_sides [8][L] and
        d_pw_evals [nPw][L].  Asynchronous on `stream`."""
        L = self.field.L
        opt = lambda t, n: _addr(t, n) if t is not None else None  # noqa: E731
        _status(lib().rg_buckler_verify_checks_dev(
            self.h, _addr(d_evals, self.n_evals * L), opt(d_pw, self.nPw * self.rank * L), _addr(d_chal, 5 * L),
            opt(d_mask_sums, 2 * L), _addr(d_verdict, 1), opt(d_sides, 8 * L), opt(d_pw_evals, self.nPw * L),
            opt(d_scratch, self.scratch_bytes() // 8), _stream(stream)))

    def checks(self, evals, pw, chal, maskSums):
        """rg_buckler_verify_checks (host arrays, synchronous) -> (verdict, sides [8][L], pwEvals [nPw][L])."""
        L = self.field.L
        arr = lambda a, n: None if a is None else np.ascontiguousarray(np.asarray(a, np.uint64).reshape(n, L))  # noqa: E731
        ev, ch, ms = arr(evals, self.n_evals), arr(chal, 5), arr(maskSums, 2)
        pwa = None if self.nPw == 0 else np.ascontiguousarray(np.asarray(pw, np.uint64).reshape(self.nPw, self.rank, L))
        verdict = np.full(1, 2 ** 64 - 1, np.uint64)
        sides = np.full((8, L), 2 ** 64 - 1, np.uint64)
        pwe = np.full((max(self.nPw, 1), L), 2 ** 64 - 1, np.uint64)
        _status(lib().rg_buckler_verify_checks(self.h, ptr(ev), ptr(pwa), ptr(ch), ptr(ms), ptr(verdict), ptr(sides),
                                               ptr(pwe)))
        return int(verdict[0]), sides, pwe[:self.nPw]

    def scratch_bytes_multi(self, n_proofs):
        return lib().rg_buckler_verify_checks_multi_scratch_bytes(self.h, n_proofs)

    def checks_multi_dev(self, n_proofs, d_evals, d_pw, d_xof, d_chal, d_mask_sums, d_verdict, d_sides=None,
                         d_pw_evals=None, d_scratch=None, stream=None):
        """rg_buckler_verify_checks_multi_dev: checks_dev for n_proofs proofs of this plan in one call,
        every buffer proof-major ([n_proofs] in front of checks_dev's shapes); d_xof [n_proofs][rank * 32]
        uint8, each proof's projection matrix (None iff the linear check has no projection checker);
        d_verdict n_proofs words.  Asynchronous on `stream`."""
        L, n = self.field.L, n_proofs
        opt = lambda t, w: _addr(t, w) if t is not None else None  # noqa: E731
        _status(lib().rg_buckler_verify_checks_multi_dev(
            self.h, n, _addr(d_evals, n * self.n_evals * L), opt(d_pw, n * self.nPw * self.rank * L),
            _xof_addr(d_xof, n * self.rank * 32), _addr(d_chal, n * 5 * L), opt(d_mask_sums, n * 2 * L),
            _addr(d_verdict, n), opt(d_sides, n * 8 * L), opt(d_pw_evals, n * self.nPw * L),
            opt(d_scratch, self.scratch_bytes_multi(n) // 8), _stream(stream)))

    def checks_multi(self, evals, pw, xof, chal, maskSums):
        """rg_buckler_verify_checks_multi (host arrays, synchronous): evals [n][n_evals][L], pw
        [n][nPw][rank][L] (None iff nPw = 0), xof n * rank * 32 bytes or None, chal [n][5][L], maskSums
        [n][2][L] -> (verdicts [n], sides [n][8][L], pwEvals [n][nPw][L])."""
        L = self.field.L
        ev = np.ascontiguousarray(np.asarray(evals, np.uint64).reshape(-1, self.n_evals, L))
        n = ev.shape[0]
        arr = lambda a, k: None if a is None else np.ascontiguousarray(np.asarray(a, np.uint64).reshape(n, k, L))  # noqa: E731
        ch, ms = arr(chal, 5), arr(maskSums, 2)
        pwa = None if self.nPw == 0 else np.ascontiguousarray(
            np.asarray(pw, np.uint64).reshape(n, self.nPw, self.rank, L))
        if xof is not None:
            xof = bytes(xof)
            if len(xof) < n * self.rank * 32:
                raise RingoPanic("index out of range")
        verdict = np.full(max(n, 1), 2 ** 64 - 1, np.uint64)
        sides = np.full((max(n, 1), 8, L), 2 ** 64 - 1, np.uint64)
        pwe = np.full((max(n, 1), max(self.nPw, 1), L), 2 ** 64 - 1, np.uint64)
        _status(lib().rg_buckler_verify_checks_multi(self.h, n, ptr(ev), ptr(pwa), xof, ptr(ch), ptr(ms), ptr(verdict),
                                                     ptr(sides), ptr(pwe)))
        return [int(x) for x in verdict[:n]], sides[:n], pwe[:n, :self.nPw]


def VerifyChecks(field, rank, jindoRank, wCnt, challenges, maskSums, evals, pw, checkers, linConstraints,
                 arithConstraints, sumConstraints):
    """Verifier.Verify after the transcript and polyVerifier.Verify (verifier.go:178-216): returns
    (verdict, sides, pwEvals); verdict 0 <=> arithCheck, linCheck and sumCheck all return true.
    challenges [5][L] = evalPoint, arithBatchConst, linCheckBatchConst, linCheckConst,
    sumCheckBatchConst; maskSums [2][L] = LinCheckMaskSum, SumCheckMaskSum; evals = pf.Evals; pw =
    the public-witness vectors [nPw][rank][L] (None without any).  A check whose constraints are
    None is absent (HasLinearCheck / HasArithmeticCheck / HasSumCheck false)."""
    lin = None
    if linConstraints is not None:  # the embedding rank plays no part in the verifier's checks
        lin = linConstraints if isinstance(linConstraints, LinCheckPlan) else LinCheckPlan(field, rank, rank, checkers,
                                                                                           linConstraints)
    nPw = 0 if pw is None else len(pw)
    plan = VerifyPlan(field, rank, jindoRank, wCnt, nPw, lin, arithConstraints, sumConstraints)
    if np.asarray(evals).reshape(-1, field.L).shape[0] < plan.n_evals:
        raise RingoPanic("index out of range")  # pf.Evals[roundComIdx]
    return plan.checks(np.asarray(evals, np.uint64).reshape(-1, field.L)[:plan.n_evals], pw, challenges, maskSums)


# ---- the prover's checks for a batch of proofs (buckler/prover.go:399-485) --------------------------
class ProvePlan:
    """What Prover.arithCheck / linCheck / sumCheck take from the compiled context (rg_bprover): the
    encoder's plan at `rank`, the evaluator's at `embRank`, jindoRank, the numbers of witnesses and
    public witnesses, and the linear check (a LinCheckPlan), the arithmetic and the sum-check
    constraints (Circuit objects or constraint lists) with ctx.arithCheckMaxRank / sumCheckMaxRank,
    each check optional."""

    def __init__(self, field, rank, embRank, jindoRank, nW, nPw, lin=None, arith=None, arithMaxRank=0, sum=None,
                 sumMaxRank=0, enc=None, emb=None):
        self.field, self.rank, self.embRank, self.jindoRank, self.nW, self.nPw = field, rank, embRank, jindoRank, nW, nPw
        self.enc = enc if enc is not None else (lin.enc if lin is not None else NewCyclicTransformer(field, rank))
        self.emb = emb if emb is not None else (lin.emb if lin is not None else NewCyclicTransformer(field, embRank))
        as_circ = lambda c: c if c is None or isinstance(c, Circuit) else Circuit(field, c)  # noqa: E731
        self.lin, self.arith, self.sum = lin, as_circ(arith), as_circ(sum)  # kept alive: the handle borrows them
        self.hasProj = lin is not None and any(isinstance(c, ProjChecker) for c in lin.checkers)
        # elements per proof of the eight outputs, in the order of the C call (None: the check is absent)
        self.nQuo = (arithMaxRank - rank if self.arith is not None else None, rank if lin is not None else None,
                     sumMaxRank - rank if self.sum is not None else None)
        h = vp()
        _status(lib().rg_buckler_prover_create(
            self.enc.h, self.emb.h, jindoRank, nW, nPw, lin.h if lin is not None else None,
            self.arith.h if self.arith is not None else None, arithMaxRank,
            self.sum.h if self.sum is not None else None, sumMaxRank, ctypes.byref(h)))
        self.h = h
        self._L = lib()

    def __del__(self):
        if getattr(self, "h", None) and getattr(self, "_L", None):
            self._L.rg_buckler_prover_destroy(self.h)
            self.h = None

    def scratch_bytes(self, n_proofs):
        return lib().rg_buckler_prove_checks_scratch_bytes(self.h, n_proofs)

    def out_elems(self):
        """Elements per proof of (arithQuo, linQuo, linRemLo, linRemHi, sumQuo, sumRemLo, sumRemHi, rem0);
        None for the outputs of an absent check."""
        a, l, s = self.nQuo
        lo, hi = self.rank - 1, self.jindoRank
        return (a, l, None if l is None else lo, None if l is None else hi, s, None if s is None else lo,
                None if s is None else hi, 2)

    def checks_dev(self, n_proofs, d_w, d_pw, d_xof, d_chal, d_lin_mask, d_sum_mask, d_arith_quo, d_lin_quo,
                   d_lin_rem_lo, d_lin_rem_hi, d_sum_quo, d_sum_rem_lo, d_sum_rem_hi, d_rem0=None, d_scratch=None,
                   stream=None):
        """rg_buckler_prove_checks_dev: every buffer proof-major.  d_w [n][nW][embRank][L], d_pw
        [n][nPw][embRank][L] (None iff nPw = 0), d_xof [n][rank * 32] uint8 (None iff the linear check has
        no projection checker), d_chal [n][4][L] (arithBatchConst, linCheckBatchConst, linCheckConst,
        sumCheckBatchConst), the masks [n][embRank][L]; outputs quo [n][n_quo][L], remLo [n][rank-1][L],
        remHi [n][jindoRank][L], optional d_rem0 [n][2][L].  The buffers of an absent check are None.
        Asynchronous on `stream`."""
        L, n, emb = self.field.L, n_proofs, self.embRank
        opt = lambda t, w: _addr(t, w) if t is not None else None  # noqa: E731
        outs = (d_arith_quo, d_lin_quo, d_lin_rem_lo, d_lin_rem_hi, d_sum_quo, d_sum_rem_lo, d_sum_rem_hi, d_rem0)
        _status(lib().rg_buckler_prove_checks_dev(
            self.h, n, opt(d_w, n * self.nW * emb * L), opt(d_pw, n * self.nPw * emb * L),
            _xof_addr(d_xof, n * self.rank * 32), _addr(d_chal, n * 4 * L), opt(d_lin_mask, n * emb * L),
            opt(d_sum_mask, n * emb * L), *[opt(t, n * (k or 0) * L) for t, k in zip(outs, self.out_elems())],
            opt(d_scratch, self.scratch_bytes(n) // 8), _stream(stream)))

    def checks(self, w, pw, xof, chal, linMask, sumMask):
        """rg_buckler_prove_checks (host arrays, synchronous): w [n][nW][embRank][L], pw
        [n][nPw][embRank][L] (None iff nPw = 0), xof n * rank * 32 bytes or None, chal [n][4][L], the masks
        [n][embRank][L] (None for an absent check) -> (arithQuo, linQuo, linRemLo, linRemHi, sumQuo,
        sumRemLo, sumRemHi, rem0), each [n][.][L], None for an absent check."""
        L, emb = self.field.L, self.embRank
        ch = np.ascontiguousarray(np.asarray(chal, np.uint64).reshape(-1, 4, L))
        n = ch.shape[0]
        arr = lambda a, *s: None if a is None else np.ascontiguousarray(np.asarray(a, np.uint64).reshape(n, *s, L))  # noqa: E731
        wa = None if self.nW == 0 else arr(w, self.nW, emb)
        pwa = None if self.nPw == 0 else arr(pw, self.nPw, emb)
        if xof is not None:
            xof = bytes(xof)
            if len(xof) < n * self.rank * 32:
                raise RingoPanic("index out of range")
        outs = [None if k is None else np.full((max(n, 1), max(k, 1), L), 2 ** 64 - 1, np.uint64)
                for k in self.out_elems()]
        _status(lib().rg_buckler_prove_checks(self.h, n, ptr(wa), ptr(pwa), xof, ptr(ch), ptr(arr(linMask, emb)),
                                              ptr(arr(sumMask, emb)), *[ptr(o) for o in outs]))
        return tuple(None if o is None else o[:n, :k] for o, k in zip(outs, self.out_elems()))


def ProveChecks(field, rank, embRank, jindoRank, challenges, linCheckMasks, sumCheckMasks, checkers, linConstraints,
                arithConstraints, arithCheckMaxRank, sumConstraints, sumCheckMaxRank, wEcdNTT, pwEcdNTT, xof=None):
    """Prover.arithCheck, linCheck and sumCheck (prover.go:399-485) of a batch of proofs of one
    circuit.  challenges [n][4][L] = arithBatchConst, linCheckBatchConst, linCheckConst,
    sumCheckBatchConst per proof; linCheckMasks / sumCheckMasks [n][embRank][L]; wEcdNTT
    [n][nW][embRank][L] and pwEcdNTT [n][nPw][embRank][L] (None without any); xof = the n proofs'
    projection bytes, rank * 32 each (None without a projection checker).  A check whose constraints
    are None is absent.  Returns one tuple per proof: (arithQuo, (linQuo, linRemLo, linRemHi),
    (sumQuo, sumRemLo, sumRemHi), (linRem0, sumRem0)), None in place of an absent check."""
    lin = None
    if linConstraints is not None:
        lin = linConstraints if isinstance(linConstraints, LinCheckPlan) else LinCheckPlan(field, rank, embRank,
                                                                                           checkers, linConstraints)
    w = None if wEcdNTT is None else np.asarray(wEcdNTT, np.uint64)
    pw = None if pwEcdNTT is None else np.asarray(pwEcdNTT, np.uint64)
    nW = 0 if w is None else w.shape[1]
    nPw = 0 if pw is None else pw.shape[1]
    plan = ProvePlan(field, rank, embRank, jindoRank, nW, nPw, lin, arithConstraints, arithCheckMaxRank,
                     sumConstraints, sumCheckMaxRank)
    aq, lq, llo, lhi, sq, slo, shi, rem0 = plan.checks(w, pw, xof, challenges, linCheckMasks if lin is not None else None,
                                                       sumCheckMasks if plan.sum is not None else None)
    return [(None if aq is None else aq[i], None if lq is None else (lq[i], llo[i], lhi[i]),
             None if sq is None else (sq[i], slo[i], shi[i]), (rem0[i, 0], rem0[i, 1])) for i in range(rem0.shape[0])]


# ---- the projection round and the masks for a batch of proofs (buckler/prover.go:165-240) ------------
class ProjRoundPlan:
    """What the projection round (prover.go:165-193) takes from the compiled context (rg_bproj): the
    witness rank, the number of witnesses nW of the table, and the approximate infinity-norm
    constraints as (src, proj, dcmp, decomposer) tuples: three witness IDs and the Decomposer of
    decomposeBase(rank * bound), or the bound itself (an int)."""

    def __init__(self, field, rank, nW, constraints):
        self.field, self.rank, self.nW = field, rank, nW
        self.constraints = [(int(s), int(p), int(d), dc if isinstance(dc, Decomposer) else Decomposer(field, rank * dc))
                            for s, p, d, dc in constraints]  # the decomposers kept alive: the handle borrows them
        flat = [i for c in self.constraints for i in c[:3]]
        cons = (ctypes.c_uint64 * max(1, len(flat)))(*flat)
        hs = (vp * max(1, len(self.constraints)))(*[c[3].h.value for c in self.constraints])
        h = vp()
        _status(lib().rg_buckler_proj_round_create(field.h, rank, nW, len(self.constraints), cons, hs, ctypes.byref(h)))
        self.h = h
        self._L = lib()

    def __del__(self):
        if getattr(self, "h", None) and getattr(self, "_L", None):
            self._L.rg_buckler_proj_round_destroy(self.h)
            self.h = None

    def scratch_bytes(self, n_proofs):
        return lib().rg_buckler_prove_proj_round_scratch_bytes(self.h, n_proofs)

    def round_dev(self, n_proofs, d_w, d_xof, d_scratch=None, stream=None):
        """rg_buckler_prove_proj_round_dev: d_w [n][nW][rank][L], the plain witness table, whose proj and
        dcmp rows are written in place; d_xof [n][rank * 32] uint8.  Asynchronous on `stream`."""
        n = n_proofs
        _status(lib().rg_buckler_prove_proj_round_dev(
            self.h, n, _addr(d_w, n * self.nW * self.rank * self.field.L), _xof_addr(d_xof, n * self.rank * 32),
            _addr(d_scratch, self.scratch_bytes(n) // 8) if d_scratch is not None else None, _stream(stream)))

    def round(self, w, xof):
        """rg_buckler_prove_proj_round (host arrays, synchronous): w [n][nW][rank][L], xof n * rank * 32
        bytes -> the table with the proj and dcmp rows of every proof filled in (a copy)."""
        w = np.array(np.asarray(w, np.uint64).reshape(-1, self.nW, self.rank, self.field.L), order="C")
        n = w.shape[0]
        xof = bytes(xof)
        if len(xof) < n * self.rank * 32:
            raise RingoPanic("index out of range")
        _status(lib().rg_buckler_prove_proj_round(self.h, n, ptr(w), xof))
        return w


def SumCheckMaskBatch(field, rank, maskRank, embRank, rand):
    """Prover.sumCheckMask(maskRank) (prover.go:381-397) of a batch of proofs; rand [n][maskRank][L] =
    each proof's MustSetRandom draws in the reference's order.  Returns (mask [n][embRank][L], maskCom
    [n][maskRank][L] = mask.Coeffs[:maskRank], maskSum [n][L])."""
    L = field.L
    if maskRank > embRank:
        raise RingoPanic("index out of range")
    r = np.ascontiguousarray(np.asarray(rand, np.uint64).reshape(-1, maskRank, L))
    n = r.shape[0]
    mask = np.zeros((max(n, 1), embRank, L), np.uint64)
    com = np.zeros((max(n, 1), maskRank, L), np.uint64)
    msum = np.zeros((max(n, 1), L), np.uint64)
    _status(lib().rg_buckler_sumcheck_mask_batch(field.h, rank, maskRank, embRank, n, ptr(r), ptr(mask), ptr(com),
                                                 ptr(msum)))
    return mask[:n], com[:n], msum[:n]


def sumcheck_mask_batch_dev(field, rank, maskRank, embRank, n_proofs, d_rand, d_mask, d_mask_sum, d_mask_com=None,
                            stream=None):
    """rg_buckler_sumcheck_mask_batch_dev: d_rand [n][maskRank][L] -> d_mask [n][embRank][L], d_mask_sum
    [n][L] and, when given, d_mask_com [n][maskRank][L]."""
    L, n = field.L, n_proofs
    _status(lib().rg_buckler_sumcheck_mask_batch_dev(
        field.h, rank, maskRank, embRank, n, _addr(d_rand, n * maskRank * L), _addr(d_mask, n * embRank * L),
        _addr(d_mask_com, n * maskRank * L) if d_mask_com is not None else None, _addr(d_mask_sum, n * L),
        _stream(stream)))


# ---- the prover's MustSetRandom draws on the device (element.go:299-343) ---------------------------
class FieldSampler:
    """rg_fsampler: NewUniformSamplerWithSeed(seed) in place of crypto/rand on any built field.  Element i
    of a call is Uint.SetRandom reading from instance first + i of that sampler; the limbs are the
    accepted candidate's words as they stand (no domain conversion, as in the reference).  A prover
    gives each consumer of draws its own seed or a disjoint range of instances."""

    def __init__(self, field, seed):
        self.field = field
        seed = bytes(seed)
        h = vp()
        _status(lib().rg_field_sampler_create(field.h, seed, len(seed), ctypes.byref(h)))
        self.h = h
        self._L = lib()

    def __del__(self):
        if getattr(self, "h", None) and getattr(self, "_L", None):
            self._L.rg_field_sampler_destroy(self.h)
            self.h = None

    def scratch_bytes(self):
        return lib().rg_field_sampler_scratch_bytes(self.h)

    def elems_dev(self, first, n, d_out, d_scratch, stream=None):
        """rg_field_sampler_elems_dev: d_out [n][L] <- the elements of instances first .. first + n - 1;
        d_scratch: scratch_bytes() bytes.  Asynchronous on `stream`."""
        _status(lib().rg_field_sampler_elems_dev(self.h, first, n, _addr(d_out, n * self.field.L),
                                                 _addr(d_scratch, self.scratch_bytes() // 8), _stream(stream)))

    def elems(self, first, n):
        """rg_field_sampler_elems (synchronous) -> [n][L] uint64."""
        out = np.zeros((max(n, 1), self.field.L), np.uint64)
        _status(lib().rg_field_sampler_elems(self.h, first, n, ptr(out)))
        return out[:n]


def SumCheckMaskBatchSampled(sampler, rank, maskRank, embRank, n_proofs, first):
    """Prover.sumCheckMask(maskRank) (prover.go:381-397) of n_proofs proofs whose draw k of proof p is
    the element of instance first + p * maskRank + k of `sampler`.  Returns (mask [n][embRank][L],
    maskCom [n][maskRank][L] = mask.Coeffs[:maskRank], maskSum [n][L])."""
    L, n = sampler.field.L, n_proofs
    if maskRank > embRank:
        raise RingoPanic("index out of range")
    mask = np.zeros((max(n, 1), embRank, L), np.uint64)
    com = np.zeros((max(n, 1), maskRank, L), np.uint64)
    msum = np.zeros((max(n, 1), L), np.uint64)
    _status(lib().rg_buckler_sumcheck_mask_batch_sampled(sampler.h, rank, maskRank, embRank, n, first, ptr(mask),
                                                         ptr(com), ptr(msum)))
    return mask[:n], com[:n], msum[:n]


def sumcheck_mask_batch_sampled_dev(sampler, rank, maskRank, embRank, n_proofs, first, d_mask, d_mask_sum, d_scratch,
                                    d_mask_com=None, stream=None):
    """rg_buckler_sumcheck_mask_batch_sampled_dev: the draws of instances first .. first + n * maskRank - 1
    -> d_mask [n][embRank][L], d_mask_sum [n][L] and, when given, d_mask_com [n][maskRank][L]; d_scratch:
    sampler.scratch_bytes() bytes."""
    L, n = sampler.field.L, n_proofs
    _status(lib().rg_buckler_sumcheck_mask_batch_sampled_dev(
        sampler.h, rank, maskRank, embRank, n, first, _addr(d_mask, n * embRank * L),
        _addr(d_mask_com, n * maskRank * L) if d_mask_com is not None else None, _addr(d_mask_sum, n * L),
        _addr(d_scratch, sampler.scratch_bytes() // 8), _stream(stream)))


# ---- norm decomposition (buckler/utils.go:34-56, buckler/prover.go:77-111, 182-192) ---------------
def decomposeBig(x, base, q):
    """decomposeBig (utils.go:34-56) on Python ints: x in [0, q) -> len(base) digits in {-1, 0, 1}."""
    xSigned = int(x)
    if xSigned > (q >> 1):
        xSigned -= q
    dcmpOut = [0] * len(base)
    for i, b in enumerate(base):
        if xSigned >= b:
            dcmpOut[i] = 1
            xSigned -= b
        elif xSigned <= -b:
            dcmpOut[i] = -1
            xSigned += b
    return dcmpOut


class Decomposer:
    """decomposeBig over an rg_dcmp handle: `bound_or_base` is a bound (an int: the base is
    decomposeBase(bound)) or the base itself (a sequence of positive ints).  Witnesses are [rank][L]
    arrays of Montgomery elements; the digits come back as field elements (SetInt64)."""

    def __init__(self, field, bound_or_base):
        self.field = field
        self.dcmpBase = decomposeBase(bound_or_base) if isinstance(bound_or_base, int) else [int(b) for b in
                                                                                             bound_or_base]
        if not self.dcmpBase or min(self.dcmpBase) < 1:
            raise RingoPanic("inconsistent input(s)")
        # |x| <= q / 2 < 2^(64L) - 1, so a base element of 2^(64L) or more is never reached: it is
        # stored saturated to 2^(64L) - 1, which is never reached either; the digits are unchanged
        top = (1 << (64 * field.L)) - 1
        base = np.ascontiguousarray(field.to_limbs([min(b, top) for b in self.dcmpBase]))
        h = vp()
        _status(lib().rg_buckler_dcmp_create(field.h, ptr(base), len(self.dcmpBase), ctypes.byref(h)))
        self.h = h
        self._L = lib()

    def __del__(self):
        if getattr(self, "h", None) and getattr(self, "_L", None):
            self._L.rg_buckler_dcmp_destroy(self.h)
            self.h = None

    def _vec(self, w, ndim):
        w = np.ascontiguousarray(np.asarray(w, np.uint64))
        if w.ndim != ndim or w.shape[-1] != self.field.L:
            raise RingoPanic("inconsistent input(s)")
        return w

    def DecomposeInf(self, w):
        """prover.go:77-86: w [rank][L] -> [nb][rank][L], digit witness j at index j (or
        [batch][rank][L] -> [batch][nb][rank][L])."""
        w = np.asarray(w, np.uint64)
        single = w.ndim == 2
        w = self._vec(w[None] if single else w, 3)
        batch, rank, L = w.shape
        out = np.zeros((batch, len(self.dcmpBase), rank, L), np.uint64)
        _status(lib().rg_buckler_dcmp_inf(self.h, ptr(w), batch, rank, ptr(out)))
        return out[0] if single else out

    def DecomposeProj(self, w):
        """prover.go:182-192: w [rank][L] (the projected witness) -> [rank][L] with digit j of w[i],
        i < 128, at i nb + j and zeros from 128 nb."""
        w = self._vec(w, 2)
        rank = w.shape[0]
        if rank < 128 or 128 * len(self.dcmpBase) > rank:
            raise RingoPanic("index out of range")
        out = np.zeros((rank, self.field.L), np.uint64)
        _status(lib().rg_buckler_dcmp_proj(self.h, ptr(w), rank, ptr(out)))
        return out

    def DecomposeTwoNorm(self, w):
        """prover.go:99-110: w [rank][L] -> (digits [rank][L] with the nb digits of sqNm first and
        zeros after, sqNm [L] in Montgomery form); [batch][rank][L] -> ([batch][rank][L], [batch][L])."""
        w = np.asarray(w, np.uint64)
        single = w.ndim == 2
        w = self._vec(w[None] if single else w, 3)
        batch, rank, L = w.shape
        if len(self.dcmpBase) > rank:
            raise RingoPanic("index out of range")
        out = np.zeros((batch, rank, L), np.uint64)
        sq = np.zeros((batch, L), np.uint64)
        _status(lib().rg_buckler_dcmp_two(self.h, ptr(w), batch, rank, ptr(out), ptr(sq)))
        return (out[0], sq[0]) if single else (out, sq)

    def scratch_bytes(self, batch, rank):
        return lib().rg_buckler_dcmp_two_scratch_bytes(self.h, batch, rank)

    def inf_dev(self, d_out, d_w, batch, rank, stream=None):
        """rg_buckler_dcmp_inf_dev: [batch][rank][L] -> [batch][nb][rank][L]."""
        n = batch * rank * self.field.L
        _status(lib().rg_buckler_dcmp_inf_dev(self.h, _addr(d_w, n), batch, rank,
                                              _addr(d_out, n * len(self.dcmpBase)), _stream(stream)))

    def proj_dev(self, d_out, d_w, rank, stream=None):
        """rg_buckler_dcmp_proj_dev: d_w (at least 128 elements) -> d_out [rank][L]."""
        L = self.field.L
        _status(lib().rg_buckler_dcmp_proj_dev(self.h, _addr(d_w, 128 * L), rank, _addr(d_out, rank * L),
                                               _stream(stream)))

    def two_dev(self, d_out, d_w, batch, rank, d_sq=None, d_scratch=None, stream=None):
        """rg_buckler_dcmp_two_dev: [batch][rank][L] -> d_out [batch][rank][L], d_sq [batch][L]."""
        L = self.field.L
        n = batch * rank * L
        _status(lib().rg_buckler_dcmp_two_dev(
            self.h, _addr(d_w, n), batch, rank, _addr(d_out, n), _addr(d_sq, batch * L) if d_sq is not None else None,
            _addr(d_scratch, self.scratch_bytes(batch, rank) // 8) if d_scratch is not None else None,
            _stream(stream)))


# ---- the witness rounds for a batch of proofs (buckler/prover.go:77-111, 136-153, 195-201) ------------
def _u64s(xs):
    return (ctypes.c_uint64 * max(1, len(xs)))(*xs)


class DcmpRoundPlan:
    """What the norm decompositions (prover.go:77-111) take from the compiled context (rg_bdcmp): the
    witness rank, the number of witnesses nW of the table, the infinity-norm constraints as (src, bound,
    [digit rows]) and the two-norm constraints as (src, bound, dst).  A bound is an int (the base is
    decomposeBase(bound)) or a Decomposer; an infinity-norm constraint has one digit row per base element."""

    def __init__(self, field, rank, nW, inf=(), two=()):
        self.field, self.rank, self.nW = field, rank, nW

        def dcmp(b):  # the decomposers kept alive: the handle borrows them
            return b if isinstance(b, Decomposer) else Decomposer(field, b)

        self.inf = [(int(s), dcmp(b), [int(r) for r in rows]) for s, b, rows in inf]
        self.two = [(int(s), dcmp(b), int(d)) for s, b, d in two]
        for _, dc, rows in self.inf:
            if len(rows) != len(dc.dcmpBase):
                raise RingoPanic("inconsistent input(s)")  # one digit row per base element
        h = vp()
        _status(lib().rg_buckler_dcmp_round_create(
            field.h, rank, nW, len(self.inf), _u64s([s for s, _, _ in self.inf]),
            (vp * max(1, len(self.inf)))(*[dc.h.value for _, dc, _ in self.inf]),
            _u64s([r for _, _, rows in self.inf for r in rows]), len(self.two),
            _u64s([i for s, _, d in self.two for i in (s, d)]),
            (vp * max(1, len(self.two)))(*[dc.h.value for _, dc, _ in self.two]), ctypes.byref(h)))
        self.h = h
        self._L = lib()

    def __del__(self):
        if getattr(self, "h", None) and getattr(self, "_L", None):
            self._L.rg_buckler_dcmp_round_destroy(self.h)
            self.h = None

    def scratch_bytes(self, n_proofs):
        return lib().rg_buckler_prove_dcmp_round_scratch_bytes(self.h, n_proofs)

    def round_dev(self, n_proofs, d_w, d_sq=None, d_scratch=None, stream=None):
        """rg_buckler_prove_dcmp_round_dev: d_w [n][nW][rank][L], the plain witness table, whose digit and
        dst rows are written in place; d_sq (optional) [n][n_two][L].  Asynchronous on `stream`."""
        n, L = n_proofs, self.field.L
        _status(lib().rg_buckler_prove_dcmp_round_dev(
            self.h, n, _addr(d_w, n * self.nW * self.rank * L),
            _addr(d_sq, n * len(self.two) * L) if d_sq is not None else None,
            _addr(d_scratch, self.scratch_bytes(n) // 8) if d_scratch is not None else None, _stream(stream)))

    def round(self, w):
        """rg_buckler_prove_dcmp_round (host arrays, synchronous): w [n][nW][rank][L] -> (the table with
        the digit and dst rows of every proof filled in (a copy), sqNm [n][n_two][L] in Montgomery form,
        or None without a two-norm constraint)."""
        w = np.array(np.asarray(w, np.uint64).reshape(-1, self.nW, self.rank, self.field.L), order="C")
        n = w.shape[0]
        sq = np.zeros((max(n, 1), len(self.two), self.field.L), np.uint64) if self.two else None
        _status(lib().rg_buckler_prove_dcmp_round(self.h, n, ptr(w), ptr(sq)))
        return w, (None if sq is None else sq[:n])


class EncodeRoundPlan:
    """What the encodings of one commit round (prover.go:136-153, 195-201) take from the compiled context
    (rg_bencode): the witness rank, the embedding rank, the number of witnesses nW of the table and `sel`,
    the rows of this round (the first-round rows, or ctx.wSecond)."""

    def __init__(self, field, rank, embRank, nW, sel):
        self.field, self.rank, self.embRank, self.nW = field, rank, embRank, nW
        self.sel = [int(s) for s in sel]
        self.ntt = NewCyclicTransformer(field, rank)  # kept alive: the handle borrows it
        h = vp()
        _status(lib().rg_buckler_encode_round_create(self.ntt.h, embRank, nW, len(self.sel), _u64s(self.sel),
                                                     ctypes.byref(h)))
        self.h = h
        self._L = lib()

    def __del__(self):
        if getattr(self, "h", None) and getattr(self, "_L", None):
            self._L.rg_buckler_encode_round_destroy(self.h)
            self.h = None

    def scratch_bytes(self, n_proofs):
        return lib().rg_buckler_prove_encode_round_scratch_bytes(self.h, n_proofs)

    def round_dev(self, n_proofs, d_w, d_wecd, d_rand=None, d_com=None, d_scratch=None, stream=None):
        """rg_buckler_prove_encode_round_dev: d_w [n][nW][rank][L] -> rows `sel` of d_wecd [n][nW][embRank][L]
        and, when given, d_com [n][n_sel][rank + 1][L]; d_rand [n][n_sel][L] or None (EncodeTo).
        Asynchronous on `stream`."""
        n, L, ns = n_proofs, self.field.L, len(self.sel)
        _status(lib().rg_buckler_prove_encode_round_dev(
            self.h, n, _addr(d_w, n * self.nW * self.rank * L),
            _addr(d_rand, n * ns * L) if d_rand is not None else None, _addr(d_wecd, n * self.nW * self.embRank * L),
            _addr(d_com, n * ns * (self.rank + 1) * L) if d_com is not None else None,
            _addr(d_scratch, self.scratch_bytes(n) // 8) if d_scratch is not None else None, _stream(stream)))

    def round(self, w, rand=None, wecd=None):
        """rg_buckler_prove_encode_round (host arrays, synchronous): w [n][nW][rank][L], rand [n][n_sel][L]
        or None, wecd [n][nW][embRank][L] (the table so far; zeros when None) -> (wecd with the rows `sel`
        of every proof filled in (a copy), com [n][n_sel][rank + 1][L], or None without rand)."""
        L, ns = self.field.L, len(self.sel)
        w = np.ascontiguousarray(np.asarray(w, np.uint64).reshape(-1, self.nW, self.rank, L))
        n = w.shape[0]
        r = None if rand is None else np.ascontiguousarray(np.asarray(rand, np.uint64).reshape(n, ns, L))
        out = np.zeros((n, self.nW, self.embRank, L), np.uint64) if wecd is None else \
            np.array(np.asarray(wecd, np.uint64).reshape(n, self.nW, self.embRank, L), order="C")
        com = None if r is None else np.zeros((max(n, 1), ns, self.rank + 1, L), np.uint64)
        _status(lib().rg_buckler_prove_encode_round(self.h, n, ptr(w), ptr(r), ptr(out), ptr(com)))
        return out, (None if com is None else com[:n])


def TwoNormPublic(field, rank, bound):
    """The public witnesses of a two-norm bound (prover.go:92-97): (pwBase, pwMask), [rank][L] each,
    with pwBase[i] = SetBigInt(base[i]) and pwMask[i] = SetInt64(1) for i < len(base), zero above."""
    base = decomposeBase(bound)
    if len(base) > rank:
        raise RingoPanic("index out of range")
    pwBase = np.zeros((rank, field.L), np.uint64)
    pwMask = np.zeros((rank, field.L), np.uint64)
    pwBase[:len(base)] = field.mont(base)
    pwMask[:len(base)] = field.mont([1] * len(base))
    return pwBase, pwMask


def proj_xof_dev(chal_bytes, rank, d_xof, n_proofs, sponge=None, stream=None):
    """The projection XOF of n_proofs proofs on the device (prover.go:165-176): SHAKE128 over each proof's 32
    projConst challenge bytes (chal_bytes [n_proofs][32], a device buffer), 32 * rank bytes squeezed per
    proof into d_xof [n_proofs][32 * rank], the layout rg_buckler_prove_proj_round_dev, the verifier and
    prover plans and ProjChecker.set_xof_dev take.  Two asynchronous stream items, nothing copied to the
    host.  sponge: a ringo.xof.Shake128(n_proofs) to reuse (it is reset); returns the one used.
    The sponge is serial per proof (one permutation per 168 bytes), so this pays off for large batches
    only: at rank 2^15 it measured 601 against 2,151 us per proof at 64 proofs, but 4,649 against 1,236 us
    at 8 and 36,841 against 1,306 us at one proof, against a host squeeze plus the upload
    (profiles/xof_transcript_timing.txt)."""
    from . import xof
    h = sponge or xof.Shake128(n_proofs)
    if h.n_states != n_proofs:
        raise RingoPanic("the sponge holds another number of states")
    h.reset(stream)
    h.absorb(chal_bytes, 32, stream=stream)
    h.squeeze(d_xof, 32 * rank, stream=stream)
    return h
