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
