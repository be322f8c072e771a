"""Test reference for the Buckler linear check and sum check: a Python restatement of
buckler/linear.go, buckler/utils.go:7-32 and buckler/prover.go:381-485, loop by loop and in the
reference's order (sumCheckMask's in-place loop included), over Python integers.  The NTTs,
Encoder.EncodeTo, QuoRemByVanishing and AutTo come from the C oracle (coracle.CField).

Field elements are Montgomery-form integers (what a zp.Uint holds, R = 2^(64 L)): a vector is a
list of ints, and `arr` / `ints` convert to and from the [n][L] limb arrays of the C ABI."""
import numpy as np

import coracle as co


class Ref:
    def __init__(self, q, cf=None):
        self.q = q
        self.cf = cf or co.CField(q)
        self.L = self.cf.L
        self.R = 1 << (64 * self.L)
        self.Rinv = pow(self.R, -1, q)
        self._tabs = {}

    # -- elements ---------------------------------------------------------------------------
    def arr(self, xs):
        return co.to_limbs(list(xs), self.L)

    def ints(self, a):
        a = np.asarray(a, np.uint64)
        return co.from_limbs(a.reshape(-1, self.L))

    def mul(self, a, b):  # Montgomery product
        return a * b * self.Rinv % self.q

    def set_uint64(self, v):
        return v * self.R % self.q

    def plain(self, a):  # fromMont
        return a * self.Rinv % self.q

    def tables(self, n, cyclic):
        k = (n, cyclic)
        if k not in self._tabs:
            self._tabs[k] = self.cf.tables(n, cyclic=cyclic)
        return self._tabs[k]

    def fwd(self, xs, cyclic):
        tw, _, _ = self.tables(len(xs), cyclic)
        return self.ints(self.cf.ntt_fwd(self.arr(xs)[None], tw)[0])

    def inv(self, xs, cyclic):
        _, twi, ninv = self.tables(len(xs), cyclic)
        return self.ints(self.cf.ntt_inv(self.arr(xs)[None], twi, ninv)[0])

    def encode(self, v, emb):  # Encoder.EncodeTo (encoder.go:32-38)
        return self.ints(self.cf.buckler_encode(self.arr(v), emb))

    def rand_encode(self, v, emb, r):  # Encoder.RandEncodeTo (encoder.go:50-54)
        return self.ints(self.cf.buckler_encode(self.arr(v), emb, rnd=self.arr([r])[0]))


# ---- utils.go:7-32 ---------------------------------------------------------------------------------
def decomposeBase(x):
    dcmpLen = x.bit_length()
    tz = 0
    while x and not (x >> tz) & 1:
        tz += 1
    if (1 << tz) == x:
        dcmpLen -= 1
    base = [None] * dcmpLen
    for i in range(dcmpLen - 1):
        s = 0
        for j in range(i):
            s += base[j]
        b = x - s
        quo, rem = b >> 1, b & 1
        base[i] = quo + rem
    base[dcmpLen - 1] = 1
    return base


# ---- linear.go -------------------------------------------------------------------------------------
def modInverse(x, m):  # linear.go:75-91 (Python ints in place of wrapping uint64)
    x %= m
    a, b, u, v = x, m, 1, 0
    while b != 0:
        qq = a // b
        a, b = b, a - qq * b
        u, v = v, u - qq * v
    if a != 1:
        raise ValueError("modular inverse does not exist")
    return u % m


class NTTChecker:  # linear.go:20-43
    def __init__(self, ref, rank):
        self.ref, self.rank = ref, rank
        self.scale = ref.set_uint64(rank)

    def transform(self, v):
        return self.ref.fwd(v, cyclic=False)

    def transpose(self, v):
        out = [None] * self.rank
        for i in range(self.rank):
            out[i] = self.ref.mul(v[self.rank - 1 - i], self.scale)
        return self.ref.inv(out, cyclic=False)


class AutChecker:  # linear.go:46-73
    def __init__(self, ref, rank, idx, isNTT):
        self.ref, self.rank, self.idx, self.isNTT = ref, rank, idx, isNTT
        self.idxInv = modInverse(idx, 2 * rank)

    def _aut(self, v, idx):
        return self.ref.ints(self.ref.cf.aut(self.ref.arr(v), idx, self.isNTT))

    def transform(self, v):
        return self._aut(v, self.idx)

    def transpose(self, v):
        return self._aut(v, self.idxInv)


class ProjChecker:  # linear.go:94-137
    def __init__(self, ref, rank):
        self.ref, self.rank = ref, rank
        self.proj = [[False] * rank for _ in range(128)]

    def set_xof(self, xof):  # prover.go:168-176
        for j in range(self.rank):
            projBuf = xof[32 * j:32 * j + 32]
            for i in range(128):
                self.proj[i][j] = (projBuf[i // 8] >> (i % 8)) & 1 == 0
        return self

    def transform(self, v):
        q = self.ref.q
        out = [0] * self.rank
        for i in range(128):
            row, acc = self.proj[i], 0
            for j in range(self.rank):
                if row[j]:
                    acc = (acc + v[j]) % q
            out[i] = acc
        return out

    def transpose(self, v):
        q = self.ref.q
        out = [0] * self.rank
        for i in range(128):
            row, vi = self.proj[i], v[i]
            for j in range(self.rank):
                if row[j]:
                    out[j] = (out[j] + vi) % q
        return out


class RecomposeChecker:  # linear.go:140-180
    def __init__(self, ref, rank, base):
        """base: the decomposition base as plain integers (decomposeBase(bound))."""
        self.ref, self.rank = ref, rank
        self.dcmpBase = [b % ref.q * ref.R % ref.q for b in base]  # SetBigInt

    def transform(self, v):
        ref, nb, n = self.ref, len(self.dcmpBase), self.rank
        out = [None] * n
        for i in range(n // nb):
            out[i] = 0
            for j in range(nb):
                out[i] = (out[i] + ref.mul(self.dcmpBase[j], v[i * nb + j])) % ref.q
        for i in range(n // nb, n):
            out[i] = 0
        return out

    def transpose(self, v):
        ref, nb, n = self.ref, len(self.dcmpBase), self.rank
        out = [None] * n
        for i in range(n // nb):
            for j in range(nb):
                out[i * nb + j] = ref.mul(self.dcmpBase[j], v[i])
        for i in range((n // nb) * nb, n):
            out[i] = 0
        return out


# ---- prover.go:381-485 ---------------------------------------------------------------------------
def sumCheckMask(ref, rank, maskRank, emb, rand):
    """prover.go:381-397; rand = the MustSetRandom draws in call order."""
    draws = iter(rand)
    mask = [0] * emb
    for i in range(rank):
        mask[i] = next(draws)
    maskSum = mask[0]
    for i in range(rank, maskRank):
        mask[i] = next(draws)
        mask[i - rank] = (mask[i - rank] - mask[i]) % ref.q
    return mask, maskSum


def powers(ref, c, n):  # prover.go:409-413
    vec = [None] * n
    vec[0] = ref.set_uint64(1)
    for i in range(1, n):
        vec[i] = ref.mul(vec[i - 1], c)
    return vec


def checkTail(ref, ev, rank, scale, mask, n_quo, jindoRank):
    """The shared tail (prover.go:439-458, 465-484, 401-403) from the NTT-domain eval:
    returns (quo, remLo, remHi, remPoly)."""
    q, emb = ref.q, len(ev)
    if scale is not None:
        ev = [ref.mul(x, scale) for x in ev]  # ScalarMulTo(eval, eval, batchConst)
    ev = ref.inv(ev, cyclic=True)  # InvNTTTo
    if mask is not None:
        ev = [(x + m) % q for x, m in zip(ev, mask)]  # AddTo(eval, eval, mask)
    quoA, remA = ref.cf.quorem_vanishing(ref.arr(ev), rank)
    quoPoly, remPoly = ref.ints(quoA), ref.ints(remA)
    remLo = [None] * (rank - 1)
    for i in range(rank - 1):
        remLo[i] = remPoly[i + 1]
    remHi = [None] * jindoRank
    for i in range(jindoRank - (rank - 1)):
        remHi[i] = 0
    ii = jindoRank - (rank - 1)
    for i in range(rank - 1):
        remHi[ii] = remLo[i]
        ii += 1
    assert emb >= n_quo
    return quoPoly[:n_quo], remLo, remHi, remPoly


def linCheckEval(ref, rank, emb, batchConst, linCheckConst, checkers, constraints, wEcdNTT):
    """prover.go:409-438: the NTT-domain eval before the final scale.  wEcdNTT: list of int lists."""
    q = ref.q
    vec = powers(ref, linCheckConst, rank)
    ecd = ref.fwd(ref.encode(vec, emb), cyclic=True)
    ev = [0] * emb
    for tr, pairs in zip(checkers, constraints):
        vecTr = tr.transpose(vec)
        ecdTr = ref.fwd(ref.encode(vecTr, emb), cyclic=True)
        for wOutID, wInID in pairs:
            wOut, wIn = wEcdNTT[wOutID], wEcdNTT[wInID]
            term = [ref.mul(a, b) for a, b in zip(ecdTr, wIn)]                      # MulTo
            term = [(t - ref.mul(a, b)) % q for t, a, b in zip(term, ecd, wOut)]    # MulSubTo
            ev = [ref.mul(x, batchConst) for x in ev]                               # ScalarMulTo
            ev = [(x + t) % q for x, t in zip(ev, term)]                            # AddTo
    return ev


def linCheck(ref, rank, emb, jindoRank, batchConst, linCheckConst, linCheckMask, checkers, constraints, wEcdNTT):
    """prover.go:406-459 -> (quo, remLo, remHi, remPoly)."""
    ev = linCheckEval(ref, rank, emb, batchConst, linCheckConst, checkers, constraints, wEcdNTT)
    return checkTail(ref, ev, rank, batchConst, linCheckMask, rank, jindoRank)


def sumCheck(ref, rank, jindoRank, sumCheckMaxRank, batchConst, sumCheckMask, evalNTT):
    """prover.go:461-485 after evalCircuit (evalNTT = its output as ints)."""
    return checkTail(ref, evalNTT, rank, batchConst, sumCheckMask, sumCheckMaxRank - rank, jindoRank)[:3]


def arithCheck(ref, rank, arithCheckMaxRank, evalNTT):
    """prover.go:399-404 after evalCircuit."""
    return checkTail(ref, evalNTT, rank, None, None, arithCheckMaxRank - rank, rank - 1)[0]


# ---- verifier.go:249-294, on the coefficient vectors ------------------------------------------------
def evaluate(ref, coeffs, x):
    """Poly.Evaluate (poly.go:64-76): Horner over Montgomery-form ints."""
    z = 0
    for c in reversed(coeffs):
        z = (ref.mul(z, x) + c) % ref.q
    return z


def mexp(ref, x, e):
    r = ref.set_uint64(1)
    for _ in range(e):
        r = ref.mul(r, x)
    return r


def verifierLinCheck(ref, rank, emb, jindoRank, batchConst, linCheckConst, maskEval, x, maskSum, quoEval, remLoEval,
                     remHiEval, checkers, constraints, evals):
    """Verifier.linCheck (verifier.go:249-294): (remHi identity holds, main identity holds)."""
    q = ref.q
    shift = ref.mul(mexp(ref, x, jindoRank - (rank - 1)), remLoEval)
    vanishEval = (mexp(ref, x, rank) - ref.set_uint64(1)) % q
    vec = powers(ref, linCheckConst, rank)
    linCheckEval_ = evaluate(ref, ref.encode(vec, emb), x)
    ev = 0
    for tr, pairs in zip(checkers, constraints):
        trEval = evaluate(ref, ref.encode(tr.transpose(vec), emb), x)
        for wOutID, wInID in pairs:
            term = (ref.mul(trEval, evals[wInID]) - ref.mul(linCheckEval_, evals[wOutID])) % q
            ev = (ref.mul(ev, batchConst) + term) % q
    ev = (ref.mul(ev, batchConst) + maskEval) % q
    test = (ref.mul(quoEval, vanishEval) + ref.mul(remLoEval, x) + maskSum) % q
    return remHiEval == shift, ev == test
