"""Shared by test_buckler_wide_ref.py (CPU) and test_gpu_buckler_verify_wide.py (GPU): seeded circuits
wider than the 256 lanes of verify_decide_kernel, in the style of buckler_lin_util.py and
buckler_verify_util.py.  No GPU and no torch here.

  * wide_lin_circuit: completeness_circuit over six checkers and any list of pair counts (zeros
    included), every pair honest; WideLinProof is the linear-check proof of such a circuit as
    HonestProof makes it (R.linCheck, the evaluations from R.evaluate).
  * wide_constraints / saturating_constraints: term lists of any length with the edge cases a walk
    over them can get wrong (empty constraints, a public witness on the program's term 0 and on a term
    without witnesses, 0 / one / q - 1 coefficients).
  * forge: pf.Evals and mask sums the restatement accepts for ANY circuit.  The verifier's checks are
    identities between scalars, and each has free slots that enter one side only (arithQuo; linMask
    and sumMask; both remHi), so random evaluations can be completed to an accepted proof without a
    prover -- which is what lets a test reach 570 constraints and 600 pairs in milliseconds.
  * WideCircuit: one such circuit with everything a verifier call takes."""
import functools

import numpy as np

from tests import buckler_lin_ref as R
from tests import buckler_verify_ref as V
from tests.buckler_lin_util import RECOMPOSE_BOUND, rand_ints, xof_bytes

N_CHECKERS = 6
LANES = 256  # kDecideLanes of buckler_verify.hip


def six_checkers(ref, rank, xof):
    """(reference checkers, spec for the device's): NTT, Aut(5, coeff), Proj(xof), Aut(3, NTT domain),
    Recompose(RECOMPOSE_BOUND), Aut(2 rank - 1, coeff)."""
    base = R.decomposeBase(RECOMPOSE_BOUND)
    checkers = [R.NTTChecker(ref, rank), R.AutChecker(ref, rank, 5, False), R.ProjChecker(ref, rank).set_xof(xof),
                R.AutChecker(ref, rank, 3, True), R.RecomposeChecker(ref, rank, base),
                R.AutChecker(ref, rank, 2 * rank - 1, False)]
    spec = [("ntt",), ("aut", 5, False), ("proj", xof), ("aut", 3, True), ("recompose", RECOMPOSE_BOUND),
            ("aut", 2 * rank - 1, False)]
    return checkers, spec


def wide_lin_circuit(ref, rank, emb, npairs, seed):
    """completeness_circuit with npairs[c] honest pairs (wOut = M wIn) on checker c of six_checkers.
    Returns the same dict: checkers, spec, constraints, w, wEcd, wEcdNTT, bc, lc, rand, xof."""
    assert len(npairs) == N_CHECKERS
    rng = np.random.default_rng(seed)
    q = ref.q
    xof = xof_bytes("random", rank, rng)
    checkers, spec = six_checkers(ref, rank, xof)
    w, constraints = [], []
    for chk, n in zip(checkers, npairs):
        pairs = []
        for _ in range(n):
            wIn = rand_ints(q, rank, rng)
            wOut = chk.transform(wIn)
            pairs.append((len(w), len(w) + 1))
            w += [wOut, wIn]
        constraints.append(pairs)
    blind = rand_ints(q, len(w), rng)
    wEcd = [ref.rand_encode(v, emb, r) for v, r in zip(w, blind)]
    wEcdNTT = [ref.fwd(p, cyclic=True) for p in wEcd]
    bc, lc = rand_ints(q, 2, rng)
    rand = rand_ints(q, 2 * rank, rng)
    return dict(checkers=checkers, spec=spec, constraints=constraints, w=w, wEcd=wEcd, wEcdNTT=wEcdNTT, bc=bc, lc=lc,
                rand=rand, xof=xof)


def _trim(p):
    n = len(p)
    while n and p[n - 1] == 0:
        n -= 1
    return p[:n]


class WideLinProof:
    """The linear check's part of buckler_verify_util.HonestProof on wide_lin_circuit: the mask from
    R.sumCheckMask, quo / remLo from R.linCheck, pf.Evals by R.evaluate at a random point, in the
    layout of a context that has the linear check only."""

    def __init__(self, ref, rank, emb, npairs, seed):
        self.ref, self.rank, self.emb = ref, rank, emb
        circ = self.circ = wide_lin_circuit(ref, rank, emb, npairs, seed)
        self.checkers, self.spec, self.lin = circ["checkers"], circ["spec"], circ["constraints"]
        self.wCnt = len(circ["w"])
        self.bcL, self.lc = circ["bc"], circ["lc"]
        self.x = rand_ints(ref.q, 1, np.random.default_rng(seed + 1000))[0]
        self.linMask, self.linMaskSum = R.sumCheckMask(ref, rank, 2 * rank, emb, circ["rand"])
        self.linQuo, self.linLo, _, self.rem = R.linCheck(ref, rank, emb, rank - 1, self.bcL, self.lc, self.linMask,
                                                          self.checkers, self.lin, circ["wEcdNTT"])
        ev = lambda p: R.evaluate(ref, _trim(list(p)), self.x)  # noqa: E731
        self.wEvals = [ev(p) for p in circ["wEcd"]]
        self.maskEval, self.quoEval, self.loEval = ev(self.linMask), ev(self.linQuo), ev(self.linLo)

    def chal(self):
        return [self.x, 0, self.bcL, self.lc, 0]  # no arithmetic and no sum check: their constants are not read

    def mask_sums(self):
        return [self.linMaskSum, 0]

    def evals(self, jindoRank):
        """pf.Evals: the witnesses, linMask, linQuo, remLo, remHi (jindoRank - (rank - 1) zeros, then remLo)."""
        hi = R.evaluate(self.ref, [0] * (jindoRank - (self.rank - 1)) + list(self.linLo), self.x)
        ix = V.layout(self.wCnt, True, False, False)
        assert (ix["linMask"], ix["linQuo"], ix["n"]) == (self.wCnt, self.wCnt + 1, self.wCnt + 4)
        return list(self.wEvals) + [self.maskEval, self.quoEval, self.loEval, hi]

    def perturbations(self, jindoRank):
        """name -> (evals, expected bits): lin_quo, lin_remlo, and the wIn of the last pair bumped."""
        q, base = self.ref.q, self.evals(jindoRank)
        ix = V.layout(self.wCnt, True, False, False)

        def bump(i):
            e = list(base)
            e[i] = (e[i] + 1) % q
            return e

        last = [p for ps in self.lin for p in ps][-1]
        return {"lin_quo": (bump(ix["linQuo"]), V.LIN), "lin_remlo": (bump(ix["linQuo"] + 1), V.LIN_REM | V.LIN),
                "last_pair_witness": (bump(last[1]), V.LIN)}


# ---- constraint lists ----------------------------------------------------------------------------------
def mont_one(q):
    """SetUint64(1) of the field of q: 2^(64 L) mod q."""
    return (1 << (64 * ((q.bit_length() + 63) // 64))) % q


MAX_TERMS, MAX_WITNESSES = 4, 5


def wide_constraints(q, n_constraints, w_cnt, n_pw, rng):
    """n_constraints term lists (coeff, pw or None, [witness ids]): 0 to MAX_TERMS terms each, the
    first, the middle and the last constraint empty; 0 to MAX_WITNESSES witnesses a term; a public
    witness on about a third of the terms (none with n_pw = 0).  Constraint 0 being empty, "term 0"
    is the program's first term, that of constraint 1: it carries a public witness and witnesses, so
    a walk that starts one place before the term's witnesses starts at -1.  Constraint 2 is a public
    witness with no witness; constraint 3 has MAX_TERMS terms, the first of MAX_WITNESSES witnesses
    with the coefficients 0, one and q - 1 on the next three."""
    assert n_constraints >= 8 and w_cnt >= 1
    one = mont_one(q)
    wits = lambda n: [int(x) for x in rng.integers(0, w_cnt, n)]  # noqa: E731
    pwi = lambda: int(rng.integers(0, n_pw)) if n_pw else None  # noqa: E731
    empty = {0, n_constraints // 2, n_constraints - 1}
    out = []
    for c in range(n_constraints):
        if c in empty:
            out.append([])
        elif c == 1:
            out.append([(rand_ints(q, 1, rng)[0], 0 if n_pw else None, wits(2)), (one, None, wits(1))])
        elif c == 2:
            out.append([(rand_ints(q, 1, rng)[0], n_pw - 1 if n_pw else None, [])])
        elif c == 3:
            out.append([(rand_ints(q, 1, rng)[0], None, wits(MAX_WITNESSES)), (0, pwi(), wits(2)),
                        (one, None, wits(3)), (q - 1, None, wits(1))])
        else:
            terms = []
            for _ in range(int(rng.integers(0, MAX_TERMS + 1))):
                coeff = (0, one, q - 1)[int(rng.integers(0, 3))] if rng.integers(0, 8) == 0 else rand_ints(q, 1, rng)[0]
                pw = pwi() if rng.integers(0, 3) == 0 else None
                terms.append((coeff, pw, wits(int(rng.integers(0, MAX_WITNESSES + 1)))))
            out.append(terms)
    return out


def saturating_constraints(q, n):
    """n constraints of one constant-only term q - 1: a lane that holds one has the accumulator q - 1,
    so every addition of the fold wraps."""
    return [[(q - 1, None, [])] for _ in range(n)]


def shape(cons):
    """What a constraint list is made of: dict(n, empty = the empty constraints' places, terms,
    max_terms, max_wits, pw_terms, pw_term0 = the program's first term has a public witness and
    witnesses, pw_alone = some term has a public witness and no witness, coeffs = the set of
    coefficients)."""
    terms = [t for c in cons for t in c]
    return dict(n=len(cons), empty=[i for i, c in enumerate(cons) if not c], terms=len(terms),
                max_terms=max((len(c) for c in cons), default=0), max_wits=max((len(t[2]) for t in terms), default=0),
                pw_terms=sum(t[1] is not None for t in terms),
                pw_term0=bool(terms) and terms[0][1] is not None and len(terms[0][2]) > 0,
                pw_alone=any(t[1] is not None and not t[2] for t in terms), coeffs={t[0] for t in terms})


def wide_pairs(npairs, w_cnt, rng):
    """Per checker, npairs[c] pairs (wOut, wIn) of random witness ids below w_cnt."""
    return [[(int(a), int(b)) for a, b in rng.integers(0, w_cnt, (n, 2))] for n in npairs]


def lanes_of_pairs(npairs):
    """How verify_decide_kernel spreads the pairs: dict(n, trips = the most pairs one lane takes,
    lane64 = lane 64 (a lane with a power of its own to compute first) holds a pair, second_trip =
    lane 0 takes pair 256, empty = the empty checkers' places, starts = the first pair of each
    non-empty checker)."""
    n = sum(npairs)
    starts = [sum(npairs[:c]) for c in range(len(npairs)) if npairs[c]]
    return dict(n=n, trips=-(-n // LANES), lane64=n > 64, second_trip=n > LANES,
                empty=[c for c, k in enumerate(npairs) if k == 0], starts=starts)


# ---- forged proofs -------------------------------------------------------------------------------------
def _reads(cons, w):
    return cons is not None and any(w in ws for c in cons for _, _, ws in c)


def _neighbours(cons, w):
    """The witnesses that share a term with w."""
    return {v for c in cons or [] for _, _, ws in c if w in ws for v in ws}


def forge(ref, rank, jr, w_cnt, chal, own, lin, arith, sum, rng):
    """Random pf.Evals and mask sums, then the free slots solved so that V.decide accepts (verdict 0)
    with the circuit (lin, arith, sum: constraint lists or None), the challenges `chal` and the
    verifier's own evaluations `own` = V.own_evals(...).  0, one and q - 1 are planted on three
    witnesses.  Returns (evals, maskSums, rejections): rejections is name -> (evals, maskSums, bits),
    each one value bumped by 1 -- the seven slots of buckler_verify_util.perturbations, a mask sum of
    each check and, where one witness is read by all three checks, that witness."""
    q = ref.q
    x, bcA, bcL, _, bcS = chal
    linEval, trEvals, pwEvals = own
    ix = V.layout(w_cnt, lin is not None, arith is not None, sum is not None)
    one = ref.set_uint64(1)
    vanishEval = (V.exp(ref, x, rank) - one) % q
    assert vanishEval != 0, "evalPoint is a root of X^rank - 1: arithQuo cannot be solved for"
    # a witness all three checks read, where there is one; the planted values keep clear of it
    shared = None
    if lin is not None and arith is not None and sum is not None:
        in_pairs = {w for ps in lin for p in ps for w in p}
        shared = next((w for w in range(w_cnt) if w in in_pairs and _reads(arith, w) and _reads(sum, w)), None)
    evals = rand_ints(q, ix["n"], rng)
    keep = _neighbours(arith, shared) | _neighbours(sum, shared) | {shared}
    free = [w for w in range(w_cnt) if w not in keep]
    assert len(free) >= 3
    planted = [free[int(i)] for i in rng.choice(len(free), 3, replace=False)]
    for w, v in zip(planted, (0, one, q - 1)):
        evals[w] = v
    ms = rand_ints(q, 2, rng)
    van_inv = pow(vanishEval, -1, q)
    if arith is not None:  # ev = mul(quo, van) = quo van / R
        ev = V.evalCircuit(ref, bcA, arith, evals, pwEvals)
        evals[ix["arithQuo"]] = ev * ref.R * van_inv % q
    if lin is not None:
        i = ix["linQuo"]
        evals[i + 2] = V.remShift(ref, rank, jr, x, evals[i + 1])
        ev, test = V.linCheck(ref, bcL, 0, x, vanishEval, ms[0], evals[i], evals[i + 1], linEval, trEvals, lin, evals)
        evals[ix["linMask"]] = (test - ev) % q
    if sum is not None:
        i = ix["sumQuo"]
        evals[i + 2] = V.remShift(ref, rank, jr, x, evals[i + 1])
        ev, test = V.sumCheck(ref, bcS, 0, x, vanishEval, ms[1], evals[i], evals[i + 1], sum, evals, pwEvals)
        evals[ix["sumMask"]] = (test - ev) % q

    def bump(i):
        e = list(evals)
        e[i] = (e[i] + 1) % q
        return e

    rej = {}
    if arith is not None:
        rej["arith_quo"] = (bump(ix["arithQuo"]), ms, V.ARITH)
    if lin is not None:
        i = ix["linQuo"]
        rej.update(lin_remhi=(bump(i + 2), ms, V.LIN_REM), lin_quo=(bump(i), ms, V.LIN),
                   lin_remlo=(bump(i + 1), ms, V.LIN_REM | V.LIN), lin_mask_sum=(evals, [(ms[0] + 1) % q, ms[1]], V.LIN))
    if sum is not None:
        i = ix["sumQuo"]
        rej.update(sum_remhi=(bump(i + 2), ms, V.SUM_REM), sum_quo=(bump(i), ms, V.SUM),
                   sum_remlo=(bump(i + 1), ms, V.SUM_REM | V.SUM), sum_mask_sum=(evals, [ms[0], (ms[1] + 1) % q], V.SUM))
    if shared is not None:
        rej["shared_witness"] = (bump(shared), ms, V.ARITH | V.LIN | V.SUM)
    return evals, ms, rej


# ---- a whole wide circuit ------------------------------------------------------------------------------
def n_pw_for(L):
    """Public witnesses enough that n_pw L words pass the 256 lanes of the pwEvals copy and are no
    multiple of them: 300 for one limb, 40 for 14."""
    n = max(40, -(-300 // L))
    assert n * L > LANES and n * L % LANES
    return n


class WideCircuit:
    """A verifier's circuit over w_cnt witnesses with pair counts `npairs` on six_checkers (None: no
    linear check), nc0 arithmetic and nc1 sum constraints (None: the check is absent; `saturate`: both
    lists from saturating_constraints), and per proof (`proof_seed`) the public witnesses, the XOF bytes
    and the five challenges.  The circuit (pairs, constraints) depends on `seed` alone."""

    def __init__(self, ref, rank, npairs, nc0, nc1, w_cnt, n_pw, seed, proof_seed=0, saturate=False):
        self.ref, self.rank, self.wCnt, self.nPw = ref, rank, w_cnt, n_pw
        q = ref.q
        rng = np.random.default_rng(seed)
        self.npairs = npairs
        self.lin = wide_pairs(npairs, w_cnt, rng) if npairs is not None else None

        def make(n):
            if saturate:
                return saturating_constraints(q, n)
            if n >= 8:
                return wide_constraints(q, n, w_cnt, n_pw, rng)
            return wide_constraints(q, 8, w_cnt, n_pw, rng)[1:1 + n]  # a short list: the head after the empty one

        self.arith = make(nc0) if nc0 is not None else None
        self.sum = make(nc1) if nc1 is not None else None
        prng = np.random.default_rng([seed, proof_seed, 1])
        self.xof = xof_bytes("random", rank, prng)
        self.checkers, self.spec = six_checkers(ref, rank, self.xof) if npairs is not None else (None, None)
        self.pw = [rand_ints(q, rank, prng) for _ in range(n_pw)]
        self.challenges = rand_ints(q, 5, prng)
        self.has = (self.lin is not None, self.arith is not None, self.sum is not None)

    def chal(self):
        return list(self.challenges)

    def cons(self):
        return self.lin, self.arith, self.sum

    def own(self):
        ch = self.challenges
        return V.own_evals(self.ref, self.rank, ch[0], ch[3], self.checkers, self.pw)

    def forge(self, jr, own=None, seed=0):
        """forge on this circuit: (evals, maskSums, rejections)."""
        return forge(self.ref, self.rank, jr, self.wCnt, self.chal(), own if own is not None else self.own(),
                     self.lin, self.arith, self.sum, np.random.default_rng([seed, jr, 2]))

    def decide(self, jr, own, evals, ms):
        return V.decide(self.ref, self.rank, jr, self.wCnt, self.chal(), ms, evals, own, self.lin, self.arith, self.sum)


# ---- the circuits of the wide tests, built once and shared (read-only) ------------------------------------
RANK = 128  # the rank-sized stage is not the subject
W_CNT, NC0, NC1 = 600, 300, 270
WIDE_PAIRS = [1, 0, 298, 0, 300, 1]
WIDE_FIELDS = ["p63", "mult_zp", "jindo_zp", "zp440", "zp880"]  # 1, 2, 4, 7 and 14 limbs
HONEST_PAIRS = [1, 0, 130, 0, 125, 1]
HONEST_FIELDS = ["p63", "mult_zp", "jindo_zp"]  # a 14-limb prover in Python integers takes too long
BOUNDARY_FIELDS = ["p63", "jindo_zp"]
SPLITS = [(256, None), (1, 255), (257, 0)]  # (arithmetic, sum) constraints; None: no sum check
# 64: lane 64 has its power and no pair, the first and the last checker are empty; 65: pair 64, the
# first of its checker after an empty one, on lane 64; 256: every lane one pair, a checker starts on
# lane 64; 257: lane 0 takes pair 256, the only pair of the last checker, past two empty ones
BOUNDARY_PAIRS = [[0, 10, 20, 30, 4, 0], [30, 34, 0, 1, 0, 0], [64, 100, 0, 92, 0, 0], [64, 96, 96, 0, 0, 1]]


@functools.lru_cache(maxsize=None)
def honest_lin_proof(ref):
    return WideLinProof(ref, RANK, 2 * RANK, HONEST_PAIRS, seed=257)


@functools.lru_cache(maxsize=None)
def wide_circuit(ref, proof_seed=0):
    return WideCircuit(ref, RANK, WIDE_PAIRS, NC0, NC1, W_CNT, n_pw_for(ref.L), seed=600, proof_seed=proof_seed)


@functools.lru_cache(maxsize=None)
def _boundary(ref, split, npairs):
    return WideCircuit(ref, RANK, list(npairs), split[0], split[1], W_CNT, 3, seed=sum(npairs) + split[0])


def boundary_circuit(ref, split, npairs):
    return _boundary(ref, tuple(split), tuple(npairs))


@functools.lru_cache(maxsize=None)
def saturated_circuit(ref):
    return WideCircuit(ref, RANK, None, LANES, 2 * LANES - 1, 8, 0, seed=9, saturate=True)


def assert_wide_shape(wc):
    """What makes wide_circuit wide, so that a later edit cannot shrink it back under a wave."""
    nc0, nc1, L = len(wc.arith), len(wc.sum), wc.ref.L
    assert nc0 > LANES and nc1 > LANES  # both lists reach lanes past 255 of the first trip
    assert nc0 + nc1 > 2 * LANES  # some lanes take a third constraint
    assert nc0 - LANES == 44  # the lists meet on lane 44 of the second trip
    p = lanes_of_pairs(wc.npairs)
    assert p["n"] > 2 * LANES and p["trips"] == 3 and p["lane64"] and p["second_trip"]
    assert p["empty"] == [1, 3] and len(wc.npairs) == N_CHECKERS
    assert wc.nPw * L > LANES and wc.nPw * L % LANES  # the pwEvals copy strides and ends inside a trip
    assert max(w for ps in wc.lin for pr in ps for w in pr) < wc.wCnt == W_CNT
