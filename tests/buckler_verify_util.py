"""Shared by test_buckler_verify_ref.py (CPU), test_gpu_buckler_verify.py and
test_gpu_capi_c_bverify.py (GPU): an honest Buckler proof for the verifier's checks, made with the
restated prover (tests/buckler_lin_ref.py) and the C oracle.

The linear check is buckler_lin_util.completeness_circuit (one checker of each kind, wOut = M wIn).
On top of it:
  * an arithmetic circuit that holds on the witness domain, with a term of three witnesses and a
    SubTerm (a b c - d), a public-witness coefficient with a constant (k pw0 a - e) and a
    constant-only term (k2 - g);
  * two sum-check constraints whose values sum to zero over the witness domain (pw1 a s1 - s2 with
    s2's last entry chosen so, and s1 - s3 with s3 = s1 reversed);
  * a third public witness nobody reads.
`a` is witness 1, the wIn of the first linear pair, so one evaluation is read by all three checks.
Quotients and remainders come from R.linCheck / R.sumCheck / R.arithCheck, the evaluations from
R.evaluate at a random point."""
import numpy as np

from tests import buckler_lin_ref as R
from tests import buckler_verify_ref as V
from tests.buckler_lin_util import completeness_circuit, rand_ints

A_ID = 1  # the witness all three checks read


def _trim(p):
    n = len(p)
    while n and p[n - 1] == 0:
        n -= 1
    return p[:n]


def _ev(ref, p, x):
    return R.evaluate(ref, _trim(list(p)), x)


def _oracle_cons(ref, cons):
    return [[(ref.arr([coeff])[0], pw, ws) for coeff, pw, ws in c] for c in cons]


class HonestProof:
    def __init__(self, ref, rank, seed, two_pairs=False):
        self.ref, self.rank = ref, rank
        q, mul = ref.q, ref.mul
        emb = self.emb = 4 * rank  # a b c has 3 rank + 1 coefficients
        circ = completeness_circuit(ref, rank, emb, seed, two_pairs=two_pairs)
        rng = np.random.default_rng(seed + 1000)
        one, neg1 = ref.set_uint64(1), (-ref.set_uint64(1)) % q
        self.checkers, self.spec, self.lin = circ["checkers"], circ["spec"], circ["constraints"]
        w = [list(v) for v in circ["w"]]
        n0 = len(w)
        a = w[A_ID]
        k, k2 = rand_ints(q, 2, rng)
        self.pw = pw = [rand_ints(q, rank, rng) for _ in range(3)]
        b, c, s1 = (rand_ints(q, rank, rng) for _ in range(3))
        d = [mul(mul(x, y), z) for x, y, z in zip(a, b, c)]
        e = [mul(mul(k, p), x) for p, x in zip(pw[0], a)]
        g = [k2] * rank
        s2 = rand_ints(q, rank, rng)
        prod = [mul(mul(p, x), y) for p, x, y in zip(pw[1], a, s1)]
        s2[-1] = (sum(prod) - sum(s2[:-1])) % q
        s3 = s1[::-1]
        B, C, D, E, G, S1, S2, S3 = range(n0, n0 + 8)
        w += [b, c, d, e, g, s1, s2, s3]
        self.w, self.wCnt = w, len(w)
        self.arith = [[(one, None, [A_ID, B, C]), (neg1, None, [D])],
                      [(k, 0, [A_ID]), (neg1, None, [E])],
                      [(k2, None, []), (neg1, None, [G])]]
        self.sum = [[(one, 1, [A_ID, S1]), (neg1, None, [S2])],
                    [(one, None, [S1]), (neg1, None, [S3])]]
        # the prover (prover.go): RandEncode, NTT, the three checks
        blind = rand_ints(q, len(w) - n0, rng)
        self.wEcd = list(circ["wEcd"]) + [ref.rand_encode(v, emb, r) for v, r in zip(w[n0:], blind)]
        self.wEcdNTT = list(circ["wEcdNTT"]) + [ref.fwd(p, cyclic=True) for p in self.wEcd[n0:]]
        pwEcdNTT = [ref.fwd(ref.encode(v, emb), cyclic=True) for v in pw]
        self.x, self.bcA, self.bcL, self.lc, self.bcS = rand_ints(q, 5, rng)
        wA = np.stack([ref.arr(p) for p in self.wEcdNTT])
        pwA = np.stack([ref.arr(p) for p in pwEcdNTT])
        self.wEcdNTT_arr, self.pwEcdNTT_arr = wA, pwA
        jr0 = rank - 1
        self.linMask, self.linMaskSum = R.sumCheckMask(ref, rank, 2 * rank, emb, circ["rand"])
        self.linRand = circ["rand"]
        self.linQuo, self.linLo, _, rem = R.linCheck(ref, rank, emb, jr0, self.bcL, self.lc, self.linMask,
                                                     self.checkers, self.lin, self.wEcdNTT)
        assert rem[0] == self.linMaskSum
        evA = ref.ints(ref.cf.buckler_eval_circuit(_oracle_cons(ref, self.arith), ref.arr([self.bcA])[0], wA, pwA))
        self.arithMaxRank = 3 * rank + 1  # constraint.go:56-70 of a b c
        self.arithQuo = R.arithCheck(ref, rank, self.arithMaxRank, evA)
        evS = ref.ints(ref.cf.buckler_eval_circuit(_oracle_cons(ref, self.sum), ref.arr([self.bcS])[0], wA, pwA))
        self.sumMaxRank = 3 * rank  # pw1 a s1: rank - 1 + 2 rank, + 1
        self.sumRand = rand_ints(q, self.sumMaxRank, rng)
        self.sumMask, self.sumMaskSum = R.sumCheckMask(ref, rank, self.sumMaxRank, emb, self.sumRand)
        self.sumQuo, self.sumLo, _ = R.sumCheck(ref, rank, jr0, self.sumMaxRank, self.bcS, self.sumMask, evS)
        # pf.Evals, part by part
        x = self.x
        self.wEvals = [_ev(ref, p, x) for p in self.wEcd]
        self.parts = dict(linMask=_ev(ref, self.linMask, x), sumMask=_ev(ref, self.sumMask, x),
                          arithQuo=_ev(ref, self.arithQuo, x), linQuo=_ev(ref, self.linQuo, x),
                          linLo=_ev(ref, self.linLo, x), sumQuo=_ev(ref, self.sumQuo, x),
                          sumLo=_ev(ref, self.sumLo, x))

    def chal(self):
        return [self.x, self.bcA, self.bcL, self.lc, self.bcS]

    def mask_sums(self):
        return [self.linMaskSum, self.sumMaskSum]

    def rem_hi_eval(self, lo, jindoRank):
        """remHi = jindoRank - (rank - 1) zeros, then remLo (prover.go:450-456), evaluated as it stands."""
        return R.evaluate(self.ref, [0] * (jindoRank - (self.rank - 1)) + list(lo), self.x)

    def evals(self, jindoRank, lin=True, arith=True, sum=True):
        """pf.Evals in the roundComIdx order for a context with the given checks."""
        p = self.parts
        ix = V.layout(self.wCnt, lin, arith, sum)
        out = list(self.wEvals) + [None] * (ix["n"] - self.wCnt)
        if lin:
            out[ix["linMask"]] = p["linMask"]
            out[ix["linQuo"]:ix["linQuo"] + 3] = p["linQuo"], p["linLo"], self.rem_hi_eval(self.linLo, jindoRank)
        if sum:
            out[ix["sumMask"]] = p["sumMask"]
            out[ix["sumQuo"]:ix["sumQuo"] + 3] = p["sumQuo"], p["sumLo"], self.rem_hi_eval(self.sumLo, jindoRank)
        if arith:
            out[ix["arithQuo"]] = p["arithQuo"]
        assert None not in out
        return out

    def cons(self, lin=True, arith=True, sum=True):
        return (self.lin if lin else None, self.arith if arith else None, self.sum if sum else None)


def perturbations(hp, jindoRank):
    """The one-change rejections of the honest proof with all three checks: name -> (evals, maskSums,
    pw, chal, expected bits).  Every change adds 1 to one value."""
    q = hp.ref.q
    ix = V.layout(hp.wCnt, True, True, True)
    base = hp.evals(jindoRank)

    def bump(i):
        e = list(base)
        e[i] = (e[i] + 1) % q
        return e

    ms, pw, ch = hp.mask_sums(), hp.pw, hp.chal()
    out = {
        "lin_remhi": (bump(ix["linQuo"] + 2), ms, pw, ch, V.LIN_REM),
        "sum_remhi": (bump(ix["sumQuo"] + 2), ms, pw, ch, V.SUM_REM),
        "arith_quo": (bump(ix["arithQuo"]), ms, pw, ch, V.ARITH),
        "lin_quo": (bump(ix["linQuo"]), ms, pw, ch, V.LIN),
        "sum_quo": (bump(ix["sumQuo"]), ms, pw, ch, V.SUM),
        "lin_remlo": (bump(ix["linQuo"] + 1), ms, pw, ch, V.LIN_REM | V.LIN),
        "sum_remlo": (bump(ix["sumQuo"] + 1), ms, pw, ch, V.SUM_REM | V.SUM),
        "lin_mask_sum": (base, [(ms[0] + 1) % q, ms[1]], pw, ch, V.LIN),
        "sum_mask_sum": (base, [ms[0], (ms[1] + 1) % q], pw, ch, V.SUM),
        "shared_witness": (bump(A_ID), ms, pw, ch, V.ARITH | V.LIN | V.SUM),
    }
    for i, bits in ((0, V.ARITH), (1, V.SUM), (2, 0)):  # pw0: arith, pw1: sum, pw2: nobody
        p2 = [list(v) for v in pw]
        p2[i][5] = (p2[i][5] + 1) % q
        out[f"pw{i}"] = (base, ms, p2, ch, bits)
    # evalPoint changed after the evals were taken: every main identity fails; the remHi identities
    # read evalPoint only through evalPoint^(jindoRank - (rank - 1)), so they hold on at exponent 0
    rem_bits = 0 if jindoRank == hp.rank - 1 else V.LIN_REM | V.SUM_REM
    out["eval_point"] = (base, ms, pw, [(ch[0] + 1) % q] + ch[1:], V.ARITH | V.LIN | V.SUM | rem_bits)
    return out
