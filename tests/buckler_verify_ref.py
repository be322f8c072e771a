"""Test reference for the Buckler verifier's checks: a Python-integer restatement of
buckler/verifier.go:178-315 -- pwEvals, vanishEval, the scalar evalCircuit, arithCheck, linCheck,
sumCheck and the roundComIdx layout of pf.Evals -- statement by statement, on tests/buckler_lin_ref.py
(Montgomery-form integers; Encode and the checkers' transposes as restated there).

The reference returns at the first failing check; `decide` goes on and reports every failure as the
bits of include/ringo.h (RG_BK_VERIFY_*), with the eight sides the comparisons were made on.

A constraint is a list of terms (coeff, public-witness index or None, [witness IDs]), coeff a
Montgomery-form integer (ArithmeticConstraint, constraint.go:6-12)."""
from tests import buckler_lin_ref as R

ARITH, LIN_REM, LIN, SUM_REM, SUM = 1, 2, 4, 8, 16


def layout(wCnt, hasLin, hasArith, hasSum):
    """Where verifier.go:120-214 reads pf.Evals: roundComIdx starts at wCnt."""
    ix = {}
    roundComIdx = wCnt
    if hasLin:
        ix["linMask"] = roundComIdx  # verifier.go:124
        roundComIdx += 1
    if hasSum:
        ix["sumMask"] = roundComIdx  # verifier.go:134
        roundComIdx += 1
    if hasArith:
        ix["arithQuo"] = roundComIdx  # verifier.go:189
        roundComIdx += 1
    if hasLin:
        ix["linQuo"] = roundComIdx  # verifier.go:199: quo, remLo, remHi
        roundComIdx += 3
    if hasSum:
        ix["sumQuo"] = roundComIdx  # verifier.go:209
        roundComIdx += 3
    ix["n"] = roundComIdx
    return ix


def exp(ref, x, e):  # bignum.Exp (math/bignum/bignum.go:34-46)
    r = ref.set_uint64(1)
    t = x
    while e > 0:
        if e & 1 == 1:
            r = ref.mul(r, t)
        t = ref.mul(t, t)
        e >>= 1
    return r


def evalCircuit(ref, batchConst, constraints, evals, pwEvals):  # verifier.go:219-240
    out = 0
    for c in constraints:
        ev = 0
        for coeff, pw, ws in c:
            term = coeff
            if pw is not None:
                term = ref.mul(term, pwEvals[pw])
            for w in ws:
                term = ref.mul(term, evals[w])
            ev = (ev + term) % ref.q
        ev = ref.mul(ev, batchConst)
        out = (out + ev) % ref.q
    return out


def own_evals(ref, rank, x, linCheckConst, checkers, pw):
    """The evaluations of the verifier's own vectors: (linCheckEval, [linCheckTrEval per checker],
    pwEvals) (verifier.go:181-184, 258-263, 273-275).  checkers None: no linear check."""
    linEval, trEvals = None, []
    if checkers is not None:
        vec = R.powers(ref, linCheckConst, rank)
        linEval = R.evaluate(ref, ref.encode(vec, rank), x)
        trEvals = [R.evaluate(ref, ref.encode(tr.transpose(vec), rank), x) for tr in checkers]
    pwEvals = [R.evaluate(ref, ref.encode(v, rank), x) for v in pw]
    return linEval, trEvals, pwEvals


def arithCheck(ref, batchConst, vanishEval, quoEval, constraints, evals, pwEvals):  # verifier.go:242-247
    ev = evalCircuit(ref, batchConst, constraints, evals, pwEvals)
    test = ref.mul(quoEval, vanishEval)
    return ev, test


def remShift(ref, rank, jindoRank, x, remLoEval):  # verifier.go:252-253, 299-300
    return ref.mul(exp(ref, x, jindoRank - (rank - 1)), remLoEval)


def linCheck(ref, batchConst, maskEval, x, vanishEval, maskSum, quoEval, remLoEval, linEval, trEvals, constraints,
             evals):  # verifier.go:271-293
    q = ref.q
    ev = 0
    for trEval, pairs in zip(trEvals, constraints):
        for wOutID, wInID in pairs:
            wOut, wIn = evals[wOutID], evals[wInID]
            term = ref.mul(trEval, wIn)
            termMul = ref.mul(linEval, wOut)
            term = (term - termMul) % q
            ev = ref.mul(ev, batchConst)
            ev = (ev + term) % q
    ev = ref.mul(ev, batchConst)
    ev = (ev + maskEval) % q
    test = ref.mul(quoEval, vanishEval)
    rem = ref.mul(remLoEval, x)
    test = (test + rem) % q
    test = (test + maskSum) % q
    return ev, test


def sumCheck(ref, batchConst, maskEval, x, vanishEval, maskSum, quoEval, remLoEval, constraints, evals,
             pwEvals):  # verifier.go:305-314
    q = ref.q
    ev = evalCircuit(ref, batchConst, constraints, evals, pwEvals)
    ev = ref.mul(ev, batchConst)
    ev = (ev + maskEval) % q
    test = ref.mul(quoEval, vanishEval)
    rem = ref.mul(remLoEval, x)
    test = (test + rem) % q
    test = (test + maskSum) % q
    return ev, test


def decide(ref, rank, jindoRank, wCnt, chal, maskSums, evals, own, linCons, arithCons, sumCons):
    """verifier.go:178-216 after pwEvals.  chal = (evalPoint, arithBatchConst, linCheckBatchConst,
    linCheckConst, sumCheckBatchConst), maskSums = (LinCheckMaskSum, SumCheckMaskSum), own =
    own_evals(...); a constraint list that is None is an absent check.  Returns (verdict, sides):
    sides = arith (eval, test), lin (shift * remLo, eval, test), sum (shift * remLo, eval, test)."""
    x, bcA, bcL, _, bcS = chal
    linEval, trEvals, pwEvals = own
    ix = layout(wCnt, linCons is not None, arithCons is not None, sumCons is not None)
    vanishEval = (exp(ref, x, rank) - ref.set_uint64(1)) % ref.q  # verifier.go:178-179
    verdict, sides = 0, [0] * 8
    if arithCons is not None:
        ev, test = arithCheck(ref, bcA, vanishEval, evals[ix["arithQuo"]], arithCons, evals, pwEvals)
        sides[0:2] = ev, test
        if ev != test:
            verdict |= ARITH
    if linCons is not None:
        i = ix["linQuo"]
        quoEval, remLoEval, remHiEval = evals[i], evals[i + 1], evals[i + 2]
        sh = remShift(ref, rank, jindoRank, x, remLoEval)
        ev, test = linCheck(ref, bcL, evals[ix["linMask"]], x, vanishEval, maskSums[0], quoEval, remLoEval, linEval,
                            trEvals, linCons, evals)
        sides[2:5] = sh, ev, test
        if remHiEval != sh:
            verdict |= LIN_REM
        if ev != test:
            verdict |= LIN
    if sumCons is not None:
        i = ix["sumQuo"]
        quoEval, remLoEval, remHiEval = evals[i], evals[i + 1], evals[i + 2]
        sh = remShift(ref, rank, jindoRank, x, remLoEval)
        ev, test = sumCheck(ref, bcS, evals[ix["sumMask"]], x, vanishEval, maskSums[1], quoEval, remLoEval, sumCons,
                            evals, pwEvals)
        sides[5:8] = sh, ev, test
        if remHiEval != sh:
            verdict |= SUM_REM
        if ev != test:
            verdict |= SUM
    return verdict, sides


def verify(ref, rank, jindoRank, wCnt, chal, maskSums, evals, pw, checkers, linCons, arithCons, sumCons):
    """-> (verdict, sides, pwEvals)."""
    own = own_evals(ref, rank, chal[0], chal[3], checkers if linCons is not None else None, pw)
    verdict, sides = decide(ref, rank, jindoRank, wCnt, chal, maskSums, evals, own, linCons, arithCons, sumCons)
    return verdict, sides, own[2]
