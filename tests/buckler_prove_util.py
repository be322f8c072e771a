"""Shared by test_gpu_buckler_prove_multi.py: the proofs of a batch for rg_buckler_prove_checks* and
the restatement's answer for each.  Proof `seed` is the completeness circuit of the linear check
(tests/buckler_lin_util.py: one checker of each kind, wOut = M wIn) with its own witnesses, XOF
bytes, challenges and masks, plus an arithmetic and a sum-check circuit over the same witnesses and
two public witnesses.  The NTT-domain circuit values come from coracle.buckler_eval_circuit, the
linear check and the tails from tests/buckler_lin_ref.py, imported as they are."""
import functools

import numpy as np

from tests import buckler_lin_ref as R
from tests import synth_util as su
from tests.buckler_lin_util import completeness_circuit, rand_ints

N_W, N_PW = 8, 2  # the completeness circuit's witnesses; the public witnesses of the two circuits


@functools.lru_cache(maxsize=None)
def ctx(key):
    import ringo
    q = su.modulus(key)
    return ringo.Field(q), R.Ref(q)


def circuits(F, ref):
    """(arith, sum) constraint lists: products, a public-witness coefficient, a constant term, an
    empty constraint.  The widest term is pw * w * w: maxRank 3 rank <= emb = 4 rank."""
    import ringo.buckler as buckler
    k = ref.arr(rand_ints(ref.q, 3, np.random.default_rng(77)))
    a0 = buckler.ArithmeticConstraint(F)
    a0.AddTerm(None, 0, 1)
    a0.SubTerm(None, 2)
    a1 = buckler.ArithmeticConstraint(F)
    a1.AddTermWithConst(k[0], 1, 3, 0)
    a1.AddTerm(0, 2, 2)
    a1.AddTermWithConst(k[1], None)
    a2 = buckler.ArithmeticConstraint(F)
    a3 = buckler.ArithmeticConstraint(F)
    a3.AddTerm(None, 7)
    s0 = buckler.ArithmeticConstraint(F)
    s0.AddTerm(None, 4, 5)
    s0.AddTermWithConst(k[2], 0, 6)
    s1 = buckler.ArithmeticConstraint(F)
    s1.SubTerm(1, 1, 1)
    return [a0, a1, a2, a3], [s0, s1]


def oracle_cons(cons):
    return [[(c.coeffs[i], c.coeffsPublicWitness[i] if c.hasCoeffPublicWitness[i] else None, c.witness[i])
             for i in range(len(c.coeffs))] for c in cons]


@functools.lru_cache(maxsize=None)
def proof(key, rank, seed, perturb=False):
    """One proof's inputs as limb arrays and its three NTT-domain evals before the tail (ints).
    Read-only: shared among the tests."""
    F, ref = ctx(key)
    emb = 4 * rank
    circ = completeness_circuit(ref, rank, emb, seed=1000 * rank + seed, perturb=perturb)
    assert len(circ["w"]) == N_W
    rng = np.random.default_rng(5000 * rank + seed)
    chal = rand_ints(ref.q, 4, rng)  # arithBatchConst, linCheckBatchConst, linCheckConst, sumCheckBatchConst
    lin_mask, lin_mask_sum = R.sumCheckMask(ref, rank, 2 * rank, emb, circ["rand"])
    sum_mask = rand_ints(ref.q, emb, rng)
    w = np.stack([ref.arr(p) for p in circ["wEcdNTT"]])
    pw = np.stack([ref.arr(rand_ints(ref.q, emb, rng)) for _ in range(N_PW)])
    arith, sumc = circuits(F, ref)
    ch = ref.arr(chal)
    ev_arith = ref.ints(ref.cf.buckler_eval_circuit(oracle_cons(arith), ch[0], w, pw))
    ev_sum = ref.ints(ref.cf.buckler_eval_circuit(oracle_cons(sumc), ch[3], w, pw))
    ev_lin = R.linCheckEval(ref, rank, emb, chal[1], chal[2], circ["checkers"], circ["constraints"], circ["wEcdNTT"])
    return dict(circ=circ, chal=chal, chal_arr=ch, lin_mask=lin_mask, lin_mask_arr=ref.arr(lin_mask),
                lin_mask_sum=lin_mask_sum, sum_mask=sum_mask, sum_mask_arr=ref.arr(sum_mask), w=w, pw=pw,
                xof=circ["xof"], ev_arith=ev_arith, ev_lin=ev_lin, ev_sum=ev_sum)


@functools.lru_cache(maxsize=None)
def want(key, rank, seed, jindo_rank, arith_max, sum_max, perturb=False):
    """The restatement's eight outputs of one proof as limb arrays: arithQuo, linQuo, linRemLo,
    linRemHi, sumQuo, sumRemLo, sumRemHi, rem0 [2][L]."""
    _, ref = ctx(key)
    p = proof(key, rank, seed, perturb)
    aq = R.arithCheck(ref, rank, arith_max, p["ev_arith"])
    lq, llo, lhi, lrem = R.checkTail(ref, p["ev_lin"], rank, p["chal"][1], p["lin_mask"], rank, jindo_rank)
    sq, slo, shi, srem = R.checkTail(ref, p["ev_sum"], rank, p["chal"][3], p["sum_mask"], sum_max - rank, jindo_rank)
    arr = lambda xs: ref.arr(xs).reshape(len(xs), ref.L) if len(xs) else np.zeros((0, ref.L), np.uint64)  # noqa: E731
    return tuple(arr(x) for x in (aq, lq, llo, lhi, sq, slo, shi, [lrem[0], srem[0]]))
