"""Shared by test_buckler_verify_multi_ref.py (CPU) and test_gpu_buckler_verify_multi.py (GPU): several
honest Buckler proofs of ONE compiled circuit, for the verifier's batch entry.

buckler_verify_util.HonestProof draws the circuit's constants k and k2 from its seed, so proofs of
different seeds are proofs of different circuits and cannot share a verifier handle.  CircuitProof is the
same proof (same witness numbering, same constraints, same prover steps) with what Compile fixes taken
from the circuit -- the constraint coefficients k and k2, the checker kinds, the automorphism index, the
recompose bound -- and everything a proof owns drawn from the proof's seed: the witnesses, the three
public witnesses, the XOF bytes of the projection matrix, all five challenges and both mask draws.
Two proofs that share one of these could not show an index slip in it, so `proofs` asserts that they
differ pairwise."""
import numpy as np

from tests import buckler_lin_ref as R
from tests import buckler_verify_ref as V
from tests.buckler_lin_util import completeness_circuit, rand_ints
from tests.buckler_verify_util import A_ID, HonestProof, _ev, _oracle_cons

PROJ = 2  # the projection checker's place among completeness_circuit's checkers


def circuit_constants(ref, seed):
    """(k, k2): the coefficients of the arithmetic circuit, fixed per circuit."""
    return tuple(rand_ints(ref.q, 2, np.random.default_rng(seed + 77)))


class CircuitProof(HonestProof):
    """HonestProof with the circuit's k, k2 given and every other value from `seed`."""

    def __init__(self, ref, rank, consts, seed):
        self.ref, self.rank = ref, rank
        q, mul = ref.q, ref.mul
        emb = self.emb = 4 * rank
        circ = completeness_circuit(ref, rank, emb, seed)
        rng = np.random.default_rng(seed + 1000)
        one, neg1 = ref.set_uint64(1), (-ref.set_uint64(1)) % q
        self.checkers, self.spec, self.lin, self.xof = circ["checkers"], circ["spec"], circ["constraints"], circ["xof"]
        w = [list(v) for v in circ["w"]]
        n0 = len(w)
        a = w[A_ID]
        k, k2 = consts
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
        blind = rand_ints(q, len(w) - n0, rng)
        self.wEcd = list(circ["wEcd"]) + [ref.rand_encode(v, emb, r) for v, r in zip(w[n0:], blind)]
        self.wEcdNTT = list(circ["wEcdNTT"]) + [ref.fwd(p, cyclic=True) for p in self.wEcd[n0:]]
        pwEcdNTT = [ref.fwd(ref.encode(v, emb), cyclic=True) for v in pw]
        self.x, self.bcA, self.bcL, self.lc, self.bcS = rand_ints(q, 5, rng)
        wA = np.stack([ref.arr(p) for p in self.wEcdNTT])
        pwA = np.stack([ref.arr(p) for p in pwEcdNTT])
        jr0 = rank - 1
        self.linRand = circ["rand"]
        self.linMask, self.linMaskSum = R.sumCheckMask(ref, rank, 2 * rank, emb, self.linRand)
        self.linQuo, self.linLo, _, rem = R.linCheck(ref, rank, emb, jr0, self.bcL, self.lc, self.linMask,
                                                     self.checkers, self.lin, self.wEcdNTT)
        assert rem[0] == self.linMaskSum
        evA = ref.ints(ref.cf.buckler_eval_circuit(_oracle_cons(ref, self.arith), ref.arr([self.bcA])[0], wA, pwA))
        self.arithMaxRank = 3 * rank + 1
        self.arithQuo = R.arithCheck(ref, rank, self.arithMaxRank, evA)
        evS = ref.ints(ref.cf.buckler_eval_circuit(_oracle_cons(ref, self.sum), ref.arr([self.bcS])[0], wA, pwA))
        self.sumMaxRank = 3 * rank
        self.sumRand = rand_ints(q, self.sumMaxRank, rng)
        self.sumMask, self.sumMaskSum = R.sumCheckMask(ref, rank, self.sumMaxRank, emb, self.sumRand)
        self.sumQuo, self.sumLo, _ = R.sumCheck(ref, rank, jr0, self.sumMaxRank, self.bcS, self.sumMask, evS)
        x = self.x
        self.wEvals = [_ev(ref, p, x) for p in self.wEcd]
        self.parts = dict(linMask=_ev(ref, self.linMask, x), sumMask=_ev(ref, self.sumMask, x),
                          arithQuo=_ev(ref, self.arithQuo, x), linQuo=_ev(ref, self.linQuo, x),
                          linLo=_ev(ref, self.linLo, x), sumQuo=_ev(ref, self.sumQuo, x),
                          sumLo=_ev(ref, self.sumLo, x))

    def checkers_with_xof(self, xof):
        """The reference checkers with the projection matrix drawn from other XOF bytes."""
        out = list(self.checkers)
        out[PROJ] = R.ProjChecker(self.ref, self.rank).set_xof(xof)
        return out

    def own(self, checkers=None, pw=None, chal=None):
        """The evaluations of the verifier's own vectors for this proof (V.own_evals)."""
        ch = chal if chal is not None else self.chal()
        return V.own_evals(self.ref, self.rank, ch[0], ch[3], checkers if checkers is not None else self.checkers,
                           pw if pw is not None else self.pw)


def _distinct(vals, what):
    for i in range(len(vals)):
        for j in range(i + 1, len(vals)):
            assert vals[i] != vals[j], f"proofs {i} and {j} share {what}"


def proofs(ref, rank, n, circuit_seed=5):
    """n honest proofs of one circuit; every per-proof input differs pairwise."""
    consts = circuit_constants(ref, circuit_seed)
    out = [CircuitProof(ref, rank, consts, seed=circuit_seed * 1000 + 17 * i + rank) for i in range(n)]
    for hp in out[1:]:  # one circuit: the same program in every proof
        assert (hp.arith, hp.sum, hp.lin, hp.wCnt) == (out[0].arith, out[0].sum, out[0].lin, out[0].wCnt)
        assert [s if s[0] != "proj" else "proj" for s in hp.spec] == [s if s[0] != "proj" else "proj" for s in out[0].spec]
    _distinct([hp.xof for hp in out], "the XOF bytes")
    _distinct([hp.w for hp in out], "the witnesses")
    for k in range(3):
        _distinct([hp.pw[k] for hp in out], f"public witness {k}")
    for k in range(5):
        _distinct([hp.chal()[k] for hp in out], f"challenge {k}")
    for k in range(2):
        _distinct([hp.mask_sums()[k] for hp in out], f"mask sum {k}")
    _distinct([hp.linRand for hp in out], "the lin mask draws")
    _distinct([hp.sumRand for hp in out], "the sum mask draws")
    g = len(out[0].w) - 4  # witness g = [k2] * rank is the circuit's constant: the one vector all proofs share
    for i in range(len(out[0].w)):  # every other witness vector on its own, not only the list
        if i != g:
            _distinct([hp.w[i] for hp in out], f"witness {i}")
    _distinct([hp.evals(rank - 1) for hp in out], "pf.Evals")
    return out


def swapped_xof(hp, other):
    """`hp` presented with `other`'s XOF bytes: (checkers the reference then uses, the XOF bytes)."""
    return hp.checkers_with_xof(other.xof), other.xof
