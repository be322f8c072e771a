"""CPU: pins tests/buckler_lin_ref.py, the restatement of buckler/linear.go, utils.go:7-32 and
prover.go:381-485 that the GPU tests compare against -- by properties the reference's own
verifier relies on, with no GPU: the decomposition bases, adjointness of every checker's
TransformTo / TransposeTo, and completeness of linCheck (verifier.go:249-294)."""
import numpy as np
import pytest

from tests import buckler_lin_ref as R
from tests.buckler_lin_util import completeness_circuit, rand_ints, xof_bytes
from ringo import buckler

KEYS = ["p63", "jindo_zp"]
RANK, EMB, JINDO_RANK = 128, 512, 1024


def test_decompose_base_worked_examples():
    # utils.go by hand: 8 = 2^3 drops one digit: 8 -> 4, 4 -> 2, then the closing 1;
    # 10: 10 -> 5, 5 -> 3, 2 -> 1, then the closing 1
    assert R.decomposeBase(8) == [4, 2, 1]
    assert R.decomposeBase(10) == [5, 3, 1, 1]
    # The base sums to its bound; a power of two 2^k loses one digit (utils.go:11-13) and gets
    # 2^(k-1), ..., 2, 1, which sum to 2^k - 1 (the worked [4, 2, 1] above).
    for bound in list(range(2, 70)) + [1 << 20, (1 << 20) + 1, (1 << 61) - 1, 3 ** 50]:
        base = R.decomposeBase(bound)
        pow2 = bound & (bound - 1) == 0
        assert sum(base) == bound - (1 if pow2 else 0), bound
        assert base[-1] == 1 and all(a >= b for a, b in zip(base, base[1:])), bound
        assert buckler.decomposeBase(bound) == base, bound  # the mirror's host restatement


def _dot(ref, a, b):
    return sum(ref.mul(x, y) for x, y in zip(a, b)) % ref.q


def _checkers(ref, rng):
    out = [("ntt", R.NTTChecker(ref, RANK)), ("aut coeff", R.AutChecker(ref, RANK, 5, False)),
           ("aut ntt", R.AutChecker(ref, RANK, 2 * RANK - 3, True)),
           ("proj", R.ProjChecker(ref, RANK).set_xof(xof_bytes("random", RANK, rng)))]
    for nb in (1, 3, 7):
        out.append((f"recompose nb={nb}", R.RecomposeChecker(ref, RANK, rand_ints(ref.q, nb, rng))))
    return out


@pytest.mark.parametrize("key", KEYS)
def test_transform_and_transpose_are_adjoint(fields, key):
    ref = R.Ref(fields[key])
    rng = np.random.default_rng(11)
    for name, chk in _checkers(ref, rng):
        v, u = rand_ints(ref.q, RANK, rng), rand_ints(ref.q, RANK, rng)
        assert _dot(ref, chk.transform(v), u) == _dot(ref, v, chk.transpose(u)), name


def test_proj_bit_order():
    """Entry (i, j) is true iff bit i % 8 of byte i / 8 of column j is 0 (prover.go:173-175)."""
    ref = R.Ref((1 << 61) - 1)
    chk = R.ProjChecker(ref, RANK).set_xof(xof_bytes("rows_0_127", RANK, None))
    for j in (0, 77):
        assert [i for i in range(128) if chk.proj[i][j]] == [0, 127]


def test_sum_check_mask_loop():
    ref = R.Ref((1 << 61) - 1)
    r = list(range(1, 301))
    mask, s = R.sumCheckMask(ref, 128, 300, 512, r)
    assert s == 1 and mask[0] == (1 - 129) % ref.q and mask[44] == (45 - 173) % ref.q
    assert mask[171] == (172 - 300) % ref.q and mask[172] == 173  # k + rank < maskRank ends at k = 171
    assert mask[299] == 300 and mask[300:] == [0] * 212


def _prove_and_verify(ref, circ, seed):
    rng = np.random.default_rng(seed)
    mask, maskSum = R.sumCheckMask(ref, RANK, 2 * RANK, EMB, circ["rand"])
    quo, remLo, remHi, remPoly = R.linCheck(ref, RANK, EMB, JINDO_RANK, circ["bc"], circ["lc"], mask, circ["checkers"],
                                            circ["constraints"], circ["wEcdNTT"])
    x = rand_ints(ref.q, 1, rng)[0]
    evals = [R.evaluate(ref, p, x) for p in circ["wEcd"]]
    hi_ok, main_ok = R.verifierLinCheck(ref, RANK, EMB, JINDO_RANK, circ["bc"], circ["lc"], R.evaluate(ref, mask, x),
                                        x, maskSum, R.evaluate(ref, quo, x), R.evaluate(ref, remLo, x),
                                        R.evaluate(ref, remHi, x), circ["checkers"], circ["constraints"], evals)
    return remPoly[0] == maskSum, hi_ok, main_ok


@pytest.mark.parametrize("key", KEYS)
def test_lin_check_completeness(fields, key):
    """wOut = M wIn for every constraint: the remainder's constant term is linCheckMaskSum and the
    verifier's equations eval(x) = quo(x) (x^rank - 1) + x remLo(x) + maskSum and
    remHi(x) = x^(jindoRank - rank + 1) remLo(x) hold at a random point; one perturbed wOut
    coefficient breaks the first."""
    ref = R.Ref(fields[key])
    good = completeness_circuit(ref, RANK, EMB, seed=21)
    assert _prove_and_verify(ref, good, 22) == (True, True, True)
    bad = completeness_circuit(ref, RANK, EMB, seed=21, perturb=True)
    rem0_ok, hi_ok, main_ok = _prove_and_verify(ref, bad, 22)
    assert hi_ok and not rem0_ok and not main_ok
