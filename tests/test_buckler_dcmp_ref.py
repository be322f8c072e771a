"""CPU: pins tests/buckler_dcmp_ref.py (the restatement of buckler/utils.go:34-56 and
buckler/prover.go:77-111, 182-192 the GPU parity tests compare with) by algebra, not by the same
loop: the digits are ternary, they recompose to the centred value exactly when it lies within the
sum of the base, the residual beyond that is what is left over, and sqNm is the sum of squares in
Python integers.  Also the host-only parts of the mirror (ringo.buckler.decomposeBig, TwoNormPublic)."""
import numpy as np
import pytest

import ringo
from ringo import buckler
from tests import buckler_dcmp_ref as D
from tests import buckler_lin_ref as R
from tests.buckler_lin_util import rand_ints

BOUNDS = list(range(1, 300)) + [1000, 1023, 1024, 1025, 65536, 65537, (1 << 20) - 1]


def base_of(bound):
    """decomposeBase(1) indexes an empty slice in the reference (a panic); its base is taken as [1]."""
    return [1] if bound == 1 else D.decomposeBase(bound)


def _centred_values(S, rng):
    """Centred values around every edge of [-S, S], and all of them when the range is small."""
    if S <= 700:
        return list(range(-S - 4, S + 5))
    vals = {0, 1, -1, S, -S, S + 1, -S - 1, S - 1, 1 - S, S + 2, -S - 2, 2 * S, -2 * S, 3 * S + 1}
    vals.update(int(v) for v in rng.integers(-S - 50, S + 51, size=400))
    return sorted(vals)


def test_decompose_base_of_8_sums_to_7():
    assert D.decomposeBase(8) == [4, 2, 1] and sum(D.decomposeBase(8)) == 7
    assert D.decomposeBase(2) == [1] and D.decomposeBase(3) == [2, 1]


@pytest.mark.parametrize("q", [(1 << 61) - 1, (1 << 127) - 1], ids=["q61", "q127"])
def test_digits_recompose_iff_within_sum_of_base(q):
    rng = np.random.default_rng(11)
    for bound in BOUNDS:
        base = base_of(bound)
        S = sum(base)
        assert all(b >= 1 for b in base)
        for xs in _centred_values(S, rng):
            x = xs % q
            d = D.decomposeBig(x, base, q)
            assert len(d) == len(base) and set(d) <= {-1, 0, 1}, (bound, xs)
            rec = sum(dj * bj for dj, bj in zip(d, base))
            if abs(xs) <= S:
                assert rec == xs, (bound, xs)
            else:
                assert rec != xs, (bound, xs)
            assert D.residual(x, base, q) == xs - rec
            # the digits all carry the sign of the value: the sign-magnitude form of the core
            assert all(dj == 0 or (dj > 0) == (xs > 0) for dj in d), (bound, xs)


def test_centring_edges():
    q = 97
    base = D.decomposeBase(q - 1)
    assert D.decomposeBig(q >> 1, base, q)[0] == 1       # 48 stays positive
    assert D.decomposeBig((q >> 1) + 1, base, q)[0] == -1  # 49 stands for -48
    assert D.decomposeBig(0, base, q) == [0] * len(base)
    assert sum(d * b for d, b in zip(D.decomposeBig(q - 1, base, q), base)) == -1


def test_mirror_decompose_big_is_the_restatement():
    rng = np.random.default_rng(3)
    q = (1 << 61) - 1
    for bound in (2, 3, 8, 10, 1000, (1 << 20) - 1, q - 1):
        base = base_of(bound)
        for x in [0, 1, q - 1, q >> 1, (q >> 1) + 1] + rand_ints(q, 200, rng) + [int(v) for v in
                                                                                 rng.integers(0, 2 * bound, size=50)]:
            assert buckler.decomposeBig(x % q, base, q) == D.decomposeBig(x % q, base, q)


@pytest.fixture(scope="module")
def ctx(fields):
    q = fields["p63"]
    return ringo.Field(q), R.Ref(q)


def test_inf_and_proj_restatement_layouts(ctx):
    _, ref = ctx
    q = ref.q
    rng = np.random.default_rng(5)
    base = D.decomposeBase(1000)
    S = sum(base)
    plain = [int(v) % q for v in rng.integers(-S, S + 1, size=130)]
    w = [p * ref.R % q for p in plain]
    dig = D.infDcmp(ref, w, base)
    assert len(dig) == len(base) and all(len(v) == len(w) for v in dig)
    one, neg = ref.R % q, (q - ref.R) % q
    for i, p in enumerate(plain):
        ds = [{0: 0, one: 1, neg: -1}[dig[j][i]] for j in range(len(base))]
        assert sum(d * b for d, b in zip(ds, base)) % q == p
    rank = 128 * len(base) + 5
    pr = D.projDcmp(ref, w, base, rank)
    assert len(pr) == rank and pr[128 * len(base):] == [0] * 5
    for i in range(128):
        assert pr[i * len(base):(i + 1) * len(base)] == [dig[j][i] for j in range(len(base))]


def test_two_norm_sum_of_squares(ctx):
    _, ref = ctx
    q = ref.q
    rng = np.random.default_rng(9)
    base = D.decomposeBase(q - 1)
    for w_plain in ([q - 1] * 200, [q >> 1] * 7, rand_ints(q, 300, rng), [3, 4], [0] * 64 + [q - 2]):
        rank = max(len(w_plain), len(base))
        w_plain = w_plain + [0] * (rank - len(w_plain))
        w = [p * ref.R % q for p in w_plain]
        wDcmp, sqNm = D.twoDcmp(ref, w, base)
        assert sqNm == sum(p * p for p in w_plain) % q
        centred = [p - q if p > (q >> 1) else p for p in w_plain]
        assert sqNm == sum(c * c for c in centred) % q
        assert len(wDcmp) == rank and wDcmp[len(base):] == [0] * (rank - len(base))
        assert wDcmp[:len(base)] == [D.set_int64(ref, d) for d in D.decomposeBig(sqNm, base, q)]
    # all q - 1: every square is 1, the sum is the rank
    assert D.twoDcmp(ref, [(q - 1) * ref.R % q] * 200, D.decomposeBase(1000))[1] == 200


def test_two_norm_public_witnesses(ctx):
    F, ref = ctx
    for bound, rank in ((8, 4), (1000, 16), ((1 << 20) - 1, 64)):
        base = D.decomposeBase(bound)
        pwBase, pwMask = buckler.TwoNormPublic(F, rank, bound)
        wantBase, wantMask = D.twoNormPublic(ref, rank, base)
        assert (pwBase == ref.arr(wantBase)).all() and (pwMask == ref.arr(wantMask)).all()
    with pytest.raises(ringo.RingoPanic):
        buckler.TwoNormPublic(F, 2, 1000)
