"""CPU: pins tests/buckler_verify_ref.py, the restatement of buckler/verifier.go:178-315 that the GPU
tests compare against, before the GPU sees it: it accepts the honest proof of
tests/buckler_verify_util.py at two fields and three jindo ranks, its linear check is
buckler_lin_ref.verifierLinCheck (written earlier, separately), and every one-change rejection flips
exactly the bits it should."""
import functools

import pytest

from tests import buckler_lin_ref as R
from tests import buckler_verify_ref as V
from tests import synth_util as su
from tests.buckler_verify_util import HonestProof, perturbations

KEYS = ["p63", "jindo_zp"]
RANK = 128
JINDO_RANKS = [RANK - 1, RANK, 4 * RANK + 3]  # shift exponent 0, 1 and 3 rank + 4


@functools.lru_cache(maxsize=None)
def _proof(key):
    return HonestProof(R.Ref(su.modulus(key)), RANK, seed=len(key), two_pairs=True)


def test_layout_is_the_round_commit_order():
    assert V.layout(5, True, True, True) == dict(linMask=5, sumMask=6, arithQuo=7, linQuo=8, sumQuo=11, n=14)
    assert V.layout(5, True, False, False) == dict(linMask=5, linQuo=6, n=9)
    assert V.layout(5, False, True, False) == dict(arithQuo=5, n=6)
    assert V.layout(5, False, False, True) == dict(sumMask=5, sumQuo=6, n=9)
    assert V.layout(0, True, False, True) == dict(linMask=0, sumMask=1, linQuo=2, sumQuo=5, n=8)


def test_exp_is_a_power():
    ref = R.Ref(su.modulus("p63"))
    x = ref.set_uint64(3)
    assert V.exp(ref, x, 0) == ref.set_uint64(1) and V.exp(ref, 0, 0) == ref.set_uint64(1)
    for e in (1, 2, 5, 388):
        assert ref.plain(V.exp(ref, x, e)) == pow(3, e, ref.q)
        assert V.exp(ref, x, e) == R.mexp(ref, x, e)


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("jindo_rank", JINDO_RANKS)
def test_accepts_the_honest_proof(key, jindo_rank):
    hp = _proof(key)
    ref = hp.ref
    verdict, sides, pw_evals = V.verify(ref, RANK, jindo_rank, hp.wCnt, hp.chal(), hp.mask_sums(), hp.evals(jindo_rank),
                                        hp.pw, hp.checkers, *hp.cons())
    assert verdict == 0
    assert sides[0] == sides[1] and sides[3] == sides[4] and sides[6] == sides[7]
    assert len({sides[0], sides[3], sides[6]}) == 3 and 0 not in sides  # three different, non-trivial identities
    assert pw_evals == [R.evaluate(ref, ref.encode(v, 2 * RANK), hp.x) for v in hp.pw]  # the embedding adds nothing
    # each check alone, in its own layout
    for has in ((True, False, False), (False, True, False), (False, False, True)):
        v1, s1, _ = V.verify(ref, RANK, jindo_rank, hp.wCnt, hp.chal(), hp.mask_sums(), hp.evals(jindo_rank, *has),
                             hp.pw, hp.checkers, *hp.cons(*has))
        assert v1 == 0
        lo = (2, 0, 5)[has.index(True)]
        n = 2 if has[1] else 3
        assert s1[lo:lo + n] == sides[lo:lo + n] and sum(x != 0 for x in s1) == n


@pytest.mark.parametrize("key", KEYS)
def test_lin_check_part_is_verifier_lin_check(key):
    hp = _proof(key)
    ref = hp.ref
    jr = 4 * RANK + 3
    ix = V.layout(hp.wCnt, True, True, True)
    for name in ("honest", "lin_remhi", "lin_quo", "lin_remlo", "lin_mask_sum", "shared_witness"):
        evals, ms, pw, ch, _ = perturbations(hp, jr)[name] if name != "honest" else (
            hp.evals(jr), hp.mask_sums(), hp.pw, hp.chal(), 0)
        verdict, _, _ = V.verify(ref, RANK, jr, hp.wCnt, ch, ms, evals, pw, hp.checkers, *hp.cons())
        i = ix["linQuo"]
        hi_ok, main_ok = R.verifierLinCheck(ref, RANK, hp.emb, jr, ch[2], ch[3], evals[ix["linMask"]], ch[0], ms[0],
                                            evals[i], evals[i + 1], evals[i + 2], hp.checkers, hp.lin, evals)
        assert (not verdict & V.LIN_REM, not verdict & V.LIN) == (hi_ok, main_ok), name


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("jindo_rank", [RANK - 1, 4 * RANK + 3])
def test_each_rejection_flips_its_bits(key, jindo_rank):
    hp = _proof(key)
    for name, (evals, ms, pw, ch, bits) in perturbations(hp, jindo_rank).items():
        verdict, _, _ = V.verify(hp.ref, RANK, jindo_rank, hp.wCnt, ch, ms, evals, pw, hp.checkers, *hp.cons())
        assert verdict == bits, (name, verdict, bits)
