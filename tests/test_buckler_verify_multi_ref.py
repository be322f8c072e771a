"""CPU: the proofs tests/buckler_verify_multi_util.py makes for the verifier's batch entry are honest
proofs of one circuit under the restated verifier (tests/buckler_verify_ref.py), and the rejections the
GPU test puts into its mixed batch give the bits it expects -- so the GPU test's expectations are the
reference's, not the device's."""
import functools

import pytest

from tests import buckler_lin_ref as R
from tests import buckler_verify_ref as V
from tests import synth_util as su
from tests.buckler_verify_multi_util import proofs, swapped_xof
from tests.buckler_verify_util import perturbations

RANK = 128
MIXED = ("lin_remlo", "pw0", "eval_point", "sum_mask_sum")  # proofs 1..4 of the GPU test's mixed batch


@functools.lru_cache(maxsize=None)
def _pool(key):
    ref = R.Ref(su.modulus(key))
    return ref, proofs(ref, RANK, 6)


def _verify(ref, hp, jr, evals, ms, pw, ch, checkers=None):
    return V.verify(ref, RANK, jr, hp.wCnt, ch, ms, evals, pw, checkers or hp.checkers, *hp.cons())


@pytest.mark.parametrize("key", ["p63", "jindo_zp"])
def test_every_proof_of_the_circuit_is_accepted(key):
    ref, pool = _pool(key)
    for jr in (RANK - 1, 4 * RANK + 3):
        for hp in pool:
            assert _verify(ref, hp, jr, hp.evals(jr), hp.mask_sums(), hp.pw, hp.chal())[0] == 0


@pytest.mark.parametrize("key", ["p63", "jindo_zp"])
def test_mixed_batch_rejections_give_the_expected_bits(key):
    ref, pool = _pool(key)
    for jr in (RANK - 1, 4 * RANK + 3):
        for hp, name in zip(pool[1:], MIXED):
            evals, ms, pw, ch, bits = perturbations(hp, jr)[name]
            assert _verify(ref, hp, jr, evals, ms, pw, ch)[0] == bits, (name, jr)
        # a proof presented with another proof's XOF bytes: the projection checker's transpose of
        # linCheckVec is another vector, so the linear check's main identity fails and nothing else
        hp = pool[5]
        chk, _ = swapped_xof(hp, pool[0])
        got = _verify(ref, hp, jr, hp.evals(jr), hp.mask_sums(), hp.pw, hp.chal(), chk)
        assert got[0] == V.LIN, (jr, got[0])


def test_proofs_share_the_circuit_and_nothing_else():
    """The helper's own assertions ran; the constraint lists are equal objects across the pool."""
    ref, pool = _pool("p63")
    assert all(hp.cons() == pool[0].cons() for hp in pool)
    assert len({hp.xof for hp in pool}) == len(pool)
