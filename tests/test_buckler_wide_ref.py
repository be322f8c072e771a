"""CPU: pins tests/buckler_wide_util.py, the builders of the circuits wider than verify_decide_kernel's
256 lanes, so that the GPU tests on them (test_gpu_buckler_verify_wide.py) cannot pass vacuously: the
honest 257-pair linear check is accepted by the restatement, a forged proof of every wide circuit is
accepted and each of its one-change rejections flips exactly its bits, and the circuits have the
shapes they promise."""
import functools

import numpy as np
import pytest

from tests import buckler_lin_ref as R
from tests import buckler_verify_ref as V
from tests import buckler_wide_util as W
from tests import synth_util as su

RANK = 128
NOSPARE = sorted(k for k, v in su.SYNTH.items() if v["bits"] == 64 * v["limbs"] and v["limbs"] in (1, 2, 4, 7, 14))


@functools.lru_cache(maxsize=None)
def _ref(key):
    return R.Ref(su.modulus(key))


@pytest.mark.parametrize("key", W.HONEST_FIELDS)
def test_honest_257_pairs_are_accepted(key):
    """R.linCheck on 257 honest pairs over six checkers, two of them empty: rem[0] is the mask sum and
    V.decide accepts at every jindo rank; each rejection flips its bits."""
    ref = _ref(key)
    hp = W.honest_lin_proof(ref)
    assert [len(p) for p in hp.lin] == W.HONEST_PAIRS and sum(W.HONEST_PAIRS) == 257 and hp.wCnt == 514
    assert hp.rem[0] == hp.linMaskSum
    own = V.own_evals(ref, RANK, hp.x, hp.lc, hp.checkers, [])
    for jr in (RANK - 1, RANK, 4 * RANK + 3):
        verdict, sides = V.decide(ref, RANK, jr, hp.wCnt, hp.chal(), hp.mask_sums(), hp.evals(jr), own, hp.lin, None,
                                  None)
        assert verdict == 0 and sides[3] == sides[4] != 0 and sides[:2] == [0, 0] and sides[5:] == [0, 0, 0]
    jr = 4 * RANK + 3
    rej = hp.perturbations(jr)
    assert set(rej) == {"lin_quo", "lin_remlo", "last_pair_witness"}
    assert hp.lin[5][0][1] == 513  # the bumped witness is the wIn of pair 256
    for name, (evals, bits) in rej.items():
        verdict, _ = V.decide(ref, RANK, jr, hp.wCnt, hp.chal(), hp.mask_sums(), evals, own, hp.lin, None, None)
        assert verdict == bits, (name, verdict, bits)


def _accepts_and_rejects(wc, jrs):
    own = wc.own()
    for jr in jrs:
        evals, ms, rej = wc.forge(jr, own)
        verdict, sides = wc.decide(jr, own, evals, ms)
        assert verdict == 0
        if wc.has[1]:
            assert sides[0] == sides[1]
        if wc.has[0]:
            assert evals[V.layout(wc.wCnt, *wc.has)["linQuo"] + 2] == sides[2] and sides[3] == sides[4]
        if wc.has[2]:
            assert sides[6] == sides[7]
        want = {"arith_quo"} if wc.has[1] else set()
        if wc.has[0]:
            want |= {"lin_remhi", "lin_quo", "lin_remlo", "lin_mask_sum"}
        if wc.has[2]:
            want |= {"sum_remhi", "sum_quo", "sum_remlo", "sum_mask_sum"}
        want |= {"shared_witness"} & set(rej)  # where all three checks read one witness
        assert set(rej) == want
        for name, (e, m, bits) in rej.items():
            assert wc.decide(jr, own, e, m)[0] == bits, (name, jr)
    return own


@pytest.mark.parametrize("key", W.WIDE_FIELDS + NOSPARE[:1])
def test_forged_wide_circuit(key):
    """The 570-constraint, 600-pair circuit: forged evals are accepted, unforged ones fail every check."""
    ref = _ref(key)
    wc = W.wide_circuit(ref)
    own = _accepts_and_rejects(wc, (RANK - 1, 4 * RANK + 3))
    n = V.layout(wc.wCnt, True, True, True)["n"]
    assert n == W.W_CNT + 9
    rnd = W.rand_ints(ref.q, n + 2, np.random.default_rng(5))
    all_bits = V.ARITH | V.LIN_REM | V.LIN | V.SUM_REM | V.SUM
    assert wc.decide(4 * RANK + 3, own, rnd[:n], rnd[n:])[0] == all_bits
    # the planted values are there, and the forged proof reads them
    evals, _, rej = wc.forge(RANK - 1, own)
    assert "shared_witness" in rej
    assert {0, ref.set_uint64(1), ref.q - 1} <= set(evals[:wc.wCnt])
    # another proof of the same circuit: the same program, other inputs
    other = W.wide_circuit(ref, proof_seed=1)
    assert other.cons() == wc.cons() and other.chal() != wc.chal() and other.pw != wc.pw and other.xof != wc.xof


def test_wide_circuit_shape():
    """Both lists pass 256 constraints, together 512; the pairs pass 512; two checkers are empty; the
    public witnesses' words pass 256 and are no multiple of it -- for every limb count."""
    ref = _ref("p63")
    wc = W.wide_circuit(ref)
    W.assert_wide_shape(wc)
    for L, n_pw in ((1, 300), (2, 150), (4, 75), (7, 43), (14, 40)):
        assert W.n_pw_for(L) == n_pw
    for cons, n in ((wc.arith, W.NC0), (wc.sum, W.NC1)):
        s = W.shape(cons)
        assert s["n"] == n and s["empty"][0] == 0 and s["empty"][-1] == n - 1 and n // 2 in s["empty"]
        assert s["max_terms"] == W.MAX_TERMS and s["max_wits"] == W.MAX_WITNESSES
        assert s["pw_term0"] and s["pw_alone"] and cons[1][0][1] == 0 and cons[2][0][1] == wc.nPw - 1
        assert 0.2 < s["pw_terms"] / s["terms"] < 0.45  # "about a third"
        assert {0, W.mont_one(ref.q), ref.q - 1} <= s["coeffs"]
        assert max(w for c in cons for t in c for w in t[2]) < wc.wCnt
        assert len({t[1] for c in cons for t in c if t[1] is not None}) > 100  # most public witnesses are read
    assert W.mont_one(ref.q) == ref.set_uint64(1)
    assert W.mont_one(su.modulus("zp880")) == _ref("zp880").set_uint64(1)


@pytest.mark.parametrize("key", W.BOUNDARY_FIELDS)
def test_forged_boundary_circuits(key):
    """Every (constraint split, pair layout) of the trip-boundary cases is accepted when forged."""
    ref = _ref(key)
    for split in W.SPLITS:
        for npairs in W.BOUNDARY_PAIRS:
            _accepts_and_rejects(W.boundary_circuit(ref, split, npairs), (4 * RANK + 3,))


def test_boundary_shapes():
    """The pair layouts put a checker's first pair on lane 64 and on lane 0's second trip, with and
    without that pair being there; one has an empty first and an empty last checker."""
    assert sorted(sum(p) for p in W.BOUNDARY_PAIRS) == [64, 65, 256, 257]
    by_n = {sum(p): W.lanes_of_pairs(p) for p in W.BOUNDARY_PAIRS}
    assert [by_n[n]["lane64"] for n in (64, 65, 256, 257)] == [False, True, True, True]
    assert [by_n[n]["second_trip"] for n in (64, 65, 256, 257)] == [False, False, False, True]
    assert all(64 in by_n[n]["starts"] for n in (65, 256, 257)) and 256 in by_n[257]["starts"]
    assert all(by_n[n]["empty"] for n in by_n)
    assert any(p[0] == 0 and p[-1] == 0 for p in W.BOUNDARY_PAIRS)
    assert sorted((a, b) for a, b in W.SPLITS) == [(1, 255), (256, None), (257, 0)]
    ref = _ref("p63")
    wc = W.boundary_circuit(ref, (1, 255), W.BOUNDARY_PAIRS[0])
    assert (len(wc.arith), len(wc.sum)) == (1, 255) and wc.arith[0][0][1] == 0  # the one constraint reads pw0 first
    wc = W.boundary_circuit(ref, (256, None), W.BOUNDARY_PAIRS[0])
    assert len(wc.arith) == 256 and wc.sum is None and wc.has == (True, True, False)
    wc = W.boundary_circuit(ref, (257, 0), W.BOUNDARY_PAIRS[0])
    assert len(wc.arith) == 257 and wc.sum == []


@pytest.mark.parametrize("key", ["p63"] + NOSPARE)
def test_saturated_circuit(key):
    """256 and 511 constants q - 1: the arithmetic list's sum is 256 (q - 1) and the sum list's
    511 (q - 1), whatever the evals; forged evals are accepted."""
    ref = _ref(key)
    q = ref.q
    wc = W.saturated_circuit(ref)
    assert wc.has == (False, True, True) and wc.nPw == 0
    assert wc.arith == [[(q - 1, None, [])]] * 256 and wc.sum == [[(q - 1, None, [])]] * 511
    own = _accepts_and_rejects(wc, (4 * RANK + 3,))
    n = V.layout(wc.wCnt, *wc.has)["n"]
    verdict, sides = wc.decide(4 * RANK + 3, own, [q - 1] * n, [q - 1] * 2)
    bcA, bcS = wc.chal()[1], wc.chal()[4]
    assert sides[0] == ref.mul(256 * (q - 1) % q, bcA)
    assert sides[6] == (ref.mul(ref.mul(511 * (q - 1) % q, bcS), bcS) + q - 1) % q
    assert verdict == V.ARITH | V.SUM_REM | V.SUM
