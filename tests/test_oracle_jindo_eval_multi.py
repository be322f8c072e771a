"""CPU: the accumulator-width cases of test_gpu_jindo_eval_multi.py are what they claim to be, before
the GPU test takes the C oracle as its reference on them.

  * "rows21" (syn_d256_q62top with rows = 21, rank = 640) is a shape the ABI promises and the oracle
    accepts, and the oracle's Evaluate on it equals a big-int statement of the same sums;
  * by launch_mac's criterion the sum over a batch of 20 at syn_d256_q62top needs the third accumulator
    word and the sum over its 5 rows does not, and at rows21 with a batch of 2 it is the reverse;
  * the crafted batch case really holds an exact sum of at least 2^128 (the assertion is in
    tests/jindo_eval_multi_util.py), so a two-word accumulator over the batch gives a wrong residue on
    it.  The sum over the rows has no such case: its left factors are fixed by the point, and with 21
    rows sum_j left[j] reaches the 16 q it takes only by luck, so the rows21 runs show that the wide path
    computes what the oracle does, not that a narrow one would fail.

rg_jindo_create builds the ring tables on the device, so its acceptance of rows21 is the first thing
test_gpu_jindo_eval_multi.py's width test does."""
import numpy as np

import coracle as co
import pyref
from tests import jindo_eval_multi_util as eu


def test_rows21_is_a_shape_the_abi_promises():
    P, fq = eu.params("rows21")
    assert P["rows"] == 21 and P["rank"] == 640 == (P["rows"] - 1) * P["cols"] * P["slots"]
    assert P["in_com_dcmp_len"] == (P["cols"] + 1) * P["in_msis"] and P["slots"] * P["exp"] <= P["d"]
    for q in P["q"] + P["qo"]:
        assert pyref.is_prime(q) and (q - 1) % (2 * P["d"]) == 0 and P["base"] < q < 1 << 62
    cj = co.CJindo(P, fq)  # raises where the oracle refuses the set
    assert cj.eval_shapes()["ob_enc"] == (P["cols"] + 1, 21, len(P["q"]), P["d"])


def test_widths_are_the_ones_the_cases_are_for():
    top, _ = eu.params("syn_d256_q62top")
    assert eu.acc_wide(top["q"], 20) and not eu.acc_wide(top["q"], top["rows"])
    r21, _ = eu.params("rows21")
    assert not eu.acc_wide(r21["q"], 2) and eu.acc_wide(r21["q"], r21["rows"])
    assert 20 * (max(top["q"]) - 1) ** 2 >= 1 << 128 > 5 * (max(top["q"]) - 1) ** 2
    assert 21 * (max(r21["q"]) - 1) ** 2 >= 1 << 128 > 2 * (max(r21["q"]) - 1) ** 2


def _bigint_partial(P, left, ob_enc):
    """Partial[i] = sum_j left[j] * openBatch.Encode[i][j] * 2^-64 mod q, in Python ints."""
    out = np.zeros((P["cols"] + 1, len(P["q"]), P["d"]), np.uint64)
    for l, q in enumerate(P["q"]):
        rinv = pow(1 << 64, -1, q)
        s = (left[None, :, l, :].astype(object) * ob_enc[:, :, l, :].astype(object)).sum(axis=1)
        out[:, l, :] = (s * rinv % q).astype(np.uint64)
    return out


def test_oracle_is_exact_on_the_width_cases():
    # crafted_batch asserts its sum of at least 2^128 while the case is made
    for c in (eu.make_case("syn_d256_q62top", 20, seed=5, fill="crafted"), eu.make_case("rows21", 2, seed=6, fill="top")):
        P, o = c["P"], eu.oracle(c)
        for p in range(eu.N):
            assert (o["pf_partial"][p] == _bigint_partial(P, o["left"][p], o["ob_enc"][p])).all(), c["name"]
        # openBatch.Encode of proof 0 at one position per limb (the crafted one where there is one), in Python ints
        for l, k in [c.get("crafted_at", (0, 5)), (len(P["q"]) - 1, P["d"] - 1)]:
            q = P["q"][l]
            want = sum(int(o["bq"][0][t, l, k]) * c["enc"][0, t, :, :, l, k].astype(object) for t in range(c["batch"]))
            assert (o["ob_enc"][0][:, :, l, k] == (want * pow(1 << 64, -1, q) % q).astype(np.uint64)).all(), c["name"]
