"""CPU: the restatement of Uint.SetRandom that the field sampler's GPU tests compare with
(tests/set_random_ref.py over the C oracle's UniformSampler words) does what element.go:299-343
says, and the draws those tests use do take the rejection paths: elements of two, three and more
tries on the whole-word route (q255) and on a byte-serial field whose k is no multiple of 8, where a
retry starts in the middle of a word."""
import pytest

from tests import set_random_ref as sr

FIELDS = sr.FIELDS + ("mult_zp",)


@pytest.mark.parametrize("key", FIELDS)
def test_values_below_q_and_read_from_the_tries_own_bytes(key):
    q = sr.modulus(key)
    k, top = sr.shape(q)
    bitlen = (q - 1).bit_length()
    assert k == (bitlen + 7) // 8 and top == (1 << (bitlen - 8 * (k - 1))) - 1
    for first in sr.FIRSTS:
        n = sr.N
        vals, tries = sr.draws(sr.SEED, q, first, n)
        assert len(vals) == n and all(0 <= v < q for v in vals)
        assert all(v >> bitlen == 0 for v in vals)  # the unused top bits are clear
        for i in range(0, n, 7):  # an element of t tries is bytes [(t - 1) k, t k) of its instance's stream
            t = tries[i]
            raw = bytearray(sr.stream(sr.SEED, first + i, t * k))
            for u in range(t):
                cand = bytearray(raw[u * k:(u + 1) * k])
                cand[-1] &= top
                v = int.from_bytes(cand, "little")
                assert (v == vals[i]) if u == t - 1 else (v >= q), (key, first, i, u)


def test_instances_are_independent_of_the_range_they_are_drawn_in():
    q = sr.modulus(sr.Q255)
    vals, _ = sr.draws(sr.SEED, q, 0, sr.N)
    again, _ = sr.draws(sr.SEED, q, 100, 50)
    assert again == vals[100:150]
    other, _ = sr.draws(b"another seed", q, 100, 50)
    assert other != again


@pytest.mark.parametrize("key", [sr.Q255, "zp110", "zp440"])
def test_census_of_the_tests_draws(key):
    """The draws of the GPU tests (first = 0, n = N): >= 30 elements of two or more tries and >= 5 of
    three or more, on the whole-word route and on byte-serial fields with k % 8 != 0 (14 and 55)."""
    q = sr.modulus(key)
    k, _ = sr.shape(q)
    assert (k % 8 == 0) == (key == sr.Q255)
    _, tries = sr.draws(sr.SEED, q, 0, sr.N)
    assert sum(t >= 2 for t in tries) >= 30 and sum(t >= 3 for t in tries) >= 5, (key, max(tries))


def test_census_of_the_fixup_and_mask_draws():
    """What tests/test_gpu_field_sampler_fixup.py and the sampled mask's cases draw at q255: the first
    600 instances and the instances from 2^32 - 100 on hold elements of one, two and three tries."""
    q = sr.modulus(sr.Q255)
    for first, n in ((0, sr.FIXUP_ELEMS), (2 ** 32 - 100, 3 * 128)):
        _, tries = sr.draws(sr.SEED, q, first, n)
        assert {1, 2, 3} <= set(tries)
        assert sum(t >= 2 for t in tries) >= 30 and sum(t >= 3 for t in tries) >= 5
