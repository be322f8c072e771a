"""Uint.SetRandom (jindo/internal/zp/element.go:299-343) over Python integers, reading from the C
oracle's UniformSampler words (coracle.uniform_words, oracle.c): k = ceil(bitLen(q - 1) / 8) bytes,
the last byte's unused top bits cleared, the candidate rejected while it is >= q.  An instance's
words are one little-endian byte stream, so the bytes a try leaves unread in its last word are the
first bytes of the same instance's next try: try t reads bytes [(t - 1) k, t k).

Shared by the tests of the field sampler (rg_field_sampler_*) and of the sampled mask
(rg_buckler_sumcheck_mask_batch_sampled*): one element is one instance, draws are cached per
(seed, q, first, n) and read-only."""
import functools
import json
import os

import numpy as np

import coracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = bytes(range(7, 39))  # the tests' NewUniformSamplerWithSeed seed
# one field per limb count the kernels are built for; q255 (jindo_zp) and mult_zp take the whole-word
# route (even L, k = 8 L), the others the byte-serial one
Q255 = "jindo_zp"
FIELDS = ("p63", "zp110", Q255, "zp220", "zp440", "zp880")
N = 1500  # not a multiple of 512, more than one workgroup
FIRSTS = (0, 2 ** 32 - 700, 2 ** 40 + 3)
# what tests/exp_child_fsampler.py draws at q255 with the whole-word kernels' tries capped
FIXUP_ELEMS = 600
FIXUP_MASK = dict(rank=128, mask_rank=256, emb=256, n_proofs=2, first=2 ** 32 - 100)


@functools.lru_cache(maxsize=None)
def modulus(key):
    F = json.load(open(os.path.join(ROOT, "tests", "golden", "fields.json")))
    return int(F[key]["q_hex"], 16)


def shape(q):
    """(k bytes, the last byte's mask) of SetRandom at modulus q (element.go:305-318)."""
    bitlen = (q - 1).bit_length()
    bb = bitlen % 8 or 8
    return (bitlen + 7) // 8, (1 << bb) - 1


def stream(seed, inst, nbytes):
    """The first nbytes bytes of instance `inst`'s Sample() stream."""
    return co.uniform_words(seed, inst, 0, (nbytes + 7) // 8).astype("<u8").tobytes()[:nbytes]


def draw(seed, inst, q):
    """SetRandom reading instance `inst` -> (value, tries)."""
    k, top = shape(q)
    have = b""
    t = 0
    while True:
        if len(have) < (t + 1) * k:
            have = stream(seed, inst, (t + 4) * k)
        cand = bytearray(have[t * k:(t + 1) * k])
        cand[-1] &= top
        v = int.from_bytes(cand, "little")
        t += 1
        if v < q:
            return v, t


@functools.lru_cache(maxsize=None)
def draws(seed, q, first, n):
    """Elements of instances first .. first + n - 1 -> (values, tries), two tuples of ints."""
    out = [draw(seed, first + i, q) for i in range(n)]
    return tuple(v for v, _ in out), tuple(t for _, t in out)


def limbs(values, q, L=None):
    """[n][L] uint64: the values' little-endian words, as the device stores them."""
    return co.to_limbs(list(values), L or (q.bit_length() + 63) // 64)
