"""Shared by test_gpu_buckler_proj_round.py and test_gpu_buckler_mask_batch.py: the fields, the five
proofs of a projection-round case and the restatement's answer for each, built from what the
repository already trusts -- buckler_lin_ref.ProjChecker (linear.go:94-137 with prover.go:168-176),
buckler_dcmp_ref.projDcmp (prover.go:182-192) and buckler_lin_ref.sumCheckMask (prover.go:381-397),
imported as they are.  Everything is computed once per key and shared read-only among the tests."""
import functools

import numpy as np

from tests import buckler_dcmp_ref as D
from tests import buckler_lin_ref as R
from tests import synth_util as su
from tests.buckler_lin_util import rand_ints
from tests.buckler_prove_util import ctx  # (ringo.Field, R.Ref) per key  # noqa: F401

GOLD = ["p63", "mult_zp", "jindo_zp", "zp440", "zp880"]  # one golden field per limb count 1, 2, 4, 7, 14
NOSPARE = sorted(k for k, v in su.SYNTH.items() if v["bits"] == 64 * v["limbs"] and v["limbs"] in (1, 2, 4, 7, 14))
# one modulus without a spare top bit per supported limb count, as test_gpu_buckler_prove_multi.py has it
NOSPARE_PER_L = [next(k for k in NOSPARE if su.SYNTH[k]["limbs"] == L) for L in
                 sorted({su.SYNTH[k]["limbs"] for k in NOSPARE})]
FIELDS = GOLD + NOSPARE_PER_L

# the bases by their length: [1], decomposeBase(3) = [2, 1], decomposeBase(8) = [4, 2, 1]
BASES = {1: (1,), 2: tuple(R.decomposeBase(3)), 3: tuple(R.decomposeBase(8))}
# (rank, nb): one chunk and no zero tail in proj; a partial chunk and both zero tails; 128 nb = rank, no
# digit tail; eight chunks = two workgroups of columns
SHAPES = [(128, 1), (200, 1), (256, 2), (1024, 3)]
N_PROOFS = 5


@functools.lru_cache(maxsize=None)
def proofs(key, rank, nb):
    """The five proofs of a case, every one with its own witness and its own XOF bytes:
      0  small signed entries (plain 0, 1, q - 1, q - bound, bound = the sum of the base), random XOF
         bytes: the projected sums take both signs
      1  the zero vector, random XOF bytes
      2  small signed entries, XOF bytes all 0xFF: the matrix is all false and proj = 0
      3  small signed entries, XOF bytes all 0x00: every row is the sum of v
      4  every entry bound + 1, random XOF bytes: every projection exceeds the sum of the base (the
         residual case, which is not an error)
    Each is (v as Montgomery ints, the XOF bytes)."""
    _, ref = ctx(key)
    q, S = ref.q, sum(BASES[nb])
    rng = np.random.default_rng(97 * rank + nb)

    def small():
        pick = rng.choice(4, size=rank, p=[0.9, 0.04, 0.04, 0.02])
        return [(0, 1, q - 1, q - S)[i] * ref.R % q for i in pick]

    return ((small(), rng.bytes(32 * rank)), ([0] * rank, rng.bytes(32 * rank)), (small(), b"\xff" * (32 * rank)),
            (small(), bytes(32 * rank)), ([(S + 1) * ref.R % q] * rank, rng.bytes(32 * rank)))


@functools.lru_cache(maxsize=None)
def projected(key, rank, nb, i):
    """TransformTo of proof i's witness under its own matrix, as Montgomery ints [rank]."""
    _, ref = ctx(key)
    v, xof = proofs(key, rank, nb)[i]
    return tuple(R.ProjChecker(ref, rank).set_xof(xof).transform(list(v)))


@functools.lru_cache(maxsize=None)
def want(key, rank, nb, i, base_nb=None):
    """(proj, dcmp) rows [rank][L] of proof i; base_nb: decompose with another base than the case's."""
    _, ref = ctx(key)
    proj = list(projected(key, rank, nb, i))
    dcmp = D.projDcmp(ref, proj, list(BASES[base_nb or nb]), rank)
    return ref.arr(proj), ref.arr(dcmp)


def digit_census(key):
    """Over every shape and proof of `key`: the set of digits the reference emits and the number of
    projected values that leave a residual."""
    _, ref = ctx(key)
    digits, residuals = set(), 0
    for rank, nb in SHAPES:
        base = list(BASES[nb])
        for i in range(N_PROOFS):
            for x in projected(key, rank, nb, i)[:128]:
                p = ref.plain(x)
                digits.update(D.decomposeBig(p, base, ref.q))
                residuals += D.residual(p, base, ref.q) != 0
    return digits, residuals


def table(key, rank, n_w, rows, seed):
    """One proof's witness table [n_w][rank][L]: rows = {index: Montgomery ints}, every other row seeded
    random residues."""
    _, ref = ctx(key)
    t = su.rand_residues(ref.q, ref.L, n_w * rank, np.random.default_rng(seed)).reshape(n_w, rank, ref.L)
    for k, v in rows.items():
        t[k] = ref.arr(v)
    return t


@functools.lru_cache(maxsize=None)
def mask_case(key, rank, mask_rank, emb, i):
    """Proof i's draws [mask_rank][L] and the restatement's (mask [emb][L], maskSum [L])."""
    _, ref = ctx(key)
    rand = rand_ints(ref.q, mask_rank, np.random.default_rng(13 * rank + 7 * mask_rank + i))
    mask, msum = R.sumCheckMask(ref, rank, mask_rank, emb, rand)
    return ref.arr(rand), ref.arr(mask), ref.arr([msum])[0]
