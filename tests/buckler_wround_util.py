"""Shared by test_buckler_wround_cases.py, test_gpu_buckler_wround_dcmp.py, test_gpu_buckler_wround_encode.py
and test_gpu_buckler_wround_chain.py: the fields, the five proofs of a case and the expected tables of the
prover's two witness rounds, built from what the repository already trusts -- buckler_dcmp_ref.infDcmp /
twoDcmp (prover.go:77-111) and the oracle's Encode (coracle.CField.buckler_encode, encoder.go:32-54),
imported as they are.  Everything is computed once per key and shared read-only among the tests."""
import functools

import numpy as np

from tests import buckler_dcmp_ref as D
from tests import buckler_lin_ref as R
from tests import synth_util as su
from tests.buckler_proj_util import FIELDS, ctx  # noqa: F401

FF = np.uint64(2 ** 64 - 1)
N_PROOFS = 5
BATCHES = ((0,), (2, 3, 4), (0, 1, 2, 3, 4))  # 1, 3 and 5 proofs; the batch of 5 holds all five kinds

# ---- the decomposition round -------------------------------------------------------------------------
# the bases by their length: [1], decomposeBase(3) = [2, 1], decomposeBase(8) = [4, 2, 1]; 300: a base of
# more than 256 digits, whose walk in the final kernel crosses a workgroup
BASES = {1: (1,), 2: tuple(R.decomposeBase(3)), 3: tuple(R.decomposeBase(8)), 300: tuple(R.decomposeBase(1 << 300))}
BOUND = 7  # the sum of the largest short base: `bound + 1` lies beyond every short base
# rank 200: no multiple of 256 and a partial chunk of the sum of squares; 1024: exactly one chunk; 2500:
# three chunks with the last partial
RANKS = (200, 1024, 2500)
# name -> (n_w, inf [(src, nb, rows)], two [(src, nb, dst)]); every table keeps at least one bystander row
TABLES = {
    "shared_src": (7, ((1, 3, (4, 5, 6)),), ((1, 2, 0),)),          # rows 2, 3 stand by
    "two_inf": (8, ((0, 1, (5,)), (2, 3, (7, 1, 4))), ()),          # different nb, rows neither consecutive nor ordered
    "only_two": (5, (), ((1, 1, 3), (4, 3, 0))),
    "only_inf": (4, ((2, 2, (0, 1)),), ()),
    "long_base": (3, (), ((0, 300, 2),)),                            # zp440, zp880 at ranks >= 300 only
}
LONG_KEYS = ("zp440", "zp880")


def tables_of(key, rank):
    return [t for t in TABLES if t != "long_base" or (key in LONG_KEYS and rank >= 300)]


def srcs_of(table):
    _, inf, two = TABLES[table]
    return sorted({c[0] for c in inf} | {c[0] for c in two})


def outs_of(table):
    _, inf, two = TABLES[table]
    return sorted([r for c in inf for r in c[2]] + [c[2] for c in two])


@functools.lru_cache(maxsize=None)
def witness(key, rank, i, row):
    """Witness `row` of proof i as Montgomery ints [rank].  The five proofs are of five kinds:
      0  small signed entries (plain 0, 1, q - 1, BOUND, q - BOUND, 3, q - 2)
      1  the zero vector (its two-norm sum is 0)
      2  all q - 1 (plain -1: every square is 1, the sum is the rank)
      3  every entry BOUND + 1: beyond the sum of every short base (the residual, which is no error)
      4  random full-width entries (the two-norm sum is a random residue: above q / 2 for about half)"""
    _, ref = ctx(key)
    q = ref.q
    rng = np.random.default_rng(7919 * rank + 31 * i + row)
    if i == 0:
        vals = (0, 1, q - 1, BOUND, q - BOUND, 3, q - 2)
        return tuple(vals[k] * ref.R % q for k in rng.choice(7, size=rank, p=[0.7, 0.06, 0.06, 0.04, 0.04, 0.05, 0.05]))
    if i == 1:
        return (0,) * rank
    if i == 2:
        return ((q - 1) * ref.R % q,) * rank
    if i == 3:
        return ((BOUND + 1) * ref.R % q,) * rank
    return tuple(ref.ints(su.rand_residues(q, ref.L, rank, rng)))


@functools.lru_cache(maxsize=None)
def _digit_rows(key):
    """The three digit elements SetInt64 makes, as limb rows, by their Montgomery int."""
    _, ref = ctx(key)
    return {D.set_int64(ref, d): ref.arr([D.set_int64(ref, d)])[0] for d in (-1, 0, 1)}


def _arr(key, ints):
    """ref.arr for a digit witness: only three values occur."""
    lut = _digit_rows(key)
    return np.stack([lut[x] for x in ints])


@functools.lru_cache(maxsize=None)
def inf_want(key, rank, i, src, nb):
    """The nb digit witnesses [nb][rank][L] of witness src of proof i (prover.go:77-86)."""
    _, ref = ctx(key)
    return np.stack([_arr(key, d) for d in D.infDcmp(ref, list(witness(key, rank, i, src)), list(BASES[nb]))])


@functools.lru_cache(maxsize=None)
def two_want(key, rank, i, src, nb):
    """(row dst [rank][L], sqNm [L] in Montgomery form, sqNm as a plain int) of witness src of proof i."""
    _, ref = ctx(key)
    wDcmp, sq = D.twoDcmp(ref, list(witness(key, rank, i, src)), list(BASES[nb]))
    return _arr(key, wDcmp), ref.arr([sq * ref.R % ref.q])[0], sq


def dcmp_table(key, rank, table, i):
    """Proof i's plain table [n_w][rank][L] before the round: the src rows, the output rows -1, random
    words in the bystanders (never read, so they need not be residues)."""
    _, ref = ctx(key)
    n_w = TABLES[table][0]
    t = np.random.default_rng(1000 * rank + i).integers(0, 1 << 64, size=(n_w, rank, ref.L), dtype=np.uint64)
    for s in srcs_of(table):
        t[s] = ref.arr(witness(key, rank, i, s))
    for o in outs_of(table):
        t[o] = FF
    return t


def dcmp_expect(key, rank, table, i, before):
    """(the table after the round, sq [n_two][L]) of proof i."""
    _, inf, two = TABLES[table]
    want = before.copy()
    for src, nb, rows in inf:
        digits = inf_want(key, rank, i, src, nb)
        for j, r in enumerate(rows):
            want[r] = digits[j]
    sq = np.zeros((len(two), before.shape[-1]), np.uint64)
    for c, (src, nb, dst) in enumerate(two):
        want[dst], sq[c], _ = two_want(key, rank, i, src, nb)
    return want, sq


def dcmp_census(key):
    """Over every rank, table and proof of `key`, on the reference's output: the digits of the
    infinity-norm constraints, the number of coefficients that leave a residual, the digits of the
    two-norm constraints, and the two-norm sums."""
    _, ref = ctx(key)
    inf_digits, residuals, two_digits, sums = set(), 0, set(), []
    for rank in RANKS:
        for table in tables_of(key, rank):
            _, inf, two = TABLES[table]
            for i in range(N_PROOFS):
                for src, nb, _ in inf:
                    base = list(BASES[nb])
                    for x in sorted(set(witness(key, rank, i, src))):
                        p = ref.plain(x)
                        inf_digits.update(D.decomposeBig(p, base, ref.q))
                        residuals += D.residual(p, base, ref.q) != 0
                for src, nb, _ in two:
                    sq = two_want(key, rank, i, src, nb)[2]
                    sums.append(sq)
                    two_digits.update(D.decomposeBig(sq, list(BASES[nb]), ref.q))
    return inf_digits, residuals, two_digits, sums


# ---- the encode round ------------------------------------------------------------------------------------
ENC_RANKS = (64, 128, 1024)  # with embedding ranks 2 rank and 4 rank
# name -> (n_w, sel): the identity (no gather), a subset out of order, one row
SELS = {"identity": (3, (0, 1, 2)), "subset": (5, (3, 0)), "one_row": (4, (2,))}


@functools.lru_cache(maxsize=None)
def enc_row(key, rank, i, row):
    """Plain row `row` of proof i as limbs [rank][L]: the kinds of `witness`."""
    _, ref = ctx(key)
    return ref.arr(witness(key, rank, i, 100 + row))


@functools.lru_cache(maxsize=None)
def enc_draw(key, rank, i, row):
    """The MustSetRandom draw of row `row` of proof i, [L]."""
    _, ref = ctx(key)
    return su.rand_residues(ref.q, ref.L, 1, np.random.default_rng(104729 * rank + 17 * i + row))[0]


@functools.lru_cache(maxsize=None)
def enc_want(key, rank, emb, i, row, with_rand):
    """The oracle's RandEncode (or Encode) of that row, [emb][L]."""
    _, ref = ctx(key)
    return ref.cf.buckler_encode(enc_row(key, rank, i, row), emb, rnd=enc_draw(key, rank, i, row) if with_rand else None)


def enc_tables(key, rank, emb, sel_name, idx, rng_seed=0):
    """(w [n][n_w][rank][L], rand [n][n_sel][L], wecd before [n][n_w][emb][L]) of the proofs idx: the
    selected rows of wecd are -1, the others random words that must come back unchanged."""
    n_w, sel = SELS[sel_name]
    _, ref = ctx(key)
    w = np.stack([np.stack([enc_row(key, rank, i, r) for r in range(n_w)]) for i in idx])
    rand = np.stack([np.stack([enc_draw(key, rank, i, r) for r in sel]) for i in idx])
    wecd = np.random.default_rng(rng_seed + 3 * rank + emb).integers(0, 1 << 64, size=(len(idx), n_w, emb, ref.L),
                                                                    dtype=np.uint64)
    wecd[:, list(sel)] = FF
    return w, rand, wecd


def enc_expect(key, rank, emb, sel_name, idx, before, with_rand):
    """(wecd after the round, com [n][n_sel][rank + 1][L])."""
    _, sel = SELS[sel_name]
    want = before.copy()
    com = np.zeros((len(idx), len(sel), rank + 1, before.shape[-1]), np.uint64)
    for k, i in enumerate(idx):
        for s, r in enumerate(sel):
            want[k, r] = enc_want(key, rank, emb, i, r, with_rand)
            com[k, s] = want[k, r, :rank + 1]
    return want, com


# ---- device helpers ----------------------------------------------------------------------------------------
def dev(a, dtype=np.uint64):
    import torch
    a = np.ascontiguousarray(a, dtype)
    return torch.from_numpy(a.view(np.int64) if dtype == np.uint64 else a).cuda()


def dev_guarded(a, L):
    """A device copy of `a` with one guard element of -1 behind it."""
    return dev(np.concatenate([np.ascontiguousarray(a, np.uint64).reshape(-1), np.full(L, FF, np.uint64)]))


def filled(words, L):
    """`words` words of -1 on the device and a guard element behind them."""
    import torch
    return torch.full((words + L,), -1, dtype=torch.int64, device="cuda")


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def unguard(t, shape, L, what):
    """The buffer read back, its guard element checked and cut off."""
    h = host(t)
    n = int(np.prod(shape))
    assert h.size == n + L and (h[n:] == FF).all(), f"guard element behind {what} overwritten"
    return h[:n].reshape(shape)
