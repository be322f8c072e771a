"""Shared by test_buckler_lin_ref.py (CPU) and test_gpu_buckler_lin.py (GPU): seeded field
elements and the completeness circuit of the linear check -- one checker of each kind, every
constraint a pair (wOut, wIn) with wOut = M wIn, witnesses RandEncoded at the embedding rank."""
import numpy as np

from tests import buckler_lin_ref as R


def rand_ints(q, n, rng):
    nb = (q.bit_length() + 7) // 8 + 8
    return [int.from_bytes(rng.bytes(nb), "little") % q for _ in range(n)]


# bytes that make exactly rows 0 and 127 of a column true: bit 0 of byte 0 and bit 7 of byte 15
# clear, every other bit of the first 16 bytes set (bytes 16..31 are never read)
ROWS_0_127 = bytes([0xFE] + [0xFF] * 14 + [0x7F] + [0xA5] * 16)


def xof_bytes(kind, rank, rng):
    if kind == "random":
        return rng.bytes(32 * rank)
    if kind == "zeros":
        return bytes(32 * rank)
    if kind == "ones":
        return b"\xff" * (32 * rank)
    assert kind == "rows_0_127"
    return ROWS_0_127 * rank


RECOMPOSE_BOUND = 8  # decomposeBase(8) = [4, 2, 1]: nb = 3


def completeness_circuit(ref, rank, emb, seed, two_pairs=False, perturb=False):
    """Returns a dict: checkers (reference objects), spec (how to build the same checkers on the
    device), constraints (per checker, the (wOut, wIn) pairs), w (witness vectors), wEcd / wEcdNTT
    (int lists), bc, lc, rand (mask draws), xof."""
    rng = np.random.default_rng(seed)
    q = ref.q
    xof = xof_bytes("random", rank, rng)
    base = R.decomposeBase(RECOMPOSE_BOUND)
    checkers = [R.NTTChecker(ref, rank), R.AutChecker(ref, rank, 5, False), R.ProjChecker(ref, rank).set_xof(xof),
                R.RecomposeChecker(ref, rank, base)]
    spec = [("ntt",), ("aut", 5, False), ("proj", xof), ("recompose", RECOMPOSE_BOUND)]
    npairs = [2 if two_pairs else 1, 1, 1, 1]
    w, constraints = [], []
    for chk, n in zip(checkers, npairs):
        pairs = []
        for _ in range(n):
            wIn = rand_ints(q, rank, rng)
            wOut = chk.transform(wIn)
            pairs.append((len(w), len(w) + 1))
            w += [wOut, wIn]
        constraints.append(pairs)
    if perturb:
        w[0] = list(w[0])
        w[0][3] = (w[0][3] + 1) % q
    blind = rand_ints(q, len(w), rng)
    wEcd = [ref.rand_encode(v, emb, r) for v, r in zip(w, blind)]
    wEcdNTT = [ref.fwd(p, cyclic=True) for p in wEcd]
    bc, lc = rand_ints(q, 2, rng)
    rand = rand_ints(q, 2 * rank, rng)
    return dict(checkers=checkers, spec=spec, constraints=constraints, w=w, wEcd=wEcd, wEcdNTT=wEcdNTT, bc=bc, lc=lc,
                rand=rand, xof=xof)
