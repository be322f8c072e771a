"""Shared by the synthetic-field tests (test_oracle_synthetic.py on the CPU,
test_gpu_ntt_synthetic.py on the GPU): the fixture loader, a vectorised sampler of canonical
residues, and the structured extremal input batch; and by the evaluator / Buckler edge tests
(test_oracle_polyops_synthetic.py, test_gpu_polyops_synthetic.py, test_gpu_buckler_synthetic.py):
their field sets and the inputs both sides feed.

Everything here works on raw limb values, the domain the kernels work in: "q - 1" is the
residue whose limbs are those of q - 1 (the largest canonical value), whatever it means in
Montgomery form."""
import functools
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SYNTH = json.load(open(os.path.join(HERE, "golden", "synthetic_fields.json")))
_GOLDEN = json.load(open(os.path.join(HERE, "golden", "fields.json")))

M64 = (1 << 64) - 1


def modulus(name):
    """q of a synthetic field or of one of the reference's fields."""
    return int((SYNTH.get(name) or _GOLDEN[name])["q_hex"], 16)


def limbs_of(v, L):
    return np.array([(v >> (64 * i)) & M64 for i in range(L)], dtype=np.uint64)


def rand_residues(q, L, n, rng):
    """[n, L] canonical residues without per-element big-int work: low limbs uniform, the top
    limb uniform below q's top limb (for L = 1: uniform below q).  Every value is < q; the sliver
    of residues sharing q's top limb is left to the structured inputs."""
    top = q >> (64 * (L - 1))
    out = rng.integers(0, 1 << 64, size=(n, L), dtype=np.uint64)
    out[:, L - 1] = rng.integers(0, top, size=n, dtype=np.uint64)
    return out


# the structured polynomials, most telling first: a batch smaller than the list takes its head
STRUCTURED = ["all_qm1", "pre_fwd_qm1", "pre_inv_qm1", "alt_0_qm1", "zero", "qm1_first", "qm1_last", "ones"]


def structured_batch(cf, q, N, tabs, batch, rng):
    """[batch, N, L] input: the STRUCTURED polynomials (head of the list when batch is smaller),
    then random ones.
      all_qm1      every coefficient q - 1
      pre_fwd_qm1  the oracle's inverse transform of all_qm1: every OUTPUT of the forward
                   transform is q - 1, so the last stage's canonical reduction sits on its edge
                   in every lane
      pre_inv_qm1  the oracle's forward transform of all_qm1: the same for the inverse
      alt_0_qm1    0, q - 1, 0, q - 1, ...
      zero, qm1_first (q - 1 at index 0 only), qm1_last (at index N - 1 only), ones (raw 1)
    `tabs` = cf.tables(N, cyclic=...)."""
    L = cf.L
    tw, twi, ninv = tabs
    qm1 = limbs_of(q - 1, L)
    polys = {}
    polys["all_qm1"] = np.broadcast_to(qm1, (N, L)).copy()
    polys["pre_fwd_qm1"] = cf.ntt_inv(polys["all_qm1"][None], twi, ninv)[0]
    polys["pre_inv_qm1"] = cf.ntt_fwd(polys["all_qm1"][None], tw)[0]
    alt = np.zeros((N, L), np.uint64)
    alt[1::2] = qm1
    polys["alt_0_qm1"] = alt
    polys["zero"] = np.zeros((N, L), np.uint64)
    first = np.zeros((N, L), np.uint64)
    first[0] = qm1
    polys["qm1_first"] = first
    last = np.zeros((N, L), np.uint64)
    last[N - 1] = qm1
    polys["qm1_last"] = last
    ones = np.zeros((N, L), np.uint64)
    ones[:, 0] = 1
    polys["ones"] = ones
    names = STRUCTURED[:batch]
    a = np.empty((batch, N, L), np.uint64)
    for i, k in enumerate(names):
        a[i] = polys[k]
    nr = batch - len(names)
    if nr:
        a[len(names):] = rand_residues(q, L, nr * N, rng).reshape(nr, N, L)
    return a


def edge_values(q, L):
    """The vec-op edge set as raw values: 0, 1, 2, q-2, q-1, (q-1)/2, (q+1)/2, R mod q,
    R^2 mod q, q with its top limb zeroed, 2^64 (L > 1); canonical ones only, no repeats.
    Pairs from it hit x + y = q exactly, x + y = q - 1, x - x, 0 - (q-1), (q-1)(q-1), neg(0)."""
    R = 1 << (64 * L)
    vals = [0, 1, 2, q - 2, q - 1, (q - 1) // 2, (q + 1) // 2, R % q, R * R % q, q & ((1 << (64 * (L - 1))) - 1)]
    if L > 1:
        vals.append(1 << 64)
    out = []
    for v in vals:
        if 0 <= v < q and v not in out:
            out.append(v)
    return out


# ---- the bigpoly-evaluator and Buckler edge tests (test_oracle_polyops_synthetic.py on the CPU,
# test_gpu_polyops_synthetic.py / test_gpu_buckler_synthetic.py on the GPU) ------------------------
# L = 1, 2, 4, 7, 14, with and without a spare top bit, and both 64-bit single-word kinds
ALL = ["p63", "s30", "s63_top", "s64_gold", "s64_lo", "mult_zp", "zp110", "jindo_zp", "s256_top", "s256_lo", "zp440",
       "s448_top", "zp880", "s896_top"]
MS = [n for n in ALL if n != "s63_top"]  # ModSwitch has no Shoup path: s63_top would repeat p63


def plain_batch(q, L, N, names, batch, rng):
    """[batch, N, L]: the STRUCTURED polynomials `names` that need no transform (all_qm1,
    alt_0_qm1, zero, ones), in that order, then random ones."""
    qm1 = limbs_of(q - 1, L)
    a = np.zeros((batch, N, L), np.uint64)
    for i, k in enumerate(names):
        if k == "all_qm1":
            a[i] = qm1
        elif k == "alt_0_qm1":
            a[i, 1::2] = qm1
        elif k == "ones":
            a[i, :, 0] = 1
        else:
            assert k == "zero", k
    nr = batch - len(names)
    if nr:
        a[len(names):] = rand_residues(q, L, nr * N, rng).reshape(nr, N, L)
    return a


def eval_points(q, L, rng):
    """[5, L] evaluation points as raw limb values: 0, 1, q - 1, R mod q (the Montgomery 1), random."""
    return np.stack([limbs_of(0, L), limbs_of(1, L), limbs_of(q - 1, L), limbs_of((1 << (64 * L)) % q, L),
                     rand_residues(q, L, 1, rng)[0]])


def aut_indices(N):
    """The automorphism indices fed at rank N, as given (not reduced): one per residue mod 2N."""
    if N == 1:
        return [1]
    out, seen = [], set()
    for idx in (1, 3, N - 1 if (N - 1) & 1 else N + 1, 2 * N - 1, -1, 2 * N + 3, -(2 * N + 5)):
        if idx % (2 * N) not in seen:
            seen.add(idx % (2 * N))
            out.append(idx)
    return out


# -- ModSwitch ---------------------------------------------------------------------------------
MS_MAX_BITS = 511  # rg_poly_modswitch: operands are 8-word two's complement values


def modswitch_qbigs(q):
    """The qBig set: the fixed values, then q - 1, q + 1, 2q + 1, q where they fit 511 bits."""
    fixed = [1, 2, 3, 2**63 - 1, 2**64, 2**64 + 1, 2**127 - 1, 3 * 2**100 + 8, 2**300 - 2**17, 2**447 - 1, 2**510,
             2**511 - 1]
    return fixed + [v for v in (q - 1, q + 1, 2 * q + 1, q) if v.bit_length() <= MS_MAX_BITS]


def _fits(p):
    return -(1 << MS_MAX_BITS) <= p < (1 << MS_MAX_BITS)


def _rand_signed(max_bits, n, rng):
    out = []
    for _ in range(n):
        bits = int(rng.integers(0, max_bits + 1))
        v = int.from_bytes(rng.bytes(64), "little") & ((1 << bits) - 1)
        out.append(-v if rng.integers(0, 2) else v)
    return out


def modswitch_ties(q, qbig):
    """The tie family, or [] when q has no inverse mod qBig: for t in {0, 1, h - 1, h, h + 1,
    h + 2, qBig - 1} mod qBig (h = floor(qBig / 2)) and p0 = t q^-1 mod qBig, the values p0,
    p0 - qBig, -p0 and p0 + 5 qBig.  |p| q mod qBig is then exactly t (-t for p0 - qBig): on
    floor(qBig/2) + 1 (the threshold for p >= 0) and on qBig - floor(qBig/2) (for p < 0), which
    are h + 1 and h + 1 for odd qBig, h + 1 and h for even qBig, and one step either side of
    both.  Values that do not fit 8 words (p0 + 5 qBig from 2^508 up) are left out."""
    import math
    if math.gcd(q, qbig) != 1:
        return []
    qinv = pow(q, -1, qbig)
    h = qbig >> 1
    out = []
    for t in sorted({x % qbig for x in (0, 1, h - 1, h, h + 1, h + 2, qbig - 1)}):
        p0 = t * qinv % qbig
        for p in (p0, p0 - qbig, -p0, p0 + 5 * qbig):
            assert abs(p) * q % qbig == (-t % qbig if p == p0 - qbig else t)
            if _fits(p):
                out.append(p)
    return out


def modswitch_carries(q, qbig):
    """Values whose quotient increments carry across words, for k = 1, 2 and both signs, where
    |p| fits 8 words:
      * +-qBig 2^(64k): |p| q is an exact multiple of qBig with a quotient ending in k zero words.
        The Barrett estimate of an exact multiple is one short unless qBig is a power of two, so it
        ends in k words of ones and the correction ++quo carries through them;
      * where q is invertible mod qBig 2^(64k): |p| q = (2^(64k) - 1 + j 2^(64k)) qBig + t with t
        on the threshold of p's sign, so the rounding ++Q carries through k words of ones."""
    import math
    out = []
    h = qbig >> 1
    for k in (1, 2):
        m = qbig << (64 * k)
        if m.bit_length() > MS_MAX_BITS:
            continue
        out += [m, -m]
        if math.gcd(q, m) != 1:
            continue
        for sign, t in ((1, h + 1), (-1, qbig - h)):
            if t < qbig:  # qBig = 1: the thresholds are out of reach
                a = (t + qbig * ((1 << (64 * k)) - 1)) * pow(q, -1, m) % m
                assert a * q % qbig == t and (a * q // qbig + 1) % (1 << (64 * k)) == 0
                out.append(sign * a)
    return out


def modswitch_inputs(q, qbig, rng):
    """(narrow, wide, number of tie values) for one (q, qBig).
      narrow  0, 1, -1, the tie family, 30 random values of random bit length up to
              bits(qBig) + 2 (511 at most) and random sign
      wide    2^511 - 1, -(2^511 - 1), -2^511, 2^510 + 12345, 30 random values of random bit length
              up to 510 and random sign: the quotient handed to the second division (by q) has up
              to 511 + bits(q) - bits(qBig) bits."""
    ties = modswitch_ties(q, qbig)
    narrow = [0, 1, -1] + ties + _rand_signed(min(qbig.bit_length() + 2, MS_MAX_BITS), 30, rng)
    wide = [2**511 - 1, -(2**511 - 1), -2**511, 2**510 + 12345] + _rand_signed(510, 30, rng)
    assert all(_fits(p) for p in narrow + wide)
    return narrow, wide, len(ties)


def modswitch_min_words(ps, qbig):
    """The smallest word count that holds qBig and every p as signed values (what the Python
    mirror of ModSwitchTo picks)."""
    bits = max([qbig.bit_length()] + [(p if p >= 0 else -p - 1).bit_length() for p in ps]) + 1
    return (bits + 63) // 64


def signed_words(ps, w):
    """[n, w] two's complement words of Python ints."""
    mask = (1 << (64 * w)) - 1
    return np.array([[((p & mask) >> (64 * i)) & M64 for i in range(w)] for p in ps], np.uint64).reshape(len(ps), w)


# -- Buckler Encode / RandEncode -----------------------------------------------------------------
ENCODE_ROWS = ["all_qm1", "pre_inv_qm1", "zero", "random"]


def encode_rows(cf, q, rank, rng):
    """[4, rank, L] witness rows: all q - 1; the oracle's forward cyclic NTT of all q - 1 (every
    InvNTT output is q - 1); zero; random."""
    L = cf.L
    tw, _, _ = cf.tables(rank, cyclic=True)
    v = np.zeros((4, rank, L), np.uint64)
    v[0] = limbs_of(q - 1, L)
    v[1] = cf.ntt_fwd(v[0][None], tw)[0]
    v[3] = rand_residues(q, L, rank, rng)
    return v


def encode_rands(q, L, c0, rng):
    """The RandEncode draws for a row whose plain encoding has coeff[0] = c0 (a raw value), as
    [L] limbs or None: r = c0 (coeff[0] becomes 0), 0, q - 1, c0 + 1 mod q (coeff[0] becomes
    q - 1), random, and no draw (Encode)."""
    return [limbs_of(c0, L), limbs_of(0, L), limbs_of(q - 1, L), limbs_of((c0 + 1) % q, L),
            rand_residues(q, L, 1, rng)[0], None]


# -- evalCircuit ---------------------------------------------------------------------------------
CIRCUIT_NW, CIRCUIT_NPW = 5, 2


def circuit_witnesses(q, L, rank, rng):
    """(w [5, rank, L], pw [2, rank, L]): witness 0 all q - 1, witness 1 zero, public witness 0
    alternating 0 / q - 1, the rest random."""
    w = rand_residues(q, L, CIRCUIT_NW * rank, rng).reshape(CIRCUIT_NW, rank, L)
    pw = rand_residues(q, L, CIRCUIT_NPW * rank, rng).reshape(CIRCUIT_NPW, rank, L)
    w[0] = limbs_of(q - 1, L)
    w[1] = 0
    pw[0] = plain_batch(q, L, rank, ["alt_0_qm1"], 1, rng)[0]
    return w, pw


def circuit_terms(q, L, rng):
    """The edge circuit in the oracle's form: constraints as lists of (coeff [L], public witness
    or None, [witnesses])."""
    c, k, k2, k3 = (int(x) for x in from_limbs(rand_residues(q, L, 4, rng)))
    c = c or 1
    lim = lambda v: limbs_of(v, L)  # noqa: E731
    return [
        [(lim(q - 1), None, [0, 0, 0])],                        # (q - 1) w0^3 on w0 = q - 1
        [(lim(c), None, [2]), (lim(q - c), None, [2])],         # c w2 + (q - c) w2: 0 through exactly q
        [(lim(0), None, [3]), (lim(k), None, [1, 4])],          # a zero coefficient, a zero witness
        [],                                                     # no terms
        [(lim(k), None, [])],                                   # a constant
        [(lim(k2), 0, [3, 3, 4]), (lim(k3), 1, [4]), (lim(q - 1), 0, [0])],  # public witnesses, a repeat
    ]


def circuit_cancel_terms(q, L, rng):
    """Two constraints c w2 and (q - c) w2, then an empty one: their scaled evaluations are a and
    q - a, so pOut's accumulation passes through exactly q and must leave 0.  (Inside one
    constraint, as in circuit_terms, the sum is multiplied by batchConst next, which maps an
    unreduced q to 0 as well: only the accumulation across constraints shows the edge.)"""
    c = int(from_limbs(rand_residues(q, L, 1, rng))[0]) or 1
    return [[(limbs_of(c, L), None, [2])], [(limbs_of(q - c, L), None, [2])], []]


def batch_consts(q, L, rng):
    """[4, L]: 0, raw 1, q - 1, random."""
    return np.stack([limbs_of(0, L), limbs_of(1, L), limbs_of(q - 1, L), rand_residues(q, L, 1, rng)[0]])


def from_limbs(a):
    a = np.asarray(a, np.uint64)
    a = a.reshape(-1, a.shape[-1])
    return [sum(int(x) << (64 * j) for j, x in enumerate(row)) for row in a]


@functools.lru_cache(maxsize=None)
def cfield(name):
    import coracle as co
    return co.CField(modulus(name))


@functools.lru_cache(maxsize=4)
def oracle_tables(name, logn, cyclic):
    """The oracle's table triple, computed once per (field, rank, kind) and shared; read-only."""
    tabs = cfield(name).tables(1 << logn, cyclic=cyclic)
    for t in tabs:
        t.setflags(write=False)
    return tabs
