"""Shared by test_oracle_jindo_synth.py (CPU) and test_gpu_jindo_synth.py (GPU): the synthetic
Jindo parameter sets (tests/golden/jindo_synth_params.json), commit inputs that hit the digit
boundaries, exact-integer polynomials that put the rounding and centring decisions in front of
the round kernels, and a big-int statement of the verifier's two norm sums."""
import json
import math
import os

import numpy as np

import coracle as co
import pyref
from tests.jindo_proto import VERIFY_KEYS, honest_proof, random_ck
from tests.jindo_util import make_randomness

HERE = os.path.dirname(os.path.abspath(__file__))
SYNTH = json.load(open(os.path.join(HERE, "golden", "jindo_synth_params.json")))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "jindo_params.json")))
NAMES = list(SYNTH)
HUGE = 1e300  # a norm bound no sum of kNormW words reaches


def params(name):
    P = SYNTH[name] if name in SYNTH else FIXTURE[name]
    return P, int(P["field_q_hex"], 16)


def is_jindo_field(P, fq):
    """DecodeTo is a ring homomorphism (so an honest proof passes verifyEval) only when
    X^slots = b is consistent with X^d = -1: p = b^exp + 1 and slots * exp = d."""
    return fq == P["base"] ** P["exp"] + 1 and P["slots"] * P["exp"] == P["d"]


def synth_v(P, fq, nv, seed):
    """v [nv][L] (Montgomery form) whose canonical values start 0, q-1, q-2, 1, b^k +- 1 for
    k = 1 and exp-1, then uniform values; nv = 1 keeps q-1 alone."""
    L = (fq.bit_length() + 63) // 64
    R = 1 << (64 * L)
    b, e = P["base"], P["exp"]
    vals = [fq - 1, 0, fq - 2, 1, b - 1, b + 1, b ** (e - 1) - 1, b ** (e - 1) + 1]
    rng = np.random.default_rng(seed)
    vals += [int.from_bytes(rng.bytes(8 * L + 8), "little") % fq for _ in range(max(0, nv - len(vals)))]
    out = np.zeros((nv, L), np.uint64)
    for i, c in enumerate(vals[:nv]):
        m = (c % fq) * R % fq
        for j in range(L):
            out[i, j] = (m >> (64 * j)) & ((1 << 64) - 1)
    return out


# ---- rounding and centring edges ----------------------------------------------------------
def edge_values(primes, cut):
    """[(value mod Q, label)], duplicates (one-limb rings: q == Q) removed."""
    Q = math.prod(primes)
    h, c = Q >> 1, 1 << cut
    ev = [(0, "0"), (1, "1"), (-1, "-1"), (h, "Q>>1 (the tie)"), (h + 1, "(Q>>1)+1"), (h - 1, "(Q>>1)-1"),
          (Q - 1, "Q-1"), (c, "2^cut"), (c - 1, "2^cut-1"), (-c, "-2^cut"), (-c + 1, "-2^cut+1"),
          (-c - 1, "-2^cut-1"), (-3 * c, "-3*2^cut"), ((h >> cut) << cut, "((Q>>1)>>cut)<<cut"),
          (-(((h - 1) >> cut) << cut), "-((((Q>>1)-1)>>cut)<<cut)")]
    for q in primes:
        ev += [(q >> 1, f"{q}>>1"), ((q >> 1) + 1, f"({q}>>1)+1"), (-(q >> 1), f"-({q}>>1)"),
               (-(q >> 1) - 1, f"-({q}>>1)-1"), (q, f"+{q}"), (-q, f"-{q}"), ((Q // 3 // q) * q, f"(Q/3/{q})*{q}")]
    seen, out = set(), []
    for v, lab in ev:
        if v % Q not in seen:
            seen.add(v % Q)
            out.append((v % Q, lab))
    return out


def edge_polys(primes, cut, d, npoly, seed):
    """npoly polynomials of d (value in [0, Q), label): the edges, then uniform values.  Where d
    is smaller than the edge list (d = 8) the edges are dealt over the polynomials in order."""
    Q = math.prod(primes)
    ev = edge_values(primes, cut)
    rng = np.random.default_rng(seed)
    uni = lambda: (int.from_bytes(rng.bytes(40), "little") % Q, "uniform")  # noqa: E731
    if len(ev) <= d:
        return [ev + [uni() for _ in range(d - len(ev))] for _ in range(npoly)]
    assert npoly * d >= len(ev), "not enough coefficients for every edge"
    flat = ev + [uni() for _ in range(npoly * d - len(ev))]
    return [flat[p * d:(p + 1) * d] for p in range(npoly)]


def ntt_mform(primes, d, vals):
    """NTT(MForm(vals mod q_l)) per limb: [len(primes)][d] uint64."""
    return np.array([pyref.subring(d, q).ntt(pyref.subring(d, q).mform([v % q for v in vals])) for q in primes],
                    np.uint64)


def coeffs(primes, d, limbs):
    """The centred integer coefficients of an NTT-domain Montgomery polynomial [nl][d]."""
    c = []
    for l, q in enumerate(primes):
        sr = pyref.subring(d, q)
        c.append(sr.intt(sr.imform([int(x) for x in limbs[l]])))
    return [pyref.reconstruct(list(primes), [c[l][k] for l in range(len(primes))]) for k in range(d)]


def inner_edge_case(P, seed):
    """commit_core inputs whose inner MAC output (i, j) is exactly polys[i * in_msis + j]: zero
    encodes, zero MLWE secrets, the added term MLWE[i][mlwe + j] = NTT(MForm(values))."""
    d, nq, nm = P["d"], len(P["q"]), P["in_msis"] + P["mlwe"]
    polys = edge_polys(P["q"], P["log_in_cut"], d, (P["cols"] + 1) * P["in_msis"], seed)
    enc = np.zeros((P["cols"] + 1, P["rows"], nq, d), np.uint64)
    mlwe = np.zeros((P["cols"] + 1, nm, nq, d), np.uint64)
    for i in range(P["cols"] + 1):
        for j in range(P["in_msis"]):
            mlwe[i, P["mlwe"] + j] = ntt_mform(P["q"], d, [v for v, _ in polys[i * P["in_msis"] + j]])
    return enc, mlwe, polys


def outer_edge_case(P, seed):
    """(ck, enc, mlwe, polys): InCommit[0] is the constant 1 (inner value 2^log_in_cut at
    coefficient 0), ck_out[i][0] = NTT(MForm(polys[i])) and every other ck_out entry is zero, so the
    outer MAC output of row i is exactly polys[i]."""
    d, nq, nm = P["d"], len(P["q"]), P["in_msis"] + P["mlwe"]
    polys = edge_polys(P["qo"], P["log_out_cut"], d, P["out_msis"], seed)
    ck_in, ck_mlwe, ck_out = random_ck(P, seed + 1)
    ck_out[:] = 0
    for i in range(P["out_msis"]):
        ck_out[i, 0] = ntt_mform(P["qo"], d, [v for v, _ in polys[i]])
    enc = np.zeros((P["cols"] + 1, P["rows"], nq, d), np.uint64)
    mlwe = np.zeros((P["cols"] + 1, nm, nq, d), np.uint64)
    mlwe[0, P["mlwe"]] = ntt_mform(P["q"], d, [1 << P["log_in_cut"]] + [0] * (d - 1))
    return (ck_in, ck_mlwe, ck_out), enc, mlwe, polys


def rounded(P, src, dst, polys, cut):
    """pyref.round_to of each polynomial of (value, label) pairs given in ring `src`: [npoly][len(dst)][d]."""
    from types import SimpleNamespace
    ns = SimpleNamespace(d=P["d"])
    ring = pyref.Ring(P["d"], dst)
    return np.array([pyref.round_to(ns, list(src), ring, ntt_mform(src, P["d"], [v for v, _ in p]).tolist(), cut)
                     for p in polys], np.uint64)


def explain(got, want, dst, d, labels, what):
    """Assert got == want ([nl][d] NTT-domain); a mismatch names the first differing coefficient and
    the edge it held."""
    if (np.asarray(got) == np.asarray(want)).all():
        return
    g, w = coeffs(dst, d, got), coeffs(dst, d, want)
    k = next((i for i in range(d) if g[i] != w[i]), None)
    raise AssertionError(f"{what}: coefficient {k} held {labels[k] if k is not None else '?'}: got "
                         f"{g[k] if k is not None else '?'}, want {w[k] if k is not None else '?'}")


# ---- honest proofs and the verifier's norms --------------------------------------------------
def synth_proof(name, seed):
    """(P with norm bounds, fq, ck, proof, S_outer, S_inner) for a synthetic set: an honest proof by
    the oracle with injected randomness; the bounds are 2 * float(isqrt(S)) of its exact norms."""
    P, fq = params(name)
    P = dict(P)
    ck = random_ck(P, seed)
    nv = P["rank"]
    v = synth_v(P, fq, nv, seed + 1)[None]
    rnd = make_randomness(P, fq, seed=seed + 2, batch=1)
    pr = honest_proof(P, fq, ck, seed=seed, rnd=rnd, v=v)
    r = verify_nm(P, fq, ck, pr, HUGE, HUGE)
    P["in_com_dcmp_two_nm"] = 2.0 * float(math.isqrt(r["outer_sq"]))
    P["res_two_nm"] = 2.0 * float(math.isqrt(r["inner_sq"]))
    return P, fq, ck, pr, r["outer_sq"], r["inner_sq"]


def verify_nm(P, fq, ck, pr, nm_out, nm_in):
    """The oracle's Verify with explicit norm bounds."""
    return co.CJindo(P, fq).verify(ck, pr["batch"], *[pr[k] for k in VERIFY_KEYS], nm_out, nm_in)


def crafted(P, pr, seed):
    """The proof with pf_incom[0], pf_enc[0], pf_mlwe[0] replaced by NTT(MForm(edge values)), cut 0."""
    bad = dict(pr)
    for k, primes, s in (("pf_incom", P["qo"], 0), ("pf_enc", P["q"], 1), ("pf_mlwe", P["q"], 2)):
        bad[k] = pr[k].copy()
        poly = edge_polys(primes, 0, P["d"], 1, seed + s)[0]
        bad[k][0] = ntt_mform(primes, P["d"], [v for v, _ in poly])
    return bad


def bigint_norms(P, ck, pr):
    """(outer, inner) sums of squares of Verifier.Verify (verifier.go:136-200) for a batch-1 proof,
    from pyref.reconstruct and SubRing alone:
      outer = sum centred(pf_incom)^2 + sum centred(A 2^logOutCut - ck_out . pf_incom)^2
      inner = sum centred(pf_enc)^2 + sum centred(pf_mlwe)^2 + sum centred(A' 2^logInCut - (ck_in . pf_enc +
              ck_mlwe . pf_mlwe + pf_mlwe[mlwe + i]))^2, A' = sum_j chals[j] lift[j inMSIS + i] + lift[cols inMSIS + i],
      lift = the centred pf_incom taken into ringQ."""
    assert pr["batch"] == 1
    d, q, qo = P["d"], list(P["q"]), list(P["qo"])
    sq = lambda primes, limbs: sum(c * c for c in coeffs(primes, d, limbs))  # noqa: E731
    ints = lambda a: [[int(x) for x in row] for row in a]  # noqa: E731

    def mac(primes, pairs, add=None):
        out = []
        for l, p in enumerate(primes):
            sr = pyref.subring(d, p)
            acc = [0] * d
            for a, b in pairs:
                acc = sr.mul_mont_add([int(x) for x in a[l]], [int(x) for x in b[l]], acc)
            if add is not None:
                acc = [(x + int(y)) % p for x, y in zip(acc, add[l])]
            out.append(acc)
        return out

    def combine(primes, A, B, cut):
        return [[(int(a) * (1 << cut) - b) % p for a, b in zip(A[l], B[l])] for l, p in enumerate(primes)]

    ck_in, ck_mlwe, ck_out = ck
    outer = sum(sq(qo, pr["pf_incom"][j]) for j in range(P["in_com_dcmp_len"]))
    for i in range(P["out_msis"]):
        B = mac(qo, [(ck_out[i][j], pr["pf_incom"][j]) for j in range(P["in_com_dcmp_len"])])
        outer += sq(qo, combine(qo, ints(pr["com"][0][i][:len(qo)]), B, P["log_out_cut"]))
    lift = [ntt_mform(q, d, coeffs(qo, d, pr["pf_incom"][j])) for j in range(P["in_com_dcmp_len"])]
    nm = P["in_msis"] + P["mlwe"]
    inner = sum(sq(q, pr["pf_enc"][j]) for j in range(P["rows"])) + sum(sq(q, pr["pf_mlwe"][j]) for j in range(nm))
    for i in range(P["in_msis"]):
        A = mac(q, [(pr["chals"][j], lift[j * P["in_msis"] + i]) for j in range(P["cols"])],
                add=lift[P["cols"] * P["in_msis"] + i])
        B = mac(q, [(ck_in[i][j], pr["pf_enc"][j]) for j in range(P["rows"])] +
                [(ck_mlwe[i][j], pr["pf_mlwe"][j]) for j in range(P["mlwe"])], add=pr["pf_mlwe"][P["mlwe"] + i])
        inner += sq(q, combine(q, A, B, P["log_in_cut"]))
    return outer, inner
