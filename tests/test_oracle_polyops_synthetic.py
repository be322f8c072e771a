"""CPU: pin the C oracle's bigpoly evaluators and Buckler restatements (oracle.c
of_quorem_vanishing / of_aut / of_poly_evaluate / of_buckler_encode / of_buckler_eval_circuit) on
the synthetic fields, on plain Python integers, at the inputs test_gpu_polyops_synthetic.py and
test_gpu_buckler_synthetic.py feed the kernels.

test_oracle_polyops.py and test_oracle_buckler.py pin these functions on p63 and jindo_zp only, on
random data; the GPU files compare the library with the oracle on moduli without a spare top bit
and on extremal inputs, which means nothing unless the oracle is right there.  Raw limb values are
Montgomery representatives, in and out: a product is a b R^-1 mod q, sums and negations are plain.
  * quorem: p = quo (X^M - 1) + rem with rem[M:] = 0, on a random and on the all-(q - 1) polynomial;
  * aut: the signed permutation out[i idx mod N] = +-p[i] in integers, -0 = 0 included, and the
    NTT-domain path commutes with the oracle's negacyclic NTT (pinned by test_oracle_synthetic.py);
  * evaluate: sum p_i x^i in integers at 0, raw 1, raw q - 1, R mod q and a random point;
  * buckler_encode: the oracle's cyclic inverse NTT plus r (X^rank - 1) in integers, at the
    coeff[0] edges (r = coeff[0], 0, q - 1, coeff[0] + 1);
  * buckler_eval_circuit: sum_c bc sum_t coeff pw prod w in integers, on the edge circuit;
  * the ModSwitch tie family puts |p| q mod qBig where it says, and pyref.mod_switch rounds half
    down there."""
import numpy as np
import pytest

import coracle as co
from tests import synth_util as su

NAMES = sorted(su.SYNTH) + ["mult_zp", "zp880"]


def _ctx(name):
    q = su.modulus(name)
    cf = su.cfield(name)
    return q, cf, cf.L


@pytest.mark.parametrize("name", NAMES)
def test_quorem_identity(name):
    q, cf, L = _ctx(name)
    rank = 64
    polys = su.plain_batch(q, L, rank, ["all_qm1"], 2, np.random.default_rng(1))
    for M in (1, 24, 63, 64, 100, 0):
        for p in polys:
            quo, rem = cf.quorem_vanishing(p, M)
            P, Q, R = co.from_limbs(p), co.from_limbs(quo), co.from_limbs(rem)
            assert max(Q) < q and max(R) < q
            if M == 0:  # X^0 - 1 = 0: the reference's loop moves every coefficient to the quotient
                assert Q == P and R == [0] * rank
                continue
            prod = [0] * (rank + M)  # quo (X^M - 1)
            for i, c in enumerate(Q):
                prod[i + M] += c
                prod[i] -= c
            assert [(prod[i] + R[i]) % q for i in range(rank)] == P, M
            assert all(x == 0 for x in prod[rank:]), M  # deg quo < rank - M
            assert all(r == 0 for r in R[M:]), M


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("N", [64, 1])
def test_aut_is_signed_permutation_and_commutes_with_ntt(name, N):
    q, cf, L = _ctx(name)
    polys = su.plain_batch(q, L, N, ["alt_0_qm1", "zero", "all_qm1"], 4, np.random.default_rng(2))
    tw, _, _ = cf.tables(N)
    for idx in (1, 3, 127, -1, 2 * 64 + 5):
        for p in polys:
            P = co.from_limbs(p)
            want = [None] * N
            for i, v in enumerate(P):
                j = (i * idx) % (2 * N)
                want[j % N] = v if j < N else (q - v) % q  # -0 = 0, not q
            a = cf.aut(p, idx, False)
            assert co.from_limbs(a) == want, idx
            assert (cf.ntt_fwd(a[None], tw)[0] == cf.aut(cf.ntt_fwd(p[None], tw)[0], idx, True)).all(), idx


@pytest.mark.parametrize("name", NAMES)
def test_evaluate_is_sum_of_powers(name):
    q, cf, L = _ctx(name)
    rng = np.random.default_rng(3)
    rinv = pow(1 << (64 * L), -1, q)
    pts = su.eval_points(q, L, rng)
    assert co.from_limbs(pts[:4]) == [0, 1, q - 1, (1 << (64 * L)) % q]
    for n in (0, 1, 64, 65, 300):
        for p in su.plain_batch(q, L, n, ["all_qm1"], 2, rng):
            P = [c * rinv % q for c in co.from_limbs(p)] if n else []
            for x in pts:
                xv = co.from_limbs(x[None])[0] * rinv % q
                want = sum(c * pow(xv, i, q) for i, c in enumerate(P)) % q
                got = co.from_limbs(cf.evaluate(p, x)[None])[0]
                assert got < q and got * rinv % q == want, (n, hex(xv))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("rank,emb", [(8, 9), (64, 128), (64, 64)])
def test_buckler_encode_is_invntt_plus_fixup(name, rank, emb):
    q, cf, L = _ctx(name)
    rng = np.random.default_rng(4)
    _, twi, ninv = cf.tables(rank, cyclic=True)
    rows = su.encode_rows(cf, q, rank, rng)
    for k, v in enumerate(rows):
        base = co.from_limbs(cf.ntt_inv(v[None], twi, ninv)[0])
        if su.ENCODE_ROWS[k] == "pre_inv_qm1":
            assert base == [q - 1] * rank
        assert co.from_limbs(cf.buckler_encode(v, emb)) == base + [0] * (emb - rank)
        if emb == rank:
            continue  # RandEncode needs coefficient `rank`
        for r in su.encode_rands(q, L, base[0], rng)[:-1]:
            rv = co.from_limbs(r[None])[0]
            want = [(base[0] - rv) % q] + base[1:] + [rv] + [0] * (emb - rank - 1)
            assert co.from_limbs(cf.buckler_encode(v, emb, rnd=r)) == want, (su.ENCODE_ROWS[k], hex(rv))
        edges = [co.from_limbs(cf.buckler_encode(v, emb, rnd=r))[0] for r in su.encode_rands(q, L, base[0], rng)[:4]]
        assert edges[0] == 0 and edges[1] == base[0] and edges[3] == q - 1


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("rank", [1, 33])
def test_buckler_eval_circuit_is_integer_sum(name, rank):
    q, cf, L = _ctx(name)
    rng = np.random.default_rng(5)
    rinv = pow(1 << (64 * L), -1, q)
    mm = lambda a, b: a * b * rinv % q  # noqa: E731
    w, pw = su.circuit_witnesses(q, L, rank, rng)
    W = [co.from_limbs(x) for x in w]
    P = [co.from_limbs(x) for x in pw]
    assert W[0] == [q - 1] * rank and W[1] == [0] * rank and P[0] == [0, q - 1] * (rank // 2) + [0] * (rank % 2)
    for cons, cancelling in ((su.circuit_terms(q, L, rng), False), (su.circuit_cancel_terms(q, L, rng), True)):
        eval_q, acc_q = 0, 0  # sums that reach exactly q: inside a constraint, across constraints
        for bc in su.batch_consts(q, L, rng):
            B = co.from_limbs(bc[None])[0]
            got = co.from_limbs(cf.buckler_eval_circuit(cons, bc, w, pw))
            for j in range(rank):
                acc = 0
                for c in cons:
                    ev, raw = 0, 0
                    for coeff, p, ws in c:
                        t = co.from_limbs(coeff[None])[0]
                        if p is not None:
                            t = mm(t, P[p][j])
                        for k in ws:
                            t = mm(t, W[k][j])
                        raw += t
                        ev = (ev + t) % q
                    eval_q += raw == q
                    acc_q += acc + mm(ev, B) == q
                    acc = (acc + mm(ev, B)) % q
                assert got[j] == acc and (acc == 0 or not cancelling), (j, hex(B))
        # the cancelling terms summed to exactly q, not to 0 + 0 (batchConst = 0 gives acc 0 + 0)
        assert (acc_q >= 3) if cancelling else (eval_q >= 4)


@pytest.mark.parametrize("name", su.MS)
def test_modswitch_tie_family_sits_on_the_thresholds(name):
    """The inputs of the GPU ModSwitch test: the family is built for every qBig but q itself, it
    puts |p| q mod qBig on both rounding thresholds and next to them for both signs, and
    pyref.mod_switch is round-half-down there in exact rationals."""
    import math
    from fractions import Fraction

    import pyref
    q = su.modulus(name)
    qbigs = su.modswitch_qbigs(q)
    assert len(qbigs) == (12 if q.bit_length() > 509 else 16)
    for qbig in qbigs:
        ties = su.modswitch_ties(q, qbig)
        assert bool(ties) == (qbig != q), hex(qbig)
        if not ties:
            continue
        h = qbig >> 1
        hit_pos = {abs(p) * q % qbig for p in ties if p >= 0}
        hit_neg = {abs(p) * q % qbig for p in ties if p < 0}
        for t in (h, h + 1, h + 2):  # floor(qBig/2) + 1 and one step either side
            assert t % qbig in hit_pos
        for t in (qbig - h - 1, qbig - h, qbig - h + 1):
            assert t % qbig in hit_neg
        carries = su.modswitch_carries(q, qbig)
        per_k = 2 + min(qbig - 1, 2)  # no threshold in reach at qBig = 1, only the negative one at 2
        assert len(carries) == sum(per_k for k in (1, 2) if qbig.bit_length() + 64 * k <= su.MS_MAX_BITS)
        for p in carries:
            quo, ra = divmod(abs(p) * q, qbig)
            if abs(p) % qbig == 0:  # an exact multiple whose quotient ends in a zero word
                assert ra == 0 and quo % 2**64 == 0
            else:  # on p's threshold, and the quotient that ++Q increments ends in 2^64 - 1
                assert ra == (h + 1 if p > 0 else qbig - h) and quo % 2**64 == 2**64 - 1
        ties = ties + carries
        want = [math.ceil(Fraction(p * q, qbig) - Fraction(1, 2)) % q for p in ties]
        assert pyref.mod_switch(ties, qbig, q) == want, hex(qbig)
    narrow, wide, _ = su.modswitch_inputs(q, qbigs[4], np.random.default_rng(6))
    assert su.modswitch_min_words(narrow, qbigs[4]) == 2 and su.modswitch_min_words(wide, qbigs[4]) == 8
    assert (su.signed_words([-1, 1 << 64], 2) == np.array([[su.M64, su.M64], [0, 1]], np.uint64)).all()
