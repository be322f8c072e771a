"""CPU: the C oracle pinned on the synthetic Jindo parameter sets
(tests/golden/jindo_synth_params.json: d = 8 .. 1024, four unequal ring primes, primes up to
2^62, bases and exponents off the configs) before the GPU tests take it as their reference:

  * the fixture regenerates byte for byte from its generator;
  * CJindo.commit == the big-int pyref.commit on all four outputs, full and ragged v whose values
    hit the digit boundaries;
  * CJindo.commit_core == pyref.round_to on polynomials of exact integers at every rounding and
    centring edge (the tie Q>>1, Q/2 +- 1, negative exact multiples of 2^cut, -(2^cut) +- 1,
    residues that vanish in one limb), through the inner and the outer round;
  * CJindo.verify's two norm sums == a big-int statement of them, on honest proofs and on proofs
    whose responses hold those edges (|value| = (Q + 1) / 2 terms, the lift's round at the tie).
"""
import importlib.util
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

import coracle as co
import pyref
from tests import jindo_synth_util as su
from tests.jindo_proto import random_ck
from tests.jindo_util import make_randomness

HERE = os.path.dirname(os.path.abspath(__file__))
ROUND_SHAPES = [n for n in su.NAMES if su.SYNTH[n]["d"] != 256] + ["syn_d256_q62", "syn_d256_q62top", "t10_b1",
                                                                  "zp880_t10_b1", "mult_t8193_b12"]
CRAFTED_SHAPES = ["syn_d128_mixed4", "syn_d128_q2", "t10_b1", "mult_t8193_b12"]


def test_fixture_regenerates_byte_for_byte(tmp_path):
    spec = importlib.util.spec_from_file_location("make_jindo_synth_params",
                                                  os.path.join(HERE, "golden", "make_jindo_synth_params.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = tmp_path / "synth.json"
    mod.main(str(out))
    assert out.read_bytes() == open(os.path.join(HERE, "golden", "jindo_synth_params.json"), "rb").read()


def test_sets_are_what_the_abi_promises():
    for name, P in su.SYNTH.items():
        assert P["rank"] == (P["rows"] - 1) * P["cols"] * P["slots"], name
        assert P["in_com_dcmp_len"] == (P["cols"] + 1) * P["in_msis"] and P["batch"] == 1, name
        assert P["rows"] <= 5 and P["cols"] <= 2 and P["slots"] * P["exp"] <= P["d"], name
        assert len(set(P["q"] + P["qo"])) == len(P["q"]) + len(P["qo"]), name
        for q in P["q"] + P["qo"]:
            assert pyref.is_prime(q) and (q - 1) % (2 * P["d"]) == 0 and P["base"] < q < 1 << 62, (name, q)


@pytest.mark.parametrize("name", su.NAMES)
def test_c_commit_equals_bigint_commit(name):
    P, fq = su.params(name)
    F = pyref.Field(fq)
    Pn = SimpleNamespace(**P)
    ck = random_ck(P, 7)
    ckl = [x.tolist() for x in ck]
    cj = co.CJindo(P, fq)
    for nv in sorted({P["rank"], max(1, P["rank"] - 3), 1}, reverse=True):
        v = su.synth_v(P, fq, nv, seed=nv)
        rnd = make_randomness(P, fq, seed=nv + 3)
        prnd = dict(last_row=co.from_limbs(rnd["last_row"]),
                    mask=[co.from_limbs(rnd["mask"][j]) for j in range(P["rows"])],
                    enc_noise=rnd["enc_noise"].tolist(), mlwe_noise=rnd["mlwe_noise"].tolist())
        com, op = pyref.commit(Pn, F, ckl, co.from_limbs(v), prnd)
        o = cj.commit(*ck, v, rnd["last_row"], rnd["mask"], rnd["enc_noise"], rnd["mlwe_noise"])
        assert (o["enc"] == np.array(op["Encode"], np.uint64)).all(), (name, nv)
        assert (o["mlwe"] == np.array(op["MLWE"], np.uint64)).all(), (name, nv)
        assert (o["incom"] == np.array(op["InCommit"], np.uint64)).all(), (name, nv)
        assert (o["com"] == np.array(com, np.uint64)).all(), (name, nv)


@pytest.mark.parametrize("name", ROUND_SHAPES)
def test_c_round_edges_equal_bigint_round(name):
    P, fq = su.params(name)
    cj = co.CJindo(P, fq)
    nqo, d = len(P["qo"]), P["d"]
    # inner round: ringQ -> ringQOut, cut = log_in_cut
    enc, mlwe, polys = su.inner_edge_case(P, seed=5)
    got = cj.commit_core(*random_ck(P, 9), enc, mlwe)["incom"]
    want = su.rounded(P, P["q"], P["qo"], polys, P["log_in_cut"])
    for p in range(len(polys)):
        su.explain(got[p], want[p], P["qo"], d, [lab for _, lab in polys[p]], f"{name} inner round, polynomial {p}")
    # outer round: ringQOut -> ringQOut, cut = log_out_cut
    ck, enc, mlwe, polys = su.outer_edge_case(P, seed=6)
    o = cj.commit_core(*ck, enc, mlwe)
    one = su.ntt_mform(P["qo"], d, [1] + [0] * (d - 1))
    assert (o["incom"][0] == one).all() and not o["incom"][1:].any(), name
    want = su.rounded(P, P["qo"], P["qo"], polys, P["log_out_cut"])
    for p in range(len(polys)):
        su.explain(o["com"][p][:nqo], want[p], P["qo"], d, [lab for _, lab in polys[p]],
                   f"{name} outer round, polynomial {p}")
        assert not o["com"][p][nqo:].any(), name


def test_every_edge_is_placed():
    """Each shape's polynomials together hold every edge of the list (d = 8 deals them out)."""
    for name in ROUND_SHAPES:
        P, _ = su.params(name)
        for primes, cut, polys in ((P["q"], P["log_in_cut"], su.inner_edge_case(P, 5)[2]),
                                   (P["qo"], P["log_out_cut"], su.outer_edge_case(P, 6)[3])):
            held = {lab for p in polys for _, lab in p}
            assert {lab for _, lab in su.edge_values(primes, cut)} <= held, name
            Q = math.prod(primes)
            assert any(v == Q >> 1 for p in polys for v, _ in p), name


_PROOFS = {}


def _proof(name):
    if name not in _PROOFS:
        if name in su.SYNTH:
            _PROOFS[name] = su.synth_proof(name, seed=31)
        else:
            from tests.jindo_proto import honest_proof
            P, fq = su.params(name)
            ck = random_ck(P, 31)
            pr = honest_proof(P, fq, ck, seed=31, B=1)
            r = su.verify_nm(P, fq, ck, pr, su.HUGE, su.HUGE)
            _PROOFS[name] = (P, fq, ck, pr, r["outer_sq"], r["inner_sq"])
    return _PROOFS[name]


@pytest.mark.parametrize("name", su.NAMES)
def test_honest_synth_proof_accepted_with_bigint_norms(name):
    P, fq, ck, pr, so, si = _proof(name)
    r = su.verify_nm(P, fq, ck, pr, P["in_com_dcmp_two_nm"], P["res_two_nm"])
    # verifyEval needs DecodeTo to be a ring homomorphism: p = b^exp + 1 and slots * exp = d.  The
    # three digit-loop sets pair p63 / jindo_zp with other bases, so there (and only there) an
    # honest proof fails verifyEval and passes the other three checks.
    assert r["flags"] == [True, True, True, su.is_jindo_field(P, fq)], (name, r["flags"])
    assert r["ok"] == su.is_jindo_field(P, fq)
    assert (so, si) == su.bigint_norms(P, ck, pr), name


@pytest.mark.parametrize("name", CRAFTED_SHAPES)
def test_crafted_proof_norms_equal_bigint(name):
    P, fq, ck, pr, _, _ = _proof(name)
    bad = su.crafted(P, pr, seed=77)
    r = su.verify_nm(P, fq, ck, bad, su.HUGE, su.HUGE)
    assert (r["outer_sq"], r["inner_sq"]) == su.bigint_norms(P, ck, bad), name
    h = math.prod(P["qo"]) >> 1
    assert r["outer_sq"] > (h + 1) ** 2  # terms of magnitude Q/2 (the tie and its neighbours) are in the sum
