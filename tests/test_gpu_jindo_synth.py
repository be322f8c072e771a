"""GPU: the Jindo kernels on parameter sets NewParameters never produces
(tests/golden/jindo_synth_params.json; DESIGN.md, "Which Jindo shape takes which kernel"), bit for
bit against the C oracle, which test_oracle_jindo_synth.py pins against big-int restatements on
these same inputs.  No tolerances anywhere.

  * Commit (host entry and commit_dev, batch 3) with injected randomness, full and ragged v whose
    values sit on the digit boundaries; the extreme-noise vector; commit_core on uniform and on
    all-(q - 1) operands;
  * Evaluate's three device steps and Verify on an honest proof and on six tampered ones;
  * the rounding and centring decisions of round_kernel and round256_kernel on polynomials of exact
    integers (the tie Q>>1, Q/2 +- 1, negative exact multiples of 2^cut, -(2^cut) +- 1, residues
    that vanish in one limb), through the inner and the outer round;
  * the verifier's norms on proofs holding those edges, and the library's norm_below at the accept
    boundary float(isqrt(S)) and its two neighbours;
  * device sampling refused, with a reason, for d != 256.
"""
import math

import numpy as np
import pytest

import coracle as co
from ringo import jindo
from tests import jindo_synth_util as su
from tests.jindo_proto import VERIFY_KEYS, random_ck
from tests.jindo_util import make_randomness

pytestmark = pytest.mark.gpu

# (inner, outer) MAC of each set: the MFMA digit MAC needs d % 16 == 0 and T q^2 < 2^126
MAC_KINDS = {n: ("mfma", "mfma") for n in su.NAMES}
MAC_KINDS["syn_d8_p63"] = MAC_KINDS["syn_d256_q62top"] = ("generic", "generic")
ROUND_SYNTH = [n for n in su.NAMES if su.SYNTH[n]["d"] != 256] + ["syn_d256_q62", "syn_d256_q62top"]
ROUND_FIXTURE = ["t10_b1", "zp880_t10_b1", "mult_t8193_b12"]  # round256_kernel: one-limb outer / inner ring, three limbs
EXT = np.array([2**63 - 1, -(2**63 - 1), 2**62 + 12345, -(2**61), 2**45 + 1, -(2**44), 2**40, -7], dtype=np.int64)


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda")


def _h(t):
    return t.cpu().numpy().view(np.uint64)


def _poison():
    """Hand the runtime back a block of all-ones words, so that a kernel reading words nobody wrote
    is likelier to read garbage than zeros."""
    import torch
    x = torch.full((1 << 21,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    del x
    torch.cuda.empty_cache()


_PRV = {}


def _prover(name, key="uniform"):
    """A cached prover of the set with a uniform random key, or the all-(q_l - 1) key."""
    if (name, key) not in _PRV:
        P, fq = su.params(name)
        params = jindo.Parameters.from_dict(P, fq)
        ck = random_ck(P, 7)
        if key == "max":
            for a, primes in zip(ck, (P["q"], P["q"], P["qo"])):
                for l, p in enumerate(primes):
                    a[..., l, :] = p - 1
        _poison()
        _PRV[(name, key)] = (P, fq, params, ck, jindo.Prover(params, ck=ck))
    return _PRV[(name, key)]


def _same4(got_com, got_op, want, what):
    assert (got_op[1] == want["enc"]).all(), (what, "Encode")
    assert (got_op[2] == want["mlwe"]).all(), (what, "MLWE")
    assert (got_op[0] == want["incom"]).all(), (what, "InCommit")
    assert (got_com == want["com"]).all(), (what, "Commitment")


@pytest.mark.parametrize("name", su.NAMES)
def test_create_takes_the_expected_mac(name):
    assert _prover(name)[4].mac_kinds() == MAC_KINDS[name]


@pytest.mark.parametrize("name", su.NAMES)
def test_commit_matches_oracle(name):
    import torch
    P, fq, params, ck, prv = _prover(name)
    cj = co.CJindo(P, fq)
    nvs = sorted({P["rank"], max(1, P["rank"] - 3), 1}, reverse=True)
    for nv in nvs:
        v = su.synth_v(P, fq, nv, seed=nv)
        rnd = make_randomness(P, fq, seed=nv + 3)
        com, op = prv.Commit(v, jindo.Randomness(**rnd))
        want = cj.commit(*ck, v, rnd["last_row"], rnd["mask"], rnd["enc_noise"], rnd["mlwe_noise"])
        _same4(com.Value, (op.InCommit, op.Encode, op.MLWE), want, (name, nv))
    B = 3
    sh = params.shapes(B)
    for nv in nvs:
        vs = np.stack([su.synth_v(P, fq, nv, seed=50 + b) for b in range(B)])
        rnd = make_randomness(P, fq, seed=60 + nv, batch=B)
        o = {k: torch.full(sh[k], 0x5a5a, dtype=torch.int64, device="cuda") for k in ("incom", "enc", "mlwe_out", "com")}
        prv.commit_dev(B, _t(vs), nv, _t(rnd["last_row"]), _t(rnd["mask"]), _t(rnd["enc_noise"]), _t(rnd["mlwe_noise"]),
                       o["incom"], o["enc"], o["mlwe_out"], o["com"])
        torch.cuda.synchronize()
        for b in range(B):
            want = cj.commit(*ck, vs[b], *[rnd[k][b] for k in ("last_row", "mask", "enc_noise", "mlwe_noise")])
            _same4(_h(o["com"][b]), (_h(o["incom"][b]), _h(o["enc"][b]), _h(o["mlwe_out"][b])), want, (name, nv, b))


@pytest.mark.parametrize("name", ["syn_d128_q2", "syn_d256_q62", "syn_d128_mixed4"])
def test_commit_extreme_noise_matches_oracle(name):
    """test_gpu_jindo.py's extreme-noise vector (|s| up to 2^63 - 1) at the same positions, through
    prep_kernel's signed_residue."""
    P, fq, params, ck, prv = _prover(name)
    v = su.synth_v(P, fq, P["rank"], seed=3)
    rnd = make_randomness(P, fq, seed=11)
    rng = np.random.default_rng(12)
    en = rnd["enc_noise"]
    idx = rng.integers(0, en.size, size=4000)
    en.reshape(-1)[idx] = EXT[rng.integers(0, EXT.size, size=idx.size)]
    mn = rnd["mlwe_noise"]
    mn.reshape(-1)[rng.integers(0, mn.size, size=500)] = EXT[rng.integers(0, EXT.size, size=500)]
    com, op = prv.Commit(v, jindo.Randomness(**rnd))
    want = co.CJindo(P, fq).commit(*ck, v, rnd["last_row"], rnd["mask"], rnd["enc_noise"], rnd["mlwe_noise"])
    _same4(com.Value, (op.InCommit, op.Encode, op.MLWE), want, name)


@pytest.mark.parametrize("name", su.NAMES)
def test_commit_core_uniform_and_max_operands(name):
    P, fq, params, ck, prv = _prover(name)
    sh = params.shapes()
    rng = np.random.default_rng(5)
    enc, mlwe = np.zeros(sh["enc"], np.uint64), np.zeros(sh["mlwe_out"], np.uint64)
    for l, p in enumerate(P["q"]):
        enc[..., l, :] = rng.integers(0, p, size=enc[..., l, :].shape, dtype=np.uint64)
        mlwe[..., l, :] = rng.integers(0, p, size=mlwe[..., l, :].shape, dtype=np.uint64)
    com, incom = prv.commit_core(enc, mlwe)
    want = co.CJindo(P, fq).commit_core(*ck, enc, mlwe)
    assert (incom == want["incom"]).all() and (com == want["com"]).all(), (name, "uniform")
    _, _, _, ckm, prm = _prover(name, "max")
    for l, p in enumerate(P["q"]):
        enc[..., l, :] = p - 1
        mlwe[..., l, :] = p - 1
    com, incom = prm.commit_core(enc, mlwe)
    want = co.CJindo(P, fq).commit_core(*ckm, enc, mlwe)
    assert (incom == want["incom"]).all() and (com == want["com"]).all(), (name, "all q - 1")


# ---- Evaluate and Verify ----------------------------------------------------------------------
_PROOF = {}


def _proof(name):
    """(P with bounds, fq, ck, proof, S_outer, S_inner, verifier) of a synthetic set, cached."""
    if name not in _PROOF:
        P, fq, ck, pr, so, si = su.synth_proof(name, seed=31)
        _PROOF[name] = (P, fq, ck, pr, so, si, jindo.Verifier(jindo.Parameters.from_dict(P, fq), ck=ck))
    return _PROOF[name]


def _same(r, want):
    assert r.outer_norm_sq == want["outer_sq"]
    assert r.inner_norm_sq == want["inner_sq"]
    assert [r.outer_ok, r.inner_ok, r.consistency_ok, r.eval_ok] == want["flags"]
    assert (r.eval_lhs == want["eval_lhs"]).all() and (r.eval_rhs == want["eval_rhs"]).all()
    assert r.ok == want["ok"]


def _gpu_verify(vrf, pr, nm_out=None, nm_in=None, dev=None):
    """verify_dev with the given bounds (default: the parameters'); dev: the proof's device buffers."""
    p = vrf.params
    keep = (p.in_com_dcmp_two_nm, p.res_two_nm)
    try:
        if nm_out is not None:
            p.in_com_dcmp_two_nm, p.res_two_nm = nm_out, nm_in
        return vrf.verify_dev(pr["batch"], *(dev or [_t(pr[k]) for k in VERIFY_KEYS]))
    finally:
        p.in_com_dcmp_two_nm, p.res_two_nm = keep


@pytest.mark.parametrize("name", su.NAMES)
def test_evaluate_steps_and_verify_match_oracle(name):
    import torch
    P, fq, ck, pr, so, si, vrf = _proof(name)
    prv = vrf._p
    es = prv.eval_shapes()
    e = {k: torch.full(es[k], 0x5a5a, dtype=torch.int64, device="cuda") for k in es}
    op = pr["opens"]
    prv.eval_batch_dev(1, _t(op["incom"]), _t(op["enc"]), _t(op["mlwe"]), None, None, e["ob_incom"], e["ob_enc"],
                       e["ob_mlwe"])
    prv.eval_partial_dev(e["ob_enc"], _t(pr["left"]), e["partial"])
    prv.eval_respond_dev(e["ob_enc"], e["ob_mlwe"], _t(pr["chals"]), e["pf_enc"], e["pf_mlwe"])
    torch.cuda.synchronize()
    for k, w in (("ob_incom", "pf_incom"), ("partial", "pf_partial"), ("pf_enc", "pf_enc"), ("pf_mlwe", "pf_mlwe")):
        assert (_h(e[k]) == pr[w]).all(), (name, w)
    want = su.verify_nm(P, fq, ck, pr, P["in_com_dcmp_two_nm"], P["res_two_nm"])
    # an honest proof passes; verifyEval only where DecodeTo is a ring homomorphism (p = b^exp + 1 and
    # slots * exp = d: not the three digit-loop sets, which pair a field with another base)
    assert want["flags"] == [True, True, True, su.is_jindo_field(P, fq)], (name, want["flags"])
    assert (want["outer_sq"], want["inner_sq"]) == (so, si)
    _same(_gpu_verify(vrf, pr), want)


def _tamper(P, fq, pr, what):
    bad = dict(pr)
    bad[what] = pr[what].copy()
    flat = bad[what].reshape(-1)
    if what == "y":
        flat[0] ^= np.uint64(1)
        assert flat.size > 1 or int(flat[0]) < fq
    else:  # one residue of limb 0 moved to another canonical residue
        p = (P["qo"] if what in ("pf_incom", "com") else P["q"])[0]
        i = min(5, P["d"] - 1)
        flat[i] = (int(flat[i]) + 12345) % p
    assert not (bad[what] == pr[what]).all()
    return bad


@pytest.mark.parametrize("name", su.NAMES)
@pytest.mark.parametrize("what", ["pf_enc", "pf_incom", "pf_partial", "pf_mlwe", "y", "com"])
def test_tampered_verify_matches_oracle(name, what):
    """One changed word of each proof part.  pf_enc / pf_partial / y trip verifyConsistency or
    verifyEval, so the oracle rejects them.  pf_incom / pf_mlwe / com are caught by the norm checks
    alone, and on these sets no bound of 2 ||honest|| can: with cuts of 20 / 10 bits against 40- to
    62-bit primes InCommit wraps mod Q', so an honest proof's polynomials already have the norm of
    uniform residues and the oracle (the reference's verifyNorm) accepts the changed word.  There the
    change must show in the exact sums, and the verdict is also compared at the tight bound
    float(isqrt(S_honest)), which rejects the honest proof itself."""
    P, fq, ck, pr, so, si, vrf = _proof(name)
    bad = _tamper(P, fq, pr, what)
    want = su.verify_nm(P, fq, ck, bad, P["in_com_dcmp_two_nm"], P["res_two_nm"])
    _same(_gpu_verify(vrf, bad), want)
    if what in ("pf_enc", "pf_partial", "y"):
        assert not want["ok"], (name, what)
        assert not all(want["flags"][2:]), (name, what, want["flags"])
    else:
        assert want["outer_sq"] != so if what in ("pf_incom", "com") else want["inner_sq"] != si, (name, what)
        fo, fi = float(math.isqrt(so)), float(math.isqrt(si))
        tight = su.verify_nm(P, fq, ck, bad, fo, fi)
        assert tight["flags"][:2] == [float(math.isqrt(tight["outer_sq"])) < fo, float(math.isqrt(tight["inner_sq"])) < fi]
        _same(_gpu_verify(vrf, bad, fo, fi), tight)


@pytest.mark.parametrize("name", [n for n in su.NAMES if su.SYNTH[n]["d"] != 256])
def test_device_sampling_refused_off_d256(name):
    import torch
    from ringo._lib import RingoError
    P, fq = su.params(name)
    params = jindo.Parameters.from_dict(P, fq)
    params.stddevs = (4.8, 1.2e6, 1.7e3, 4.2e8, 6.8, 2.5e3)  # the order of magnitude of NewParameters' widths
    prv = jindo.Prover(params, ck=random_ck(P, 7))
    v = su.synth_v(P, fq, 1, seed=5)[None]
    sh = params.shapes(1)
    o = {k: torch.zeros(sh[k], dtype=torch.int64, device="cuda") for k in sh}
    seeds = jindo.Seeds.derive(b"synth")
    with pytest.raises(RingoError, match="device sampling needs d = 256"):
        prv.sample_dev(1, _t(v), 1, seeds, 0, o["last_row"], o["mask"], o["enc_noise"], o["mlwe_noise"])
    with pytest.raises(RingoError, match="device sampling needs d = 256"):
        prv.commit_sampled_dev(1, _t(v), 1, seeds, 0, o["incom"], o["enc"], o["mlwe_out"], o["com"])


# ---- rounding and centring edges on both round kernels ---------------------------------------------
def _fixture_prover(name):
    """The cached prover of test_gpu_verify.py's module for a jindo_params.json shape."""
    from tests.test_gpu_verify import _setup
    P, fq, params, vrf, ck, _ = _setup(name)
    return P, fq, params, ck, vrf._p


@pytest.mark.parametrize("name", ROUND_SYNTH + ROUND_FIXTURE)
def test_inner_round_edges(name):
    P, fq, params, ck, prv = _prover(name) if name in su.SYNTH else _fixture_prover(name)
    enc, mlwe, polys = su.inner_edge_case(P, seed=5)
    _, incom = prv.commit_core(enc, mlwe)
    want = co.CJindo(P, fq).commit_core(*ck, enc, mlwe)["incom"]
    for p in range(len(polys)):
        su.explain(incom[p], want[p], P["qo"], P["d"], [lab for _, lab in polys[p]], f"{name} inner round, polynomial {p}")


@pytest.mark.parametrize("name", ROUND_SYNTH + ROUND_FIXTURE)
def test_outer_round_edges(name):
    P, fq = su.params(name)
    ck, enc, mlwe, polys = su.outer_edge_case(P, seed=6)
    prv = jindo.Prover(jindo.Parameters.from_dict(P, fq), ck=ck)
    com, incom = prv.commit_core(enc, mlwe)
    want = co.CJindo(P, fq).commit_core(*ck, enc, mlwe)
    assert (incom == want["incom"]).all(), name
    nqo = len(P["qo"])
    for p in range(len(polys)):
        su.explain(com[p][:nqo], want["com"][p][:nqo], P["qo"], P["d"], [lab for _, lab in polys[p]],
                   f"{name} outer round, polynomial {p}")
    assert (com == want["com"]).all(), name


# ---- verifier norm edges and the accept boundary -------------------------------------------------
def _any_proof(name):
    """(P, fq, ck, proof, verifier): a synthetic set's, or test_gpu_verify.py's cached honest proof."""
    if name in su.SYNTH:
        P, fq, ck, pr, _, _, vrf = _proof(name)
        return P, fq, ck, pr, vrf
    from tests.test_gpu_verify import _setup
    P, fq, params, vrf, ck, pr = _setup(name)
    return P, fq, ck, pr, vrf


@pytest.mark.parametrize("name", ["syn_d128_mixed4", "syn_d128_q2", "t10_b1", "mult_t8193_b12"])
def test_crafted_proof_norms_match_oracle(name):
    """Responses holding the centring edges: norm sums with |value| about Q/2 terms, the lift's
    round with cut 0 at the tie."""
    P, fq, ck, pr, vrf = _any_proof(name)
    bad = su.crafted(P, pr, seed=77)
    want = su.verify_nm(P, fq, ck, bad, P["in_com_dcmp_two_nm"], P["res_two_nm"])
    assert not want["ok"]
    assert want["outer_sq"] > (math.prod(P["qo"]) >> 1) ** 2 and want["inner_sq"] > (math.prod(P["q"]) >> 1) ** 2
    _same(_gpu_verify(vrf, bad), want)


@pytest.mark.parametrize("name", ["t10_b1", "t10_b8", "syn_d128_mixed4"])
def test_norm_accept_boundary(name):
    """The library's norm_below at float(isqrt(S)) and its two neighbours, at 0 and at a bound whose
    square exceeds the sum's 640 bits: the flag is the reference's float(isqrt(S)) < nm (verifyNorm)."""
    P, fq, ck, pr, vrf = _any_proof(name)
    dev = [_t(pr[k]) for k in VERIFY_KEYS]
    big = su.verify_nm(P, fq, ck, pr, su.HUGE, su.HUGE)
    so, si = big["outer_sq"], big["inner_sq"]
    if name == "t10_b8":
        assert si > 1 << 64  # a sum above one word
    fo, fi = float(math.isqrt(so)), float(math.isqrt(si))
    for f, outer in ((fo, True), (fi, False)):
        for nm in (float(np.nextafter(f, 0)), f, float(np.nextafter(f, np.inf)), 0.0, 1e200):
            no, ni = (nm, 1e200) if outer else (1e200, nm)
            r = _gpu_verify(vrf, pr, no, ni, dev=dev)
            assert (r.outer_norm_sq, r.inner_norm_sq) == (so, si)
            want = float(math.isqrt(so if outer else si)) < nm
            assert (r.outer_ok if outer else r.inner_ok) == want, (name, "outer" if outer else "inner", nm)
            assert (r.inner_ok if outer else r.outer_ok) is True
            w = su.verify_nm(P, fq, ck, pr, no, ni)
            assert [r.outer_ok, r.inner_ok, r.consistency_ok, r.eval_ok] == w["flags"]
