"""GPU: the Jindo verifier's batch entry (rg_jindo_verify_multi_dev: n_proofs proofs against one handle
in one asynchronous call, a record per proof left on the device) against the C oracle's Verify of
each proof and, word for word, against the single entry rg_jindo_verify_dev on that proof alone.

Every proof slot has its own seed, so x, left, right, chals, bq / bo, com, y and the proof differ
pairwise: a dropped or mis-scaled proof stride gives a wrong record, not a lucky match.  A batch
shares one handle, hence one commit key: the synthetic sets take the key of su.synth_proof(name, 31)
and build the other slots' proofs against it as synth_proof does (its own key follows its seed).
`out` and `scratch` are all-ones words before every call, so a word nobody wrote shows up."""
import json
import math
import os

import numpy as np
import pytest

import coracle as co
from ringo import _lib, jindo
from tests import jindo_synth_util as su
from tests.jindo_proto import VERIFY_KEYS, honest_proof, left_right, mont, oracle_verify
from tests.jindo_util import make_randomness, make_v

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PARAMS = json.load(open(os.path.join(HERE, "golden", "jindo_params.json")))
W = jindo.VERIFY_WORDS
INVALID = _lib.STATUS["RG_ERR_INVALID"]


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to("cuda")


_SETS = {}


def _set(name):
    """{P (with bounds), fq, ck, vrf, proofs: []} of a golden or a synthetic set, cached."""
    if name not in _SETS:
        if name in su.SYNTH:
            P, fq, ck, pr, _, _ = su.synth_proof(name, seed=31)
            vrf = jindo.Verifier(jindo.Parameters.from_dict(P, fq), ck=ck)
        else:
            P = PARAMS[name]
            fq = int(P["field_q_hex"], 16)
            vrf = jindo.Verifier(jindo.Parameters.from_dict(P, fq), crs=b"Jindo!")
            ck = vrf._p.commit_key()
            pr = honest_proof(P, fq, ck, seed=31)
        _SETS[name] = dict(P=P, fq=fq, ck=ck, vrf=vrf, proofs=[pr], want={}, single={})
    return _SETS[name]


def _proofs(name, k):
    """The set and its first k honest proofs; slot i is drawn from seed 31 + 10 i."""
    s = _set(name)
    P, fq, ck = s["P"], s["fq"], s["ck"]
    while len(s["proofs"]) < k:
        seed = 31 + 10 * len(s["proofs"])
        if name in su.SYNTH:  # su.synth_proof's steps with this set's key
            v = su.synth_v(P, fq, P["rank"], seed + 1)[None]
            s["proofs"].append(honest_proof(P, fq, ck, seed=seed, rnd=make_randomness(P, fq, seed=seed + 2, batch=1), v=v))
        else:
            s["proofs"].append(honest_proof(P, fq, ck, seed=seed))
    return s, s["proofs"][:k]


def _want(s, pr, nm=None):
    """The oracle's Verify of one proof at the set's bounds (or nm = (outer, inner))."""
    no, ni = nm or (s["P"]["in_com_dcmp_two_nm"], s["P"]["res_two_nm"])
    return su.verify_nm(s["P"], s["fq"], s["ck"], pr, no, ni)


def _stack(proofs):
    """The proofs' Verify inputs, proof-major, on the device."""
    return [None if proofs[0][k] is None else _t(np.stack([pr[k] for pr in proofs])) for k in VERIFY_KEYS]


class _bounds:
    """The verifier's parameters with other norm bounds for the length of a with block."""

    def __init__(self, vrf, nm):
        self.p, self.nm = vrf.params, nm

    def __enter__(self):
        self.keep = (self.p.in_com_dcmp_two_nm, self.p.res_two_nm)
        if self.nm is not None:
            self.p.in_com_dcmp_two_nm, self.p.res_two_nm = self.nm

    def __exit__(self, *exc):
        self.p.in_com_dcmp_two_nm, self.p.res_two_nm = self.keep


def _buffers(vrf, n, batch):
    import torch
    nbytes = vrf.verify_multi_scratch_bytes(n, batch)
    assert nbytes > 0 and nbytes % 8 == 0
    return (torch.full((n, W), -1, dtype=torch.int64, device="cuda"),
            torch.full((nbytes // 8,), -1, dtype=torch.int64, device="cuda"))


def _enqueue(vrf, batch, dev, n, nm=None, stream=None):
    """One verify_multi_dev into all-ones buffers; returns (out, scratch) without synchronising."""
    out, scratch = _buffers(vrf, n, batch)
    with _bounds(vrf, nm):
        assert vrf.verify_multi_dev(n, batch, *dev, out, scratch, stream=stream) is None
    return out, scratch


def _words(out):
    return out.cpu().numpy().view(np.uint64)


def _multi(s, proofs, nm=None):
    """(records [n][W], unpacked results) of one call on the proofs."""
    out, _ = _enqueue(s["vrf"], proofs[0]["batch"], _stack(proofs), len(proofs), nm)
    w = _words(out)
    return w, s["vrf"].unpack_verify_words(w)


def _same(r, want):
    assert r.outer_norm_sq == want["outer_sq"]
    assert r.inner_norm_sq == want["inner_sq"]
    assert [r.outer_ok, r.inner_ok, r.consistency_ok, r.eval_ok] == want["flags"]
    assert (r.eval_lhs == want["eval_lhs"]).all() and (r.eval_rhs == want["eval_rhs"]).all()
    assert r.ok == want["ok"]


def _record_of(r, L):
    """The record the batch entry must leave for the single entry's result r."""
    rec = np.zeros(W, np.uint64)
    rec[0] = int(r.ok)
    rec[1] = int(r.outer_ok) | int(r.inner_ok) << 1 | int(r.consistency_ok) << 2 | int(r.eval_ok) << 3
    for i in range(10):
        rec[2 + i] = (r.outer_norm_sq >> (64 * i)) & ((1 << 64) - 1)
        rec[12 + i] = (r.inner_norm_sq >> (64 * i)) & ((1 << 64) - 1)
    rec[22:22 + L] = r.eval_lhs
    rec[38:38 + L] = r.eval_rhs
    return rec


def _single(s, pr, nm=None):
    with _bounds(s["vrf"], nm):
        return s["vrf"].verify_dev(pr["batch"], *[_t(pr[k]) for k in VERIFY_KEYS])


def _check(s, proofs, nm=None):
    """One batch call: every record equals the oracle's Verify and the single entry's result."""
    w, res = _multi(s, proofs, nm)
    L = s["vrf"].params.L
    for i, pr in enumerate(proofs):
        _same(res[i], _want(s, pr, nm))
        assert (w[i] == _record_of(_single(s, pr, nm), L)).all(), i
    return w, res


# ---- 1. parity with the oracle and with the single entry --------------------------------------------
SETS = ["t10_b1", "t10_b8", "p63_t10_b2", "zp880_t10_b1", "syn_d8_p63", "syn_d128_mixed4", "syn_d1024_mult",
        "syn_d256_q62top"]


@pytest.mark.parametrize("n", [1, 2, 3, 5])  # 3: a partial group of mac_kernel's 4 columns; 5: a group and a tail
@pytest.mark.parametrize("name", SETS)
def test_records_match_oracle_and_single_entry(name, n):
    s, proofs = _proofs(name, n)
    for a in range(n):  # the slots' inputs differ pairwise
        for b in range(a):
            for k in VERIFY_KEYS:
                if proofs[a][k] is not None and not (name == "zp880_t10_b1" and k == "chals"):
                    assert not (proofs[a][k] == proofs[b][k]).all(), (a, b, k)
    w, res = _check(s, proofs)
    if name not in su.SYNTH:
        assert all(r.ok for r in res)  # honest proofs verify (TestJindo)
    if name == "t10_b8":
        assert all(r.inner_norm_sq > 1 << 64 for r in res)  # a sum above one word


def test_wide_accumulators():
    """The sets above keep pdot_kernel and consistency_kernel on the two-word accumulator:
    2 log2(q - 1) + log2(terms + 1) < 127.5.  syn_d256_q62top's primes just below 2^62 with 11 columns
    and 12 rows put both kernels' products (11 and 12 terms: 127.58 and 127.70) on the third word."""
    P = dict(su.SYNTH["syn_d256_q62top"], rows=12, cols=11, in_com_dcmp_len=24)
    fq = int(P["field_q_hex"], 16)
    for terms in (P["rows"], P["cols"]):
        assert 2 * math.log2(max(P["q"]) - 1) + math.log2(terms + 1) >= 127.5
    ck = su.random_ck(P, 31)
    proofs = []
    for i in range(3):
        v = su.synth_v(P, fq, P["rank"], 32 + 10 * i)[None]
        proofs.append(honest_proof(P, fq, ck, seed=31 + 10 * i, rnd=make_randomness(P, fq, seed=33 + 10 * i, batch=1), v=v))
    sums = su.verify_nm(P, fq, ck, proofs[0], su.HUGE, su.HUGE)
    P["in_com_dcmp_two_nm"] = 2.0 * float(math.isqrt(sums["outer_sq"]))  # su.synth_proof's bounds
    P["res_two_nm"] = 2.0 * float(math.isqrt(sums["inner_sq"]))
    s = dict(P=P, fq=fq, ck=ck, vrf=jindo.Verifier(jindo.Parameters.from_dict(P, fq), ck=ck))
    _, res = _check(s, proofs)
    assert all(r.ok for r in res)
    bad = [_tampered(proofs[0], "pf_partial"), proofs[1], _tampered(proofs[2], "pf_enc")]
    _, res = _check(s, bad)
    assert [r.consistency_ok for r in res] == [False, True, False]


# ---- 2. a mixed batch: a rejection never leaks into a neighbour -------------------------------------
def _tampered(pr, what):
    """test_gpu_verify.py's change of one word."""
    bad = dict(pr)
    bad[what] = pr[what].copy()
    flat = bad[what].reshape(-1)
    i = min(5, flat.size - 1)
    flat[i] = (int(flat[i]) + 12345) % (1 << 40)
    return bad


@pytest.mark.parametrize("name", ["t10_b1", "t10_b8"])
def test_mixed_batch(name):
    """Six slots with one changed word each and an honest one between them, then the same slots in
    reversed order.  Seven slots, but two oracle proofs: the slots alternate between them."""
    s, proofs = _proofs(name, 2)
    kinds = ["pf_enc", "pf_incom", "y", "honest", "pf_partial", "pf_mlwe", "com"]
    batch = [proofs[i % 2] if k == "honest" else _tampered(proofs[i % 2], k) for i, k in enumerate(kinds)]
    want = [_want(s, pr) for pr in batch]
    assert [w["ok"] for w in want] == [k == "honest" for k in kinds]
    for order in (batch, batch[::-1]):
        _, res = _multi(s, order)
        for r, pr, w in zip(res, order, want if order is batch else want[::-1]):
            _same(r, w)


# ---- 3. the norm decision on the device is norm_below's ---------------------------------------------
@pytest.mark.parametrize("name", ["t10_b8", "syn_d128_mixed4"])
def test_norm_boundary_on_the_device(name):
    """test_norm_accept_boundary's bounds around proof 0's float(isqrt(S)); each proof's flag is the
    reference's float(isqrt(S_p)) < nm (verifyNorm :278-281)."""
    s, proofs = _proofs(name, 2)
    big = [_want(s, pr, (su.HUGE, su.HUGE)) for pr in proofs]
    so, si = [b["outer_sq"] for b in big], [b["inner_sq"] for b in big]
    assert so[0] != so[1] and si[0] != si[1]
    dev = _stack(proofs)
    for f, outer in ((float(math.isqrt(so[0])), True), (float(math.isqrt(si[0])), False)):
        for nm in (float(np.nextafter(f, 0)), f, float(np.nextafter(f, np.inf)), 0.0, 1e200):
            bounds = (nm, 1e200) if outer else (1e200, nm)
            out, _ = _enqueue(s["vrf"], proofs[0]["batch"], dev, 2, bounds)
            for p, r in enumerate(s["vrf"].unpack_verify_words(_words(out))):
                assert (r.outer_norm_sq, r.inner_norm_sq) == (so[p], si[p])
                want = float(math.isqrt(so[p] if outer else si[p])) < nm
                assert (r.outer_ok if outer else r.inner_ok) == want, (name, p, outer, nm)
                assert (r.inner_ok if outer else r.outer_ok) is True
                assert r.ok == (want and big[p]["flags"][2] and big[p]["flags"][3])


# ---- 4. crafted norms ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["syn_d128_mixed4", "t10_b1"])
def test_crafted_norms(name):
    """Responses holding the centring edges (|value| about Q / 2), another seed per slot."""
    s, proofs = _proofs(name, 2)
    bad = [su.crafted(s["P"], pr, seed=77 + 5 * i) for i, pr in enumerate(proofs)]
    want = [_want(s, pr) for pr in bad]
    assert want[0]["outer_sq"] != want[1]["outer_sq"] and want[0]["inner_sq"] != want[1]["inner_sq"]
    for w in want:
        assert w["outer_sq"] > (math.prod(s["P"]["qo"]) >> 1) ** 2 and w["inner_sq"] > (math.prod(s["P"]["q"]) >> 1) ** 2
    _, res = _multi(s, bad)
    for r, w in zip(res, want):
        _same(r, w)


# ---- 5. streams and the const handle -------------------------------------------------------------------
def test_two_streams_and_repeat():
    import torch
    s, proofs = _proofs("t10_b1", 5)
    a, b = proofs[:3], proofs[:1:-1]  # slots 0 1 2 and 4 3 2
    vrf = s["vrf"]
    da, db = _stack(a), _stack(b)
    (oa, sa), (ob, sb) = _buffers(vrf, 3, 1), _buffers(vrf, 3, 1)
    torch.cuda.synchronize()  # the uploads and the all-ones fills ran on the null stream
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    vrf.verify_multi_dev(3, 1, *da, oa, sa, stream=s1)
    vrf.verify_multi_dev(3, 1, *db, ob, sb, stream=s2)
    torch.cuda.synchronize()
    for out, batch in ((oa, a), (ob, b)):
        for r, pr in zip(s["vrf"].unpack_verify_words(_words(out)), batch):
            _same(r, _want(s, pr))
    o2, _ = _enqueue(s["vrf"], 1, da, 3)
    assert (_words(o2) == _words(oa)).all()


# ---- 6. refusals with a live handle --------------------------------------------------------------------
def test_refusals_leave_out_untouched():
    import torch
    s, proofs = _proofs("t10_b8", 2)
    vrf, B = s["vrf"], proofs[0]["batch"]
    lib = _lib.lib()
    dev = _stack(proofs)
    out, scratch = _buffers(vrf, 2, B)
    ptr = {k: t.data_ptr() for k, t in zip(VERIFY_KEYS, dev)}
    ptr.update(out=out.data_ptr(), scratch=scratch.data_ptr())

    def call(n=2, batch=B, **kw):
        a = dict(ptr, **kw)
        return lib.rg_jindo_verify_multi_dev(vrf.h, n, batch, *[a[k] for k in VERIFY_KEYS], 1e200, 1e200, a["out"],
                                             a["scratch"], None)

    cases = [dict(out=None), dict(scratch=None), dict(n=0), dict(n=65536), dict(batch=0), dict(bq=None), dict(bo=None),
             dict(out=ptr["y"]), dict(scratch=ptr["out"]), dict(com=None), dict(pf_mlwe=None),
             dict(batch=1)]  # batch == 1 with d_bq / d_bo given
    for kw in cases:
        assert call(**kw) == INVALID, kw
        assert "jindo verify multi" in lib.rg_last_error().decode(), kw
    assert lib.rg_jindo_verify_multi_scratch_bytes(vrf.h, 0, B) == 0
    assert lib.rg_jindo_verify_multi_scratch_bytes(vrf.h, 65536, B) == 0
    assert lib.rg_jindo_verify_multi_scratch_bytes(vrf.h, 65535, B) > 0
    torch.cuda.synchronize()
    assert (out == -1).all() and (scratch == -1).all()
    assert call() == 0  # the same arguments, unchanged, are accepted
    torch.cuda.synchronize()
    assert (_words(out)[:, 0] == 1).all()
    # the mirror's panics are verify_dev's
    p = vrf.params
    keep = p.res_two_nm
    p.res_two_nm = None
    try:
        with pytest.raises(jindo.RingoPanic, match="two-norm bounds"):
            vrf.verify_multi_dev(2, B, *dev, out, scratch)
    finally:
        p.res_two_nm = keep
    with pytest.raises(jindo.RingoPanic, match="words, need"):
        vrf.verify_multi_dev(3, B, *dev, out, scratch)  # buffers of two proofs
    host = [None if proofs[0][k] is None else np.stack([pr[k] for pr in proofs]) for k in VERIFY_KEYS]
    with pytest.raises(jindo.RingoPanic, match="params.batch"):
        vrf.VerifyMulti(B - 1, *host)
    assert [r.ok for r in vrf.VerifyMulti(B, *host)] == [True, True]


# ---- 7. TestJindo's flow for three provers, verified in one call ----------------------------------------
def test_three_provers_flow_verified_in_one_call():
    """test_jindo_flow_on_gpu's steps (device-sampled commits, Evaluate's device work) per prover."""
    import torch
    name = "t10_b1"
    s = _set(name)
    P, fq, ck, vrf = s["P"], s["fq"], s["ck"], s["vrf"]
    params = vrf.params
    prv = jindo.Prover(params, ck=ck)
    cj, F = co.CJindo(P, fq), co.CField(fq)
    nv, L = P["rank"], params.L
    sh, es = params.shapes(1), prv.eval_shapes()
    per = {k: [] for k in VERIFY_KEYS}
    for i in range(3):
        rng = np.random.default_rng(41 + i)
        v = make_v(fq, nv, seed=500 + i)[None]
        o = {k: torch.zeros(sh[k], dtype=torch.int64, device="cuda") for k in ("incom", "enc", "mlwe_out", "com")}
        prv.commit_sampled_dev(1, _t(v), nv, jindo.Seeds.derive(b"flow-multi-%d" % i), 0, o["incom"], o["enc"],
                               o["mlwe_out"], o["com"])
        x = mont(F, int.from_bytes(rng.bytes(40), "little"))
        e = {k: torch.zeros(es[k], dtype=torch.int64, device="cuda") for k in es}
        prv.eval_batch_dev(1, o["incom"], o["enc"], o["mlwe_out"], None, None, e["ob_incom"], e["ob_enc"], e["ob_mlwe"])
        left_e, right_e = left_right(P, F, x)
        left = np.stack([cj.encode(co.to_limbs([a], L)) for a in left_e])
        prv.eval_partial_dev(e["ob_enc"], _t(left), e["partial"])
        chals = np.stack([cj.encode_challenge(0, rng.bytes(16)) for _ in range(P["cols"])])
        prv.eval_respond_dev(e["ob_enc"], e["ob_mlwe"], _t(chals), e["pf_enc"], e["pf_mlwe"])
        y = F.evaluate(v[0], co.to_limbs([x], L)[0])[None]
        one = dict(com=o["com"], chals=_t(chals), left=_t(left), right=_t(co.to_limbs(right_e, L)), y=_t(y),
                   pf_incom=e["ob_incom"], pf_partial=e["partial"], pf_enc=e["pf_enc"], pf_mlwe=e["pf_mlwe"])
        for k, t in one.items():
            per[k].append(t.reshape(-1))
    dev = [None if not per[k] else torch.stack(per[k]).contiguous() for k in VERIFY_KEYS]
    out, _ = _enqueue(vrf, 1, dev, 3)
    res = vrf.unpack_verify_words(_words(out))
    assert [(r.ok, r.outer_ok, r.inner_ok, r.consistency_ok, r.eval_ok) for r in res] == [(True,) * 5] * 3
    dev[VERIFY_KEYS.index("pf_enc")][1, 7] += 1  # one response word of proof 1
    out, _ = _enqueue(vrf, 1, dev, 3)
    bad = vrf.unpack_verify_words(_words(out))
    assert [r.ok for r in bad] == [True, False, True]
    for i in (0, 2):
        assert (bad[i].outer_norm_sq, bad[i].inner_norm_sq) == (res[i].outer_norm_sq, res[i].inner_norm_sq)
