"""GPU: Prover.Evaluate for a batch of proofs in two asynchronous calls (include/ringo.h
rg_jindo_eval_open_multi_dev, rg_jindo_eval_respond_multi_dev), N = 3 proofs unless said otherwise,
every proof with its own point and its own bytes.

The comparator is twofold, both word for word (the results are canonical residues): the C oracle's
eval_batch / eval_partial / eval_respond / encode_challenge / encode with jindo_proto.left_right
(tests/jindo_eval_multi_util.oracle), and a loop of the single device entries.  Outputs and scratch are
poison words before every call, and guard words follow every output and the scratch.

The openings are residues dealt over the slots (Evaluate's arithmetic does not care whether they are
honest), except in the end-to-end test, whose proofs are jindo_proto.honest_proof's and go on into
rg_jindo_verify_multi_dev."""
import numpy as np
import pytest

import coracle as co
import ringo
from ringo import _lib, bigpoly, jindo
from tests import jindo_eval_multi_util as eu
from tests.jindo_proto import VERIFY_KEYS, random_ck

pytestmark = pytest.mark.gpu
N = eu.N
POISON = 0x5a5a5a5a5a5a5a5a
GUARD = 8
INVALID = _lib.STATUS["RG_ERR_INVALID"]


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to("cuda")


def _h(t):
    return t.cpu().numpy().view(np.uint64)


def _bytes(strs):
    import torch
    return torch.from_numpy(np.frombuffer(b"".join(strs), np.uint8).copy()).to("cuda")


_PRV, _WANT = {}, {}


def _prover(name):
    """One handle per parameter set (Evaluate never reads the commit key: a random one)."""
    if name not in _PRV:
        P, fq = eu.params(name)
        _PRV[name] = jindo.Prover(jindo.Parameters.from_dict(P, fq), ck=random_ck(P, 7))
    return _PRV[name]


def _case(name, batch, seed, fill="uniform"):
    """(case, oracle outputs), made once and left unchanged."""
    key = (name, batch, seed, fill)
    if key not in _WANT:
        c = eu.make_case(name, batch, seed, fill)
        _WANT[key] = (c, eu.oracle(c))
    return _WANT[key]


class _Bufs:
    """The outputs of both calls and their scratch, each followed by a guard, in one poisoned buffer."""

    def __init__(self, prv, n, batch):
        import torch
        es = prv.eval_shapes()
        w = lambda k: n * int(np.prod(es[k]))
        s1, s2 = prv.eval_open_multi_scratch_bytes(n, batch), prv.eval_respond_multi_scratch_bytes(n)
        assert s1 > 0 and s1 % 8 == 0 and s2 > 0 and s2 % 8 == 0
        self.words = dict(ob_enc=w("ob_enc") if batch > 1 else 0, ob_mlwe=w("ob_mlwe") if batch > 1 else 0,
                          pf_incom=w("ob_incom"), pf_partial=w("partial"), pf_enc=w("pf_enc"), pf_mlwe=w("pf_mlwe"),
                          scratch1=s1 // 8, scratch2=s2 // 8)
        self.buf = torch.full((sum(self.words.values()) + GUARD * len(self.words),), POISON, dtype=torch.int64,
                              device="cuda")
        self.t, self.guards, at = {}, [], 0
        for k, n_w in self.words.items():
            self.t[k] = self.buf[at:at + n_w] if n_w else None
            self.guards.append(self.buf[at + n_w:at + n_w + GUARD])
            at += n_w + GUARD

    def guards_intact(self):
        return all((_h(g) == np.uint64(POISON)).all() for g in self.guards)

    def all_poison(self):
        return bool((_h(self.buf) == np.uint64(POISON)).all())

    def ptr(self, k):
        return None if self.t[k] is None else self.t[k].data_ptr()


def _upload(c, layout="pc", n=N):
    """The case's inputs on the device: (incom, enc, mlwe, proof stride, commit stride, points, batch bytes,
    challenge bytes).  "pc": openings [proof][commit]; "cp": [commit][proof], as a commit per round leaves them."""
    B, L = c["batch"], co.CField(c["fq"]).L
    opens = [c[k][:n] for k in ("incom", "enc", "mlwe")]
    if layout == "cp":
        opens = [np.swapaxes(a, 0, 1) for a in opens]
    ps, cs = (B, 1) if layout == "pc" else (1, n)
    d_x = _t(co.to_limbs(c["xs"][:n], L))
    bb = _bytes([b for p in range(n) for b in c["bbytes"][p]]) if B > 1 else None
    cb = _bytes([b for p in range(n) for b in c["cbytes"][p]])
    return [_t(a) for a in opens] + [ps, cs, d_x, bb, cb]


def _run_multi(prv, c, layout="pc", n=N):
    """Both calls on the case into poisoned buffers; the host does nothing in between but hand over the bytes."""
    import torch
    B = c["batch"]
    b = _Bufs(prv, n, B)
    incom, enc, mlwe, ps, cs, d_x, bb, cb = _upload(c, layout, n)
    prv.eval_open_multi_dev(n, B, incom, enc, mlwe, ps, cs, d_x, 1, bb, b.t["ob_enc"], b.t["ob_mlwe"], b.t["pf_incom"],
                            b.t["pf_partial"], b.t["scratch1"])
    if B > 1:
        prv.eval_respond_multi_dev(n, b.t["ob_enc"], b.t["ob_mlwe"], 1, cb, b.t["pf_enc"], b.t["pf_mlwe"], b.t["scratch2"])
    else:  # openBatch = open[0]: the openings themselves, at their proof stride
        prv.eval_respond_multi_dev(n, enc, mlwe, ps, cb, b.t["pf_enc"], b.t["pf_mlwe"], b.t["scratch2"])
    torch.cuda.synchronize()
    return b


def _outputs(prv, b, n=N):
    es = prv.eval_shapes()
    shape = dict(ob_enc=es["ob_enc"], ob_mlwe=es["ob_mlwe"], pf_incom=es["ob_incom"], pf_partial=es["partial"],
                 pf_enc=es["pf_enc"], pf_mlwe=es["pf_mlwe"])
    return {k: _h(b.t[k]).reshape((n,) + shape[k]) for k in eu.OUT_KEYS if b.t[k] is not None}


def _run_single(prv, c, n=N):
    """The same proofs through the single entries, one proof at a time."""
    import torch
    P, B, p = c["P"], c["batch"], prv.params
    es, L = prv.eval_shapes(), prv.params.L
    new = lambda *s: torch.full(s, POISON, dtype=torch.int64, device="cuda")
    out = {k: [] for k in eu.OUT_KEYS}
    for i in range(n):
        d = {k: _t(c[k][i]) for k in ("incom", "enc", "mlwe")}
        e = {k: new(*es[k]) for k in es}
        left, chals = new(P["rows"], p.nq, P["d"]), new(P["cols"], p.nq, P["d"])
        bq = bo = None
        if B > 1:
            bq, bo, bb = new(B, p.nq, P["d"]), new(B, p.nqo, P["d"]), _bytes(c["bbytes"][i])
            prv.encode_challenges_dev(0, bb, B, bq)
            prv.encode_challenges_dev(1, bb, B, bo)
        prv.eval_batch_dev(B, d["incom"], d["enc"], d["mlwe"], bq, bo, e["ob_incom"], e["ob_enc"], e["ob_mlwe"])
        prv.eval_point_dev(_t(co.to_limbs([c["xs"][i]], L)[0]), left)
        prv.eval_partial_dev(e["ob_enc"], left, e["partial"])
        prv.encode_challenges_dev(0, _bytes(c["cbytes"][i]), P["cols"], chals)
        prv.eval_respond_dev(e["ob_enc"], e["ob_mlwe"], chals, e["pf_enc"], e["pf_mlwe"])
        torch.cuda.synchronize()
        for k, src in (("ob_enc", "ob_enc"), ("ob_mlwe", "ob_mlwe"), ("pf_incom", "ob_incom"), ("pf_partial", "partial"),
                       ("pf_enc", "pf_enc"), ("pf_mlwe", "pf_mlwe")):
            out[k].append(_h(e[src]))
    return {k: np.stack(v) for k, v in out.items()}


def _check(prv, c, want, n=N, layout="pc", single=True):
    b = _run_multi(prv, c, layout, n)
    got = _outputs(prv, b, n)
    tag = (c["name"], c["batch"], c["fill"], layout, n)
    if c["batch"] == 1:
        assert set(got) == set(eu.OUT_KEYS) - {"ob_enc", "ob_mlwe"}, tag
    for k, g in got.items():
        assert (g == want[k][:n]).all(), tag + (k, "oracle")
    assert b.guards_intact(), tag
    if single:
        one = _run_single(prv, c, n)
        for k, g in got.items():
            assert (g == one[k]).all(), tag + (k, "single entries")
    return got


# ---- 1. parity on golden sets ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t10_b8", "p63_t10_b2", "zp880_t10_b1"])
def test_parity_on_golden_sets(name):
    P, _ = eu.params(name)
    c, want = _case(name, P["batch"], seed=11)
    prv = _prover(name)
    got = _check(prv, c, want)
    if name == "zp880_t10_b1":  # ChallengeBound 1: the challenges are zero polynomials
        assert prv.challenge_bound() == 1
        assert (got["pf_enc"] == c["enc"][:, 0, P["cols"]]).all()


# ---- 2. both layouts ---------------------------------------------------------------------------
def test_both_opening_layouts_give_identical_outputs():
    c, want = _case("t10_b8", 8, seed=11)
    prv = _prover("t10_b8")
    a = _check(prv, c, want, layout="pc", single=False)
    b = _check(prv, c, want, layout="cp", single=False)
    for k in a:
        assert (a[k] == b[k]).all(), k


# ---- 3. shapes the tile can get wrong ----------------------------------------------------------
@pytest.mark.parametrize("name", ["syn_d8_p63", "syn_d128_mixed4", "syn_d1024_mult"])
def test_shapes_the_tile_can_get_wrong(name):
    P, _ = eu.params(name)
    if name == "syn_d8_p63":
        assert len(P["q"]) * P["d"] == 16  # a quarter of a tile
    if name == "syn_d128_mixed4":
        assert len(P["q"]) == 4 and len(P["qo"]) == 3 and len(set(q.bit_length() for q in P["q"])) == 4
    c, want = _case(name, 3, seed=13)
    _check(_prover(name), c, want)


@pytest.mark.parametrize("name,batch", [("syn_d8_p63", 32), ("syn_d8_p63", 33), ("syn_d64@rows=31", 2),
                                        ("syn_d64@rows=32", 2), ("syn_d64@rows=33", 33)])
def test_both_sides_of_the_kernel_thresholds(name, batch):
    """The fused kernel keeps the batch challenges in LDS up to 32 commits and reads them from global
    memory above, and splits the rows over 16 waves from 32 rows on and over 4 below (33 rows: one wave
    has three rows, the others two)."""
    c, want = _case(name, batch, seed=19)
    _check(_prover(name), c, want)


# ---- 4. accumulator widths ---------------------------------------------------------------------
@pytest.mark.parametrize("name,batch,fills", [("syn_d256_q62top", 20, ("uniform", "top", "crafted")),
                                              ("rows21", 2, ("uniform", "top"))])
def test_accumulator_widths(name, batch, fills):
    """syn_d256_q62top at batch 20: the sum over the batch needs the third word, the sum over its 5 rows
    does not; rows21 at batch 2: the reverse (tests/test_oracle_jindo_eval_multi.py pins both, and that the
    crafted fill holds a batch sum of at least 2^128).  Creating the handle is rg_jindo_create accepting the
    set."""
    P, _ = eu.params(name)
    assert eu.acc_wide(P["q"], batch) != eu.acc_wide(P["q"], P["rows"])
    prv = _prover(name)
    for fill in fills:
        c, want = _case(name, batch, seed=17, fill=fill)
        _check(prv, c, want, single=fill != "top")


# ---- 5. one proof ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t10_b8", "zp880_t10_b1"])
def test_one_proof_equals_the_single_entries(name):
    P, _ = eu.params(name)
    c, want = _case(name, P["batch"], seed=11)
    _check(_prover(name), c, want, n=1)


# ---- 6. refusals on the device -----------------------------------------------------------------
def _refusal_calls(prv, c, b, up, h=None):
    """(call1, call2): the raw entries with keyword overrides over the case's valid arguments."""
    lib = _lib.lib()
    incom, enc, mlwe, ps, cs, d_x, bb, cb = up
    B = c["batch"]
    a1 = dict(h=prv.h, n=N, batch=B, incom=incom.data_ptr(), enc=enc.data_ptr(), mlwe=mlwe.data_ptr(), ps=ps, cs=cs,
              x=d_x.data_ptr(), xs=1, bb=None if bb is None else bb.data_ptr(), ob_enc=b.ptr("ob_enc"),
              ob_mlwe=b.ptr("ob_mlwe"), pf_incom=b.ptr("pf_incom"), pf_partial=b.ptr("pf_partial"),
              scratch=b.ptr("scratch1"))
    ob = (b.ptr("ob_enc"), b.ptr("ob_mlwe"), 1) if B > 1 else (enc.data_ptr(), mlwe.data_ptr(), ps)
    a2 = dict(h=prv.h, n=N, ob_enc=ob[0], ob_mlwe=ob[1], stride=ob[2], cb=cb.data_ptr(), pf_enc=b.ptr("pf_enc"),
              pf_mlwe=b.ptr("pf_mlwe"), scratch=b.ptr("scratch2"))

    def call1(**kw):
        a = dict(a1, **kw)
        return lib.rg_jindo_eval_open_multi_dev(a["h"], a["n"], a["batch"], a["incom"], a["enc"], a["mlwe"], a["ps"],
                                                a["cs"], a["x"], a["xs"], a["bb"], a["ob_enc"], a["ob_mlwe"],
                                                a["pf_incom"], a["pf_partial"], a["scratch"], None)

    def call2(**kw):
        a = dict(a2, **kw)
        return lib.rg_jindo_eval_respond_multi_dev(a["h"], a["n"], a["ob_enc"], a["ob_mlwe"], a["stride"], a["cb"],
                                                   a["pf_enc"], a["pf_mlwe"], a["scratch"], None)

    return call1, call2, a1, a2


@pytest.mark.parametrize("name", ["t10_b8", "zp880_t10_b1"])
def test_refusals_touch_nothing_and_the_same_arguments_are_then_accepted(name):
    import torch
    lib = _lib.lib()
    P, _ = eu.params(name)
    B = P["batch"]
    c, want = _case(name, B, seed=11)
    prv = _prover(name)
    b, up = _Bufs(prv, N, B), _upload(c)
    call1, call2, a1, a2 = _refusal_calls(prv, c, b, up)
    spare = torch.full((64,), POISON, dtype=torch.int64, device="cuda")  # stands in for a buffer the rule forbids
    sp = spare.data_ptr()
    es = prv.eval_shapes()
    enc_words = int(np.prod(es["ob_enc"]))
    last_opening = a1["enc"] + 8 * enc_words * ((N - 1) * up[3] + (B - 1) * up[4])  # the strided extent's last opening
    cases1 = [dict(h=None), dict(n=0), dict(n=65536), dict(batch=0), dict(ps=0), dict(cs=0), dict(xs=0),
              dict(incom=None), dict(enc=None), dict(mlwe=None), dict(x=None), dict(pf_incom=None),
              dict(pf_partial=None), dict(scratch=None),
              dict(pf_partial=a1["enc"]), dict(pf_partial=last_opening + 8 * enc_words - 8), dict(scratch=a1["x"]),
              dict(pf_incom=a1["pf_partial"]), dict(scratch=a1["pf_incom"] + 8)]
    if B > 1:   # a buffer missing with batch > 1, batch == 1 claimed with the buffers given, outputs on each other
        cases1 += [dict(bb=None), dict(ob_enc=None), dict(ob_mlwe=None), dict(bb=None, ob_enc=None, ob_mlwe=None),
                   dict(batch=1), dict(ob_mlwe=a1["ob_enc"]), dict(ob_enc=a1["bb"]), dict(ob_enc=a1["mlwe"])]
    else:       # a buffer given with batch == 1
        cases1 += [dict(bb=sp), dict(ob_enc=sp), dict(ob_mlwe=sp), dict(bb=sp, ob_enc=sp + 128, ob_mlwe=sp + 256)]
    for kw in cases1:
        assert call1(**kw) == INVALID, (name, kw)
        assert lib.rg_last_error().decode().startswith("jindo eval multi"), (name, kw, lib.rg_last_error())
    cases2 = [dict(h=None), dict(n=0), dict(n=65536), dict(stride=0), dict(ob_enc=None), dict(ob_mlwe=None),
              dict(cb=None), dict(pf_enc=None), dict(pf_mlwe=None), dict(scratch=None), dict(pf_enc=a2["ob_enc"]),
              dict(pf_mlwe=a2["pf_enc"]), dict(scratch=a2["cb"]), dict(scratch=a2["pf_mlwe"] + 8),
              dict(pf_mlwe=a2["ob_enc"] + 8 * enc_words * (N - 1) * a2["stride"] + 8 * enc_words - 8)]
    for kw in cases2:
        assert call2(**kw) == INVALID, (name, kw)
        assert lib.rg_last_error().decode().startswith("jindo eval multi"), (name, kw, lib.rg_last_error())
    torch.cuda.synchronize()
    assert b.all_poison() and (_h(spare) == np.uint64(POISON)).all(), name
    for k, a in zip(("incom", "enc", "mlwe"), up[:3]):  # the inputs are as uploaded
        assert (_h(a).reshape(c[k].shape) == c[k]).all(), (name, k)
    assert call1() == 0 and call2() == 0  # the same arguments, unchanged, are accepted
    torch.cuda.synchronize()
    got = _outputs(prv, b)
    for k, g in got.items():
        assert (g == want[k]).all(), (name, k)
    assert b.guards_intact(), name
    for n, batch in ((0, B), (65536, B), (N, 0)):
        assert prv.eval_open_multi_scratch_bytes(n, batch) == 0
    assert prv.eval_respond_multi_scratch_bytes(0) == 0 and prv.eval_respond_multi_scratch_bytes(65536) == 0


def test_challenge_bound_of_zero_is_refused():
    import torch
    lib = _lib.lib()
    P, fq = eu.params("syn_d128_mixed4")
    Q = dict(P, exp=121, slots=1)  # slots * exp <= d = 128: ChallengeBound() = min(base, 1 << 0) / 2 = 0
    big = jindo.Prover(jindo.Parameters.from_dict(Q, fq), ck=random_ck(Q, 7))
    with pytest.raises(_lib.RingoError):
        big.challenge_bound()
    c, _ = _case("syn_d128_mixed4", 3, seed=13)
    b, up = _Bufs(big, N, 3), _upload(c)
    call1, call2, _, _ = _refusal_calls(big, c, b, up)
    for call in (call1, call2):
        assert call() == INVALID
        why = lib.rg_last_error().decode()
        assert why.startswith("jindo eval multi") and "ChallengeBound" in why
    torch.cuda.synchronize()
    assert b.all_poison()


# ---- 7. end to end -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t10_b8", "t10_b1"])
def test_end_to_end_into_the_batch_verifier(name):
    """Honest proofs: the two calls, rg_poly_evaluate_multi_dev, rg_jindo_verify_inputs_multi_dev on the same
    bytes, rg_jindo_verify_multi_dev.  The transcripts are replayed as test_gpu_jindo_verify_inputs_multi.py
    replays them (its _set pins the replay against the proofs' own encodings)."""
    import torch
    from tests.test_gpu_jindo_verify_inputs_multi import _set
    s = _set(name)
    P, fq, vrf, proofs, scripts = s["P"], s["fq"], s["vrf"], s["proofs"], s["scripts"]
    prv, B, L = vrf._p, P["batch"], vrf.params.L
    c = dict(name=name, P=P, fq=fq, batch=B, fill="honest", xs=[x for x, _, _ in scripts],
             bbytes=[bs for _, bs, _ in scripts], cbytes=[cs for _, _, cs in scripts],
             **{k: np.stack([pr["opens"][k] for pr in proofs]) for k in ("incom", "enc", "mlwe")})
    want = {k: np.stack([pr[k] for pr in proofs]) for k in ("pf_incom", "pf_partial", "pf_enc", "pf_mlwe")}
    new = lambda *sh: torch.full(sh, POISON, dtype=torch.int64, device="cuda")
    incom, enc, mlwe, ps, cs, d_x, bb, cb = _upload(c)

    def prove(cb2):
        b = _Bufs(prv, N, B)
        prv.eval_open_multi_dev(N, B, incom, enc, mlwe, ps, cs, d_x, 1, bb, b.t["ob_enc"], b.t["ob_mlwe"],
                                b.t["pf_incom"], b.t["pf_partial"], b.t["scratch1"])
        ob = (b.t["ob_enc"], b.t["ob_mlwe"], 1) if B > 1 else (enc, mlwe, ps)
        prv.eval_respond_multi_dev(N, *ob, cb2, b.t["pf_enc"], b.t["pf_mlwe"], b.t["scratch2"])
        return b

    def verify(b):
        p = vrf.params
        pq, nv = p.nq * P["d"], proofs[0]["v"].shape[1]
        # the evaluations: polynomial (proof, commit) at the proof's point
        RF = ringo.Field(fq)
        d_v = _t(np.stack([pr["v"] for pr in proofs]))
        y = new(N * B, L)
        scr = new((bigpoly.evaluate_multi_scratch_bytes(RF, nv, N * B, N) + 7) // 8)
        bigpoly.evaluate_multi_dev(RF, d_v, nv, nv, N * B, d_x, 1, N, B, y, scr)
        i = dict(bq=new(N * B * pq) if B > 1 else None, bo=new(N * B * p.nqo * P["d"]) if B > 1 else None,
                 chals=new(N * P["cols"] * pq), left=new(N * P["rows"] * pq), right=new(N * P["cols"] * P["slots"] * L))
        vrf.verify_inputs_multi_dev(N, B, d_x, 1, bb, cb, i["bq"], i["bo"], i["chals"], i["left"], i["right"],
                                    new(vrf.verify_inputs_multi_scratch_bytes(N) // 8))
        dev = dict(i, y=y, com=_t(np.stack([pr["com"] for pr in proofs])), **{k: b.t[k] for k in want})
        out = new(N, jindo.VERIFY_WORDS)
        vrf.verify_multi_dev(N, B, *[dev[k] for k in VERIFY_KEYS], out, new(vrf.verify_multi_scratch_bytes(N, B) // 8))
        torch.cuda.synchronize()
        assert (_h(y).reshape(N, B, L) == np.stack([pr["y"] for pr in proofs])).all(), name
        return vrf.unpack_verify_words(_h(out))

    b = prove(cb)
    res = verify(b)
    got = _outputs(prv, b)
    for k in want:
        assert (got[k] == want[k]).all(), (name, k)
    assert b.guards_intact(), name
    assert [(r.ok, r.outer_ok, r.inner_ok, r.consistency_ok, r.eval_ok) for r in res] == [(True,) * 5] * N
    # the challenge bytes of proofs 0 and 1 swapped in call 2 only
    swapped = _bytes([x for p in (1, 0, 2) for x in scripts[p][2]])
    res = verify(prove(swapped))
    for r in res[:2]:
        assert not r.ok and not (r.consistency_ok and r.inner_ok), name
    assert res[2].ok, name
