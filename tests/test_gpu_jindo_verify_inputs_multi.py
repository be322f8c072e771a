"""GPU: the batch verifier's whole front end in one call (rg_jindo_verify_inputs_multi_dev: the three
encodeChallengeTo passes and the point pass for n_proofs proofs, from the bytes of their transcripts)
against the inputs the C oracle's honest proofs were built from, and then straight into
rg_jindo_verify_multi_dev.

tests/jindo_proto.honest_proof draws its transcript from np.random.default_rng(seed) and keeps the
encodings, not the bytes; the bytes are recovered here by replaying its draws in its order (192
bytes of sampler seeds, 40 bytes of x, batch x 16, cols x 16), and the replay is pinned by encoding
the replayed bytes with the oracle and comparing with the proof's own bq, bo, chals and x.
Outputs and scratch are poison words before every call, and poison words follow every output."""
import json
import os

import numpy as np
import pytest

import coracle as co
from ringo import _lib, jindo
from tests.jindo_proto import VERIFY_KEYS, honest_proof, mont

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PARAMS = json.load(open(os.path.join(HERE, "golden", "jindo_params.json")))
SETS = ["t10_b8", "zp880_t10_b1"]  # batch 8: bq / bo present; batch 1, ChallengeBound 1, L = 14
N = 3
POISON = 0x5a5a5a5a5a5a5a5a
GUARD = 8
INVALID = _lib.STATUS["RG_ERR_INVALID"]
OUTS = ("bq", "bo", "chals", "left", "right")


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to("cuda")


def _h(t):
    return t.cpu().numpy().view(np.uint64)


def _replay(P, F, seed):
    """honest_proof's draws from its generator: (x, batch bytes, challenge bytes)."""
    rng = np.random.default_rng(seed)
    rng.bytes(192)
    x = mont(F, int.from_bytes(rng.bytes(40), "little"))
    bbytes = [rng.bytes(16) for _ in range(P["batch"])]
    cbytes = [rng.bytes(16) for _ in range(P["cols"])]
    return x, bbytes, cbytes


_SETS = {}


def _set(name):
    """The set's verifier, three honest proofs against one key and their replayed transcripts; built once."""
    if name not in _SETS:
        P = PARAMS[name]
        fq = int(P["field_q_hex"], 16)
        vrf = jindo.Verifier(jindo.Parameters.from_dict(P, fq), crs=b"Jindo!")
        ck = vrf._p.commit_key()
        cj, F = co.CJindo(P, fq), co.CField(fq)
        proofs, scripts = [], []
        for i in range(N):
            seed = 31 + 10 * i
            pr = honest_proof(P, fq, ck, seed=seed)
            x, bbytes, cbytes = _replay(P, F, seed)
            # the replay is honest_proof's transcript
            assert x == pr["x"]
            assert (np.stack([cj.encode_challenge(0, b) for b in cbytes]) == pr["chals"]).all()
            if P["batch"] > 1:
                assert (np.stack([cj.encode_challenge(0, b) for b in bbytes]) == pr["bq"]).all()
                assert (np.stack([cj.encode_challenge(1, b) for b in bbytes]) == pr["bo"]).all()
            else:
                assert pr["bq"] is None and pr["bo"] is None
            proofs.append(pr)
            scripts.append((x, bbytes, cbytes))
        _SETS[name] = dict(P=P, fq=fq, vrf=vrf, proofs=proofs, scripts=scripts)
    return _SETS[name]


class _Bufs:
    """bq | bo | chals | left | right | scratch, each followed by a guard, in one poisoned buffer."""

    def __init__(self, s):
        import torch
        P, p, vrf = s["P"], s["vrf"].params, s["vrf"]
        B, pq = P["batch"], p.nq * P["d"]
        nbytes = vrf.verify_inputs_multi_scratch_bytes(N)
        assert nbytes > 0 and nbytes % 8 == 0
        words = dict(bq=N * B * pq if B > 1 else 0, bo=N * B * p.nqo * P["d"] if B > 1 else 0, chals=N * P["cols"] * pq,
                     left=N * P["rows"] * pq, right=N * P["cols"] * P["slots"] * p.L, scratch=nbytes // 8)
        self.buf = torch.full((sum(words.values()) + GUARD * len(words),), POISON, dtype=torch.int64, device="cuda")
        self.t, self.guards, at = {}, [], 0
        for k, w in words.items():
            self.t[k] = self.buf[at:at + w] if w else None
            self.guards.append(self.buf[at + w:at + w + GUARD])
            at += w + GUARD

    def guards_intact(self):
        return all((_h(g) == np.uint64(POISON)).all() for g in self.guards)

    def all_poison(self):
        return bool((_h(self.buf) == np.uint64(POISON)).all())


def _transcripts(s, scripts):
    """(points in a poisoned [N][5][L] buffer, as the Buckler batch's d_chal holds them; batch bytes; challenge bytes)."""
    import torch
    L = s["vrf"].params.L
    xs = np.full((N, 5, L), POISON, np.uint64)
    xs[:, 0] = co.to_limbs([x for x, _, _ in scripts], L)
    up = lambda strs: torch.from_numpy(np.frombuffer(b"".join(strs), np.uint8).copy()).to("cuda")
    bb = up([b for _, bs, _ in scripts for b in bs]) if s["P"]["batch"] > 1 else None
    return _t(xs), bb, up([c for _, _, cs in scripts for c in cs])


def _inputs(s, scripts):
    """One verify_inputs_multi_dev on the transcripts into poisoned buffers."""
    b = _Bufs(s)
    d_x, bb, cb = _transcripts(s, scripts)
    assert s["vrf"].verify_inputs_multi_dev(N, s["P"]["batch"], d_x, 5, bb, cb, *[b.t[k] for k in OUTS],
                                            b.t["scratch"]) is None
    return b


def _verify(s, b):
    """verify_multi_dev on the proofs with the device buffers of _inputs as they stand."""
    import torch
    vrf, proofs, B = s["vrf"], s["proofs"], s["P"]["batch"]
    dev = [b.t[k] if k in OUTS else _t(np.stack([pr[k] for pr in proofs])) for k in VERIFY_KEYS]
    out = torch.full((N, jindo.VERIFY_WORDS), -1, dtype=torch.int64, device="cuda")
    scratch = torch.full((vrf.verify_multi_scratch_bytes(N, B) // 8,), -1, dtype=torch.int64, device="cuda")
    vrf.verify_multi_dev(N, B, *dev, out, scratch)
    return vrf.unpack_verify_words(_h(out))


@pytest.mark.parametrize("name", SETS)
def test_inputs_equal_the_proofs_and_verify(name):
    import torch
    s = _set(name)
    b = _inputs(s, s["scripts"])
    torch.cuda.synchronize()
    for k in OUTS:
        if s["proofs"][0][k] is None:
            assert b.t[k] is None
            continue
        want = np.stack([pr[k] for pr in s["proofs"]])
        assert (_h(b.t[k]).reshape(want.shape) == want).all(), (name, k)
    assert b.guards_intact(), name
    res = _verify(s, b)
    assert [(r.ok, r.outer_ok, r.inner_ok, r.consistency_ok, r.eval_ok) for r in res] == [(True,) * 5] * N


@pytest.mark.parametrize("name", SETS)
def test_swapped_points_fail_their_proofs_alone(name):
    s = _set(name)
    sc = s["scripts"]
    swapped = [(sc[1][0],) + sc[0][1:], (sc[0][0],) + sc[1][1:], sc[2]]
    res = _verify(s, _inputs(s, swapped))
    for r in res[:2]:
        assert not r.ok and not (r.eval_ok and r.consistency_ok)
        assert r.outer_ok and r.inner_ok
    assert res[2].ok


def test_batch_null_rule_is_refused_both_ways():
    import torch
    lib = _lib.lib()
    for name in SETS:
        s = _set(name)
        B, vrf = s["P"]["batch"], s["vrf"]
        b = _Bufs(s)
        d_x, bb, cb = _transcripts(s, s["scripts"])
        spare = torch.full((64,), POISON, dtype=torch.int64, device="cuda")  # stands in for a buffer the rule forbids
        ptr = dict(batch=B, bytes=None if bb is None else bb.data_ptr(),
                   **{k: None if b.t[k] is None else b.t[k].data_ptr() for k in OUTS + ("scratch",)})

        def call(**kw):
            a = dict(ptr, **kw)
            return lib.rg_jindo_verify_inputs_multi_dev(vrf.h, N, a["batch"], d_x.data_ptr(), 5, a["bytes"], cb.data_ptr(),
                                                        *[a[k] for k in OUTS], a["scratch"], None)

        if B == 1:  # a buffer given with batch == 1
            cases = [dict(bq=spare.data_ptr(), bo=spare.data_ptr() + 256), dict(bytes=spare.data_ptr()),
                     dict(bq=spare.data_ptr(), bo=spare.data_ptr() + 256, bytes=spare.data_ptr() + 384)]
        else:       # a buffer missing with batch > 1, and batch == 1 claimed with the buffers given
            cases = [dict(bq=None), dict(bo=None), dict(bytes=None), dict(bq=None, bo=None, bytes=None), dict(batch=1)]
        cases += [dict(scratch=None), dict(chals=None), dict(left=ptr["chals"]), dict(batch=0)]
        for kw in cases:
            assert call(**kw) == INVALID, (name, kw)
            assert "jindo verify inputs multi" in lib.rg_last_error().decode(), (name, kw)
        torch.cuda.synchronize()
        assert b.all_poison() and (_h(spare) == np.uint64(POISON)).all(), name
        assert call() == 0  # the same arguments, unchanged, are accepted
        torch.cuda.synchronize()
        assert b.guards_intact(), name
    assert vrf.verify_inputs_multi_scratch_bytes(0) == 0 and vrf.verify_inputs_multi_scratch_bytes(65536) == 0
