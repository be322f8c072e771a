"""GPU: the Jindo transcript on the device (ringo.jindo.Transcript, Prover.evaluate_multi_transcript_dev,
Verifier.verify_multi_transcript_dev) and the projection XOF helper (ringo.buckler.proj_xof_dev).

N = 3 proofs, each with its own point and commitments, on the smallest batch > 1 set (p63_t10_b2) and a
batch = 1 set (t10_b1), both at rank 1024.  The prover driver is held against the existing flow:
eval_open_multi_dev, hashlib.shake_128 on the host over the same framing, eval_respond_multi_dev.  The
framing is this test's (one set with lengths that are no multiple of 8, one aligned): Lattigo's is the
caller's to state (jindo.transcript_plans)."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import coracle as co
from ringo import buckler, jindo
from tests.jindo_proto import honest_proof

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PARAMS = json.load(open(os.path.join(HERE, "golden", "jindo_params.json")))
N = 3
CRS = b"Jindo!"
FRAMING = {  # name: (poly_prefix(levels, n), row_prefix(n))
    "p63_t10_b2": (lambda levels, n: b"P" + bytes([levels]) + n.to_bytes(3, "little"), lambda n: n.to_bytes(8, "little") + b"r"),
    "t10_b1": (lambda levels, n: levels.to_bytes(8, "little") + n.to_bytes(8, "little"), lambda n: n.to_bytes(8, "little")),
}


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to("cuda")


def _h(t):
    return t.cpu().numpy().view(np.uint64)


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _poly_bytes(name, poly):
    """[levels][n] residues as the test's framing writes them."""
    pp, rp = FRAMING[name]
    levels, n = poly.shape
    return pp(levels, n) + b"".join(rp(n) + np.ascontiguousarray(poly, "<u8").tobytes() for poly in poly)


_SETS = {}


def _set(name):
    """The set's verifier and prover, three honest commitments with their openings, points and evaluations
    (tests/jindo_proto.honest_proof; its own random challenges are not used), on the device; built once."""
    if name not in _SETS:
        P = PARAMS[name]
        fq = int(P["field_q_hex"], 16)
        params = jindo.Parameters.from_dict(P, fq)
        vrf = jindo.Verifier(params, crs=CRS)
        ck = vrf._p.commit_key()
        hp = [honest_proof(P, fq, ck, seed=41 + 10 * i) for i in range(N)]
        F = co.CField(fq)
        L = params.L
        Rinv = pow(1 << (64 * L), -1, fq)
        s = dict(P=P, fq=fq, params=params, vrf=vrf, prv=vrf._p, B=P["batch"], hp=hp,
                 x_marshal=[(h["x"] * Rinv % fq).to_bytes(8 * L, "big") for h in hp],
                 com=np.stack([h["com"] for h in hp]), y=np.stack([h["y"] for h in hp]),
                 d=dict(com=_t(np.stack([h["com"] for h in hp])), x=_t(co.to_limbs([h["x"] for h in hp], L)),
                        y=_t(np.stack([h["y"] for h in hp])),
                        **{k: _t(np.stack([h["opens"][k] for h in hp])) for k in ("incom", "enc", "mlwe")}))
        s["head"] = [CRS + b"".join(_poly_bytes(name, p) for c in s["com"][i] for p in c) + s["x_marshal"][i]
                     for i in range(N)]
        _SETS[name] = s
    return _SETS[name]


class _Eval:
    """The buffers of one batch Evaluate."""

    def __init__(self, s):
        prv, B = s["prv"], s["B"]
        es = prv.eval_shapes()
        z = lambda *shape: torch.zeros(shape, dtype=torch.int64, device="cuda")
        self.ob_enc = z(N, *es["ob_enc"]) if B > 1 else None
        self.ob_mlwe = z(N, *es["ob_mlwe"]) if B > 1 else None
        self.pf_incom, self.pf_partial = z(N, *es["ob_incom"]), z(N, *es["partial"])
        self.pf_enc, self.pf_mlwe = z(N, *es["pf_enc"]), z(N, *es["pf_mlwe"])
        self.open_scratch = z(prv.eval_open_multi_scratch_bytes(N, B) // 8)
        self.respond_scratch = z(prv.eval_respond_multi_scratch_bytes(N) // 8)
        self.batch_bytes = torch.zeros(N * B * 16, dtype=torch.uint8, device="cuda") if B > 1 else None
        self.chal_bytes = torch.zeros(N * s["P"]["cols"] * 16, dtype=torch.uint8, device="cuda")

    def proof(self):
        return {k: _h(getattr(self, k)) for k in ("pf_incom", "pf_partial", "pf_enc", "pf_mlwe")}


def _host_flow(name, s):
    """The existing flow: the transcript with hashlib on the host between the two calls."""
    prv, B, d, cols = s["prv"], s["B"], s["d"], s["P"]["cols"]
    e = _Eval(s)
    msgs = list(s["head"])
    if B > 1:
        bb = [hashlib.shake_128(m).digest(B * 16) for m in msgs]
        msgs = [m + b for m, b in zip(msgs, bb)]
        e.batch_bytes.copy_(torch.from_numpy(np.frombuffer(b"".join(bb), np.uint8).copy()))
    prv.eval_open_multi_dev(N, B, d["incom"], d["enc"], d["mlwe"], B, 1, d["x"], 1, e.batch_bytes, e.ob_enc, e.ob_mlwe,
                            e.pf_incom, e.pf_partial, e.open_scratch)
    partial = _h(e.pf_partial)
    cb = [hashlib.shake_128(m + b"".join(_poly_bytes(name, p) for p in partial[i])).digest(cols * 16)
          for i, m in enumerate(msgs)]
    e.chal_bytes.copy_(torch.from_numpy(np.frombuffer(b"".join(cb), np.uint8).copy()))
    if B > 1:
        prv.eval_respond_multi_dev(N, e.ob_enc, e.ob_mlwe, 1, e.chal_bytes, e.pf_enc, e.pf_mlwe, e.respond_scratch)
    else:
        prv.eval_respond_multi_dev(N, d["enc"], d["mlwe"], B, e.chal_bytes, e.pf_enc, e.pf_mlwe, e.respond_scratch)
    torch.cuda.synchronize()
    return e


def _device_flow(name, s):
    prv, B, d = s["prv"], s["B"], s["d"]
    e = _Eval(s)
    tr = jindo.Transcript(s["params"], CRS, B, N, *FRAMING[name])
    prv.evaluate_multi_transcript_dev(tr, d["com"], d["incom"], d["enc"], d["mlwe"], B, 1, d["x"], 1, e.batch_bytes,
                                      e.chal_bytes, e.ob_enc, e.ob_mlwe, e.pf_incom, e.pf_partial, e.pf_enc, e.pf_mlwe,
                                      e.open_scratch, e.respond_scratch)
    torch.cuda.synchronize()
    return e, tr


_FLOWS = {}


def _flows(name):
    if name not in _FLOWS:
        s = _set(name)
        _FLOWS[name] = (s, _host_flow(name, s)) + _device_flow(name, s)
    return _FLOWS[name]


@pytest.mark.parametrize("name", sorted(FRAMING))
def test_prover_driver_equals_the_host_transcript_flow(name):
    s, host, devf, tr = _flows(name)
    assert len(tr.plan_a) == len(s["head"][0])
    if s["B"] > 1:
        assert _bytes(devf.batch_bytes) == _bytes(host.batch_bytes)
    else:
        assert devf.batch_bytes is None
    assert _bytes(devf.chal_bytes) == _bytes(host.chal_bytes)
    assert len(set(_bytes(devf.chal_bytes)[i * 16:(i + 1) * 16] for i in range(N * s["P"]["cols"]))) == N * s["P"]["cols"]
    hp, dp = host.proof(), devf.proof()
    for k in hp:
        assert (hp[k] == dp[k]).all(), k


def _verify(s, tr, devf, pf_partial):
    vrf, B, d, P, p = s["vrf"], s["B"], s["d"], s["P"], s["params"]
    pq = p.nq * p.d
    z = lambda n: torch.zeros(n, dtype=torch.int64, device="cuda")
    bq, bo = (z(N * B * pq), z(N * B * p.nqo * p.d)) if B > 1 else (None, None)
    chals, left, right = z(N * P["cols"] * pq), z(N * P["rows"] * pq), z(N * P["cols"] * P["slots"] * p.L)
    bb = torch.zeros(N * B * 16, dtype=torch.uint8, device="cuda") if B > 1 else None
    cb = torch.zeros(N * P["cols"] * 16, dtype=torch.uint8, device="cuda")
    out = torch.full((N, jindo.VERIFY_WORDS), -1, dtype=torch.int64, device="cuda")
    vrf.verify_multi_transcript_dev(tr, d["com"], d["x"], 1, d["y"], devf.pf_incom, pf_partial, devf.pf_enc,
                                    devf.pf_mlwe, bb, cb, bq, bo, chals, left, right, out,
                                    z(vrf.verify_inputs_multi_scratch_bytes(N) // 8),
                                    z(vrf.verify_multi_scratch_bytes(N, B) // 8))
    torch.cuda.synchronize()
    return bb, cb, [r.ok for r in vrf.unpack_verify_words(_h(out))]


@pytest.mark.parametrize("name", sorted(FRAMING))
def test_verifier_driver_replays_the_transcript(name):
    s, host, devf, tr = _flows(name)
    cols = s["P"]["cols"]
    bb, cb, ok = _verify(s, tr, devf, devf.pf_partial)
    if s["B"] > 1:
        assert _bytes(bb) == _bytes(host.batch_bytes)
    assert _bytes(cb) == _bytes(host.chal_bytes)
    assert ok == [True] * N
    # one byte of proof 1's Partial flipped: that proof alone derives other challenges and fails
    bad = devf.pf_partial.clone()
    bad.view(-1).view(torch.uint8)[bad[0].numel() * 8 + 1234] ^= 0x10
    bb2, cb2, ok2 = _verify(s, tr, devf, bad)
    if s["B"] > 1:
        assert _bytes(bb2) == _bytes(host.batch_bytes)  # drawn before the proof is absorbed
    want, got = _bytes(host.chal_bytes), _bytes(cb2)
    per = cols * 16
    assert got[:per] == want[:per] and got[2 * per:] == want[2 * per:]
    assert all(got[per + 16 * c:per + 16 * c + 16] != want[per + 16 * c:per + 16 * c + 16] for c in range(cols))
    assert ok2 == [True, False, True]


def test_projection_xof_helper():
    rank = 256
    rng = np.random.default_rng(7)
    c = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    d_c = torch.from_numpy(c).to("cuda")
    guard = 64
    out = torch.full((N * 32 * rank + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    h = buckler.proj_xof_dev(d_c, rank, out, N)
    assert buckler.proj_xof_dev(d_c, rank, out, N, sponge=h) is h  # a reused sponge gives the same bytes
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[N * 32 * rank:] == 0xA5).all()
    for i in range(N):
        assert got[i * 32 * rank:(i + 1) * 32 * rank].tobytes() == hashlib.shake_128(c[i].tobytes()).digest(32 * rank)
