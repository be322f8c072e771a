"""GPU: the reference's TestJindo flow (jindo_test.go:26-52) with nothing but the transcript's bytes
coming from the host: Commit on the device, then x and the challenge bytes drawn here, the batch
challenges, column challenges, encode(leftVec(x)), rightVec(x) and the evaluations built by
rg_jindo_encode_challenges_dev, rg_jindo_eval_point_dev and rg_poly_evaluate_batch_dev, Evaluate's
device work on those buffers and Verify on the device.  Each device-built input is also compared
with the oracle's."""
import numpy as np
import pytest

import coracle as co
import ringo
from ringo import bigpoly, jindo
from tests import jindo_synth_util as su
from tests.jindo_proto import VERIFY_KEYS, left_right, mont
from tests.jindo_util import make_randomness, make_v

pytestmark = pytest.mark.gpu


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda")


def _h(t):
    return t.cpu().numpy().view(np.uint64)


def _commit(name):
    """(P with norm bounds, fq, params, verifier, prover, v [B][nv][L], device openings)."""
    import torch
    P, fq = su.params(name)
    if name in su.SYNTH:  # no sampler widths: injected randomness; bounds from an honest oracle proof
        P, fq, ck, _, _, _ = su.synth_proof(name, seed=31)
        params = jindo.Parameters.from_dict(P, fq)
        vrf = jindo.Verifier(params, ck=ck)
        B, nv = 1, P["rank"]
        v = su.synth_v(P, fq, nv, 32)[None]
        rnd = make_randomness(P, fq, seed=33, batch=1)
    else:
        params = jindo.Parameters.from_dict(P, fq)
        vrf = jindo.Verifier(params, crs=b"Jindo!")
        B, nv = P["batch"], P["rank"]
        v = np.stack([make_v(fq, nv, seed=700 + b) for b in range(B)])
        rnd = None
    prv = vrf._p
    sh = params.shapes(B)
    o = {k: torch.zeros(sh[k], dtype=torch.int64, device="cuda") for k in ("incom", "enc", "mlwe_out", "com")}
    d_v = _t(v)
    if rnd is None:
        prv.commit_sampled_dev(B, d_v, nv, jindo.Seeds.derive(b"eval-flow-" + name.encode()), 0, o["incom"], o["enc"],
                               o["mlwe_out"], o["com"])
    else:
        prv.commit_dev(B, d_v, nv, _t(rnd["last_row"]), _t(rnd["mask"]), _t(rnd["enc_noise"]), _t(rnd["mlwe_noise"]),
                       o["incom"], o["enc"], o["mlwe_out"], o["com"])
    return P, fq, params, vrf, prv, v, d_v, o


@pytest.mark.parametrize("name", ["t10_b8", "p63_t10_b2", "syn_d8_p63"])
def test_eval_flow_with_device_built_inputs(name):
    import torch
    P, fq, params, vrf, prv, v, d_v, o = _commit(name)
    cj, F, RF = co.CJindo(P, fq), co.CField(fq), ringo.Field(fq)
    B, nv, L, d = v.shape[0], v.shape[1], params.L, P["d"]
    rng = np.random.default_rng(43)
    x = mont(F, int.from_bytes(rng.bytes(40), "little"))
    xl = co.to_limbs([x], L)[0]
    d_x = _t(xl)
    bbytes, cbytes = [rng.bytes(16) for _ in range(B)], [rng.bytes(16) for _ in range(P["cols"])]
    dev_bytes = lambda bs: torch.from_numpy(np.frombuffer(b"".join(bs), np.uint8).copy()).to("cuda")  # noqa: E731
    new = lambda *shape: torch.full(shape, 0x5a5a, dtype=torch.int64, device="cuda")  # noqa: E731
    # the three new entries build every input
    bq = bo = None
    if B > 1:
        bq, bo = new(B, params.nq, d), new(B, params.nqo, d)
        prv.encode_challenges_dev(0, dev_bytes(bbytes), B, bq)
        prv.encode_challenges_dev(1, dev_bytes(bbytes), B, bo)
    chals = new(P["cols"], params.nq, d)
    prv.encode_challenges_dev(0, dev_bytes(cbytes), P["cols"], chals)
    left, right = new(P["rows"], params.nq, d), new(P["cols"] * P["slots"], L)
    prv.eval_point_dev(d_x, left, right)
    y = new(B, L)
    scr = new((bigpoly.evaluate_batch_scratch_bytes(RF, nv, B) + 7) // 8)
    bigpoly.evaluate_batch_dev(RF, d_v, nv, nv, B, d_x, y, scr)
    # Evaluate's device work and Verify on those buffers
    es = prv.eval_shapes()
    e = {k: new(*es[k]) for k in es}
    prv.eval_batch_dev(B, o["incom"], o["enc"], o["mlwe_out"], bq, bo, e["ob_incom"], e["ob_enc"], e["ob_mlwe"])
    prv.eval_partial_dev(e["ob_enc"], left, e["partial"])
    prv.eval_respond_dev(e["ob_enc"], e["ob_mlwe"], chals, e["pf_enc"], e["pf_mlwe"])
    torch.cuda.synchronize()
    args = dict(com=o["com"], bq=bq, bo=bo, chals=chals, left=left, right=right, y=y, pf_incom=e["ob_incom"],
                pf_partial=e["partial"], pf_enc=e["pf_enc"], pf_mlwe=e["pf_mlwe"])
    r = vrf.verify_dev(B, *[args[k] for k in VERIFY_KEYS])
    assert [r.outer_ok, r.inner_ok, r.consistency_ok, r.eval_ok] == [True] * 4 and r.ok, name
    # one word of one y changed: the evaluation check alone fails
    args["y"] = y.clone()
    args["y"].view(-1)[(B - 1) * L] ^= 1
    bad = vrf.verify_dev(B, *[args[k] for k in VERIFY_KEYS])
    assert not bad.eval_ok and not bad.ok
    assert [bad.outer_ok, bad.inner_ok, bad.consistency_ok] == [r.outer_ok, r.inner_ok, r.consistency_ok]
    # every device-built input equals the oracle's
    if B > 1:
        assert (_h(bq) == np.stack([cj.encode_challenge(0, b) for b in bbytes])).all()
        assert (_h(bo) == np.stack([cj.encode_challenge(1, b) for b in bbytes])).all()
    assert (_h(chals) == np.stack([cj.encode_challenge(0, b) for b in cbytes])).all()
    left_e, right_e = left_right(P, F, x)
    assert (_h(left) == np.stack([cj.encode(co.to_limbs([a], L)) for a in left_e])).all()
    assert (_h(right) == co.to_limbs(right_e, L)).all()
    assert (_h(y) == np.stack([F.evaluate(v[b], xl) for b in range(B)])).all()
