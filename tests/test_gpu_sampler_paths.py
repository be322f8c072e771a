"""GPU: the device samplers (csrc/jindo_sample.hip) on the paths random draws at NewParameters'
widths never take, bit for bit against the C oracle (oracle.c of_jindo_sample): the cases of
tests/sampler_path_cases.py -- both outcomes of a TwinCDT tail and saturated tables (small encode
widths), COSAC groups past the first 1024 words of either stream (the XOR-accumulated refill
inside cosac2_noise_kernel's state machine), the table sizes on either side of kCdtLdsMaxSize and
kMlweLdsTab, structured v.  tests/test_oracle_sampler_paths.py asserts, on the CPU, that the
oracle's draws do take those paths, and that no COSAC group of any case draws more than 16,384
words (the device's lane loop is as long as the oracle's)."""
import numpy as np
import pytest

import coracle as co
from ringo import jindo
from ringo._lib import STATUS, RingoError
from tests import sampler_path_cases as spc

pytestmark = pytest.mark.gpu
OUT = ("last_row", "mask", "enc_noise", "mlwe_noise")


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda")


def _prover(c):
    params = jindo.Parameters.from_dict(c.P, c.q)
    params.stddevs = c.stddevs()
    raw = c.seeds_raw()
    return params, jindo.NewProver(params, b"Jindo!"), jindo.Seeds(*[raw[32 * i:32 * i + 32] for i in range(6)])


def _sample_dev(c, params, prv, seeds, dv):
    import torch
    sh = params.shapes(c.B)
    o = {k: torch.zeros(sh[k], dtype=torch.int64, device="cuda") for k in OUT}
    prv.sample_dev(c.B, dv, c.nv, seeds, c.first, *[o[k] for k in OUT])
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("cid", [c.id for c in spc.CASES if not c.refused])
def test_sample_paths_match_oracle(cid):
    c = spc.BY_ID[cid]
    want, census = spc.oracle_draws(cid)
    assert max(census["cos_max_base"], census["cos_max_rnd"]) <= spc.WORD_CAP  # (the CPU test's condition)
    params, prv, seeds = _prover(c)
    o = _sample_dev(c, params, prv, seeds, _t(c.make_v()))
    for k in OUT:
        got = o[k].cpu().numpy()
        bad = np.flatnonzero((got.view(np.uint64) != want[k].view(np.uint64)).reshape(-1))
        assert bad.size == 0, (k, bad.size, bad[:8], got.reshape(-1)[bad[:8]], want[k].reshape(-1)[bad[:8]])


@pytest.mark.parametrize("cid", [c.id for c in spc.CASES if c.refused])
def test_refused_shape_before_any_launch(cid):
    """A 97-entry encode table: RG_ERR_UNSUPPORTED with the existing message from both sampled
    entry points, and nothing written."""
    import torch
    c = spc.BY_ID[cid]
    params, prv, seeds = _prover(c)
    dv = _t(c.make_v())
    sh = params.shapes(c.B)
    o = {k: torch.zeros(sh[k], dtype=torch.int64, device="cuda") for k in OUT}
    with pytest.raises(RingoError, match="TwinCDT table of <= 96 entries") as e:
        prv.sample_dev(c.B, dv, c.nv, seeds, c.first, *[o[k] for k in OUT])
    assert e.value.status == STATUS["RG_ERR_UNSUPPORTED"]
    z = {k: torch.zeros(sh[k], dtype=torch.int64, device="cuda") for k in ("incom", "enc", "mlwe_out", "com")}
    with pytest.raises(RingoError, match="TwinCDT table of <= 96 entries") as e:
        prv.commit_sampled_dev(c.B, dv, c.nv, seeds, c.first, z["incom"], z["enc"], z["mlwe_out"], z["com"])
    assert e.value.status == STATUS["RG_ERR_UNSUPPORTED"]
    torch.cuda.synchronize()
    assert all(not t.any().item() for t in list(o.values()) + list(z.values()))


@pytest.mark.parametrize("cid", spc.COMBINED)
def test_combined_commit_sampled(cid):
    """small-ecd and long-cosac at once through rg_jindo_commit_sampled_dev (the three-stream DAG)
    == rg_jindo_commit_dev on rg_jindo_sample_dev's draws == the oracle's commit on its draws."""
    import torch
    c = spc.BY_ID[cid]
    rnd, _ = spc.oracle_draws(cid)
    params, prv, seeds = _prover(c)
    v = c.make_v()
    dv = _t(v)
    sh = params.shapes(c.B)
    keys = ("incom", "enc", "mlwe_out", "com")
    a = {k: torch.zeros(sh[k], dtype=torch.int64, device="cuda") for k in keys}
    prv.commit_sampled_dev(c.B, dv, c.nv, seeds, c.first, *[a[k] for k in keys])
    r = _sample_dev(c, params, prv, seeds, dv)
    b_ = {k: torch.zeros(sh[k], dtype=torch.int64, device="cuda") for k in keys}
    prv.commit_dev(c.B, dv, c.nv, *[r[k] for k in OUT], *[b_[k] for k in keys])
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(a[k], b_[k]), k
    ck = prv.commit_key()
    cj = co.CJindo(c.P, c.q)
    for b in range(c.B):
        w = cj.commit(ck[0], ck[1], ck[2], v[b], *[rnd[k][b] for k in OUT])
        for k, wk in (("incom", "incom"), ("enc", "enc"), ("mlwe_out", "mlwe"), ("com", "com")):
            assert (a[k][b].cpu().numpy().view(np.uint64) == w[wk]).all(), (b, k)
