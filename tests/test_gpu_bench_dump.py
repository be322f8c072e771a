"""GPU: bench.py --dump-outputs.  A plain run (no --full) prints the headline line only, with
ms_per_step and the requested step count, and writes what the timed path computed in its last
step: the in-place FwdNTTTo + InvNTTTo buffer (equal to the SplitMix64 inputs) and one forward
transform of it, checked here bit for bit against the C oracle at the dumped indices.  The two
shapes cover a batch dumped whole and one larger than the sample (2^21 coefficients > 2^20)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import coracle as co

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("ringo_bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _u64(pairs):  # [..., 2] float64 (lo32, hi32) -> uint64
    return pairs[..., 0].astype(np.uint64) | (pairs[..., 1].astype(np.uint64) << np.uint64(32))


@pytest.mark.timeout(240)
@pytest.mark.parametrize("logn,batch", [(12, 4), (16, 32)])
def test_plain_run_dumps_last_step_outputs(tmp_path, logn, batch):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--logn", str(logn), "--batch", str(batch), "--dump-outputs", str(out)],
                       capture_output=True, text=True, env=env, timeout=200)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["selfcheck_fwd_inv_identity"] is True
    assert d["steps_executed"]["ntt"] >= 4
    assert abs(d["value"] - 2 * batch / (d["ms_per_step"] / 1000.0)) <= 1e-6 * d["value"]
    for moved in ("l4_ntt", "wide_ntt_zp440", "jindo_commit", "jindo_commit_2e16", "cpu_baseline"):
        assert moved not in d  # those need --full
    assert (d["roofline"]["valu"] or {}).get("compute_floor_ms_per_step") is None

    B = _bench_module()
    N = 1 << logn
    total = batch * N
    files = sorted(f.name for f in out.iterdir())
    assert files == ["ntt_fwd_out.npy", "ntt_step_out.npy", "sample_index.npy"]
    arrs = {f[:-4]: np.load(out / f) for f in files}
    assert all(a.dtype == np.float64 for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 * 10 ** 6
    idx = arrs["sample_index"].astype(np.int64)
    n = min(total, B.DUMP_SAMPLE)
    assert idx.shape == (n,) and (np.diff(idx) >= 0).all() and idx[0] >= 0 and idx[-1] < total
    if total <= B.DUMP_SAMPLE:
        assert (idx == np.arange(total)).all()
    assert arrs["ntt_step_out"].shape == (n, 1, 2) and arrs["ntt_fwd_out"].shape == (n, 1, 2)
    a = B.uniform_elems(B.P63, 1, total, 0x52494E47)  # rank 0's inputs
    assert (_u64(arrs["ntt_step_out"]) == a[idx]).all()
    cf = co.CField(B.P63)
    tw, _, _ = cf.tables(N)
    want = cf.ntt_fwd(a.reshape(batch, N, 1), tw).reshape(total, 1)
    assert (_u64(arrs["ntt_fwd_out"]) == want[idx]).all()
