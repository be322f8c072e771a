"""Times the infinity-norm decomposition on the device: rg_buckler_dcmp_inf_dev at rank 2^15 over the
255-bit Jindo field (L = 4) with decomposeBase(2^32) (32 digits), per batch size.  HIP events on the
launch stream around `iters` back-to-back calls, after `warmup` calls of the same shape.  Prints one
JSON line per batch: ms per call and the rate at which the digits are written (the kernel writes nb
times what it reads, so the copy rate of the memory bounds it).
usage: python tools/time_dcmp.py [--batches 1,8] [--iters 200] [--warmup 20] [--rank 32768]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ringo-snark_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ringo  # noqa: E402
from ringo import buckler  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1,8")
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--rank", type=int, default=1 << 15)
ap.add_argument("--bound", type=int, default=1 << 32)
args = ap.parse_args()

assert torch.cuda.is_available(), "time_dcmp.py needs the GPU"
q = int(json.load(open(os.path.join(ROOT, "tests", "golden", "fields.json")))["jindo_zp"]["q_hex"], 16)
F = ringo.Field(q)
dc = buckler.Decomposer(F, args.bound)
nb, L, rank = len(dc.dcmpBase), F.L, args.rank
rng = np.random.default_rng(1)
stream = torch.cuda.Stream()
for batch in [int(b) for b in args.batches.split(",")]:
    # centred values within the bound, both signs, as Montgomery elements
    plain = [int(v) % q for v in rng.integers(-(args.bound - 1), args.bound, size=batch * rank)]
    w = torch.from_numpy(F.mont(plain).view(np.int64)).cuda().reshape(batch, rank, L)
    out = torch.empty((batch, nb, rank, L), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for _ in range(args.warmup):
            dc.inf_dev(out, w, batch, rank, stream=stream)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        for _ in range(args.iters):
            dc.inf_dev(out, w, batch, rank, stream=stream)
        t1.record(stream)
    t1.synchronize()
    ms = t0.elapsed_time(t1) / args.iters
    written = batch * nb * rank * L * 8
    print(json.dumps({"entry": "rg_buckler_dcmp_inf_dev", "field": "jindo_zp", "L": L, "rank": rank, "nb": nb,
                      "batch": batch, "iters": args.iters, "ms_per_call": round(ms, 5),
                      "bytes_written": written, "bytes_read": batch * rank * L * 8,
                      "written_GB_per_s": round(written / ms / 1e6, 1)}), flush=True)
