"""Times three ways to get a batch of proofs' two masks (linCheckMask and sumCheckMask) onto the
device, at the shape of tools/time_bproj.py: the 255-bit Jindo field (L = 4), rank 2^15, mask rank =
embedding rank = 2^16, so a mask's draws are 2 MiB per proof:
  (a) host draws: an asynchronous copy of d_rand [n][mask_rank][L] from pinned host memory, then
      rg_buckler_sumcheck_mask_batch_dev -- the path before the field sampler.  Making the draws on
      the host (one SetRandom at a time from crypto/rand) is NOT counted, which favours this path;
  (b) composition: rg_field_sampler_elems_dev into a device buffer, then the same mask call;
  (c) sampled: rg_buckler_sumcheck_mask_batch_sampled_dev, the draws made inside the mask kernel.
Each way does both masks (two calls of each entry) with d_mask_com.  HIP events on the launch stream
around `iters` back-to-back repetitions after `warmup` of the same shape; the three legs alternate,
`--runs` times each, in one process, and the summary line gives the median with min..max.  After the
timing (b) and (c) must have left the same outputs (their draws are the same instances); (a)'s draws
are other values.  The first error ends the run.

Stream items per mask, counted from the code (csrc/buckler_sample.hip, csrc/buckler_proj.hip), not
measured: (a) 1 copy + 1 kernel; (b) 1 memset + 2 kernels, then 1 kernel; (c) 1 memset + 2 kernels.
usage: timeout 900 python tools/time_bmask_sampled.py [--proofs 1,8,64] [--runs 3] [--iters 20] [--warmup 3] [--rank 32768]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ringo-snark_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ringo  # noqa: E402
from ringo import buckler  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--proofs", type=str, default="1,8,64")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rank", type=int, default=1 << 15)
args = ap.parse_args()

assert torch.cuda.is_available(), "time_bmask_sampled.py needs the GPU"
q = int(json.load(open(os.path.join(ROOT, "tests", "golden", "fields.json")))["jindo_zp"]["q_hex"], 16)
F = ringo.Field(q)
L, rank = F.L, args.rank
mask_rank = emb = 2 * rank
rng = np.random.default_rng(1)
S = buckler.FieldSampler(F, b"time_bmask_sampled")
stream = torch.cuda.Stream()
POOL = torch.from_numpy(F.random(1 << 16, rng).view(np.int64))  # canonical elements, repeated (values do not matter to (a))

ITEMS = {"a": 2 * (1 + 1), "b": 2 * (3 + 1), "c": 2 * 3}
NAMES = {"a": "pinned copy + sumcheck_mask_batch_dev", "b": "field_sampler_elems_dev + sumcheck_mask_batch_dev",
         "c": "sumcheck_mask_batch_sampled_dev"}


def empty(*shape):
    return torch.empty((*shape, L), dtype=torch.int64, device="cuda")


def timed(fn, iters):
    with torch.cuda.stream(stream):
        for _ in range(args.warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(iters):
            fn()
        e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def leg(n):
    per = n * mask_rank  # draws of one mask; the two masks take disjoint instance ranges
    first = (0, per)
    h_rand = [POOL.repeat(-(-per // POOL.shape[0]), 1)[:per].reshape(n, mask_rank, L).contiguous().pin_memory()
              for _ in range(2)]
    d_rand = [empty(n, mask_rank) for _ in range(2)]
    out = {w: [(empty(n, emb), empty(n, mask_rank), empty(n)) for _ in range(2)] for w in "abc"}
    scr = [torch.empty(S.scratch_bytes() // 8, dtype=torch.int64, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()

    def a():
        for i in range(2):
            m, c, s = out["a"][i]
            with torch.cuda.stream(stream):
                d_rand[i].copy_(h_rand[i], non_blocking=True)
            buckler.sumcheck_mask_batch_dev(F, rank, mask_rank, emb, n, d_rand[i], m, s, d_mask_com=c, stream=stream)

    def b():
        for i in range(2):
            m, c, s = out["b"][i]
            S.elems_dev(first[i], per, d_rand[i], scr[i], stream=stream)
            buckler.sumcheck_mask_batch_dev(F, rank, mask_rank, emb, n, d_rand[i], m, s, d_mask_com=c, stream=stream)

    def c_():
        for i in range(2):
            m, c, s = out["c"][i]
            buckler.sumcheck_mask_batch_sampled_dev(S, rank, mask_rank, emb, n, first[i], m, s, scr[i], d_mask_com=c,
                                                    stream=stream)

    iters = max(2, args.iters // max(1, n // 8))
    legs = (("a", a), ("b", b), ("c", c_))
    us = {w: [] for w, _ in legs}
    for run in range(args.runs):
        for w, fn in legs:
            t = timed(fn, iters)
            us[w].append(t * 1e3 / n)
            print(json.dumps({"way": w, "entry": NAMES[w], "proofs": n, "run": run, "iters": iters, "rank": rank,
                              "mask_rank": mask_rank, "emb": emb, "L": L, "masks": 2, "ms_per_batch": round(t, 4),
                              "us_per_proof": round(t * 1e3 / n, 2), "stream_items_counted": ITEMS[w],
                              "rand_bytes": 0 if w == "c" else 2 * per * L * 8}), flush=True)
    torch.cuda.synchronize()
    for i in range(2):  # (c) is (b)'s composition, word for word; and a last (a) leaves the mask of the host draws
        for x, y in zip(out["b"][i], out["c"][i]):
            assert torch.equal(x, y), "the sampled entry and the composition differ"
    med = {w: statistics.median(v) for w, v in us.items()}
    spread = max(max(v) - min(v) for v in us.values())
    print(json.dumps({"summary": True, "proofs": n, "sampled_equals_composition": True,
                      **{f"{w}_us_per_proof": {"median": round(med[w], 2), "min": round(min(us[w]), 2),
                                               "max": round(max(us[w]), 2)} for w in "abc"},
                      "a_over_c": round(med["a"] / med["c"], 2), "b_over_c": round(med["b"] / med["c"], 2),
                      "c_below_a_by_more_than_the_spread": med["a"] - med["c"] > spread,
                      "c_below_b_by_more_than_the_spread": med["b"] - med["c"] > spread}), flush=True)


for n_proofs in (int(x) for x in args.proofs.split(",")):
    leg(n_proofs)
