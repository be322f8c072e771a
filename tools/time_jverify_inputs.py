"""Times the front end of a batch verification of N Jindo proofs two ways, alternating in one process,
both asynchronous and both timed by HIP events on one stream:
  loop   N rg_jindo_eval_point_dev calls (one point each) plus the batched
         rg_jindo_encode_challenges_dev calls (bq, bo when batch > 1, chals)
  multi  ONE rg_jindo_verify_inputs_multi_dev
from the same device-resident transcript bytes and points ([N][5][L], the Buckler batch's d_chal
layout).  Both ways must produce identical words in bq, bo, chals, left and right.

The two other ways of raising the points that were measured and removed (power tables by
rg_buckler_powers_batch_dev, powers inside the encoding kernel) and their arms of this tool are in
tools/experiments/jindo_point_pow_arms.patch.
usage: python tools/time_jverify_inputs.py [--sets t14_b1,t10_b8] [--proofs 1,8,64] [--iters 200] [--warmup 20] [--runs 3]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "ringo-snark_amd")):
    sys.path.insert(0, p)

ap = argparse.ArgumentParser()
ap.add_argument("--sets", type=str, default="t14_b1,t10_b8")
ap.add_argument("--proofs", type=str, default="1,8,64")
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ringo import jindo  # noqa: E402

assert torch.cuda.is_available(), "time_jverify_inputs.py needs the GPU"
PARAMS = json.load(open(os.path.join(ROOT, "tests", "golden", "jindo_params.json")))
stream = torch.cuda.Stream()
OUTS = ("bq", "bo", "chals", "left", "right")


def leg(name, n, vrf, P, fq):
    p = vrf.params
    B, L, pq, cs = P["batch"], p.L, p.nq * P["d"], P["cols"] * P["slots"]
    rng = np.random.default_rng(1000 + n)
    xs = np.zeros((n, 5, L), np.uint64)
    for k in range(n):  # canonical residues serve as Montgomery elements
        v = int.from_bytes(rng.bytes(8 * L + 8), "little") % fq
        xs[k, 0] = [(v >> (64 * i)) & ((1 << 64) - 1) for i in range(L)]
    d_x = torch.from_numpy(xs.view(np.int64)).cuda()
    bb = torch.from_numpy(np.frombuffer(rng.bytes(16 * n * B), np.uint8).copy()).cuda() if B > 1 else None
    cb = torch.from_numpy(np.frombuffer(rng.bytes(16 * n * P["cols"]), np.uint8).copy()).cuda()
    words = dict(bq=n * B * pq if B > 1 else 0, bo=n * B * p.nqo * P["d"] if B > 1 else 0, chals=n * P["cols"] * pq,
                 left=n * P["rows"] * pq, right=n * cs * L)

    def outs():
        return {k: torch.zeros(w, dtype=torch.int64, device="cuda") if w else None for k, w in words.items()}

    nbytes = vrf.verify_inputs_multi_scratch_bytes(n)
    scratch = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")
    lw, rw = P["rows"] * pq, cs * L
    torch.cuda.synchronize()

    def loop(o):
        if B > 1:
            vrf.encode_challenges_dev(0, bb, n * B, o["bq"], stream=stream)
            vrf.encode_challenges_dev(1, bb, n * B, o["bo"], stream=stream)
        vrf.encode_challenges_dev(0, cb, n * P["cols"], o["chals"], stream=stream)
        for k in range(n):
            vrf.eval_point_dev(d_x[k, 0], o["left"][k * lw:(k + 1) * lw], o["right"][k * rw:(k + 1) * rw], stream=stream)

    def multi(o):
        vrf.verify_inputs_multi_dev(n, B, d_x, 5, bb, cb, *[o[k] for k in OUTS], scratch, stream=stream)

    arms = [("loop of rg_jindo_eval_point_dev + rg_jindo_encode_challenges_dev", "loop", loop),
            ("rg_jindo_verify_inputs_multi_dev", "multi", multi)]
    got = {a[1]: outs() for a in arms}
    rows = {a[1]: [] for a in arms}
    for run in range(args.runs):
        for entry, key, fn in arms:
            with torch.cuda.stream(stream):
                for _ in range(args.warmup):
                    fn(got[key])
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(args.iters):
                    fn(got[key])
                e1.record(stream)
                e1.synchronize()
            t = e0.elapsed_time(e1) / args.iters
            rows[key].append(t)
            print(json.dumps({"entry": entry, "set": name, "proofs": n, "run": run, "iters": args.iters,
                              "ms_per_call": round(t, 5), "us_per_proof": round(t * 1e3 / n, 3),
                              "scratch_bytes": 0 if key == "loop" else nbytes}), flush=True)
    for key in rows:
        for k in OUTS:
            if words[k]:
                assert torch.equal(got[key][k], got["loop"][k]), (name, n, key, k, "the ways differ")
    if n == 64:  # the required direction: in every run the batch call is below the loop
        assert all(b < a for a, b in zip(rows["loop"], rows["multi"])), (name, rows)
    for key, ts in rows.items():
        med = statistics.median(ts)
        print(json.dumps({"summary": key, "set": name, "proofs": n, "median_ms_per_call": round(med, 5),
                          "median_us_per_proof": round(med * 1e3 / n, 3), "min_ms": round(min(ts), 5),
                          "max_ms": round(max(ts), 5),
                          "loop_over_this": round(statistics.median(rows["loop"]) / med, 2)}), flush=True)


for name in args.sets.split(","):
    P = PARAMS[name]
    fq = int(P["field_q_hex"], 16)
    vrf = jindo.Verifier(jindo.Parameters.from_dict(P, fq), crs=b"Jindo!")
    for n in (int(x) for x in args.proofs.split(",")):
        leg(name, n, vrf, P, fq)
