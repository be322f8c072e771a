"""Times Prover.Evaluate's device work for N proofs two ways, alternating in one process, HIP events on
one stream around each leg:

  leg A  a loop over the proofs of the single entries: rg_jindo_encode_challenges_dev (twice for the batch
         challenges), rg_jindo_eval_batch_dev, rg_jindo_eval_point_dev, rg_jindo_eval_partial_dev,
         rg_jindo_encode_challenges_dev for the response challenges, rg_jindo_eval_respond_dev.  All of them
         are asynchronous, so the loop is timed by events, not the host clock.
  leg B  rg_jindo_eval_open_multi_dev and rg_jindo_eval_respond_multi_dev, once each for the N proofs.

Neither leg includes the transcript work between the two halves (the download of the partials, the hash,
the upload of cols x 16 bytes per proof), which is the same for both.  The openings are random residues
made on the device (a timing does not depend on the values), every proof has its own point and bytes,
and both legs must agree on every output word before anything is timed.
usage: python tools/time_jeval.py [--sets t14_b1,mult_t8193_b12] [--proofs 1,8,64] [--iters 400] [--warmup 10] [--runs 3]
       [--once leg-B iterations: no timing, for a rocprofv3 --kernel-trace run]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "ringo-snark_amd")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ringo import jindo  # noqa: E402
from tests.jindo_proto import random_ck  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sets", type=str, default="t14_b1,mult_t8193_b12")
ap.add_argument("--proofs", type=str, default="1,8,64")
ap.add_argument("--iters", type=int, default=400, help="timed iterations at 1 proof; divided by the proof count, at least 20")
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--once", type=int, default=0)
args = ap.parse_args()

assert torch.cuda.is_available(), "time_jeval.py needs the GPU"
PARAMS = json.load(open(os.path.join(ROOT, "tests", "golden", "jindo_params.json")))
stream = torch.cuda.Stream()


def residues(primes, shape, gen):
    """shape[..., limb, d] of uniform canonical residues, made on the device."""
    out = torch.empty(shape, dtype=torch.int64, device="cuda")
    for l, q in enumerate(primes):
        out[..., l, :] = torch.randint(0, q, out[..., l, :].shape, dtype=torch.int64, device="cuda", generator=gen)
    return out


def leg(name, P, prv, n):
    p, B, d = prv.params, P["batch"], P["d"]
    es = prv.eval_shapes()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    rng = np.random.default_rng(7)
    opens = {k: residues(P["qo"] if k == "ob_incom" else P["q"], (n, B) + es[k], gen)
             for k in ("ob_incom", "ob_enc", "ob_mlwe")}
    # points: any canonical element serves (Montgomery form of some value)
    fq = int(P["field_q_hex"], 16)
    vals = [int.from_bytes(rng.bytes(8 * p.L + 8), "little") % fq for _ in range(n)]
    xs = np.array([[(v >> (64 * i)) & (2 ** 64 - 1) for i in range(p.L)] for v in vals], np.uint64)
    d_x = torch.from_numpy(xs.view(np.int64)).cuda()
    up = lambda k: torch.from_numpy(np.frombuffer(rng.bytes(16 * k), np.uint8).copy()).cuda()
    bb, cb = (up(n * B) if B > 1 else None), up(n * P["cols"])
    new = lambda *s: torch.zeros(s, dtype=torch.int64, device="cuda")
    keys = ("ob_enc", "ob_mlwe", "ob_incom", "partial", "pf_enc", "pf_mlwe")
    A = {k: new(n, *es[k]) for k in keys}
    Bo = {k: new(n, *es[k]) for k in keys}
    a_bq, a_bo = new(n, B, p.nq, d), new(n, B, p.nqo, d)
    a_left, a_chals = new(n, P["rows"], p.nq, d), new(n, P["cols"], p.nq, d)
    s1 = new(prv.eval_open_multi_scratch_bytes(n, B) // 8)
    s2 = new(prv.eval_respond_multi_scratch_bytes(n) // 8)
    torch.cuda.synchronize()

    def loop():
        for i in range(n):
            bq = bo = None
            if B > 1:
                bq, bo = a_bq[i], a_bo[i]
                prv.encode_challenges_dev(0, bb[16 * B * i:16 * B * (i + 1)], B, bq, stream=stream)
                prv.encode_challenges_dev(1, bb[16 * B * i:16 * B * (i + 1)], B, bo, stream=stream)
            prv.eval_batch_dev(B, opens["ob_incom"][i], opens["ob_enc"][i], opens["ob_mlwe"][i], bq, bo, A["ob_incom"][i],
                               A["ob_enc"][i], A["ob_mlwe"][i], stream=stream)
            prv.eval_point_dev(d_x[i], a_left[i], stream=stream)
            prv.eval_partial_dev(A["ob_enc"][i], a_left[i], A["partial"][i], stream=stream)
            c0 = 16 * P["cols"] * i
            prv.encode_challenges_dev(0, cb[c0:c0 + 16 * P["cols"]], P["cols"], a_chals[i], stream=stream)
            prv.eval_respond_dev(A["ob_enc"][i], A["ob_mlwe"][i], a_chals[i], A["pf_enc"][i], A["pf_mlwe"][i],
                                 stream=stream)

    def multi():
        if B > 1:
            prv.eval_open_multi_dev(n, B, opens["ob_incom"], opens["ob_enc"], opens["ob_mlwe"], B, 1, d_x, 1, bb,
                                    Bo["ob_enc"], Bo["ob_mlwe"], Bo["ob_incom"], Bo["partial"], s1, stream=stream)
            prv.eval_respond_multi_dev(n, Bo["ob_enc"], Bo["ob_mlwe"], 1, cb, Bo["pf_enc"], Bo["pf_mlwe"], s2,
                                       stream=stream)
        else:
            prv.eval_open_multi_dev(n, 1, opens["ob_incom"], opens["ob_enc"], opens["ob_mlwe"], 1, 1, d_x, 1, None,
                                    None, None, Bo["ob_incom"], Bo["partial"], s1, stream=stream)
            prv.eval_respond_multi_dev(n, opens["ob_enc"], opens["ob_mlwe"], 1, cb, Bo["pf_enc"], Bo["pf_mlwe"], s2,
                                       stream=stream)

    if args.once:
        for _ in range(args.once):
            multi()
        stream.synchronize()
        return
    # both legs agree on every output word before anything is timed
    loop()
    multi()
    stream.synchronize()
    for k in keys:
        if B == 1 and k in ("ob_enc", "ob_mlwe"):  # leg B leaves the openings where they are
            continue
        assert torch.equal(A[k], Bo[k]), f"{name}, {n} proofs: the two legs differ in {k}"
    iters = max(20, args.iters // n)

    def timed(fn):
        with torch.cuda.stream(stream):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(iters):
                fn()
            e1.record(stream)
            e1.synchronize()
        return e0.elapsed_time(e1) / iters

    for fn in (loop, multi):
        for _ in range(args.warmup):
            fn()
    stream.synchronize()
    rows = []
    for run in range(args.runs):  # the legs alternate
        ta, tb = timed(loop), timed(multi)
        rows.append((ta, tb))
        for entry, t in (("A: loop of the single entries", ta), ("B: the two multi calls", tb)):
            print(json.dumps({"leg": entry, "set": name, "proofs": n, "run": run, "iters": iters,
                              "ms_per_batch": round(t, 5), "us_per_proof": round(t * 1e3 / n, 3)}), flush=True)
    for i, entry in enumerate(("A", "B")):
        ts = [r[i] for r in rows]
        print(json.dumps({"summary": entry, "set": name, "proofs": n, "median_ms_per_batch": round(statistics.median(ts), 5),
                          "median_us_per_proof": round(statistics.median(ts) * 1e3 / n, 3), "min_ms": round(min(ts), 5),
                          "max_ms": round(max(ts), 5)}), flush=True)


for name in args.sets.split(","):
    P = PARAMS[name]
    prv = jindo.Prover(jindo.Parameters.from_dict(P, int(P["field_q_hex"], 16)), ck=random_ck(P, 7))
    for n in (int(x) for x in args.proofs.split(",")):
        leg(name, P, prv, n)
