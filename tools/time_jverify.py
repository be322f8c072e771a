"""Times the Jindo verifier on N proofs two ways, alternating in one process: a loop of N
rg_jindo_verify_dev calls (one proof each; every call allocates, launches, copies its result back and
waits, so the loop is timed on the host clock) against ONE rg_jindo_verify_multi_dev of the N proofs
(HIP events on the launch stream around the calls, then one read of the N records, timed on the host
clock and reported beside it).

The proofs are honest proofs by the C oracle (tests/jindo_proto.py) on a golden parameter set;
`--distinct` of them are built and dealt over the N slots, since a timing does not depend on the
values and an oracle proof costs more than every run here.  Both ways must accept every proof and
agree on every record word.
usage: python tools/time_jverify.py [--sets t14_b1,t10_b8] [--proofs 1,8,64] [--iters 200] [--warmup 20] [--runs 3]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "ringo-snark_amd")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ringo import jindo  # noqa: E402
from tests.jindo_proto import VERIFY_KEYS, honest_proof  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sets", type=str, default="t14_b1,t10_b8")
ap.add_argument("--proofs", type=str, default="1,8,64")
ap.add_argument("--distinct", type=int, default=2)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()

assert torch.cuda.is_available(), "time_jverify.py needs the GPU"
PARAMS = json.load(open(os.path.join(ROOT, "tests", "golden", "jindo_params.json")))
stream = torch.cuda.Stream()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


def leg(name, n, vrf, proofs):
    B = proofs[0]["batch"]
    slots = [proofs[i % len(proofs)] for i in range(n)]
    one = [[dev(pr[k]) for k in VERIFY_KEYS] for pr in proofs]
    many = [None if slots[0][k] is None else dev(np.stack([pr[k] for pr in slots])) for k in VERIFY_KEYS]
    out = torch.zeros((n, jindo.VERIFY_WORDS), dtype=torch.int64, device="cuda")
    nbytes = vrf.verify_multi_scratch_bytes(n, B)
    scratch = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")
    host = torch.empty((n, jindo.VERIFY_WORDS), dtype=torch.int64).pin_memory()
    torch.cuda.synchronize()

    def loop():
        return [vrf.verify_dev(B, *one[i % len(one)], stream=stream) for i in range(n)]

    def multi():
        vrf.verify_multi_dev(n, B, *many, out, scratch, stream=stream)

    rows = []
    for run in range(args.runs):
        for _ in range(args.warmup):
            loop()
        c0 = time.perf_counter()
        for _ in range(args.iters):
            res = loop()
        t_loop = (time.perf_counter() - c0) * 1e3 / args.iters
        with torch.cuda.stream(stream):
            for _ in range(args.warmup):
                multi()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.iters):
                multi()
            e1.record(stream)
            e1.synchronize()
            c0 = time.perf_counter()
            host.copy_(out, non_blocking=True)
            stream.synchronize()
            t_read = (time.perf_counter() - c0) * 1e3
        t_multi = e0.elapsed_time(e1) / args.iters
        rows.append((t_loop, t_multi))
        for entry, t, extra in (("loop of rg_jindo_verify_dev (host clock)", t_loop, {"scratch_bytes": 0}),
                                ("rg_jindo_verify_multi_dev (HIP events)", t_multi,
                                 {"scratch_bytes": nbytes, "final_read_ms": round(t_read, 4)})):
            print(json.dumps({"entry": entry, "set": name, "proofs": n, "run": run, "iters": args.iters,
                              "ms_per_call": round(t, 5), "us_per_proof": round(t * 1e3 / n, 3), **extra}), flush=True)
    got = vrf.unpack_verify_words(host.numpy().view(np.uint64))
    assert all(r.ok for r in res) and all(r.ok for r in got), "an honest proof was rejected"
    for a, b in zip(res, got):
        assert (a.outer_norm_sq, a.inner_norm_sq) == (b.outer_norm_sq, b.inner_norm_sq), "the two ways differ"
        assert (a.eval_lhs == b.eval_lhs).all() and (a.eval_rhs == b.eval_rhs).all(), "the two ways differ"
    for i, entry in enumerate(("loop", "multi")):
        ts = [r[i] for r in rows]
        print(json.dumps({"summary": entry, "set": name, "proofs": n, "median_ms_per_call": round(statistics.median(ts), 5),
                          "median_us_per_proof": round(statistics.median(ts) * 1e3 / n, 3),
                          "min_ms": round(min(ts), 5), "max_ms": round(max(ts), 5)}), flush=True)


for name in args.sets.split(","):
    P = PARAMS[name]
    fq = int(P["field_q_hex"], 16)
    vrf = jindo.Verifier(jindo.Parameters.from_dict(P, fq), crs=b"Jindo!")
    ck = vrf._p.commit_key()
    proofs = [honest_proof(P, fq, ck, seed=23 + i) for i in range(args.distinct)]
    for n in (int(x) for x in args.proofs.split(",")):
        leg(name, n, vrf, proofs)
