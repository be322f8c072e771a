"""Times the device entries that build Evaluate's inputs.  HIP events on the launch stream, warm-up
calls of the same shape first, one JSON line per case.

  --what eval        rg_poly_evaluate_batch_dev on `batch` polynomials of n coefficients (stride = n)
                     against the only other way to do that work: a loop of `batch` calls to
                     rg_poly_evaluate_dev on the same buffers.  Three repetitions of each; the
                     condition is that the slowest repetition of the batched call is below the
                     fastest repetition of the loop (exit status 1 otherwise).  Beside it: bytes
                     read per second and f_mul per second of the batched call, and whether the two
                     gave the same words.
  --what challenges  rg_jindo_encode_challenges_dev, n challenges, both rings (for the record)
  --what point       rg_jindo_eval_point_dev (for the record)
usage: python tools/time_eval_batch.py --what eval --field jindo_zp --batch 512 [--n 65536] [--reps 3]
       python tools/time_eval_batch.py --what challenges --params t16_b4096 [--n 4096]
       python tools/time_eval_batch.py --what point --params t16_b4096"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ringo-snark_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ringo  # noqa: E402
from ringo import _lib, bigpoly, jindo  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--what", choices=["eval", "challenges", "point"], required=True)
ap.add_argument("--field", default="jindo_zp")
ap.add_argument("--params", default="t16_b4096")
ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--n", type=int, default=None)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()

assert torch.cuda.is_available(), "time_eval_batch.py needs the GPU"
stream = torch.cuda.Stream()


def timed(fn, iters):
    """ms per call of fn over `iters` back-to-back calls on the stream."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        t0.record(stream)
        for _ in range(iters):
            fn()
        t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1) / iters


def elements(q, L, count):
    """count canonical elements [count][L] on the device: uniform words, the top limb below q's."""
    x = torch.randint(-(1 << 63), (1 << 63) - 1, (count, L), dtype=torch.int64, device="cuda")
    top = q >> (64 * (L - 1))
    x[:, L - 1] = torch.randint(0, min(top, (1 << 63) - 1), (count,), dtype=torch.int64, device="cuda") if top > 1 else 0
    return x


if args.what == "eval":
    q = int(json.load(open(os.path.join(ROOT, "tests", "golden", "fields.json")))[args.field]["q_hex"], 16)
    F = ringo.Field(q)
    L, n, batch = F.L, args.n or 1 << 16, args.batch
    torch.manual_seed(1)
    p = elements(q, L, batch * n)
    x = elements(q, L, 1)
    out_b = torch.zeros((batch, L), dtype=torch.int64, device="cuda")
    out_l = torch.zeros((batch, L), dtype=torch.int64, device="cuda")
    scr_b = torch.zeros(((bigpoly.evaluate_batch_scratch_bytes(F, n, batch) + 7) // 8,), dtype=torch.int64, device="cuda")
    scr_l = torch.zeros((_lib.lib().rg_poly_evaluate_scratch_bytes(F.h, n) // 8 + 1,), dtype=torch.int64, device="cuda")
    lib, st = _lib.lib(), stream.cuda_stream
    pp, xp, op, sp, e = p.data_ptr(), x.data_ptr(), out_l.data_ptr(), scr_l.data_ptr(), L * 8

    def batched():
        bigpoly.evaluate_batch_dev(F, p, n, n, batch, x, out_b, scr_b, stream=stream)

    def loop():  # the calls share one scratch: the stream orders them
        for b in range(batch):
            _lib.check(lib.rg_poly_evaluate_dev(F.h, pp + b * n * e, n, xp, op + b * e, sp, st))

    torch.cuda.synchronize()
    timed(batched, args.warmup)
    timed(loop, 1)
    tb = [timed(batched, args.iters) for _ in range(args.reps)]
    tl = [timed(loop, 1) for _ in range(args.reps)]
    torch.cuda.synchronize()
    equal = bool((out_b == out_l).all().item())
    ok = max(tb) < min(tl)
    read = batch * n * L * 8
    print(json.dumps({"entry": "rg_poly_evaluate_batch_dev", "field": args.field, "L": L, "n": n, "batch": batch,
                      "iters": args.iters, "batched_ms": [round(t, 4) for t in tb],
                      "loop_of_single_ms": [round(t, 3) for t in tl], "same_words": equal,
                      "slowest_batched_below_fastest_loop": ok, "loop_over_batched": round(min(tl) / max(tb), 1),
                      "bytes_read": read, "read_GB_per_s": round(read / max(tb) / 1e6, 1),
                      "f_mul_G_per_s": round(batch * n / max(tb) / 1e6, 2)}), flush=True)
    sys.exit(0 if ok and equal else 1)

P = json.load(open(os.path.join(ROOT, "tests", "golden", "jindo_params.json")))[args.params]
fq = int(P["field_q_hex"], 16)
params = jindo.Parameters.from_dict(P, fq)
rng = np.random.default_rng(1)
sh = params.ck_shapes()
ck = []
for k, primes in (("ck_in", P["q"]), ("ck_mlwe", P["q"]), ("ck_out", P["qo"])):  # any key: the entries read none of it
    a = np.zeros(sh[k], np.uint64)
    for l, pr in enumerate(primes):
        a[..., l, :] = rng.integers(0, pr, size=a[..., l, :].shape, dtype=np.uint64)
    ck.append(a)
prv = jindo.Prover(params, ck=ck)
d = P["d"]

if args.what == "challenges":
    n = args.n or P["batch"]
    byt = torch.randint(0, 256, (n * 16,), dtype=torch.uint8, device="cuda")
    for ring, nl in ((0, params.nq), (1, params.nqo)):
        out = torch.zeros((n, nl, d), dtype=torch.int64, device="cuda")
        fn = lambda: prv.encode_challenges_dev(ring, byt, n, out, stream=stream)  # noqa: E731
        torch.cuda.synchronize()
        timed(fn, args.warmup)
        ts = [timed(fn, args.iters) for _ in range(args.reps)]
        written = n * nl * d * 8
        print(json.dumps({"entry": "rg_jindo_encode_challenges_dev", "params": args.params, "ring": ring, "n": n,
                          "limbs": nl, "d": d, "iters": args.iters, "ms_per_call": [round(t, 4) for t in ts],
                          "bytes_written": written, "written_GB_per_s": round(written / max(ts) / 1e6, 1)}), flush=True)
else:
    x = elements(fq, params.L, 1)
    left = torch.zeros((P["rows"], params.nq, d), dtype=torch.int64, device="cuda")
    right = torch.zeros((P["cols"] * P["slots"], params.L), dtype=torch.int64, device="cuda")
    fn = lambda: prv.eval_point_dev(x, left, right, stream=stream)  # noqa: E731
    torch.cuda.synchronize()
    timed(fn, args.warmup)
    ts = [timed(fn, args.iters) for _ in range(args.reps)]
    print(json.dumps({"entry": "rg_jindo_eval_point_dev", "params": args.params, "rows": P["rows"],
                      "cols_slots": P["cols"] * P["slots"], "limbs": params.nq, "d": d, "iters": args.iters,
                      "ms_per_call": [round(t, 4) for t in ts]}), flush=True)
