"""Times the SHAKE128 transcript of a batch of Jindo proofs on the device against the host, in one process.

  perm  one Keccak-f[1600] of each kernel layout of xof.hip (cooperative: a state per half-wave; lane: a
        state per lane, RINGO_XOF_LAYOUT=lane, experiments build only), at 1 and 64 states: a squeeze and a
        stride-0 absorb of 2,000 blocks, HIP events around the launch, divided by 2,000.
  (a)   the device transcript alone, for both layouts: marshal x, absorb plan A, fork, squeeze the batch
        bytes, absorb them, absorb plan B over pf_partial, squeeze the challenge bytes.  HIP events.
  (b)   the host baseline: download pf_partial, hashlib.shake_128 (OpenSSL) over the same bytes proof after
        proof (the commitments are taken to be on the host already, serialised, and are hashed once: the
        state is cloned at the fork, where the reference resets and hashes them again), upload the challenge bytes.
        Host clock, the stream drained before and after.
  (c)   the whole batched Evaluate: Prover.evaluate_multi_transcript_dev (product layout) against the two-call
        flow with the host transcript between the calls.  Host clock from the first enqueue to the drained stream.
  (d)   the projection XOF at rank 2^15: buckler.proj_xof_dev against hashlib plus the 1 MiB per proof upload.

The framing is a stand-in with Lattigo's shape (8-byte counts before a polynomial and before a row); the
cost does not depend on the prefix bytes.  Openings and commitments are random residues made on the device.
Needs the experiments build for the lane layout: run with RINGO_LIB=ringo-snark_amd/lib/libringo_exp.so, or
pass --product to time the product library's layout alone.
usage: python tools/time_transcript.py [--sets t14_b1,mult_t8193_b12] [--proofs 1,8,64] [--runs 5] [--product]"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "ringo-snark_amd")):
    sys.path.insert(0, p)

ap = argparse.ArgumentParser()
ap.add_argument("--sets", type=str, default="t14_b1,mult_t8193_b12")
ap.add_argument("--proofs", type=str, default="1,8,64")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--product", action="store_true")
args = ap.parse_args()
if not args.product:
    os.environ.setdefault("RINGO_LIB", os.path.join(ROOT, "ringo-snark_amd", "lib", "libringo_exp.so"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ringo import buckler, jindo, xof  # noqa: E402
from tests.jindo_proto import random_ck  # noqa: E402

assert torch.cuda.is_available(), "time_transcript.py needs the GPU"
PARAMS = json.load(open(os.path.join(ROOT, "tests", "golden", "jindo_params.json")))
LAYOUTS = ["coop"] if args.product else ["coop", "lane"]
stream = torch.cuda.Stream()
poly_prefix = lambda levels, n: levels.to_bytes(8, "little") + n.to_bytes(8, "little")
row_prefix = lambda n: n.to_bytes(8, "little")


def with_layout(layout, make):
    """make() with the handles it creates on `layout` (the knob is read when a handle is created)."""
    if layout == "lane":
        os.environ["RINGO_XOF_LAYOUT"] = "lane"
    try:
        return make()
    finally:
        os.environ.pop("RINGO_XOF_LAYOUT", None)


def events(fn, iters=1):
    with torch.cuda.stream(stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(iters):
            fn()
        e1.record(stream)
        e1.synchronize()
    return e0.elapsed_time(e1) / iters


def wall(fn):
    stream.synchronize()
    t0 = time.perf_counter()
    fn()
    stream.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(legs, timer):
    """{name: [ms per run]}: the legs alternate within every run, after the warm-up."""
    for _ in range(args.warmup):
        for fn in legs.values():
            timer(fn)
    out = {k: [] for k in legs}
    for _ in range(args.runs):
        for k, fn in legs.items():
            out[k].append(timer(fn))
    return out


def report(what, n, ms, **extra):
    for k, ts in ms.items():
        print(json.dumps(dict(measure=what, leg=k, proofs=n, median_ms=round(statistics.median(ts), 4),
                              us_per_proof=round(statistics.median(ts) * 1e3 / n, 2), min_ms=round(min(ts), 4),
                              max_ms=round(max(ts), 4), runs=len(ts), **extra)), flush=True)


def perm_latency():
    blocks = 2000
    src = torch.zeros(168 * blocks, dtype=torch.uint8, device="cuda")
    for n in (1, 64):
        out = torch.zeros(n * 168 * blocks, dtype=torch.uint8, device="cuda")
        legs = {}
        for layout in LAYOUTS:
            h = with_layout(layout, lambda: xof.Shake128(n))

            def squeeze(h=h):
                h.reset(stream)
                h.squeeze(out, 168 * blocks, stream=stream)

            def absorb(h=h):
                h.reset(stream)
                h.absorb(src, 168 * blocks, 0, stream=stream)
            legs[f"{layout} squeeze"], legs[f"{layout} absorb"] = squeeze, absorb
        ms = measure(legs, events)
        for k, ts in ms.items():
            print(json.dumps(dict(measure="perm", leg=k, states=n, blocks=blocks,
                                  us_per_permutation=round(statistics.median(ts) * 1e3 / blocks, 3),
                                  min_us=round(min(ts) * 1e3 / blocks, 3), max_us=round(max(ts) * 1e3 / blocks, 3))),
                  flush=True)


def residues(primes, shape, gen):
    out = torch.empty(shape, dtype=torch.int64, device="cuda")
    for l, q in enumerate(primes):
        out[..., l, :] = torch.randint(0, q, out[..., l, :].shape, dtype=torch.int64, device="cuda", generator=gen)
    return out


def poly_bytes(poly):
    levels, n = poly.shape
    return poly_prefix(levels, n) + b"".join(row_prefix(n) + r.tobytes() for r in poly)


def jindo_set(name, P, prv, n):
    p, B, cols = prv.params, P["batch"], P["cols"]
    es = prv.eval_shapes()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    rng = np.random.default_rng(7)
    opens = {k: residues(P["qo"] if k == "ob_incom" else P["q"], (n, B) + es[k], gen)
             for k in ("ob_incom", "ob_enc", "ob_mlwe")}
    com = residues(P["q"], (n, B, p.out_msis, p.nq, p.d), gen)
    fq = int(P["field_q_hex"], 16)
    vals = [int.from_bytes(rng.bytes(8 * p.L + 8), "little") % fq for _ in range(n)]
    d_x = torch.from_numpy(np.array([[(v >> (64 * i)) & (2 ** 64 - 1) for i in range(p.L)] for v in vals],
                                    np.uint64).view(np.int64)).cuda()
    new = lambda *s: torch.zeros(s, dtype=torch.int64, device="cuda")
    o = {k: new(n, *es[k]) for k in ("ob_enc", "ob_mlwe", "ob_incom", "partial", "pf_enc", "pf_mlwe")}
    s1 = new(prv.eval_open_multi_scratch_bytes(n, B) // 8)
    s2 = new(prv.eval_respond_multi_scratch_bytes(n) // 8)
    bb = torch.zeros(n * B * 16, dtype=torch.uint8, device="cuda") if B > 1 else None
    cb = torch.zeros(n * cols * 16, dtype=torch.uint8, device="cuda")
    ob_enc, ob_mlwe = (o["ob_enc"], o["ob_mlwe"]) if B > 1 else (None, None)
    tr = {layout: with_layout(layout, lambda: jindo.Transcript(p, b"Jindo!", B, n, poly_prefix, row_prefix))
          for layout in LAYOUTS}
    # the host's copy of what the transcript reads before the proof: crs, commitments, x.Marshal()
    Rinv = pow(1 << (64 * p.L), -1, fq)
    h_com = com.cpu().numpy().view(np.uint64)
    head = [b"Jindo!" + b"".join(poly_bytes(q) for c in h_com[i] for q in c) + (vals[i] * Rinv % fq).to_bytes(8 * p.L, "big")
            for i in range(n)]
    h_partial = torch.empty(o["partial"].shape, dtype=torch.int64).pin_memory()
    h_cb, h_bb = torch.empty(n * cols * 16, dtype=torch.uint8).pin_memory(), torch.empty(n * max(B, 1) * 16, dtype=torch.uint8).pin_memory()
    msgs = [None] * n

    def host_batch_bytes():
        """the first reading of the transcript (batch > 1).  The head is hashed once and the state cloned,
        as the device flow does; the reference's Reset-and-rewrite would hash it twice"""
        if B > 1:
            for i in range(n):
                msgs[i] = hashlib.shake_128(head[i])
                b = msgs[i].copy().digest(B * 16)
                h_bb[i * B * 16:(i + 1) * B * 16] = torch.frombuffer(bytearray(b), dtype=torch.uint8)
                msgs[i].update(b)
            with torch.cuda.stream(stream):
                bb.copy_(h_bb[:n * B * 16], non_blocking=True)
        else:
            for i in range(n):
                msgs[i] = hashlib.shake_128(head[i])

    def host_challenges():
        with torch.cuda.stream(stream):
            h_partial.copy_(o["partial"], non_blocking=True)
        stream.synchronize()
        part = h_partial.numpy().view(np.uint64)
        for i in range(n):
            m = msgs[i].copy()
            for q in part[i]:
                m.update(poly_bytes(q))
            h_cb[i * cols * 16:(i + 1) * cols * 16] = torch.frombuffer(bytearray(m.digest(cols * 16)), dtype=torch.uint8)
        with torch.cuda.stream(stream):
            cb.copy_(h_cb, non_blocking=True)

    def call1():
        prv.eval_open_multi_dev(n, B, opens["ob_incom"], opens["ob_enc"], opens["ob_mlwe"], B, 1, d_x, 1, bb, ob_enc, ob_mlwe,
                                o["ob_incom"], o["partial"], s1, stream=stream)

    def call2():
        if B > 1:
            prv.eval_respond_multi_dev(n, ob_enc, ob_mlwe, 1, cb, o["pf_enc"], o["pf_mlwe"], s2, stream=stream)
        else:
            prv.eval_respond_multi_dev(n, opens["ob_enc"], opens["ob_mlwe"], 1, cb, o["pf_enc"], o["pf_mlwe"], s2, stream=stream)

    def host_flow():
        host_batch_bytes()
        call1()
        host_challenges()
        call2()

    def device_flow(t=tr["coop"]):
        prv.evaluate_multi_transcript_dev(t, com, opens["ob_incom"], opens["ob_enc"], opens["ob_mlwe"], B, 1, d_x, 1, bb, cb,
                                          ob_enc, ob_mlwe, o["ob_incom"], o["partial"], o["pf_enc"], o["pf_mlwe"], s1, s2,
                                          stream=stream)

    # the two flows agree on every byte and word before anything is timed
    host_flow()
    stream.synchronize()
    want = (cb.clone(), None if bb is None else bb.clone(), o["pf_enc"].clone(), o["pf_mlwe"].clone())
    for layout in LAYOUTS:
        cb.zero_()
        device_flow(tr[layout])
        stream.synchronize()
        assert torch.equal(cb, want[0]) and (bb is None or torch.equal(bb, want[1])), f"{name}: {layout} bytes differ"
        assert torch.equal(o["pf_enc"], want[2]) and torch.equal(o["pf_mlwe"], want[3]), f"{name}: {layout} proof differs"
    extra = dict(set=name, batch=B, plan_a_bytes=len(tr["coop"].plan_a), plan_b_bytes=len(tr["coop"].plan_b))

    def transcript_only(t):
        t.open_dev(com, d_x, 1, bb, stream)
        t.respond_dev(o["partial"], cb, stream)

    report("a: device transcript alone", n,
           measure({layout: (lambda t=tr[layout]: transcript_only(t)) for layout in LAYOUTS}, events), **extra)

    def host_only():
        host_batch_bytes()
        host_challenges()
    report("b: host transcript (download, hashlib, upload)", n, measure({"host": host_only}, wall), **extra)
    report("c: whole Evaluate", n, measure({"device transcript": device_flow, "host transcript between the calls": host_flow},
                                            wall), **extra)


def projection(n, rank=1 << 15):
    rng = np.random.default_rng(9)
    c = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    d_c = torch.from_numpy(c).cuda()
    d_xof = torch.zeros(n * 32 * rank, dtype=torch.uint8, device="cuda")
    h_xof = torch.empty(n * 32 * rank, dtype=torch.uint8).pin_memory()
    sponges = {layout: with_layout(layout, lambda: xof.Shake128(n)) for layout in LAYOUTS}

    def host():
        for i in range(n):
            b = hashlib.shake_128(c[i].tobytes()).digest(32 * rank)
            h_xof[i * 32 * rank:(i + 1) * 32 * rank] = torch.frombuffer(bytearray(b), dtype=torch.uint8)
        with torch.cuda.stream(stream):
            d_xof.copy_(h_xof, non_blocking=True)

    host()
    stream.synchronize()
    want = d_xof.clone()
    legs = {"host squeeze and upload": host}
    for layout in LAYOUTS:
        d_xof.zero_()
        buckler.proj_xof_dev(d_c, rank, d_xof, n, sponge=sponges[layout], stream=stream)
        stream.synchronize()
        assert torch.equal(d_xof, want), f"projection XOF: {layout} differs"
        legs[f"device {layout}"] = lambda s=sponges[layout]: buckler.proj_xof_dev(d_c, rank, d_xof, n, sponge=s, stream=stream)
    report("d: projection XOF", n, measure(legs, wall), rank=rank)


print(json.dumps(dict(lib=os.path.basename(os.environ.get("RINGO_LIB", "libringo.so")), layouts=LAYOUTS, runs=args.runs, warmup=args.warmup)), flush=True)
perm_latency()
for name in args.sets.split(","):
    P = PARAMS[name]
    prv = jindo.Prover(jindo.Parameters.from_dict(P, int(P["field_q_hex"], 16)), ck=random_ck(P, 7))
    for n in (int(x) for x in args.proofs.split(",")):
        jindo_set(name, P, prv, n)
        torch.cuda.empty_cache()
for n in (int(x) for x in args.proofs.split(",")):
    projection(n)
