"""Times what the Buckler prover does to its witness table before and at its first commit round for a batch
of proofs: ONE rg_buckler_prove_dcmp_round_dev and ONE rg_buckler_prove_encode_round_dev of N proofs
against a loop, proof by proof, of the single entries a caller needs today on the same library --
rg_buckler_dcmp_inf_dev and rg_buckler_dcmp_two_dev for the proof's constraints, rg_buckler_encode_dev for
the proof's run of first-round rows, and one device copy per commit row (wEcd[i].Coeffs[:rank + 1]).  The
shape of tools/time_bproj.py: the 255-bit Jindo field (L = 4), rank 2^15, embedding rank 2^16, one
infinity-norm constraint with decomposeBase(2^16) (16 digit rows), one two-norm constraint with
decomposeBase(rank * 2^32) (47 digits); the table holds the witness, its 16 digit rows, the two-norm row
and the two rows of a second round, so the first round's 18 rows are not the whole table and the batch
call gathers them.  Three things are timed, each both ways: the dcmp round, the first encode round, and the
two one after the other.  HIP events on the launch stream around `iters` back-to-back repetitions after
`warmup` of the same shape; the legs alternate, `--runs` times each, in one process, and the summary
lines give the median with min..max.  After the timing both ways must have left the same outputs; the
first error ends the run.

The launch counts are counted from the code (csrc/buckler_wround.hip, csrc/buckler_dcmp.hip,
csrc/buckler.hip) and leave out the NTT plan's own launches, which both ways have.  The values are random:
a timing, not a proof.
usage: timeout 900 python tools/time_bwit.py [--proofs 1,8,64] [--runs 3] [--iters 20] [--warmup 3] [--rank 32768]"""
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

assert torch.cuda.is_available(), "time_bwit.py needs the GPU"
q = int(json.load(open(os.path.join(ROOT, "tests", "golden", "fields.json")))["jindo_zp"]["q_hex"], 16)
F = ringo.Field(q)
L, rank, emb = F.L, args.rank, 2 * args.rank
dc_inf = buckler.Decomposer(F, 1 << 16)  # decomposeBase(bound), bound = 2^16
dc_two = buckler.Decomposer(F, rank << 32)
nb = len(dc_inf.dcmpBase)
SRC, DIGITS, TWO = 0, list(range(1, 1 + nb)), 1 + nb
n_first = 2 + nb          # the first round's rows: 0 .. n_first - 1, one run
n_w = n_first + 2         # and the two rows of the second round
rng = np.random.default_rng(1)

POOL = torch.from_numpy(F.random(1 << 18, rng).view(np.int64)).cuda()  # canonical elements, reused by rotation


def dev(*shape):
    """Random canonical elements [*shape][L]: rotations of one pool (drawing 2^25 residues takes minutes)."""
    n = int(np.prod(shape))
    reps = -(-n // POOL.shape[0])
    off = int(rng.integers(0, POOL.shape[0]))
    return torch.roll(POOL, off, 0).repeat(reps, 1)[:n].reshape(*shape, L).contiguous()


def empty(*shape):
    return torch.empty((*shape, L), dtype=torch.int64, device="cuda")


dplan = buckler.DcmpRoundPlan(F, rank, n_w, inf=[(SRC, dc_inf, DIGITS)], two=[(SRC, dc_two, TWO)])
eplan = buckler.EncodeRoundPlan(F, rank, emb, n_w, range(n_first))
enc = buckler.NewEncoder(F, rank, emb)
stream = torch.cuda.Stream()

# kernels per proof of the loop, from the code: the digits; the squares and the final walk; the embed pass
# and one copy per commit row (the InvNTT's own launches left out)
LOOP = {"dcmp": 1 + 2, "encode": 1 + n_first}
# kernels of the batch calls, whatever n_proofs: digits, squares, final walk; gather and embed
ONE = {"dcmp": 3, "encode": 2}


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
    w1 = dev(n, n_w, rank)
    w2 = w1.clone()
    rand = dev(n, n_first)
    e1 = dev(n, n_w, emb)  # the second round's rows must come back as they are
    e2 = e1.clone()
    sq1, sq2 = empty(n, 1), empty(n, 1)
    c1, c2 = empty(n, n_first, rank + 1), empty(n, n_first, rank + 1)
    scr_two = torch.empty(max(1, dc_two.scratch_bytes(1, rank) // 8), dtype=torch.int64, device="cuda")
    scr_enc = torch.empty(max(1, enc.scratch_bytes(n_first) // 8), dtype=torch.int64, device="cuda")
    scr_d = torch.empty(max(1, dplan.scratch_bytes(n) // 8), dtype=torch.int64, device="cuda")
    scr_e = torch.empty(max(1, eplan.scratch_bytes(n) // 8), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def dcmp_loop():
        for i in range(n):
            dc_inf.inf_dev(w1[i, 1:1 + nb], w1[i, SRC], 1, rank, stream=stream)  # the digit rows are one run
            dc_two.two_dev(w1[i, TWO], w1[i, SRC], 1, rank, d_sq=sq1[i], d_scratch=scr_two, stream=stream)

    def encode_loop():
        for i in range(n):
            enc.encode_dev(e1[i, :n_first], w1[i, :n_first], n_first, d_rand=rand[i], d_scratch=scr_enc, stream=stream)
            for s in range(n_first):
                c1[i, s].copy_(e1[i, s, :rank + 1])  # comPolys[s] = wEcd[s].Coeffs[:rank + 1], contiguous

    def dcmp_one():
        dplan.round_dev(n, w2, sq2, scr_d, stream=stream)

    def encode_one():
        eplan.round_dev(n, w2, e2, d_rand=rand, d_com=c2, d_scratch=scr_e, stream=stream)

    def both_loop():
        dcmp_loop()
        encode_loop()

    def both_one():
        dcmp_one()
        encode_one()

    iters = max(2, args.iters // max(1, n // 8))
    things = (("dcmp round", dcmp_loop, dcmp_one, n * LOOP["dcmp"], ONE["dcmp"], dplan.scratch_bytes(n)),
              ("first encode round", encode_loop, encode_one, n * LOOP["encode"], ONE["encode"], eplan.scratch_bytes(n)),
              ("both", both_loop, both_one, n * sum(LOOP.values()), sum(ONE.values()),
               dplan.scratch_bytes(n) + eplan.scratch_bytes(n)))
    us = {(name, way): [] for name, *_ in things for way in ("loop", "batch")}
    for run in range(args.runs):
        for name, loop, one, l_launch, b_launch, bytes_ in things:
            for way, fn, launches in (("loop", loop, l_launch), ("batch", one, b_launch)):
                t = timed(fn, iters)
                us[(name, way)].append(t * 1e3 / n)
                print(json.dumps({"thing": name, "way": way, "proofs": n, "run": run, "iters": iters, "rank": rank,
                                  "emb": emb, "L": L, "nb_inf": nb, "nb_two": len(dc_two.dcmpBase), "n_w": n_w,
                                  "n_sel": n_first, "ms_per_batch": round(t, 4), "us_per_proof": round(t * 1e3 / n, 2),
                                  "kernel_launches_counted_without_the_ntt": launches,
                                  "scratch_bytes": bytes_ if way == "batch" else None}), flush=True)
    torch.cuda.synchronize()
    for a, b in ((w1, w2), (sq1, sq2), (e1, e2), (c1, c2)):
        assert torch.equal(a, b), "the two ways differ"
    for name, _, _, l_launch, b_launch, bytes_ in things:
        lu, bu = us[(name, "loop")], us[(name, "batch")]
        spread = max(max(lu) - min(lu), max(bu) - min(bu))
        print(json.dumps({"summary": True, "thing": name, "proofs": n, "outputs_equal": True,
                          "loop_us_per_proof": {"median": round(statistics.median(lu), 2), "min": round(min(lu), 2),
                                                "max": round(max(lu), 2)},
                          "batch_us_per_proof": {"median": round(statistics.median(bu), 2), "min": round(min(bu), 2),
                                                 "max": round(max(bu), 2)},
                          "loop_over_batch": round(statistics.median(lu) / statistics.median(bu), 2),
                          "batch_below_loop_by_more_than_the_spread": statistics.median(lu) - statistics.median(bu) > spread,
                          "launches_loop": l_launch, "launches_batch": b_launch, "scratch_bytes_batch": bytes_}),
              flush=True)


for n_proofs in (int(x) for x in args.proofs.split(",")):
    leg(n_proofs)
