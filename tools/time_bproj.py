"""Times what the Buckler prover does between its commit rounds for a batch of proofs: ONE
rg_buckler_prove_proj_round_dev and TWO rg_buckler_sumcheck_mask_batch_dev of N proofs against a loop,
proof by proof, of the single entries on the same library -- rg_buckler_checker_set_xof_dev with the
proof's bytes, rg_buckler_checker_transform_dev, rg_buckler_dcmp_proj_dev and twice
rg_buckler_sumcheck_mask_dev.  The shape of tools/time_bprove.py: the 255-bit Jindo field (L = 4), rank
2^15, embedding rank 2^16, one projection constraint with decomposeBase(rank * 2^32) (47 digits), the
linear check's and the sum check's mask at mask rank 2 rank.  HIP events on the launch stream around
`iters` back-to-back repetitions after `warmup` of the same shape; the two legs alternate, `--runs`
times each, in one process, and the summary line gives the median with min..max.  After the timing
both ways must have left the same outputs; the first error ends the run.

The launch counts are counted from the code (csrc/buckler_proj.hip, csrc/buckler_lin.hip,
csrc/buckler_dcmp.hip), not measured.  The values are random: a timing, not a proof.
usage: timeout 900 python tools/time_bproj.py [--proofs 1,8,64] [--runs 3] [--iters 20] [--warmup 3] [--rank 32768]"""
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

assert torch.cuda.is_available(), "time_bproj.py needs the GPU"
q = int(json.load(open(os.path.join(ROOT, "tests", "golden", "fields.json")))["jindo_zp"]["q_hex"], 16)
F = ringo.Field(q)
L, rank, emb = F.L, args.rank, 2 * args.rank
mask_rank = 2 * rank
n_w, SRC, PROJ, DCMP = 3, 0, 1, 2
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


dc = buckler.Decomposer(F, rank << 32)  # decomposeBase(rank * bound), bound = 2^32
chk = buckler.ProjChecker(F, rank)
plan = buckler.ProjRoundPlan(F, rank, n_w, [(SRC, PROJ, DCMP, dc)])
stream = torch.cuda.Stream()

# kernels per proof of the loop, from the code: the pack; the transform (products per chunk, their sum);
# the decomposition; one mask kernel per mask
LOOP = {"set_xof": 1, "transform": 2, "dcmp_proj": 1, "masks": 2}
# kernels of the batch calls, whatever n_proofs and however many constraints: the products, the sum
# with the decomposition; one mask kernel per mask
ONE = {"proj_round": 2, "masks": 2}


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
    rl, rs = dev(n, mask_rank), dev(n, mask_rank)
    xof = torch.from_numpy(np.frombuffer(rng.bytes(n * 32 * rank), np.uint8).copy()).cuda().reshape(n, 32 * rank)
    lm1, sm1, ls1, ss1 = empty(n, emb), empty(n, emb), empty(n), empty(n)
    lm2, sm2, ls2, ss2 = empty(n, emb), empty(n, emb), empty(n), empty(n)
    lc2, sc2 = empty(n, mask_rank), empty(n, mask_rank)
    scr1 = torch.empty(chk.scratch_bytes(1) // 8, dtype=torch.int64, device="cuda")
    scr2 = torch.empty(plan.scratch_bytes(n) // 8, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def loop():
        for i in range(n):
            chk.set_xof_dev(xof[i], stream=stream)
            chk.transform_dev(w1[i, PROJ], w1[i, SRC], 1, scr1, stream=stream)
            dc.proj_dev(w1[i, DCMP], w1[i, PROJ], rank, stream=stream)
            buckler.sumcheck_mask_dev(F, rank, mask_rank, emb, rl[i], lm1[i], ls1[i], stream=stream)
            buckler.sumcheck_mask_dev(F, rank, mask_rank, emb, rs[i], sm1[i], ss1[i], stream=stream)

    def one():
        plan.round_dev(n, w2, xof, scr2, stream=stream)
        buckler.sumcheck_mask_batch_dev(F, rank, mask_rank, emb, n, rl, lm2, ls2, d_mask_com=lc2, stream=stream)
        buckler.sumcheck_mask_batch_dev(F, rank, mask_rank, emb, n, rs, sm2, ss2, d_mask_com=sc2, stream=stream)

    iters = max(2, args.iters // max(1, n // 8))
    legs = (("loop of the single entries", loop, n * sum(LOOP.values()), chk.scratch_bytes(1)),
            ("proj_round_dev + 2 sumcheck_mask_batch_dev", one, sum(ONE.values()), plan.scratch_bytes(n)))
    us = {name: [] for name, _, _, _ in legs}
    for run in range(args.runs):
        for name, fn, launches, bytes_ in legs:
            t = timed(fn, iters)
            us[name].append(t * 1e3 / n)
            print(json.dumps({"entry": name, "proofs": n, "run": run, "iters": iters, "rank": rank, "emb": emb, "L": L,
                              "nb": len(dc.dcmpBase), "mask_rank": mask_rank, "ms_per_batch": round(t, 4),
                              "us_per_proof": round(t * 1e3 / n, 2), "kernel_launches_counted": launches,
                              "scratch_bytes": bytes_}), flush=True)
    torch.cuda.synchronize()
    for a, b in ((w1, w2), (lm1, lm2), (sm1, sm2), (ls1, ls2), (ss1, ss2), (lm1[:, :mask_rank], lc2),
                 (sm1[:, :mask_rank], sc2)):
        assert torch.equal(a, b), "the two ways differ"
    (ln, lu), (bn, bu) = us.items()
    spread = max(max(lu) - min(lu), max(bu) - min(bu))
    print(json.dumps({"summary": True, "proofs": n, "outputs_equal": True,
                      "loop_us_per_proof": {"median": round(statistics.median(lu), 2), "min": round(min(lu), 2),
                                            "max": round(max(lu), 2)},
                      "batch_us_per_proof": {"median": round(statistics.median(bu), 2), "min": round(min(bu), 2),
                                             "max": round(max(bu), 2)},
                      "loop_over_batch": round(statistics.median(lu) / statistics.median(bu), 2),
                      "batch_below_loop_by_more_than_the_spread": statistics.median(lu) - statistics.median(bu) > spread,
                      "scratch_bytes_batch": plan.scratch_bytes(n)}), flush=True)


for n_proofs in (int(x) for x in args.proofs.split(",")):
    leg(n_proofs)
