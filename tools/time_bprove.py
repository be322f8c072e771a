"""Times the Buckler prover's three checks for a batch of proofs: ONE rg_buckler_prove_checks_dev of N
proofs against a loop, proof by proof, of the single entries on the same library --
rg_buckler_lin_check_dev (after rg_buckler_checker_set_xof_dev with the proof's bytes), and twice
rg_buckler_eval_circuit_dev + rg_buckler_check_finish_dev (arithCheck, sumCheck).  The shape of
tools/time_bverify.py: the 255-bit Jindo field (L = 4), rank 2^15, embedding rank 2^16, a linear check
of four checkers (NTT, automorphism, projection, recompose) with one pair each, plus an arithmetic
and a sum-check circuit of a few degree-2 terms, 2 public witnesses.  HIP events on the launch stream
around `iters` back-to-back repetitions after `warmup` of the same shape; the two legs alternate,
`--runs` times each, in one process.  After the timing both ways must have left the same outputs.

The launch counts are counted from the code (csrc/buckler_prove.hip, csrc/buckler_lin.hip and the
entries they call), not measured.  The values are random: a timing, not a proof.
usage: python tools/time_bprove.py [--proofs 1,8,64] [--runs 3] [--iters 20] [--warmup 3] [--rank 32768]"""
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
ap.add_argument("--proofs", type=str, default="1,8,64")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rank", type=int, default=1 << 15)
args = ap.parse_args()

assert torch.cuda.is_available(), "time_bprove.py needs the GPU"
q = int(json.load(open(os.path.join(ROOT, "tests", "golden", "fields.json")))["jindo_zp"]["q_hex"], 16)
F = ringo.Field(q)
L, rank, emb = F.L, args.rank, 2 * args.rank
jindo_rank, n_w, n_pw = 4 * rank, 8, 2
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


chks = [buckler.NewNTTChecker(F, rank), buckler.NewAutChecker(F, rank, 5, False), buckler.ProjChecker(F, rank),
        buckler.ProjRecomposeChecker(F, rank, 8)]
pairs = [[(2 * c, 2 * c + 1)] for c in range(4)]
lin = buckler.LinCheckPlan(F, rank, emb, chks, pairs)
a0 = buckler.ArithmeticConstraint(F)
a0.AddTerm(None, 0, 1)
a0.SubTerm(None, 2)
a1 = buckler.ArithmeticConstraint(F)
a1.AddTerm(0, 3, 4)
a1.SubTerm(None, 5, 5)
s0 = buckler.ArithmeticConstraint(F)
s0.AddTerm(None, 6, 7)
s0.AddTerm(1, 0)
arith, sumc = buckler.Circuit(F, [a0, a1]), buckler.Circuit(F, [s0])
arith_max, sum_max = 2 * rank, 2 * rank  # degree 2 within the embedding rank 2 rank
plan = buckler.ProvePlan(F, rank, emb, jindo_rank, n_w, n_pw, lin, arith, arith_max, sumc, sum_max)
embT = lin.emb
stream = torch.cuda.Stream()

# kernels per proof of the loop, from the code.  rg_buckler_lin_check_dev: the power vector; the
# transposes (NTT checker: reverse-and-scale + the two passes of its InvNTT; one kernel each for the
# automorphism, the projection and the recompose checker); Encode (the batched InvNTT at 2^15: two passes;
# the embedding); the forward NTT at 2^16 over 5 vectors (two passes); lin_kernel; the tail (scale, InvNTT:
# two passes, mask add, quorem, split).  set_xof_dev: the pack.  arithCheck: circuit_kernel, InvNTT (two
# passes), quorem, split.  sumCheck: the same with the scale and the mask add.
LOOP = {"set_xof": 1, "lin: powers": 1, "lin: transposes": 3 + 1 + 1 + 1, "lin: encode": 3, "lin: ntt": 2, "lin: pass": 1,
        "lin: tail": 6, "arith": 1 + 2 + 2, "sum": 1 + 1 + 2 + 1 + 2}
# kernels per call of the batch entry, whatever n_proofs: the power table; the transposes (the projection
# checker packs every proof's matrix first: one more); Encode; the forward NTT over 5 n vectors; one
# evaluation kernel per check; ONE InvNTT over 3 n evals; the finish.  At n vectors >= 8 the q255 plan runs
# a batch as two halves, the second on its helper stream: two more launches per transform.
ONE = {"powers": 1, "transposes": 3 + 1 + 2 + 1, "encode": 3, "ntt": 2, "evaluations": 3, "inv_ntt": 2, "finish": 1}


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
    w, pw = dev(n, n_w, emb), dev(n, n_pw, emb)
    chal, lm, sm = dev(n, 4), dev(n, emb), dev(n, emb)
    xof = torch.from_numpy(np.frombuffer(rng.bytes(n * 32 * rank), np.uint8).copy()).cuda().reshape(n, 32 * rank)
    shapes = [k for k in plan.out_elems()]
    o1 = [empty(n, k) for k in shapes]
    o2 = [empty(n, k) for k in shapes]
    scr1 = torch.empty(lin.scratch_bytes() // 8, dtype=torch.int64, device="cuda")
    ev = empty(emb)
    fscr = torch.empty(buckler.check_finish_scratch_bytes(embT) // 8, dtype=torch.int64, device="cuda")
    scr2 = torch.empty(plan.scratch_bytes(n) // 8, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def loop():
        for i in range(n):
            chks[2].set_xof_dev(xof[i], stream=stream)
            lin.lin_check_dev(chal[i, 1], chal[i, 2], lm[i], w[i], n_w, jindo_rank, o1[1][i], o1[2][i], o1[3][i], scr1,
                              stream=stream)
            arith.eval_dev(emb, chal[i, 0], w[i], n_w, pw[i], n_pw, ev, stream=stream)
            buckler.check_finish_dev(embT, rank, ev, None, None, arith_max - rank, 0, o1[0][i], None, None, fscr,
                                     stream=stream)
            sumc.eval_dev(emb, chal[i, 3], w[i], n_w, pw[i], n_pw, ev, stream=stream)
            buckler.check_finish_dev(embT, rank, ev, chal[i, 3], sm[i], sum_max - rank, jindo_rank, o1[4][i], o1[5][i],
                                     o1[6][i], fscr, stream=stream)

    def one():
        plan.checks_dev(n, w, pw, xof, chal, lm, sm, *o2[:7], d_rem0=o2[7], d_scratch=scr2, stream=stream)

    iters = max(2, args.iters // max(1, n // 8))
    for run in range(args.runs):
        for name, fn, launches, bytes_ in (
                ("loop of the single entries", loop, n * sum(LOOP.values()), lin.scratch_bytes()),
                ("rg_buckler_prove_checks_dev", one, sum(ONE.values()), plan.scratch_bytes(n))):
            t = timed(fn, iters)
            print(json.dumps({"entry": name, "proofs": n, "run": run, "iters": iters, "rank": rank, "emb": emb, "L": L,
                              "ms_per_batch": round(t, 4), "us_per_proof": round(t * 1e3 / n, 2),
                              "kernel_launches_counted": launches, "scratch_bytes": bytes_}), flush=True)
    torch.cuda.synchronize()
    for a, b in zip(o1[:7], o2[:7]):
        assert torch.equal(a, b), "the two ways differ"


for n_proofs in (int(x) for x in args.proofs.split(",")):
    leg(n_proofs)
