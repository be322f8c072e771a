"""Times the Buckler verifier's checks on the device: rg_buckler_verify_checks_dev at rank 2^15 over the
255-bit Jindo field (L = 4), a linear check of four checkers (NTT, automorphism, projection, recompose)
with one pair each, 4 public witnesses.  HIP events on the launch stream around `iters` back-to-back
calls, after `warmup` calls of the same shape (the method of tools/time_dcmp.py).

Beside it, the same evaluations obtained the way DESIGN.md section 7 described the composition before
this entry existed: the power vector and the transposes, then per vector one rg_buckler_encode_dev at
the embedding rank 2^16 and one rg_poly_evaluate_dev, then the nine evaluations copied back and the
stream waited for (host clock around the loop, since the copy back ends every call); the scalar
algebra that would follow on the host is not in that figure.

With --proofs N[,N...] the script times instead, per N and alternating in one process, a loop of N
rg_buckler_verify_checks_dev calls (one proof each, one scratch) against ONE
rg_buckler_verify_checks_multi_dev of the same N proofs, `--runs` times each, and prints one line per
leg and run with the time per proof and the scratch bytes; the composition leg is skipped.

The launch counts are counted from the code (csrc/buckler_verify.hip and the entries it calls), not
measured.  The values are random: a timing, not a proof.
usage: python tools/time_bverify.py [--iters 200] [--warmup 20] [--rank 32768] [--proofs 1,8,64 [--runs 3]]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ringo-snark_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ringo  # noqa: E402
from ringo import _lib, buckler  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--rank", type=int, default=1 << 15)
ap.add_argument("--proofs", type=str, default="", help="comma-separated batch sizes for the batch-entry leg")
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()

assert torch.cuda.is_available(), "time_bverify.py needs the GPU"
q = int(json.load(open(os.path.join(ROOT, "tests", "golden", "fields.json")))["jindo_zp"]["q_hex"], 16)
F = ringo.Field(q)
L, rank, emb, n_pw = F.L, args.rank, 2 * args.rank, 4
rng = np.random.default_rng(1)


def dev(n):
    return torch.from_numpy(F.random(n, rng).view(np.int64)).cuda().reshape(n, L)


chks = [buckler.NewNTTChecker(F, rank), buckler.NewAutChecker(F, rank, 5, False),
        buckler.ProjChecker(F, rank).SetXOF(rng.bytes(32 * rank)), buckler.ProjRecomposeChecker(F, rank, 8)]
pairs = [[(2 * c, 2 * c + 1)] for c in range(4)]
w_cnt = 8
lin = buckler.LinCheckPlan(F, rank, emb, chks, pairs)
plan = buckler.VerifyPlan(F, rank, 4 * rank, w_cnt, n_pw, lin, None, None)
d_evals, d_chal, d_ms = dev(plan.n_evals), dev(5), dev(2)
d_pw = dev(n_pw * rank).reshape(n_pw, rank, L)
d_verdict = torch.zeros(1, dtype=torch.int64, device="cuda")
d_pwe = torch.zeros((n_pw, L), dtype=torch.int64, device="cuda")
scr = torch.empty(plan.scratch_bytes() // 8, dtype=torch.int64, device="cuda")
stream = torch.cuda.Stream()
torch.cuda.synchronize()


def one_call():
    plan.checks_dev(d_evals, d_pw, d_chal, d_ms, d_verdict, None, d_pwe, scr, stream=stream)


with torch.cuda.stream(stream):
    for _ in range(args.warmup):
        one_call()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for _ in range(args.iters):
        one_call()
    t1.record(stream)
t1.synchronize()
ms = t0.elapsed_time(t1) / args.iters
# kernels per call, from the code: the power vector; the transposes (NTT checker: reverse-and-scale + the
# two passes of its InvNTT; one kernel each for the automorphism, the projection and the recompose
# checker); the batched InvNTT over 9 vectors (two passes, and at a batch of 8 or more the q255 plan runs
# the batch as two halves, the second on its helper stream: four launches); the batched evaluate (two
# power tables, tiles, fold); verify_decide_kernel.  The public witnesses join the batch by one
# device-to-device copy, which is no kernel.
nv = 1 + len(chks) + n_pw
parts = {"powers": 1, "transposes": 3 + 1 + 1 + 1, "inv_ntt": 4 if nv >= 8 else 2, "evaluate": 4, "decide": 1}
print(json.dumps({"entry": "rg_buckler_verify_checks_dev", "field": "jindo_zp", "L": L, "rank": rank, "checkers": 4,
                  "pairs": 4, "n_pw": n_pw, "iters": args.iters, "ms_per_call": round(ms, 5),
                  "kernel_launches_per_call": sum(parts.values()), "launches": parts, "d2d_copies_per_call": 1}),
      flush=True)

# ---- N proofs: a loop of single calls against one batch call -----------------------------------------
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


def proofs_leg(n):
    """n proofs with every input different but the XOF bytes, which are the checker's own for every proof
    so that both ways compute the same thing; they must leave the same verdicts and pwEvals."""
    m_evals, m_chal, m_ms = dev(n * plan.n_evals).reshape(n, -1, L), dev(n * 5).reshape(n, 5, L), dev(n * 2).reshape(n, 2, L)
    m_pw = dev(n * n_pw * rank).reshape(n, n_pw, rank, L)
    m_xof = torch.from_numpy(np.frombuffer(rng.bytes(32 * rank), np.uint8).copy()).cuda().repeat(n, 1)  # the checker's
    v1, v2 = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(2))
    pe1, pe2 = (torch.zeros((n, n_pw, L), dtype=torch.int64, device="cuda") for _ in range(2))
    chks[2].set_xof_dev(m_xof[0])
    torch.cuda.synchronize()
    mscr = torch.empty(plan.scratch_bytes_multi(n) // 8, dtype=torch.int64, device="cuda")

    def loop():
        for i in range(n):
            plan.checks_dev(m_evals[i], m_pw[i], m_chal[i], m_ms[i], v1[i:i + 1], None, pe1[i], scr, stream=stream)

    def multi():
        plan.checks_multi_dev(n, m_evals, m_pw, m_xof, m_chal, m_ms, v2, None, pe2, mscr, stream=stream)

    for run in range(args.runs):
        for name, fn, bytes_ in (("loop of rg_buckler_verify_checks_dev", loop, plan.scratch_bytes()),
                                 ("rg_buckler_verify_checks_multi_dev", multi, plan.scratch_bytes_multi(n))):
            t = timed(fn, args.iters)
            print(json.dumps({"entry": name, "proofs": n, "run": run, "iters": args.iters, "rank": rank, "L": L,
                              "ms_per_batch": round(t, 5), "us_per_proof": round(t * 1e3 / n, 3),
                              "scratch_bytes": bytes_}), flush=True)
    torch.cuda.synchronize()
    assert (v1.cpu() == v2.cpu()).all() and (pe1.cpu() == pe2.cpu()).all(), "the two ways differ"


if args.proofs:
    for n_proofs in (int(x) for x in args.proofs.split(",")):
        proofs_leg(n_proofs)
    sys.exit(0)

# ---- the composition of existing entries, one vector at a time ---------------------------------------
lib = _lib.lib()
enc = buckler.NewEncoder(F, rank, emb)
vec = torch.empty((nv, rank, L), dtype=torch.int64, device="cuda")
ecd = torch.empty((emb, L), dtype=torch.int64, device="cuda")
ev = torch.empty((nv, L), dtype=torch.int64, device="cuda")
escr = torch.empty(max(1, lib.rg_poly_evaluate_scratch_bytes(F.h, emb) // 8), dtype=torch.int64, device="cuda")
host = torch.empty((nv, L), dtype=torch.int64).pin_memory()
s = stream.cuda_stream


def composed():
    buckler.powers_dev(F, d_chal[3], rank, vec[0], stream=stream)
    for c, chk in enumerate(chks):
        chk.transpose_dev(vec[1 + c], vec[0], 1, stream=stream)
    vec[1 + len(chks):].copy_(d_pw, non_blocking=True)
    for i in range(nv):
        enc.encode_dev(ecd, vec[i], 1, stream=stream)
        _lib.check(lib.rg_poly_evaluate_dev(F.h, ecd.data_ptr(), emb, d_chal[0].data_ptr(), ev[i].data_ptr(),
                                            escr.data_ptr(), s))
    host.copy_(ev, non_blocking=True)
    stream.synchronize()


with torch.cuda.stream(stream):
    for _ in range(args.warmup):
        composed()
    c0 = time.perf_counter()
    for _ in range(args.iters):
        composed()
    c1 = time.perf_counter()
print(json.dumps({"entry": "composition: powers, transposes, per vector rg_buckler_encode_dev at 2^16 + "
                           "rg_poly_evaluate_dev, copy back", "vectors": nv, "iters": args.iters,
                  "ms_per_call_host_clock": round((c1 - c0) * 1e3 / args.iters, 5),
                  "not_included": "the scalar algebra of the three checks on the host"}), flush=True)
# both ways give the same evaluations
torch.cuda.synchronize()
assert (ev[1 + len(chks):].cpu() == d_pwe.cpu()).all(), "pwEvals differ between the two ways"
