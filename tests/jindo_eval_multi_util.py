"""Shared by test_gpu_jindo_eval_multi.py (GPU) and test_oracle_jindo_eval_multi.py (CPU): the cases of
the batch prover's two Evaluate calls (include/ringo.h rg_jindo_eval_open_multi_dev,
rg_jindo_eval_respond_multi_dev) and what the C oracle says their outputs are.

A case is N proofs of one parameter set, each with its own point, batch bytes and challenge bytes.
The openings are residues dealt over the slots (Evaluate's arithmetic does not care whether they are
honest): uniform, or every word at q - 1, or crafted so that the exact sum over the batch provably
passes 2^128 (crafted_batch)."""
import json
import os

import numpy as np

import coracle as co
from tests.jindo_proto import left_right, mont

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "jindo_params.json")))
SYNTH = json.load(open(os.path.join(HERE, "golden", "jindo_synth_params.json")))
N = 3
OUT_KEYS = ("ob_enc", "ob_mlwe", "pf_incom", "pf_partial", "pf_enc", "pf_mlwe")


def params(name):
    """(P, field modulus) of a golden or synthetic set, or of "rows21": syn_d256_q62top with 21 rows,
    where the sum over the rows needs the third accumulator word and a sum over a batch of 2 does not.
    A name "set@rows=R" is the set with R rows (and the rank that goes with them)."""
    if name == "rows21":
        P, _ = params("syn_d256_q62top@rows=21")
        assert P["rank"] == 640
    elif "@rows=" in name:
        base, rows = name.split("@rows=")
        P = dict(params(base)[0], rows=int(rows))
        P["rank"] = (P["rows"] - 1) * P["cols"] * P["slots"]
    else:
        P = GOLDEN[name] if name in GOLDEN else SYNTH[name]
    return P, int(P["field_q_hex"], 16)


def acc_wide(primes, terms):
    """launch_mac's criterion (ringo-snark_amd/csrc/jindo_verify.hip acc_wide): `terms` products below
    qmax^2 may reach 2^128, so the exact sum keeps a third word."""
    import math
    return 2.0 * math.log2(max(primes) - 1) + math.log2(terms + 1.0) >= 127.5


def shapes(P):
    nq, nqo, d, nm = len(P["q"]), len(P["qo"]), P["d"], P["in_msis"] + P["mlwe"]
    return dict(incom=(P["in_com_dcmp_len"], nqo, d), enc=(P["cols"] + 1, P["rows"], nq, d),
                mlwe=(P["cols"] + 1, nm, nq, d), partial=(P["cols"] + 1, nq, d), pf_enc=(P["rows"], nq, d),
                pf_mlwe=(nm, nq, d))


def residues(primes, shape, rng, top):
    """shape + (len(primes), d-last-axis given in shape): uniform canonical residues, or q - 1 everywhere."""
    out = np.zeros(shape, np.uint64)
    for l, q in enumerate(primes):
        out[..., l, :] = np.uint64(q - 1) if top else rng.integers(0, q, size=out[..., l, :].shape, dtype=np.uint64)
    return out


def make_case(name, batch, seed, fill="uniform"):
    """N proofs' inputs: openings [N][batch]..., points (Montgomery ints), batch bytes, challenge bytes."""
    P, fq = params(name)
    F = co.CField(fq)
    sh, rng = shapes(P), np.random.default_rng(seed)
    top = fill != "uniform"
    c = dict(name=name, P=P, fq=fq, batch=batch, fill=fill,
             incom=residues(P["qo"], (N, batch) + sh["incom"], rng, top),
             enc=residues(P["q"], (N, batch) + sh["enc"], rng, top),
             mlwe=residues(P["q"], (N, batch) + sh["mlwe"], rng, top),
             xs=[mont(F, int.from_bytes(rng.bytes(40), "little")) for _ in range(N)],
             bbytes=[[rng.bytes(16) for _ in range(batch)] for _ in range(N)],
             cbytes=[[rng.bytes(16) for _ in range(P["cols"])] for _ in range(N)])
    if fill == "crafted":
        crafted_batch(c, rng)
    return c


def crafted_batch(c, rng):
    """Proof 0's batch bytes are the `batch` strings, out of a pool, whose ringQ encodings are largest at
    one position (limb 0, coefficient k); with every opening word at q - 1 the exact sum over the batch
    at that position is (q - 1) * sum_t batch[t][k], asserted here to pass 2^128."""
    P, cj = c["P"], co.CJindo(c["P"], c["fq"])
    q, k = P["q"][0], 5
    pool = [rng.bytes(16) for _ in range(12 * c["batch"])]
    pool.sort(key=lambda b: int(cj.encode_challenge(0, b)[0, k]), reverse=True)
    c["bbytes"][0] = pool[:c["batch"]]
    s = (q - 1) * sum(int(cj.encode_challenge(0, b)[0, k]) for b in c["bbytes"][0])
    assert s >= 1 << 128, "the crafted batch sum stays below 2^128"
    c["crafted_at"] = (0, k)


def oracle(c):
    """The C oracle's Evaluate of every proof of the case: a dict of OUT_KEYS, each stacked over the
    proofs (ob_enc / ob_mlwe are the openings themselves when batch == 1), plus bq, bo, left, chals."""
    P, fq, B = c["P"], c["fq"], c["batch"]
    cj, F = co.CJindo(P, fq), co.CField(fq)
    out = {k: [] for k in OUT_KEYS + ("bq", "bo", "left", "chals")}
    for p in range(N):
        if B > 1:
            bq = np.stack([cj.encode_challenge(0, b) for b in c["bbytes"][p]])
            bo = np.stack([cj.encode_challenge(1, b) for b in c["bbytes"][p]])
            ob = cj.eval_batch(c["incom"][p], c["enc"][p], c["mlwe"][p], bq, bo)
            out["bq"].append(bq)
            out["bo"].append(bo)
        else:  # openBatch = open[0] (prover.go:267-269)
            ob = dict(ob_incom=c["incom"][p, 0], ob_enc=c["enc"][p, 0], ob_mlwe=c["mlwe"][p, 0])
        left = np.stack([cj.encode(co.to_limbs([e], F.L)) for e in left_right(P, F, c["xs"][p])[0]])
        chals = np.stack([cj.encode_challenge(0, b) for b in c["cbytes"][p]])
        pe, pm = cj.eval_respond(ob["ob_enc"], ob["ob_mlwe"], chals)
        for k, v in (("ob_enc", ob["ob_enc"]), ("ob_mlwe", ob["ob_mlwe"]), ("pf_incom", ob["ob_incom"]),
                     ("pf_partial", cj.eval_partial(ob["ob_enc"], left)), ("pf_enc", pe), ("pf_mlwe", pm),
                     ("left", left), ("chals", chals)):
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items() if v}
