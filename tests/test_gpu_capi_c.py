"""GPU: the C ABI called from C.  tools/abi_replay.c (built beside the library) replays the call
sequences of INTEGRATION.md as a cgo caller would make them -- ringo.h and the C library only, every
device buffer from rg_malloc, every transfer through rg_memcpy_h2d / rg_memcpy_d2h + rg_stream_sync,
the null stream -- on inputs written here, and every array it writes back is compared bit for bit
with the C oracle (coracle / pyref) and the Buckler restatements.  No tolerances.

Each test runs the program once, as a fresh child process; the 110 s limit only ends a hung child
(test_gpu_samplers.py gives its child the same) and is no performance claim."""
import hashlib
import json
import os
import subprocess
import time

import numpy as np
import pytest

import coracle as co
import pyref
from ringo import jindo
from tests import buckler_dcmp_ref as D
from tests import buckler_lin_ref as R
from tests.buckler_lin_util import RECOMPOSE_BOUND, completeness_circuit, rand_ints
from tests.jindo_proto import SD_KEYS, VERIFY_KEYS, left_right, mont
from tests.jindo_util import make_randomness, make_v

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPLAY = os.path.join(os.path.dirname(HERE), "ringo-snark_amd", "lib", "abi_replay")
PARAMS = json.load(open(os.path.join(HERE, "golden", "jindo_params.json")))
GOLD = json.load(open(os.path.join(HERE, "golden", "jindo_commit_golden.json")))


class Dir:
    """The directory abi_replay reads and writes: NAME.bin arrays and params.txt."""

    def __init__(self, path):
        self.path = path

    def put(self, name, arr):
        np.ascontiguousarray(arr).tofile(os.path.join(self.path, name + ".bin"))

    def put_bytes(self, name, b):
        with open(os.path.join(self.path, name + ".bin"), "wb") as f:
            f.write(b)

    def params(self, **kv):
        with open(os.path.join(self.path, "params.txt"), "w") as f:
            for k, v in kv.items():
                if isinstance(v, float):  # doubles travel as their bit patterns
                    v = int(np.array([v], np.float64).view(np.uint64)[0])
                f.write(f"{k} {int(v)}\n")

    def get(self, name, shape, dtype=np.uint64):
        a = np.fromfile(os.path.join(self.path, name + ".bin"), dtype=dtype)
        assert a.size == int(np.prod(shape)), (name, a.size, shape)
        return a.reshape(shape)

    def raw(self, name):
        return open(os.path.join(self.path, name + ".bin"), "rb").read()

    def run(self, mode):
        assert os.path.exists(REPLAY), f"{REPLAY} not built: run __graft_entry__.build()"
        t0 = time.perf_counter()
        r = subprocess.run([REPLAY, mode, self.path], capture_output=True, text=True, timeout=110)
        print(f"abi_replay {mode}: {time.perf_counter() - t0:.2f} s")
        assert r.returncode == 0, (r.returncode, r.stderr)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    assert (got == want).all(), f"{what}: {int((got != want).sum())} of {got.size} words differ"


def _uniform(q, shape, rng):
    """Uniform residues [*shape][L] as little-endian limbs."""
    L = (q.bit_length() + 63) // 64
    n = int(np.prod(shape))
    if L == 1:
        return rng.integers(0, q, size=tuple(shape) + (1,), dtype=np.uint64)
    return co.to_limbs(rand_ints(q, n, rng), L).reshape(tuple(shape) + (L,))


# ---- bigpoly --------------------------------------------------------------
# p63 at 2^16 runs the lazy two-pass ntt16_pass kernels, here on hipMalloc'd memory
@pytest.mark.parametrize("key,logn,batch", [("p63", 12, 3), ("p63", 16, 2), ("jindo_zp", 8, 2)])
def test_bigpoly_sequence_from_c(key, logn, batch, fields, tmp_path):
    q, N = fields[key], 1 << logn
    cf = co.CField(q)
    L = cf.L
    rng = np.random.default_rng(N + batch)
    tw, twi, ninv = cf.tables(N)
    a, b = _uniform(q, (batch, N), rng), _uniform(q, (batch, N), rng)
    x = _uniform(q, (1,), rng)[0]
    n_vanish, aut_idx, eval_n = N // 4, 2 * N - 3, N - 5  # an odd prefix of each polynomial: stride N > n
    d = Dir(str(tmp_path))
    d.params(limbs=L, rank=N, negacyclic=1, batch=batch, eval_n=eval_n, stride=N, n_vanish=n_vanish, aut_idx=aut_idx)
    d.put("q", co.to_limbs([q], L))
    for name, arr in (("tw", tw), ("tw_inv", twi), ("rank_inv", ninv), ("a", a), ("b", b), ("x", x)):
        d.put(name, arr)
    d.run("bigpoly")

    qinv, r2, one = cf.consts()
    _same(d.get("consts", (1 + 2 * L,)), np.concatenate([[np.uint64(qinv)], co.to_limbs([r2, one], L).reshape(-1)]),
          "rg_field_constants")
    _same(d.get("info", (2,)), np.array([L, N], np.uint64), "rg_field_limbs / rg_ntt_rank")
    _same(d.get("tw_out", (N, L)), tw, "rg_ntt_tables tw")
    _same(d.get("tw_inv_out", (N, L)), twi, "rg_ntt_tables tw_inv")
    _same(d.get("rank_inv_out", (L,)), ninv, "rg_ntt_tables rank_inv")
    fwd = cf.ntt_fwd(a, tw)
    _same(d.get("fwd", a.shape), fwd, "rg_ntt_fwd")
    _same(d.get("inv", a.shape), a, "rg_ntt_inv")
    flat = lambda z: np.ascontiguousarray(z).reshape(-1, L)  # noqa: E731
    mul = cf.vec("mul", np.zeros_like(flat(a)), flat(a), flat(b)).reshape(a.shape)
    _same(d.get("mul", a.shape), mul, "rg_vec MUL")
    quo, rem = cf.quorem_vanishing(a[0], n_vanish)
    _same(d.get("quo", (N, L)), quo, "rg_poly_quorem_vanishing quo")
    _same(d.get("rem", (N, L)), rem, "rg_poly_quorem_vanishing rem")
    _same(d.get("aut", (N, L)), cf.aut(a[0], aut_idx, False), "rg_poly_aut")
    _same(d.get("eval", (L,)), cf.evaluate(a[0], x), "rg_poly_evaluate")
    # the device forms on rg_malloc'd buffers
    _same(d.get("fwd_dev", a.shape), fwd, "rg_ntt_fwd_dev")
    mul_dev = cf.vec("mul", np.zeros_like(flat(a)), flat(fwd), flat(b)).reshape(a.shape)
    _same(d.get("mul_dev", a.shape), mul_dev, "rg_vec_dev MUL")
    _same(d.get("inv_dev", a.shape), cf.ntt_inv(mul_dev, twi, ninv), "rg_ntt_inv_dev in place")
    _same(d.get("eval_batch_dev", (batch, L)), np.stack([cf.evaluate(a[i, :eval_n], x) for i in range(batch)]),
          "rg_poly_evaluate_batch_dev")


# ---- jindo ----------------------------------------------------------------
def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _verify_fields(raw, L):
    r = jindo.VerifyResultC.from_buffer_copy(raw)
    word = lambda w: sum(int(x) << (64 * i) for i, x in enumerate(w))  # noqa: E731
    return dict(outer_sq=word(r.outer_norm_sq), inner_sq=word(r.inner_norm_sq),
                flags=[r.outer_ok, r.inner_ok, r.consistency_ok, r.eval_ok],
                eval_lhs=np.array(r.eval_lhs[:L], np.uint64), eval_rhs=np.array(r.eval_rhs[:L], np.uint64), ok=r.ok)


def _same_verdict(got, want, what):
    """Field by field: both norm sums, the four flags (C ints 0 / 1), both sides of the evaluation check, ok."""
    assert got["outer_sq"] == want["outer_sq"] and got["inner_sq"] == want["inner_sq"], what
    assert got["flags"] == [int(f) for f in want["flags"]], (what, got["flags"], want["flags"])
    _same(got["eval_lhs"], want["eval_lhs"], what + " eval_lhs")
    _same(got["eval_rhs"], want["eval_rhs"], what + " eval_rhs")
    assert got["ok"] == int(want["ok"]), what


@pytest.mark.parametrize("name", ["t10_b1", "p63_t10_b2"])
def test_jindo_sequence_from_c(name, tmp_path):
    P = PARAMS[name]
    fq = int(P["field_q_hex"], 16)
    cj, F = co.CJindo(P, fq), co.CField(fq)
    L, B, nv, dd = F.L, P["batch"], P["rank"], P["d"]
    nq, nqo, cols, rows, slots = len(P["q"]), len(P["qo"]), P["cols"], P["rows"], P["slots"]
    nm, c1 = P["in_msis"] + P["mlwe"], P["cols"] + 1
    rng = np.random.default_rng(len(name))
    sd, delta = [P[k] for k in SD_KEYS], pyref.delta_inv(P["base"], P["exp"])
    d = Dir(str(tmp_path))
    # host commits: the cases of jindo_commit_golden.json (nv = 1, 300, rank), randomness injected
    cases = [(n, make_v(fq, n, seed=n), make_randomness(P, fq, seed=n + 1)) for n in (1, 300, P["rank"])]
    kv = {}
    for i, (n, v, rnd) in enumerate(cases):
        kv[f"case_nv_{i}"] = n
        d.put(f"case_v_{i}", v)
        for k in ("last_row", "mask", "enc_noise", "mlwe_noise"):
            d.put(f"case_{k}_{i}", rnd[k])
    # the device batch: honest randomness (the oracle's samplers at the parameters' widths), so Verify accepts
    v = np.stack([make_v(fq, nv, seed=700 + b) for b in range(B)])
    rnd = cj.sample(sd, delta, rng.bytes(192), 0, v)
    d.put("v", v)
    for k in ("last_row", "mask", "enc_noise", "mlwe_noise"):
        d.put(k, rnd[k])
    x = mont(F, int.from_bytes(rng.bytes(40), "little"))
    xl = co.to_limbs([x], L)[0]
    bbytes, cbytes = [rng.bytes(16) for _ in range(B)], [rng.bytes(16) for _ in range(cols)]
    seeds, first = rng.bytes(192), 7
    d.put("x", xl)
    d.put_bytes("bbytes", b"".join(bbytes))
    d.put_bytes("cbytes", b"".join(cbytes))
    d.put_bytes("seeds", seeds)
    kv.update(rank=P["rank"], rows=rows, cols=cols, slots=slots, exp=P["exp"], d=dd, in_msis=P["in_msis"],
              out_msis=P["out_msis"], mlwe=P["mlwe"], dcmp=P["in_com_dcmp_len"], log_in_cut=P["log_in_cut"],
              log_out_cut=P["log_out_cut"], base=P["base"], nq=nq, nqo=nqo, field_limbs=L, ncases=len(cases), batch=B,
              nv=nv, first_commit=first, in_com_dcmp_two_nm=float(P["in_com_dcmp_two_nm"]),
              res_two_nm=float(P["res_two_nm"]))
    kv.update({f"q_{i}": p for i, p in enumerate(P["q"])})
    kv.update({f"qo_{i}": p for i, p in enumerate(P["qo"])})
    kv.update({f"field_q_{i}": (fq >> (64 * i)) & (2 ** 64 - 1) for i in range(L)})
    kv.update({k: float(P[k]) for k in SD_KEYS})
    d.params(**kv)
    d.run("jindo")

    # 1. the commit key derived from the CRS, and the handle's kernel choice
    ck = (d.get("ck_in", (P["in_msis"], rows, nq, dd)), d.get("ck_mlwe", (P["in_msis"], P["mlwe"], nq, dd)),
          d.get("ck_out", (P["out_msis"], P["in_com_dcmp_len"], nqo, dd)))
    want_ck = pyref.commit_key(pyref.JindoParams(fq, P["target_n"], P["batch"]), b"Jindo!")
    for got, w, what in zip(ck, want_ck, ("ck_in", "ck_mlwe", "ck_out")):
        _same(got, np.array(w, np.uint64).reshape(got.shape), what)
    if name == "t10_b1":
        assert [_sha(k) for k in ck] == GOLD["ck"]
    params = jindo.Parameters.from_dict(P, fq)
    kinds = {v_: k for k, v_ in jindo.Prover.MAC_KINDS.items()}
    assert [int(k) for k in d.get("mac_kinds", (2,), np.int32)] == \
        [kinds[k] for k in jindo.NewProver(params, b"Jindo!").mac_kinds()]
    # 2. rg_jindo_commit
    sh = dict(incom=(P["in_com_dcmp_len"], nqo, dd), enc=(c1, rows, nq, dd), mlwe=(c1, nm, nq, dd),
              com=(P["out_msis"], nq, dd))
    for i, (n, cv, crnd) in enumerate(cases):
        want = cj.commit(ck[0], ck[1], ck[2], cv, crnd["last_row"], crnd["mask"], crnd["enc_noise"], crnd["mlwe_noise"])
        for k in sh:
            got = d.get(f"case_{k}_{i}", sh[k])
            _same(got, want[k], f"rg_jindo_commit nv={n} {k}")
            if name == "t10_b1":
                assert _sha(got) == GOLD["cases"][str(n)][k], (n, k)
    # 3. rg_jindo_commit_dev, then Evaluate's inputs and device work
    opens = [cj.commit(ck[0], ck[1], ck[2], v[b], rnd["last_row"][b], rnd["mask"][b], rnd["enc_noise"][b],
                       rnd["mlwe_noise"][b]) for b in range(B)]
    o = {k: np.stack([op[k] for op in opens]) for k in sh}
    for k in sh:
        _same(d.get(k, (B,) + sh[k]), o[k], f"rg_jindo_commit_dev {k}")
    if B > 1:
        bq = np.stack([cj.encode_challenge(0, b) for b in bbytes])
        bo = np.stack([cj.encode_challenge(1, b) for b in bbytes])
        _same(d.get("bq", bq.shape), bq, "rg_jindo_encode_challenges_dev ringQ")
        _same(d.get("bo", bo.shape), bo, "rg_jindo_encode_challenges_dev ringQOut")
    else:
        bq = bo = None
    chals = np.stack([cj.encode_challenge(0, b) for b in cbytes])
    _same(d.get("chals", chals.shape), chals, "rg_jindo_encode_challenges_dev columns")
    left_e, right_e = left_right(P, F, x)
    left = np.stack([cj.encode(co.to_limbs([a], L)) for a in left_e])
    right = co.to_limbs(right_e, L)
    _same(d.get("left", left.shape), left, "rg_jindo_eval_point_dev left")
    _same(d.get("right", right.shape), right, "rg_jindo_eval_point_dev right")
    _same(d.get("left_only", left.shape), left, "rg_jindo_eval_point_dev left, d_right = NULL")
    y = np.stack([F.evaluate(v[b], xl) for b in range(B)])
    _same(d.get("y", y.shape), y, "rg_poly_evaluate_batch_dev")
    ob = cj.eval_batch(o["incom"], o["enc"], o["mlwe"], bq if B > 1 else np.zeros((1, nq, dd), np.uint64),
                       bo if B > 1 else np.zeros((1, nqo, dd), np.uint64))
    for k in ("ob_incom", "ob_enc", "ob_mlwe"):
        _same(d.get(k, ob[k].shape), ob[k], "rg_jindo_eval_batch_dev " + k)
    partial = cj.eval_partial(ob["ob_enc"], left)
    _same(d.get("partial", partial.shape), partial, "rg_jindo_eval_partial_dev")
    pe, pm = cj.eval_respond(ob["ob_enc"], ob["ob_mlwe"], chals)
    _same(d.get("pf_enc", pe.shape), pe, "rg_jindo_eval_respond_dev enc")
    _same(d.get("pf_mlwe", pm.shape), pm, "rg_jindo_eval_respond_dev mlwe")
    # Verify, and Verify with one word of y changed
    pr = dict(com=o["com"], bq=bq, bo=bo, chals=chals, left=left, right=right, y=y, pf_incom=ob["ob_incom"],
              pf_partial=partial, pf_enc=pe, pf_mlwe=pm)
    verify = lambda p: cj.verify(ck, B, *[p[k] for k in VERIFY_KEYS], P["in_com_dcmp_two_nm"], P["res_two_nm"])  # noqa: E731
    want = verify(pr)
    assert want["ok"] and want["flags"] == [True] * 4  # an honest proof
    good = _verify_fields(d.raw("verify"), L)
    _same_verdict(good, want, "rg_jindo_verify_dev")
    bad_y = y.copy()
    bad_y.reshape(-1)[(B - 1) * L] ^= np.uint64(1)
    bad = _verify_fields(d.raw("verify_bad_y"), L)
    _same_verdict(bad, verify(dict(pr, y=bad_y)), "rg_jindo_verify_dev, y changed")
    assert bad["flags"] == [1, 1, 1, 0] and bad["ok"] == 0  # only eval_ok and ok turn false
    assert (bad["outer_sq"], bad["inner_sq"]) == (good["outer_sq"], good["inner_sq"])
    # 4. the device samplers: rg_jindo_seeds filled in C, first_commit = 7
    assert d.raw("delta_inv") == np.array(delta, np.float64).tobytes()
    srnd = cj.sample(sd, delta, seeds, first, v)
    for b in range(B):
        want = cj.commit(ck[0], ck[1], ck[2], v[b], srnd["last_row"][b], srnd["mask"][b], srnd["enc_noise"][b],
                         srnd["mlwe_noise"][b])
        for k in sh:
            _same(d.get("sampled_" + k, (B,) + sh[k])[b], want[k], f"rg_jindo_commit_sampled_dev {k}[{b}]")


# ---- buckler --------------------------------------------------------------
DCMP_BOUND = 1 << 20


def test_buckler_sequence_from_c(fields, tmp_path):
    q, rank, emb = fields["p63"], 128, 512
    jindo_rank = 8 * rank
    ref = R.Ref(q)
    L = ref.L
    circ = completeness_circuit(ref, rank, emb, seed=rank, two_pairs=True)
    rbase = R.decomposeBase(RECOMPOSE_BOUND)
    off, pairs = [0], []
    for ps in circ["constraints"]:
        pairs += [[wo, wi] for wo, wi in ps]
        off.append(len(pairs))
    n_w = len(circ["w"])
    # the decomposition: two witnesses of centred values within the bound, its edges included
    rng = np.random.default_rng(rank)
    dbase = D.decomposeBase(DCMP_BOUND)
    plain = rng.integers(-DCMP_BOUND, DCMP_BOUND + 1, size=(2, rank))
    plain[0, :4] = [0, DCMP_BOUND, -DCMP_BOUND, 1]
    dw = [[D.set_int64(ref, int(p)) for p in row] for row in plain]
    blind = rand_ints(q, 2 * len(dbase), rng)
    d = Dir(str(tmp_path))
    d.params(limbs=L, rank=rank, emb=emb, jindo_rank=jindo_rank, n_w=n_w, recompose_nb=len(rbase), n_pairs=len(pairs),
             aut_idx=5, dcmp_nb=len(dbase), dcmp_batch=2)
    d.put("q", co.to_limbs([q], L))
    d.put("recompose_base", ref.arr([ref.set_uint64(b) for b in rbase]))  # Montgomery elements
    d.put_bytes("xof", circ["xof"])
    d.put("pair_off", np.array(off, np.uint64))
    d.put("pairs", np.array(pairs, np.uint64))
    d.put("rand", ref.arr(circ["rand"]))
    d.put("bc", ref.arr([circ["bc"]]))
    d.put("lc", ref.arr([circ["lc"]]))
    d.put("w", np.stack([ref.arr(p) for p in circ["wEcdNTT"]]))
    d.put("dcmp_base", co.to_limbs(dbase, L))  # plain integers
    d.put("dcmp_w", np.stack([ref.arr(w) for w in dw]))
    d.put("blind", ref.arr(blind))
    d.run("buckler")

    mask, mask_sum = R.sumCheckMask(ref, rank, 2 * rank, emb, circ["rand"])
    _same(d.get("mask", (emb, L)), ref.arr(mask), "rg_buckler_sumcheck_mask_dev mask")
    _same(d.get("mask_sum", (1, L)), ref.arr([mask_sum]), "rg_buckler_sumcheck_mask_dev sum")
    quo, lo, hi, rem = R.linCheck(ref, rank, emb, jindo_rank, circ["bc"], circ["lc"], mask, circ["checkers"],
                                  circ["constraints"], circ["wEcdNTT"])
    _same(d.get("quo", (rank, L)), ref.arr(quo), "rg_buckler_lin_check_dev quo")
    _same(d.get("rem_lo", (rank - 1, L)), ref.arr(lo), "rg_buckler_lin_check_dev rem_lo")
    _same(d.get("rem_hi", (jindo_rank, L)), ref.arr(hi), "rg_buckler_lin_check_dev rem_hi")
    assert rem[0] == mask_sum
    _same(d.get("rem0", (1, L)), ref.arr([rem[0]]), "rem[0] at rg_buckler_lin_check_rem_offset_bytes")
    digits = [D.infDcmp(ref, w, dbase) for w in dw]  # [2][nb] witnesses of [rank]
    _same(d.get("digits", (2, len(dbase), rank, L)), np.stack([np.stack([ref.arr(j) for j in k]) for k in digits]),
          "rg_buckler_dcmp_inf_dev")
    flat = [j for k in digits for j in k]
    _same(d.get("ecd", (len(flat), emb, L)), np.stack([ref.arr(ref.rand_encode(w, emb, r)) for w, r in zip(flat, blind)]),
          "rg_buckler_encode_dev of the digits")
