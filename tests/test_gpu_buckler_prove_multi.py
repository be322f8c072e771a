"""GPU parity: the Buckler prover's batch entry (rg_buckler_prove_checks*; arithCheck, linCheck and
sumCheck of n_proofs proofs of one rg_bprover in one call), bit for bit against
tests/buckler_lin_ref.py per proof: all seven polynomials and rem0, into buffers pre-filled with -1
that carry one guard element past their end.  The proofs are tests/buckler_prove_util.proof: one
circuit, every per-proof input different."""
import numpy as np
import pytest

import ringo
from ringo import _lib, buckler
from tests import buckler_lin_ref as R
from tests import buckler_prove_util as U
from tests import synth_util as su

pytestmark = pytest.mark.gpu

NOSPARE = sorted(k for k, v in su.SYNTH.items() if v["bits"] == 64 * v["limbs"] and v["limbs"] in (1, 2, 4, 7, 14))
# one modulus without a spare top bit per supported limb count
NOSPARE_PER_L = [next(k for k in NOSPARE if su.SYNTH[k]["limbs"] == L) for L in
                 sorted({su.SYNTH[k]["limbs"] for k in NOSPARE})]
FIELDS = ["p63", "jindo_zp", "zp880"] + NOSPARE_PER_L
ALL = ("arith", "lin", "sum")
FF = np.uint64(2 ** 64 - 1)


def _dev(a, dtype=np.uint64):
    import torch
    a = np.ascontiguousarray(a, dtype)
    return torch.from_numpy(a.view(np.int64) if dtype == np.uint64 else a).cuda()


def _filled(n):
    import torch
    return torch.full((n,), -1, dtype=torch.int64, device="cuda")


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def _checkers(F, rank, spec, keep):
    out = []
    for i in keep:
        s = spec[i]
        out.append(buckler.NewNTTChecker(F, rank) if s[0] == "ntt" else
                   buckler.NewAutChecker(F, rank, s[1], s[2]) if s[0] == "aut" else
                   buckler.ProjChecker(F, rank) if s[0] == "proj" else  # its own matrix stays unset
                   buckler.ProjRecomposeChecker(F, rank, s[1]))
    return out


def _plan(key, rank, jindo_rank, arith_max, sum_max, has=ALL, keep=(0, 1, 2, 3), n_pw=U.N_PW, cons=None):
    """The circuit's handle.  keep: the checkers of the linear check (2 is the projection checker);
    cons: (arith, sum) constraint lists in place of buckler_prove_util.circuits."""
    F, ref = U.ctx(key)
    p0 = U.proof(key, rank, 0)
    lin = None
    if "lin" in has:
        lin = buckler.LinCheckPlan(F, rank, 4 * rank, _checkers(F, rank, p0["circ"]["spec"], keep),
                                   [p0["circ"]["constraints"][i] for i in keep])
    arith, sumc = cons or U.circuits(F, ref)
    return buckler.ProvePlan(F, rank, 4 * rank, jindo_rank, U.N_W, n_pw, lin, arith if "arith" in has else None,
                             arith_max, sumc if "sum" in has else None, sum_max)


def _inputs(plan, ps):
    """The batch's device inputs in the call's order: w, pw, xof, chal, lin mask, sum mask."""
    w = _dev(np.stack([p["w"] for p in ps]))
    pw = _dev(np.stack([p["pw"] for p in ps])) if plan.nPw else None
    xof = _dev(np.frombuffer(b"".join(p["xof"] for p in ps), np.uint8).copy(), np.uint8) if plan.hasProj else None
    chal = _dev(np.stack([p["chal_arr"] for p in ps]))
    lm = _dev(np.stack([p["lin_mask_arr"] for p in ps])) if plan.lin is not None else None
    sm = _dev(np.stack([p["sum_mask_arr"] for p in ps])) if plan.sum is not None else None
    return [w, pw, xof, chal, lm, sm]


def _outputs(plan, n):
    """The eight output buffers, -1 everywhere, each with one guard element past its end; None for
    an absent check and for a quotient of no elements."""
    L = plan.field.L
    return [None if not k else _filled((n * k + 1) * L) for k in plan.out_elems()]


def _read(plan, n, outs):
    """Host copies [n][k][L] of the outputs; the guard element of each must have survived."""
    L = plan.field.L
    got = []
    for t, k in zip(outs, plan.out_elems()):
        if t is None:
            got.append(None)
            continue
        h = _host(t)
        assert (h[n * k * L:] == FF).all(), "guard element overwritten"
        got.append(h[:n * k * L].reshape(n, k, L))
    return got


def _run(plan, ps, stream=None, rem0=True):
    import torch
    n = len(ps)
    outs = _outputs(plan, n)
    if not rem0:
        outs[7] = None
    scr = torch.empty(max(1, plan.scratch_bytes(n) // 8), dtype=torch.int64, device="cuda")
    plan.checks_dev(n, *_inputs(plan, ps), *outs[:7], d_rem0=outs[7], d_scratch=scr, stream=stream)
    if stream is not None:
        stream.synchronize()
    return _read(plan, n, outs)


def _same(got, wants):
    """got: the outputs [n][k][L] (None: absent); wants: per proof, the eight arrays (None: not compared)."""
    for i, wp in enumerate(wants):
        for j, (g, x) in enumerate(zip(got, wp)):
            if x is None:
                continue
            if g is None:
                assert x.shape[0] == 0, (i, j)
                continue
            assert (g[i] == x).all(), (i, j)


def _want(key, rank, seed, jr, amax, smax, has=ALL, perturb=False):
    """U.want with the outputs of absent checks removed and their rem0 zeroed."""
    x = list(U.want(key, rank, seed, jr, amax, smax, perturb))
    rem0 = x[7].copy()
    if "arith" not in has:
        x[0] = None
    if "lin" not in has:
        x[1:4] = [None] * 3
        rem0[0] = 0
    if "sum" not in has:
        x[4:7] = [None] * 3
        rem0[1] = 0
    x[7] = rem0
    return x


# ---- parity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", FIELDS)
@pytest.mark.parametrize("rank", [128, 256])
@pytest.mark.parametrize("n_proofs", [1, 3, 5])
def test_parity(key, rank, n_proofs):
    """Rank 128 is one chunk of the projection's columns, 256 two; every proof has its own
    challenges, masks, witnesses and XOF bytes."""
    jr, amax, smax = 4 * rank, 3 * rank, 3 * rank
    plan = _plan(key, rank, jr, amax, smax)
    ps = [U.proof(key, rank, s) for s in range(n_proofs)]
    _same(_run(plan, ps), [_want(key, rank, s, jr, amax, smax) for s in range(n_proofs)])


@pytest.mark.parametrize("key", ["p63", "jindo_zp"])
@pytest.mark.parametrize("jr_of,amax_of,smax_of", [
    (lambda r: r - 1, lambda r: 2 * r - 1, lambda r: r),       # remHi without zeros; sum n_quo = 0, NULL output
    (lambda r: r + 173, lambda r: 2 * r - 1, lambda r: 3 * r),
    (lambda r: r - 1, lambda r: 3 * r, lambda r: 3 * r),
])
def test_tail_extents_that_are_no_multiple_of_a_workgroup(key, jr_of, amax_of, smax_of):
    rank, n = 128, 3
    jr, amax, smax = jr_of(rank), amax_of(rank), smax_of(rank)
    plan = _plan(key, rank, jr, amax, smax)
    assert plan.out_elems()[4] == smax - rank
    got = _run(plan, [U.proof(key, rank, s) for s in range(n)])
    assert (got[4] is None) == (smax == rank)
    _same(got, [_want(key, rank, s, jr, amax, smax) for s in range(n)])


# ---- equal to the single entries -------------------------------------------------------------------
@pytest.mark.parametrize("key", ["p63", "jindo_zp", "zp880"])
def test_equal_to_the_single_entries_bit_for_bit(key):
    """Proof p of a batch of 3 against rg_buckler_lin_check_dev with the checker set to proof p's XOF
    bytes, and against rg_buckler_eval_circuit_dev + rg_buckler_check_finish_dev."""
    import torch
    rank, emb, n = 128, 512, 3
    jr, amax, smax = 4 * rank, 3 * rank, 2 * rank + 5
    F, ref = U.ctx(key)
    L = F.L
    plan = _plan(key, rank, jr, amax, smax)
    ps = [U.proof(key, rank, s) for s in range(n)]
    got = _run(plan, ps)
    spec = ps[0]["circ"]["spec"]
    chks = _checkers(F, rank, spec, (0, 1, 2, 3))
    lin = buckler.LinCheckPlan(F, rank, emb, chks, ps[0]["circ"]["constraints"])
    arith, sumc = (buckler.Circuit(F, c) for c in U.circuits(F, ref))
    embT = ringo.NewCyclicTransformer(F, emb)
    new = lambda k: torch.full((k * L,), -1, dtype=torch.int64, device="cuda")  # noqa: E731
    for i, p in enumerate(ps):
        chks[2].SetXOF(p["xof"])
        dw, dpw, dch = _dev(p["w"]), _dev(p["pw"]), _dev(p["chal_arr"])
        q, lo, hi = new(rank), new(rank - 1), new(jr)
        scr = torch.empty(lin.scratch_bytes() // 8, dtype=torch.int64, device="cuda")
        lin.lin_check_dev(dch[1], dch[2], _dev(p["lin_mask_arr"]), dw, U.N_W, jr, q, lo, hi, scr)
        o = lin.rem_offset_words()
        rem0_lin = _host(scr)[o:o + L]
        for j, t in ((1, q), (2, lo), (3, hi)):
            assert (_host(t).reshape(-1, L) == got[j][i]).all(), (i, j)
        assert (rem0_lin == got[7][i, 0]).all()
        fscr = torch.empty(buckler.check_finish_scratch_bytes(embT) // 8, dtype=torch.int64, device="cuda")
        ev = new(emb)
        sumc.eval_dev(emb, dch[3], dw, U.N_W, dpw, U.N_PW, ev)
        q, lo, hi = new(smax - rank), new(rank - 1), new(jr)
        buckler.check_finish_dev(embT, rank, ev, dch[3], _dev(p["sum_mask_arr"]), smax - rank, jr, q, lo, hi, fscr)
        for j, t in ((4, q), (5, lo), (6, hi)):
            assert (_host(t).reshape(-1, L) == got[j][i]).all(), (i, j)
        assert (_host(ev)[:L] == got[7][i, 1]).all()  # remPoly stands over eval
        arith.eval_dev(emb, dch[0], dw, U.N_W, dpw, U.N_PW, ev)
        q = new(amax - rank)
        buckler.check_finish_dev(embT, rank, ev, None, None, amax - rank, 0, q, None, None, fscr)
        assert (_host(q).reshape(-1, L) == got[0][i]).all(), i


# ---- independence ----------------------------------------------------------------------------------
def test_a_perturbed_proof_in_the_middle():
    """completeness_circuit proofs: lin's rem0 is the proof's mask sum exactly for the honest proofs;
    for the perturbed one (wOut != M wIn) it is not, and its neighbours are untouched."""
    key, rank = "jindo_zp", 128
    jr, amax, smax = 4 * rank, 3 * rank, 3 * rank
    _, ref = U.ctx(key)
    plan = _plan(key, rank, jr, amax, smax)
    ps = [U.proof(key, rank, 0), U.proof(key, rank, 1, True), U.proof(key, rank, 2)]
    got = _run(plan, ps)
    _same(got, [_want(key, rank, 0, jr, amax, smax), _want(key, rank, 1, jr, amax, smax, perturb=True),
                _want(key, rank, 2, jr, amax, smax)])
    sums = [ref.arr([p["lin_mask_sum"]])[0] for p in ps]
    assert (got[7][0, 0] == sums[0]).all() and (got[7][2, 0] == sums[2]).all()
    assert (got[7][1, 0] != sums[1]).any()


def test_permuting_the_batch_permutes_the_outputs():
    key, rank = "p63", 128
    jr, amax, smax = rank + 173, 2 * rank - 1, 3 * rank
    plan = _plan(key, rank, jr, amax, smax)
    ps = [U.proof(key, rank, s) for s in range(4)]
    perm = [2, 0, 3, 1]
    a, b = _run(plan, ps), _run(plan, [ps[i] for i in perm])
    for x, y in zip(a, b):
        assert (x[perm] == y).all()


def test_swapping_two_proofs_xof_bytes_changes_exactly_their_lin_outputs():
    key, rank = "jindo_zp", 256
    jr, amax, smax = 4 * rank, 3 * rank, 3 * rank
    plan = _plan(key, rank, jr, amax, smax)
    ps = [U.proof(key, rank, s) for s in range(4)]
    sw = [dict(p) for p in ps]
    sw[1]["xof"], sw[3]["xof"] = ps[3]["xof"], ps[1]["xof"]
    a, b = _run(plan, ps), _run(plan, sw)
    for j in range(8):
        for i in range(4):
            same = (a[j][i] == b[j][i]).all()
            if j in (1, 2, 3) and i in (1, 3):
                assert not same, (j, i)
            elif j == 7:
                assert (a[j][i, 1] == b[j][i, 1]).all() and ((a[j][i, 0] == b[j][i, 0]).all() == (i not in (1, 3)))
            else:
                assert same, (j, i)


# ---- handles with fewer checks ---------------------------------------------------------------------
@pytest.mark.parametrize("has", [("lin",), ("arith",), ("sum",), ("arith", "sum")])
def test_handles_with_fewer_checks(has):
    key, rank, n = "jindo_zp", 128, 3
    jr, amax, smax = 4 * rank, 3 * rank, 3 * rank
    plan = _plan(key, rank, jr, amax, smax, has=has)
    got = _run(plan, [U.proof(key, rank, s) for s in range(n)])
    for j, name in ((0, "arith"), (1, "lin"), (4, "sum")):
        assert (got[j] is None) == (name not in has)
    _same(got, [_want(key, rank, s, jr, amax, smax, has=has) for s in range(n)])


def test_lin_without_a_projection_checker_and_no_public_witnesses():
    """d_xof and d_pw are NULL: the linear check keeps its NTT, automorphism and recompose checkers,
    and the circuits have no public-witness coefficient."""
    key, rank, n = "p63", 128, 3
    emb, jr, amax, smax = 4 * rank, 4 * rank, 2 * rank + 1, 2 * rank + 1
    F, ref = U.ctx(key)
    keep = (0, 1, 3)
    a0 = buckler.ArithmeticConstraint(F)
    a0.AddTerm(None, 0, 1)
    a0.SubTerm(None, 7)
    s0 = buckler.ArithmeticConstraint(F)
    s0.AddTerm(None, 4, 5)
    plan = _plan(key, rank, jr, amax, smax, keep=keep, n_pw=0, cons=([a0], [s0]))
    assert not plan.hasProj
    ps = [U.proof(key, rank, s) for s in range(n)]
    got = _run(plan, ps)
    wants = []
    for p in ps:
        c = p["circ"]
        ev = R.linCheckEval(ref, rank, emb, p["chal"][1], p["chal"][2], [c["checkers"][i] for i in keep],
                            [c["constraints"][i] for i in keep], c["wEcdNTT"])
        lq, llo, lhi, lrem = R.checkTail(ref, ev, rank, p["chal"][1], p["lin_mask"], rank, jr)
        ea = ref.ints(ref.cf.buckler_eval_circuit(U.oracle_cons([a0]), p["chal_arr"][0], p["w"], None))
        es = ref.ints(ref.cf.buckler_eval_circuit(U.oracle_cons([s0]), p["chal_arr"][3], p["w"], None))
        aq = R.arithCheck(ref, rank, amax, ea)
        sq, slo, shi, srem = R.checkTail(ref, es, rank, p["chal"][3], p["sum_mask"], smax - rank, jr)
        wants.append([ref.arr(x) for x in (aq, lq, llo, lhi, sq, slo, shi, [lrem[0], srem[0]])])
    _same(got, wants)


# ---- host form, mirror, streams ----------------------------------------------------------------------
def test_host_form_and_mirror_agree_with_the_dev_form():
    key, rank, n = "jindo_zp", 128, 3
    jr, amax, smax = rank + 173, 2 * rank - 1, 3 * rank
    F, ref = U.ctx(key)
    plan = _plan(key, rank, jr, amax, smax)
    ps = [U.proof(key, rank, s) for s in range(n)]
    dev = _run(plan, ps)
    w, pw = np.stack([p["w"] for p in ps]), np.stack([p["pw"] for p in ps])
    xof = b"".join(p["xof"] for p in ps)
    chal = np.stack([p["chal_arr"] for p in ps])
    lm, sm = np.stack([p["lin_mask_arr"] for p in ps]), np.stack([p["sum_mask_arr"] for p in ps])
    host = plan.checks(w, pw, xof, chal, lm, sm)
    for a, b in zip(dev, host):
        assert a.shape == b.shape and (a == b).all()
    arith, sumc = U.circuits(F, ref)
    c = ps[0]["circ"]
    res = buckler.ProveChecks(F, rank, 4 * rank, jr, chal, lm, sm, _checkers(F, rank, c["spec"], (0, 1, 2, 3)),
                              c["constraints"], arith, amax, sumc, smax, w, pw, xof=xof)
    assert len(res) == n
    for i, (aq, lin, sum_, rem0) in enumerate(res):
        assert (aq == dev[0][i]).all()
        assert all((x == dev[1 + j][i]).all() for j, x in enumerate(lin))
        assert all((x == dev[4 + j][i]).all() for j, x in enumerate(sum_))
        assert (rem0[0] == dev[7][i, 0]).all() and (rem0[1] == dev[7][i, 1]).all()


def test_two_streams_share_one_handle():
    """Two calls in flight on two streams with one rg_bprover (own scratch and outputs each)."""
    import torch
    key, rank = "jindo_zp", 128
    jr, amax, smax = 4 * rank, 3 * rank, 3 * rank
    plan = _plan(key, rank, jr, amax, smax)
    batches = [[U.proof(key, rank, s) for s in (0, 1, 2)], [U.proof(key, rank, s) for s in (3, 4)]]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    state = []
    for ps, st in zip(batches, streams):
        n = len(ps)
        outs = _outputs(plan, n)
        scr = torch.empty(plan.scratch_bytes(n) // 8, dtype=torch.int64, device="cuda")
        state.append((n, outs, scr, _inputs(plan, ps)))
    torch.cuda.synchronize()
    for (n, outs, scr, ins), st in zip(state, streams):
        plan.checks_dev(n, *ins, *outs[:7], d_rem0=outs[7], d_scratch=scr, stream=st)
    for st in streams:
        st.synchronize()
    for (n, outs, _, _), seeds in zip(state, ((0, 1, 2), (3, 4))):
        _same(_read(plan, n, outs), [_want(key, rank, s, jr, amax, smax) for s in seeds])


def test_zero_proofs_and_no_rem0():
    key, rank = "p63", 128
    jr, amax, smax = 4 * rank, 3 * rank, 3 * rank
    plan = _plan(key, rank, jr, amax, smax)
    L = _lib.lib()
    assert L.rg_buckler_prove_checks_dev(plan.h, 0, *([None] * 16)) == 0
    assert plan.scratch_bytes(0) == 0
    got = _run(plan, [U.proof(key, rank, 0)], rem0=False)
    assert got[7] is None
    _same(got[:7], [_want(key, rank, 0, jr, amax, smax)[:7]])


# ---- argument errors ---------------------------------------------------------------------------------
def _why():
    return _lib.lib().rg_last_error().decode()


def test_create_refusals_with_live_plans():
    """rg_buckler_prover_create's RG_ERR_INVALID cases, which need NTT plans to reach (a plan uploads
    its tables when it is created, so these cannot run without a GPU)."""
    import ctypes
    F, ref = U.ctx("p63")
    F2 = ringo.Field(su.modulus("jindo_zp"))
    rank, emb = 128, 512
    L = _lib.lib()
    enc, embT = ringo.NewCyclicTransformer(F, rank), ringo.NewCyclicTransformer(F, emb)
    neg, neg_enc = ringo.NewCyclotomicTransformer(F, emb), ringo.NewCyclotomicTransformer(F, rank)
    arith_c, sum_c = U.circuits(F, ref)
    arith, sumc = buckler.Circuit(F, arith_c), buckler.Circuit(F, sum_c)
    lin = buckler.LinCheckPlan(F, rank, emb, [buckler.NewNTTChecker(F, rank)], [[(0, 1)]])
    lin_other = buckler.LinCheckPlan(F, rank, 2 * emb, [buckler.NewNTTChecker(F, rank)], [[(0, 1)]])
    c2 = buckler.ArithmeticConstraint(F2)
    c2.AddTerm(None, 0)
    other_field = buckler.Circuit(F2, [c2])
    h = ctypes.c_void_p()

    def create(enc_=enc.h, emb_=embT.h, jr=4 * rank, n_w=8, n_pw=2, lin_=lin.h, arith_=arith.h, amax=3 * rank,
               sum_=sumc.h, smax=3 * rank):
        return L.rg_buckler_prover_create(enc_, emb_, jr, n_w, n_pw, lin_, arith_, amax, sum_, smax, ctypes.byref(h))

    cases = [(dict(lin_=None, arith_=None, sum_=None), "all NULL"), (dict(emb_=neg.h), "cyclic"),
             (dict(enc_=neg_enc.h), "cyclic"), (dict(lin_=lin_other.h), "differ"),
             (dict(arith_=other_field.h), "another field"), (dict(n_w=7), ">= n_w"), (dict(n_w=1), ">= n_w"),
             (dict(n_pw=1), ">= n_pw"), (dict(jr=rank - 2), "jindo_rank"), (dict(amax=rank - 1), "arith_max_rank"),
             (dict(amax=emb + 1), "arith_max_rank"), (dict(smax=rank - 1), "sum_max_rank"),
             (dict(smax=emb + 1), "sum_max_rank"), (dict(enc_=None), "NULL")]
    for kw, why in cases:
        assert create(**kw) == -1 and why in _why() and not h.value, kw
    assert create(arith_=None, amax=0, sum_=None, smax=emb + 9) == 0 and h.value  # an absent check's max_rank is not read
    L.rg_buckler_prover_destroy(h)
    assert create(jr=rank - 1, amax=rank, smax=emb) == 0
    L.rg_buckler_prover_destroy(h)
    # RG_ERR_UNSUPPORTED needs plans of a limb count without kernels; where the NTT builds none, the
    # case cannot be reached through the interface
    G = ringo.Field((1 << 130) + 5 | 1, limbs=3)
    try:
        g_enc, g_emb = ringo.NewCyclicTransformer(G, rank), ringo.NewCyclicTransformer(G, emb)
    except Exception:
        g_enc = None
    if g_enc is not None:
        assert create(enc_=g_enc.h, emb_=g_emb.h, lin_=None, sum_=None) == -3 and "3 limbs" in _why()


def test_argument_errors_with_live_plans():
    """Each is RG_ERR_INVALID before the device is touched: the outputs stay -1 (the addresses of the
    refused calls are real buffers, so a call that went through would have written them)."""
    key, rank, n = "p63", 128, 2
    jr, amax, smax = 4 * rank, 3 * rank, 3 * rank
    plan = _plan(key, rank, jr, amax, smax)
    L = _lib.lib()
    import torch
    ps = [U.proof(key, rank, s) for s in range(n)]
    ins = _inputs(plan, ps)
    outs = _outputs(plan, n)
    scr = torch.empty(plan.scratch_bytes(n) // 8, dtype=torch.int64, device="cuda")
    good = [t.data_ptr() for t in ins] + [t.data_ptr() for t in outs] + [scr.data_ptr()]
    W, PW, XOF, CHAL, LM, SM, AQ, LQ, LLO, LHI, SQ, SLO, SHI, REM0, SCR = range(15)

    def call(over=None, n_=n, h=plan.h):
        a = list(good)
        for k, v in (over or {}).items():
            a[k] = v
        return L.rg_buckler_prove_checks_dev(h, n_, *a, None)

    assert call(h=None) == -1 and "NULL handle" in _why()
    assert call(n_=65536) == -1 and "n_proofs" in _why()
    assert plan.scratch_bytes(65536) == 0 and plan.scratch_bytes(1 << 40) == 0 and plan.scratch_bytes(n) > 0
    for idx in (W, PW, XOF, CHAL, LM, SM, AQ, LQ, LLO, LHI, SQ, SLO, SHI, SCR):  # every required buffer, NULL
        assert call({idx: None}) == -1 and _why().startswith("buckler prover:"), idx
    for i, j in ((W, PW), (CHAL, LM), (LM, SM), (AQ, LQ), (LLO, LHI), (SQ, SHI), (REM0, SLO), (SCR, LQ), (W, SCR)):
        assert call({i: good[j]}) == -1 and "alias" in _why(), (i, j)
    # the pointers of an absent check must be NULL, and d_xof / d_pw follow the handle
    lin_only = _plan(key, rank, jr, amax, smax, has=("lin",))
    absent = {AQ: None, SM: None, SQ: None, SLO: None, SHI: None}
    for idx in (AQ, SM, SQ, SLO, SHI):
        over = dict(absent)
        over[idx] = good[idx]
        assert call(over, h=lin_only.h) == -1 and "absent" in _why(), idx
    no_proj = _plan(key, rank, jr, amax, smax, keep=(0, 1, 3))
    assert call(h=no_proj.h) == -1 and "d_xof" in _why()
    F, ref = U.ctx(key)
    a0 = buckler.ArithmeticConstraint(F)
    a0.AddTerm(None, 0, 1)
    no_pw = _plan(key, rank, jr, amax, smax, n_pw=0, cons=([a0], [a0]))
    assert call(h=no_pw.h) == -1 and "d_pw" in _why()
    torch.cuda.synchronize()
    for t in outs:
        assert (_host(t) == FF).all()
    # and the same buffers, accepted, give the answer
    assert call() == 0
    _same(_read(plan, n, outs), [_want(key, rank, s, jr, amax, smax) for s in range(n)])
