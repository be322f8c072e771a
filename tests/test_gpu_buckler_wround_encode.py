"""GPU parity: RandEncode of one commit round's rows for a batch of proofs in one call
(rg_buckler_prove_encode_round*; prover.go:136-153, 195-201), bit for bit against the oracle's Encode
(coracle.CField.buckler_encode per proof and row), into an embedding-rank table whose selected rows are
pre-filled with -1 and whose other rows must come back unchanged.  A guard element sits behind every
buffer and the scratch is pre-filled with -1.  The refusals that need a live NTT plan are here too: a plan
uploads its tables when it is made."""
import ctypes

import numpy as np
import pytest

import ringo
from ringo import _lib, buckler
from ringo.bigpoly import RingoPanic
from tests import buckler_wround_util as U

pytestmark = pytest.mark.gpu

INVALID = -1
A, B, C, D, E = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000  # distinct fake device addresses


def _why():
    return _lib.lib().rg_last_error().decode()


@pytest.fixture(scope="module")
def F(fields):
    return ringo.Field(fields["p63"])


def _u64(xs):
    return (ctypes.c_uint64 * max(1, len(xs)))(*xs)


def _enc_create(plan, emb, n_w, sel, n_sel=None, null_sel=False, out=True):
    h = ctypes.c_void_p(1)
    st = _lib.lib().rg_buckler_encode_round_create(plan, emb, n_w, len(sel) if n_sel is None else n_sel,
                                                   None if null_sel else _u64(sel), ctypes.byref(h) if out else None)
    return st, h


@pytest.fixture(scope="module")
def plans():
    """One handle per (key, rank, emb, sel), shared among the tests of the module."""
    made = {}

    def get(key, rank, emb, sel_name):
        k = (key, rank, emb, sel_name)
        if k not in made:
            n_w, sel = U.SELS[sel_name]
            made[k] = buckler.EncodeRoundPlan(U.ctx(key)[0], rank, emb, n_w, sel)
        return made[k]

    return get


def _run(plan, w, rand, wecd, with_com, stream=None):
    """The call on device copies; returns (wecd, com or None) read back, the guards checked.  rand None:
    EncodeTo."""
    n, L, ns = w.shape[0], w.shape[-1], len(plan.sel)
    d_w, d_e = U.dev_guarded(w, L), U.dev_guarded(wecd, L)
    d_r = None if rand is None else U.dev_guarded(rand, L)
    d_c = U.filled(n * ns * (plan.rank + 1) * L, L) if with_com else None
    d_s = U.filled(plan.scratch_bytes(n) // 8, L)
    plan.round_dev(n, d_w, d_e, d_rand=d_r, d_com=d_c, d_scratch=d_s, stream=stream)
    if stream is not None:
        stream.synchronize()
    U.unguard(d_s, (plan.scratch_bytes(n) // 8,), L, "the scratch")
    assert (U.unguard(d_w, w.shape, L, "the plain table") == w).all(), "the plain table changed"
    if rand is not None:
        assert (U.unguard(d_r, rand.shape, L, "the draws") == rand).all()
    com = U.unguard(d_c, (n, ns, plan.rank + 1, L), L, "com") if with_com else None
    return U.unguard(d_e, wecd.shape, L, "the encoded table"), com


def _same(got, want, what):
    for k in range(want.shape[0]):
        for r in range(want.shape[1]):
            assert (got[k, r] == want[k, r]).all(), (what, "proof", k, "row", r)


# ---- parity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", U.FIELDS)
@pytest.mark.parametrize("rank", U.ENC_RANKS)
def test_parity(key, rank, plans):
    """Embedding ranks 2 rank and 4 rank, the three selections; 5 proofs with draws and com, 3 proofs
    without draws (EncodeTo), 1 proof with draws and no com."""
    for emb in (2 * rank, 4 * rank):
        for sel_name in U.SELS:
            plan = plans(key, rank, emb, sel_name)
            for idx, with_rand, with_com in ((U.BATCHES[2], True, True), (U.BATCHES[1], False, False),
                                             (U.BATCHES[0], True, False)):
                w, rand, wecd = U.enc_tables(key, rank, emb, sel_name, idx)
                got, com = _run(plan, w, rand if with_rand else None, wecd, with_com)
                want, want_com = U.enc_expect(key, rank, emb, sel_name, idx, wecd, with_rand)
                _same(got, want, (emb, sel_name, idx))
                if with_com:
                    assert (com == want_com).all(), (emb, sel_name, idx)


# ---- equal to the single entry -----------------------------------------------------------------------
@pytest.mark.parametrize("key", U.FIELDS[:5])
@pytest.mark.parametrize("rank,sel_name", [(64, "subset"), (1024, "identity")])
def test_equal_to_the_single_entry_bit_for_bit(key, rank, sel_name, plans):
    """Each proof of a batch of 5 against rg_buckler_encode_dev on its selected rows."""
    emb = 2 * rank
    F_, _ = U.ctx(key)
    L = F_.L
    plan = plans(key, rank, emb, sel_name)
    idx = tuple(range(U.N_PROOFS))
    w, rand, wecd = U.enc_tables(key, rank, emb, sel_name, idx)
    got, com = _run(plan, w, rand, wecd, True)
    enc = buckler.NewEncoder(F_, rank, emb)
    ns = len(plan.sel)
    for k in idx:
        rows = np.stack([w[k, r] for r in plan.sel])
        out, scr = U.filled(ns * emb * L, L), U.filled(max(1, enc.scratch_bytes(ns) // 8), L)
        enc.encode_dev(out, U.dev(rows), ns, d_rand=U.dev(rand[k]), d_scratch=scr)
        single = U.unguard(out, (ns, emb, L), L, "the single entry's output")
        for s, r in enumerate(plan.sel):
            assert (single[s] == got[k, r]).all(), (k, r)
            assert (single[s, :rank + 1] == com[k, s]).all(), (k, r)


# ---- independence ----------------------------------------------------------------------------------
def test_permuting_the_batch_permutes_the_outputs(plans):
    key, rank, emb, sel_name = "jindo_zp", 128, 256, "subset"
    idx, perm = (0, 1, 2, 3, 4), [3, 0, 4, 2, 1]
    w, rand, wecd = U.enc_tables(key, rank, emb, sel_name, idx)
    plan = plans(key, rank, emb, sel_name)
    a, ca = _run(plan, w, rand, wecd, True)
    b, cb = _run(plan, w[perm], rand[perm], wecd[perm], True)
    assert (a[perm] == b).all() and (ca[perm] == cb).all()
    assert len({ca[k].tobytes() for k in range(5)}) == 5


def test_two_streams_with_one_handle_and_separate_scratch(plans):
    import torch
    key, rank, emb, sel_name = "jindo_zp", 1024, 2048, "subset"
    plan = plans(key, rank, emb, sel_name)
    L, ns = plan.field.L, len(plan.sel)
    batches = [(0, 1, 2), (3, 4)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    w0, r0, e0 = U.enc_tables(key, rank, emb, sel_name, (0,))
    _run(plan, w0, r0, e0, True)  # the handle's table is on the device before the two calls overlap
    state = []
    for idx in batches:
        w, rand, wecd = U.enc_tables(key, rank, emb, sel_name, idx)
        n = len(idx)
        state.append((wecd, U.dev(w), U.dev(rand), U.dev(wecd), U.filled(n * ns * (rank + 1) * L, L),
                      U.filled(plan.scratch_bytes(n) // 8, L)))
    torch.cuda.synchronize()
    for (wecd, d_w, d_r, d_e, d_c, d_s), st in zip(state, streams):
        plan.round_dev(wecd.shape[0], d_w, d_e, d_rand=d_r, d_com=d_c, d_scratch=d_s, stream=st)
    for st in streams:
        st.synchronize()
    for (wecd, _, _, d_e, d_c, _), idx in zip(state, batches):
        want, want_com = U.enc_expect(key, rank, emb, sel_name, idx, wecd, True)
        assert (U.host(d_e).reshape(wecd.shape) == want).all(), idx
        assert (U.unguard(d_c, want_com.shape, L, "com") == want_com).all(), idx


# ---- host form, mirror, nothing to do ----------------------------------------------------------------
@pytest.mark.parametrize("sel_name", ["subset", "identity"])
def test_host_form_and_mirror_agree_with_the_dev_form(sel_name, plans):
    key, rank, emb = "zp440", 64, 256
    plan = plans(key, rank, emb, sel_name)
    idx = (0, 3, 4)
    w, rand, wecd = U.enc_tables(key, rank, emb, sel_name, idx)
    dev, dev_com = _run(plan, w, rand, wecd, True)
    before = wecd.copy()
    host, host_com = plan.round(w, rand, wecd)
    assert (wecd == before).all()  # the mirror returns a copy
    want, want_com = U.enc_expect(key, rank, emb, sel_name, idx, wecd, True)
    assert (host == dev).all() and (host == want).all() and (host_com == dev_com).all() and (host_com == want_com).all()
    # EncodeTo: no draws, no com; a missing table starts as zeros
    host0, com0 = plan.round(w)
    want0, _ = U.enc_expect(key, rank, emb, sel_name, idx, np.zeros_like(wecd), False)
    assert com0 is None and (host0 == want0).all()


def test_zero_proofs_and_refused_calls_touch_nothing(plans):
    key, rank, emb, sel_name = "p63", 64, 128, "subset"
    plan = plans(key, rank, emb, sel_name)
    L = plan.field.L
    w, rand, wecd = U.enc_tables(key, rank, emb, sel_name, (0,))
    d_w, d_r, d_e = U.dev(w), U.dev(rand), U.dev(wecd)
    d_c, d_s = U.filled(2 * (rank + 1) * L, L), U.filled(plan.scratch_bytes(1) // 8, L)
    plan.round_dev(0, d_w, d_e, d_rand=d_r, d_com=d_c, d_scratch=d_s)
    lib = _lib.lib()
    assert lib.rg_buckler_prove_encode_round_dev(plan.h, 0, None, None, None, None, None, None) == 0
    assert plan.scratch_bytes(0) == 0
    pw, pr, pe, pc, ps = (t.data_ptr() for t in (d_w, d_r, d_e, d_c, d_s))
    # refused: com without draws, aliased buffers, a missing scratch, too many proofs
    for args in ((1, pw, None, pe, pc, ps), (1, pw, pr, pe, pe, ps), (1, pw, pr, pe, pc, pe), (1, pw, pr, pe, pc, None),
                 (65536, pw, pr, pe, pc, ps)):
        assert lib.rg_buckler_prove_encode_round_dev(plan.h, *args, None) == -1, args
    assert (U.host(d_e).reshape(wecd.shape) == wecd).all() and (U.host(d_w).reshape(w.shape) == w).all()
    assert (U.host(d_c) == U.FF).all() and (U.host(d_s) == U.FF).all()


# ---- the refusals that need a live plan ----------------------------------------------------------------
def test_scratch_bytes_of_a_live_handle(F):
    L = _lib.lib()
    T = ringo.bigpoly.NewCyclicTransformer(F, 128)
    scr = L.rg_buckler_prove_encode_round_scratch_bytes
    # n_proofs * n_sel * rank * L * 8, with or without the gather
    for n_w, sel in ((5, [3, 0]), (3, [0, 1, 2]), (4, [2]), (3, [2, 1, 0])):
        st, h = _enc_create(T.h, 256, n_w, sel)
        assert st == 0 and h.value, _why()
        assert scr(h, 1) == len(sel) * 128 * 8 and scr(h, 64) == 64 * len(sel) * 128 * 8
        L.rg_buckler_encode_round_destroy(h)
    L.rg_buckler_encode_round_destroy(None)


def test_create_refusals_with_a_live_plan(F):
    T = ringo.bigpoly.NewCyclicTransformer(F, 128)
    N = ringo.CyclotomicTransformer(F, 128)
    ok = dict(plan=T.h, emb=256, n_w=5, sel=[3, 0])

    def refused(why, **kw):
        st, h = _enc_create(**{**ok, **kw})
        assert st == INVALID and h.value is None, kw
        assert _why().startswith("buckler encode round:") and why in _why(), (kw, _why())

    refused("NULL plan", plan=None)
    refused("negacyclic", plan=N.h)
    for emb in (0, 64, 128, 129, 192, 384, 1 << 31):  # a power of two above the rank
        refused("embedding rank", emb=emb)
    refused("n_w", n_w=0)
    refused("n_sel", sel=[])
    refused("n_sel", sel=[0], n_sel=65536, n_w=1 << 20)
    refused("NULL sel", null_sel=True)
    refused(">= n_w", sel=[3, 5])
    refused(">= n_w", sel=[1 << 40])
    refused("twice", sel=[3, 0, 3])
    refused("twice", sel=[0, 1, 2, 3, 4, 0])
    st, _ = _enc_create(**ok, out=False)
    assert st == INVALID and "NULL out" in _why()
    L = _lib.lib()
    for kw in (dict(emb=512), dict(sel=[4, 3, 2, 1, 0]), dict(sel=[0, 1, 2, 3, 4]), dict(emb=1 << 30)):
        st, h = _enc_create(**{**ok, **kw})
        assert st == 0 and h.value, (kw, _why())
        L.rg_buckler_encode_round_destroy(h)


def test_round_refusals_with_a_live_handle(F):
    L = _lib.lib()
    T = ringo.bigpoly.NewCyclicTransformer(F, 128)
    st, h = _enc_create(T.h, 256, 5, [3, 0])
    assert st == 0
    rnd, host, scr = L.rg_buckler_prove_encode_round_dev, L.rg_buckler_prove_encode_round, \
        L.rg_buckler_prove_encode_round_scratch_bytes
    try:
        for n in (0, 4, 65536, 1 << 40):
            assert scr(None, n) == 0
        assert rnd(None, 4, A, B, C, D, E, None) == INVALID and "NULL handle" in _why()
        assert rnd(None, 0, A, B, C, D, E, None) == INVALID
        assert host(None, 4, None, None, None, None) == INVALID and "NULL handle" in _why()
        assert rnd(h, 0, None, None, None, None, None, None) == 0  # nothing to do
        assert host(h, 0, None, None, None, None) == 0
        assert scr(h, 0) == 0 and scr(h, 65535) == 65535 * 2 * 128 * 8
        for n in (65536, 1 << 40):
            assert rnd(h, n, A, B, C, D, E, None) == INVALID and "n_proofs" in _why()
            assert host(h, n, None, None, None, None) == INVALID and "n_proofs" in _why()
            assert scr(h, n) == 0
        assert rnd(h, 2, None, B, C, D, E, None) == INVALID and "NULL witness" in _why()
        assert rnd(h, 2, A, B, None, D, E, None) == INVALID and "NULL encoded" in _why()
        assert rnd(h, 2, A, B, C, D, None, None) == INVALID and "NULL scratch" in _why()
        assert rnd(h, 2, A, None, C, D, E, None) == INVALID and "com without rand" in _why()
        # (w, rand, wecd, com, scratch): every pair
        for a in ((A, A, C, D, E), (A, B, A, D, E), (A, B, C, A, E), (A, B, C, D, A), (A, B, B, D, E), (A, B, C, B, E),
                  (A, B, C, D, B), (A, B, C, C, E), (A, B, C, D, C), (A, B, C, D, D), (A, None, A, None, E),
                  (A, None, C, None, A), (A, None, C, None, C), (A, B, C, None, B)):
            assert rnd(h, 2, *a, None) == INVALID and "alias" in _why(), a
        one = np.ones(4, np.uint64)
        p = _lib.ptr(one)
        assert host(h, 1, None, None, p, None) == INVALID and host(h, 1, p, None, None, None) == INVALID
        assert host(h, 1, p, None, p, None) == INVALID and "alias" in _why()
        assert host(h, 1, p, None, _lib.ptr(np.ones(4, np.uint64)), _lib.ptr(np.ones(4, np.uint64))) == INVALID
        assert "com without rand" in _why()
    finally:
        L.rg_buckler_encode_round_destroy(h)


def test_the_mirror_refuses_what_the_library_refuses(F):
    enc = buckler.EncodeRoundPlan(F, 128, 512, 5, (3, 0))
    assert enc.scratch_bytes(3) == 3 * 2 * 128 * 8 and enc.scratch_bytes(65536) == 0
    with pytest.raises(RingoPanic):
        buckler.EncodeRoundPlan(F, 128, 128, 5, (3, 0))
    with pytest.raises(RingoPanic):
        buckler.EncodeRoundPlan(F, 128, 256, 5, (3, 3))
