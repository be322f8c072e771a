"""GPU parity: the norm decompositions of a batch of proofs in one call (rg_buckler_prove_dcmp_round*;
prover.go:77-111), bit for bit against the restatement of tests/buckler_wround_util.py
(buckler_dcmp_ref.infDcmp / twoDcmp per proof and constraint), in place in a proof-major witness table
whose output rows are pre-filled with -1.  A guard element sits behind every buffer, the scratch is
pre-filled with -1, and every row that is not an output must come back unchanged."""
import numpy as np
import pytest

from ringo import _lib, buckler
from tests import buckler_wround_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plans():
    """One handle per (key, rank, table), shared among the tests of the module."""
    made = {}

    def get(key, rank, table):
        k = (key, rank, table)
        if k not in made:
            F, _ = U.ctx(key)
            n_w, inf, two = U.TABLES[table]
            dcs = {nb: buckler.Decomposer(F, list(U.BASES[nb])) for nb in {c[1] for c in inf + two}}
            made[k] = buckler.DcmpRoundPlan(F, rank, n_w, inf=[(s, dcs[nb], rows) for s, nb, rows in inf],
                                            two=[(s, dcs[nb], d) for s, nb, d in two])
        return made[k]

    return get


def _tables(key, rank, table, idx):
    return np.stack([U.dcmp_table(key, rank, table, i) for i in idx])


def _expect(key, rank, table, idx, tabs):
    pairs = [U.dcmp_expect(key, rank, table, i, tabs[k]) for k, i in enumerate(idx)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def _run(plan, tabs, with_sq=True, stream=None):
    """The call on a device copy of tabs; returns (the table, sq or None) read back, the guards checked."""
    n, L, n_two = tabs.shape[0], tabs.shape[-1], len(plan.two)
    d_w = U.dev_guarded(tabs, L)
    d_sq = U.filled(n * n_two * L, L) if with_sq and n_two else None
    d_scr = U.filled(plan.scratch_bytes(n) // 8, L)
    plan.round_dev(n, d_w, d_sq, d_scr, stream=stream)
    if stream is not None:
        stream.synchronize()
    U.unguard(d_scr, (plan.scratch_bytes(n) // 8,), L, "the scratch")
    sq = None if d_sq is None else U.unguard(d_sq, (n, n_two, L), L, "sq")
    return U.unguard(d_w, tabs.shape, L, "the table"), sq


def _same(got, want, what):
    for k in range(want.shape[0]):
        for r in range(want.shape[1]):
            assert (got[k, r] == want[k, r]).all(), (what, "proof", k, "row", r)


# ---- parity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", U.FIELDS)
@pytest.mark.parametrize("rank", U.RANKS)
def test_parity(key, rank, plans):
    """Every table of the case, in batches of 1, 3 and 5 proofs; sq is asked for in the batches of 1 and 5."""
    for table in U.tables_of(key, rank):
        plan = plans(key, rank, table)
        assert plan.scratch_bytes(3) == 3 * len(plan.two) * -(-rank // 1024) * plan.field.L * 8
        for idx in U.BATCHES:
            tabs = _tables(key, rank, table, idx)
            got, sq = _run(plan, tabs, with_sq=len(idx) != 3)
            want, want_sq = _expect(key, rank, table, idx, tabs)
            _same(got, want, (table, idx))
            if sq is not None:
                assert (sq == want_sq).all(), (table, idx)


# ---- equal to the single entries -------------------------------------------------------------------
@pytest.mark.parametrize("key", U.FIELDS[:5])
@pytest.mark.parametrize("rank,table", [(200, "shared_src"), (2500, "two_inf"), (2500, "only_two")])
def test_equal_to_the_single_entries_bit_for_bit(key, rank, table, plans):
    """Each proof of a batch of 5 against rg_buckler_dcmp_inf_dev and rg_buckler_dcmp_two_dev on its rows."""
    F, _ = U.ctx(key)
    L = F.L
    idx = tuple(range(U.N_PROOFS))
    tabs = _tables(key, rank, table, idx)
    plan = plans(key, rank, table)
    got, sq = _run(plan, tabs)
    for k in idx:
        for src, dc, rows in plan.inf:
            out = U.filled(len(rows) * rank * L, L)
            dc.inf_dev(out, U.dev(tabs[k, src]), 1, rank)
            digits = U.unguard(out, (len(rows), rank, L), L, "the single entry's digits")
            for j, r in enumerate(rows):
                assert (digits[j] == got[k, r]).all(), (k, src, j)
        for c, (src, dc, dst) in enumerate(plan.two):
            out, one_sq = U.filled(rank * L, L), U.filled(L, L)
            scr = U.filled(dc.scratch_bytes(1, rank) // 8, L)
            dc.two_dev(out, U.dev(tabs[k, src]), 1, rank, d_sq=one_sq, d_scratch=scr)
            assert (U.unguard(out, (rank, L), L, "the single entry's row") == got[k, dst]).all(), (k, src)
            assert (U.unguard(one_sq, (L,), L, "the single entry's sq") == sq[k, c]).all(), (k, src)


# ---- independence ----------------------------------------------------------------------------------
def test_permuting_the_batch_permutes_the_outputs(plans):
    key, rank, table = "jindo_zp", 200, "shared_src"
    idx, perm = (0, 1, 2, 3, 4), [3, 0, 4, 2, 1]
    tabs = _tables(key, rank, table, idx)
    a, sa = _run(plans(key, rank, table), tabs)
    b, sb = _run(plans(key, rank, table), tabs[perm])
    assert (a[perm] == b).all() and (sa[perm] == sb).all()
    assert len({a[k, 0].tobytes() for k in range(5)}) > 1  # the proofs' outputs do differ


def test_two_streams_with_one_handle_and_separate_scratch(plans):
    import torch
    key, rank, table = "jindo_zp", 2500, "shared_src"
    plan = plans(key, rank, table)
    L = plan.field.L
    batches = [(0, 1, 2), (3, 4)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    _run(plan, _tables(key, rank, table, (0,)))  # the tables are on the device before the two calls overlap
    state = []
    for idx in batches:
        tabs = _tables(key, rank, table, idx)
        state.append((tabs, U.dev(tabs), U.filled(len(idx) * L, L), U.filled(plan.scratch_bytes(len(idx)) // 8, L)))
    torch.cuda.synchronize()
    for (tabs, d_w, d_sq, scr), st in zip(state, streams):
        plan.round_dev(tabs.shape[0], d_w, d_sq, scr, stream=st)
    for st in streams:
        st.synchronize()
    for (tabs, d_w, d_sq, _), idx in zip(state, batches):
        want, want_sq = _expect(key, rank, table, idx, tabs)
        assert (U.host(d_w).reshape(tabs.shape) == want).all(), idx
        assert (U.unguard(d_sq, want_sq.shape, L, "sq") == want_sq).all(), idx


# ---- host form, mirror, nothing to do ----------------------------------------------------------------
@pytest.mark.parametrize("table", ["shared_src", "only_inf"])
def test_host_form_and_mirror_agree_with_the_dev_form(table, plans):
    key, rank = "zp440", 200
    plan = plans(key, rank, table)
    idx = (0, 3, 4)
    tabs = _tables(key, rank, table, idx)
    dev, dev_sq = _run(plan, tabs)
    before = tabs.copy()
    host, host_sq = plan.round(tabs)
    assert (tabs == before).all()  # the mirror returns a copy
    want, want_sq = _expect(key, rank, table, idx, tabs)
    assert host.shape == dev.shape and (host == dev).all() and (host == want).all()
    if plan.two:
        assert (host_sq == dev_sq).all() and (host_sq == want_sq).all()
    else:
        assert host_sq is None and dev_sq is None


def test_zero_proofs_and_refused_calls_touch_nothing(plans):
    key, rank, table = "p63", 200, "shared_src"
    plan = plans(key, rank, table)
    L = plan.field.L
    tabs = _tables(key, rank, table, (0,))
    d_w, d_sq, scr = U.dev(tabs), U.filled(L, L), U.filled(plan.scratch_bytes(1) // 8, L)
    plan.round_dev(0, d_w, d_sq, scr)
    lib = _lib.lib()
    assert lib.rg_buckler_prove_dcmp_round_dev(plan.h, 0, None, None, None, None) == 0
    assert plan.scratch_bytes(0) == 0
    # refused: aliased buffers, a missing scratch, too many proofs
    for args in ((1, d_w.data_ptr(), d_sq.data_ptr(), d_w.data_ptr()), (1, d_w.data_ptr(), d_w.data_ptr(), scr.data_ptr()),
                 (1, d_w.data_ptr(), d_sq.data_ptr(), None), (65536, d_w.data_ptr(), d_sq.data_ptr(), scr.data_ptr())):
        assert lib.rg_buckler_prove_dcmp_round_dev(plan.h, *args, None) == -1, args
    assert (U.host(d_w).reshape(tabs.shape) == tabs).all()
    assert (U.host(d_sq) == U.FF).all() and (U.host(scr) == U.FF).all()
