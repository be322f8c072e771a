"""GPU parity: the projection round of a batch of proofs in one call (rg_buckler_prove_proj_round*;
prover.go:165-193), bit for bit against the restatement of tests/buckler_proj_util.py
(buckler_lin_ref.ProjChecker + buckler_dcmp_ref.projDcmp per proof), into a witness table whose output
rows are pre-filled with -1 and that carries one guard element behind it.  Every row that is neither
`proj` nor `dcmp` must come back unchanged."""
import numpy as np
import pytest

from ringo import _lib, buckler
from tests import buckler_proj_util as P

pytestmark = pytest.mark.gpu

FF = np.uint64(2 ** 64 - 1)
N_W, SRC, PROJ, DCMP = 5, 1, 3, 0  # the one-constraint table: rows 2 and 4 are bystanders


def _dev(a, dtype=np.uint64):
    import torch
    a = np.ascontiguousarray(a, dtype)
    return torch.from_numpy(a.view(np.int64) if dtype == np.uint64 else a).cuda()


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def _xof(xs):
    return _dev(np.frombuffer(b"".join(xs), np.uint8).copy(), np.uint8)


def _scratch(plan, n):
    import torch
    return torch.full((max(1, plan.scratch_bytes(n) // 8),), -1, dtype=torch.int64, device="cuda")


@pytest.fixture(scope="module")
def plans():
    """One handle per (key, rank, nb), shared among the tests of the module."""
    made = {}

    def get(key, rank, nb):
        k = (key, rank, nb)
        if k not in made:
            F, _ = P.ctx(key)
            made[k] = buckler.ProjRoundPlan(F, rank, N_W, [(SRC, PROJ, DCMP, buckler.Decomposer(F, list(P.BASES[nb])))])
        return made[k]

    return get


def _tables(key, rank, nb, idx):
    """Host tables [n][N_W][rank][L] of the proofs idx with the output rows -1, and their XOF bytes."""
    ps = P.proofs(key, rank, nb)
    t = np.stack([P.table(key, rank, N_W, {SRC: ps[i][0]}, seed=1000 * rank + i) for i in idx])
    t[:, PROJ] = FF
    t[:, DCMP] = FF
    return t, [ps[i][1] for i in idx]


def _run(plan, tabs, xofs, stream=None):
    """The call on a device copy of tabs with a guard element behind it; returns the table read back."""
    n, L = tabs.shape[0], tabs.shape[-1]
    d_w = _dev(np.concatenate([tabs.reshape(-1), np.full(L, FF, np.uint64)]))
    plan.round_dev(n, d_w, _xof(xofs), _scratch(plan, n), stream=stream)
    if stream is not None:
        stream.synchronize()
    h = _host(d_w)
    assert (h[tabs.size:] == FF).all(), "guard element overwritten"
    return h[:tabs.size].reshape(tabs.shape)


def _expect(key, rank, nb, idx, tabs):
    want = tabs.copy()
    for k, i in enumerate(idx):
        want[k, PROJ], want[k, DCMP] = P.want(key, rank, nb, i)
    return want


# ---- the reference's cases say what they claim ---------------------------------------------------------
@pytest.mark.parametrize("key", P.FIELDS)
def test_the_cases_hold_every_digit_and_a_residual(key):
    """On the reference's output, not the device's: the cases of every field contain the digits +1, -1
    and 0 and at least one projected value beyond the sum of the base."""
    digits, residuals = P.digit_census(key)
    assert digits == {-1, 0, 1} and residuals >= 1
    for rank, nb in P.SHAPES:
        assert (P.want(key, rank, nb, 2)[0] == 0).all()  # XOF bytes all 0xFF: the matrix is all false
        row = P.want(key, rank, nb, 3)[0]  # all 0x00: every row is the sum of v
        assert (row[:128] == row[0]).all() and (row[128:] == 0).all()
        assert (P.want(key, rank, nb, 1)[0] == 0).all() and (P.want(key, rank, nb, 1)[1] == 0).all()  # the zero vector


# ---- parity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", P.FIELDS)
@pytest.mark.parametrize("rank,nb", P.SHAPES)
def test_parity(key, rank, nb, plans):
    """Batches of 1, 3 and 5 proofs; the batch of 5 holds all five kinds of input."""
    plan = plans(key, rank, nb)
    for idx in ((0,), (2, 3, 4), (0, 1, 2, 3, 4)):
        tabs, xofs = _tables(key, rank, nb, idx)
        got = _run(plan, tabs, xofs)
        want = _expect(key, rank, nb, idx, tabs)
        for k in range(len(idx)):
            for r in range(N_W):
                assert (got[k, r] == want[k, r]).all(), (idx, k, r)


@pytest.mark.parametrize("key", ["p63", "jindo_zp", "zp880"])
def test_two_constraints_of_different_nb_sharing_one_src(key):
    """One launch for both: rank 384 = 128 * 3, so the nb = 3 constraint has no digit tail and the
    nb = 1 constraint has one; both project the same witness under the proof's one matrix."""
    rank, n_w = 384, 7
    F, ref = P.ctx(key)
    cons = [(1, 3, 0, buckler.Decomposer(F, list(P.BASES[1]))), (1, 5, 2, buckler.Decomposer(F, list(P.BASES[3])))]
    plan = buckler.ProjRoundPlan(F, rank, n_w, cons)
    assert plan.scratch_bytes(3) == 3 * 2 * 1 * 128 * F.L * 8
    ps = P.proofs(key, rank, 3)
    idx = (0, 3, 4)
    tabs = np.stack([P.table(key, rank, n_w, {1: ps[i][0]}, seed=i) for i in idx])
    for r in (3, 0, 5, 2):
        tabs[:, r] = FF
    got = _run(plan, tabs, [ps[i][1] for i in idx])
    for k, i in enumerate(idx):
        proj, d3 = P.want(key, rank, 3, i)
        _, d1 = P.want(key, rank, 3, i, base_nb=1)
        for r, x in ((3, proj), (0, d1), (5, proj), (2, d3), (1, tabs[k, 1]), (4, tabs[k, 4]), (6, tabs[k, 6])):
            assert (got[k, r] == x).all(), (k, r)


# ---- equal to the single entries -------------------------------------------------------------------
@pytest.mark.parametrize("key", ["p63", "mult_zp", "jindo_zp", "zp440", "zp880"])
@pytest.mark.parametrize("rank,nb", [(200, 1), (1024, 3)])
def test_equal_to_the_single_entries_bit_for_bit(key, rank, nb, plans):
    """Each proof of a batch of 5 against rg_buckler_checker_set_xof_dev + rg_buckler_checker_transform_dev
    + rg_buckler_dcmp_proj_dev."""
    import torch
    F, ref = P.ctx(key)
    idx = tuple(range(P.N_PROOFS))
    tabs, xofs = _tables(key, rank, nb, idx)
    got = _run(plans(key, rank, nb), tabs, xofs)
    chk = buckler.ProjChecker(F, rank)
    dc = buckler.Decomposer(F, list(P.BASES[nb]))
    scr = torch.empty(chk.scratch_bytes(1) // 8, dtype=torch.int64, device="cuda")
    for k in idx:
        chk.set_xof_dev(_xof([xofs[k]]))
        proj = torch.full((rank * F.L,), -1, dtype=torch.int64, device="cuda")
        dcmp = torch.full((rank * F.L,), -1, dtype=torch.int64, device="cuda")
        chk.transform_dev(proj, _dev(tabs[k, SRC]), 1, scr)
        dc.proj_dev(dcmp, proj, rank)
        assert (_host(proj).reshape(rank, F.L) == got[k, PROJ]).all(), k
        assert (_host(dcmp).reshape(rank, F.L) == got[k, DCMP]).all(), k


# ---- independence ----------------------------------------------------------------------------------
def test_permuting_the_batch_permutes_the_outputs(plans):
    key, rank, nb = "jindo_zp", 200, 1
    idx, perm = (0, 1, 2, 3, 4), [3, 0, 4, 2, 1]
    tabs, xofs = _tables(key, rank, nb, idx)
    a = _run(plans(key, rank, nb), tabs, xofs)
    b = _run(plans(key, rank, nb), tabs[perm], [xofs[i] for i in perm])
    assert (a[perm] == b).all()


def test_swapping_two_proofs_xof_bytes_changes_exactly_those_two(plans):
    """Proofs 0 and 3 (small signed entries; random and all-true matrix): with the base [1] both of their
    rows change under the other's matrix.  The zero vector and the saturated proof would keep theirs."""
    key, rank, nb = "p63", 200, 1
    idx = (0, 1, 3, 4)
    tabs, xofs = _tables(key, rank, nb, idx)
    sw = list(xofs)
    sw[0], sw[2] = xofs[2], xofs[0]
    a, b = _run(plans(key, rank, nb), tabs, xofs), _run(plans(key, rank, nb), tabs, sw)
    for k in range(4):
        for r in range(N_W):
            same = (a[k, r] == b[k, r]).all()
            assert same == (not (k in (0, 2) and r in (PROJ, DCMP))), (k, r)


def test_two_streams_with_separate_scratch(plans):
    """Two calls in flight on two streams with one handle (own table, XOF bytes and scratch each)."""
    import torch
    key, rank, nb = "jindo_zp", 1024, 3
    plan = plans(key, rank, nb)
    batches = [(0, 1, 2), (3, 4)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    state = []
    for idx in batches:
        tabs, xofs = _tables(key, rank, nb, idx)
        state.append((tabs, _dev(tabs), _xof(xofs), _scratch(plan, len(idx))))
    _run(plan, *_tables(key, rank, nb, (0,)))  # the base is on the device before the two calls overlap
    torch.cuda.synchronize()
    for (tabs, d_w, d_x, scr), st in zip(state, streams):
        plan.round_dev(tabs.shape[0], d_w, d_x, scr, stream=st)
    for st in streams:
        st.synchronize()
    for (tabs, d_w, _, _), idx in zip(state, batches):
        assert (_host(d_w).reshape(tabs.shape) == _expect(key, rank, nb, idx, tabs)).all(), idx


# ---- host form, mirror, nothing to do ----------------------------------------------------------------
def test_host_form_and_mirror_agree_with_the_dev_form(plans):
    key, rank, nb = "zp440", 256, 2
    plan = plans(key, rank, nb)
    idx = (0, 3, 4)
    tabs, xofs = _tables(key, rank, nb, idx)
    dev = _run(plan, tabs, xofs)
    before = tabs.copy()
    host = plan.round(tabs, b"".join(xofs))
    assert (tabs == before).all()  # the mirror returns a copy
    assert host.shape == dev.shape and (host == dev).all()
    assert (host == _expect(key, rank, nb, idx, tabs)).all()
    # a bound in place of a Decomposer: decomposeBase(rank * bound)
    F, _ = P.ctx(key)
    assert buckler.ProjRoundPlan(F, 2048, N_W, [(SRC, PROJ, DCMP, 5)]).constraints[0][3].dcmpBase == \
        buckler.decomposeBase(2048 * 5)


def test_zero_proofs_touch_nothing(plans):
    key, rank, nb = "p63", 128, 1
    plan = plans(key, rank, nb)
    tabs, xofs = _tables(key, rank, nb, (0,))
    d_w = _dev(tabs)
    plan.round_dev(0, d_w, _xof(xofs), _scratch(plan, 1))
    assert (_host(d_w).reshape(tabs.shape) == tabs).all()
    assert _lib.lib().rg_buckler_prove_proj_round_dev(plan.h, 0, None, None, None, None) == 0
    assert plan.scratch_bytes(0) == 0
    # a refused call leaves real buffers as they were
    assert _lib.lib().rg_buckler_prove_proj_round_dev(plan.h, 1, d_w.data_ptr(), _xof(xofs).data_ptr(),
                                                      d_w.data_ptr(), None) == -1
    assert (_host(d_w).reshape(tabs.shape) == tabs).all()
