"""GPU: the wide fields' long NTT route (zp440: 7 limbs, zp880: 14 limbs; ntt_wide_pass in three
passes for 2^17 <= N <= 2^24, ntt_route.hpp ntt_wide_long) against the C oracle, bit for bit.

  * which route a plan took (rg_ntt_route_name / rg_ntt_passes, `_Transformer.route`): wide in
    three passes at 2^17 in both directions, still two at 2^16 and 2^10, stages for a modulus
    without a spare top bit, and for a table-built plan whose rank_inv is not N^-1 wide forward
    and stages inverse;
  * parity at 2^17 (batch 1 for zp880, 2 for zp440), cyclic and cyclotomic: forward, inverse and
    inverse of the forward, in place and out of place, on uniform elements and on the polynomial
    with q - 1 in its first half and zero in its second;
  * the three-pass kernel at 2^3, 2^7, 2^9 and 2^12, the smallest ranks at which a wrong
    middle-pass stride, twiddle index or halving count shows, forced by RINGO_NTT_KERNEL=w3 on the
    experiments build in a child process (tests/exp_child_wide3.py).

The grid limit cannot be reached with a buffer that fits a device: tests/test_ntt_wide_long_host.py
has it as a host test."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import ringo
from tests import exp_child_wide3 as child
from tests import synth_util as su

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LOGN = 17
BATCH = {"zp440": 2, "zp880": 1}
KINDS = pytest.mark.parametrize("negacyclic", [False, True], ids=["cyclic", "cyclotomic"])
WIDE = pytest.mark.parametrize("name", ["zp440", "zp880"])


def _transformer(name, logn, negacyclic):
    return (ringo.CyclotomicTransformer if negacyclic else ringo.CyclicTransformer)(ringo.Field(su.modulus(name)), 1 << logn)


# ---- routes ------------------------------------------------------------------------------------------
@KINDS
@WIDE
def test_route_is_wide_in_three_passes_at_2e17(name, negacyclic):
    T = _transformer(name, LOGN, negacyclic)
    assert T.route() == ("wide", 3) and T.route(inverse=True) == ("wide", 3)
    assert ringo.lib().rg_ntt_route_name(T.h, 0) == b"wide" and ringo.lib().rg_ntt_passes(T.h, 1) == 3


@WIDE
def test_route_below_2e17_is_unchanged(name):
    for logn in (16, 10):
        T = _transformer(name, logn, True)
        assert T.route() == ("wide", 2) and T.route(inverse=True) == ("wide", 2)
    T = _transformer(name, 8, False)
    assert T.route() == ("wide", 1)


@pytest.mark.parametrize("name", ["s448_top", "s896_top"])
def test_route_without_a_spare_bit_is_stages(name):
    T = _transformer(name, LOGN, True)
    assert T.route() == ("stages", 0) and T.route(inverse=True) == ("stages", 0)


def test_route_of_the_other_families_and_of_no_plan():
    assert _transformer("p63", 16, True).route() == ("lazy64", 2)
    assert _transformer("jindo_zp", 16, True).route() == ("fast256", 2)
    assert _transformer("zp110", 12, True).route() == ("tiled", 1)
    assert _transformer("zp110", 5, True).route() == ("stages", 0)
    assert ringo.lib().rg_ntt_route_name(None, 0) is None and ringo.lib().rg_ntt_passes(None, 0) == -1


@WIDE
def test_table_built_plan_with_another_rank_inv(name):
    """rank_inv = 1 instead of N^-1: forward on the three passes, inverse per stage, which multiplies by
    the caller's rank_inv -- the oracle's inverse with that rank_inv."""
    q = su.modulus(name)
    cf = su.cfield(name)
    tw, twi, ninv = su.oracle_tables(name, LOGN, True)  # cyclic
    F = ringo.Field(q)
    mont_one = np.ascontiguousarray(F.constants()[2], np.uint64).reshape(ninv.shape)  # 1 in Montgomery form
    assert not (mont_one == ninv).all()
    T = ringo.CyclicTransformer(F, 1 << LOGN, tables=(tw, twi, mont_one))
    assert T.route() == ("wide", 3) and T.route(inverse=True) == ("stages", 0)
    a = _inputs(name)[:1]
    assert (T.FwdNTTTo(None, a) == _oracle(name, False)["fwd"][:1]).all()
    assert (T.InvNTTTo(None, a) == cf.ntt_inv(a, twi, mont_one)).all()


# ---- parity at 2^17 ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(name):
    """[2 * batch, N, L]: `batch` uniform polynomials, then `batch` whose first is q - 1 in its first half
    and zero in its second (the rest uniform again)."""
    q = su.modulus(name)
    L = (q.bit_length() + 63) // 64
    N, b = 1 << LOGN, BATCH[name]
    rng = np.random.default_rng(1700 + L)
    a = su.rand_residues(q, L, 2 * b * N, rng).reshape(2 * b, N, L)
    a[b, :N // 2] = su.limbs_of(q - 1, L)
    a[b, N // 2:] = 0
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _oracle(name, negacyclic):
    """The oracle's forward and inverse of _inputs(name): computed once, shared, read-only."""
    cf = su.cfield(name)
    tw, twi, ninv = su.oracle_tables(name, LOGN, not negacyclic)
    a = _inputs(name)
    out = {"fwd": cf.ntt_fwd(a, tw), "inv": cf.ntt_inv(a, twi, ninv)}
    for v in out.values():
        v.setflags(write=False)
    return out


def _dev(fn, a, batch, in_place):
    import torch
    x = torch.from_numpy(a.view(np.int64).reshape(-1).copy()).cuda()
    y = x if in_place else torch.full_like(x, -1)
    fn(y, x, batch)
    torch.cuda.synchronize()
    if not in_place:
        assert (x.cpu().numpy().view(np.uint64).reshape(a.shape) == a).all(), "out of place wrote its input"
    return y.cpu().numpy().view(np.uint64).reshape(a.shape)


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("inp", ["uniform", "half_qm1"])
@KINDS
@WIDE
def test_parity_at_2e17(name, negacyclic, inp, in_place):
    T = _transformer(name, LOGN, negacyclic)
    assert T.route() == ("wide", 3) and T.route(inverse=True) == ("wide", 3)
    otw, otwi, oninv = su.oracle_tables(name, LOGN, not negacyclic)
    tw, twi, ninv = T.tables()
    assert (tw == otw).all() and (twi == otwi).all() and (ninv == oninv).all(), "tables"
    b = BATCH[name]
    sl = slice(0, b) if inp == "uniform" else slice(b, 2 * b)
    a, want = _inputs(name)[sl], _oracle(name, negacyclic)
    fwd = _dev(T.fwd_dev, a, b, in_place)
    assert (fwd == want["fwd"][sl]).all(), "fwd"
    assert (_dev(T.inv_dev, a, b, in_place) == want["inv"][sl]).all(), "inv"
    assert (_dev(T.inv_dev, fwd, b, in_place) == a).all(), "inv(fwd(x)) != x"


# ---- the forced three-pass kernel ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def forced(tmp_path_factory):
    out = tmp_path_factory.mktemp("wide3") / "wide3.npz"
    r = subprocess.run([sys.executable, os.path.join(HERE, "exp_child_wide3.py"), str(out)], capture_output=True,
                       text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    return {k: v for k, v in np.load(out).items()}


@pytest.mark.parametrize("case", child.CASES, ids=[child.key(c, "w3") for c in child.CASES])
def test_forced_three_passes_equal_the_oracle(forced, case):
    name, logn, batch, negacyclic = case
    assert list(forced[child.key(case, "route")]) == [3, 3], "the child did not run the three-pass route"
    cf = su.cfield(name)
    tw, twi, ninv = su.oracle_tables(name, logn, not negacyclic)
    a = child.inputs(case)
    want = {"f": cf.ntt_fwd(a, tw), "i": cf.ntt_inv(a, twi, ninv)}
    for what in ("fo", "fi", "io", "ii"):
        got = forced[child.key(case, what)].view(np.uint64).reshape(a.shape)
        bad = [i for i in range(batch) if not (got[i] == want[what[0]][i]).all()]
        assert not bad, (case, what, bad)
