"""GPU: the 4-limb q = 1 mod 2^64 fields' long NTT route (jindo_zp = q255, zp220; ntt256.hpp's
ntt256_edge_pass and ntt256_pass over 2^16-point blocks, three passes for 2^17 <= N <= 2^19, ntt_route.hpp
ntt_fast256_long) against the C oracle, bit for bit.

  * which route a plan took (rg_ntt_route_name / rg_ntt_passes, `_Transformer.route`): fast256 in
    three passes at 2^17, 2^18 and 2^19 in both directions, still two at 2^16, tiled in two for a
    modulus with its top bit set (s256_top) or q[0] != 1 (bfv_zp), and for a table-built plan whose
    rank_inv is not N^-1 fast256 forward and tiled inverse;
  * parity, cyclic and cyclotomic: forward, inverse and inverse of the forward, in place and out of
    place (which must leave its input intact), tables equal to the oracle's, on uniform residues and
    on the polynomial with q - 1 in its first half and zero in its second, at the (logN, batch)
    that separate the runner's paths:
      (17, 1)  M = 1, 2 blocks: no split          (17, 4)  exactly 8 blocks: split 4 + 4
      (17, 5)  10 blocks: 5 + 5, the boundary inside a polynomial, the second half starts at B = 1
      (18, 1)  M = 2, 4 blocks: no split          (18, 3)  12 blocks: 6 + 6, second half at B = 2
      (19, 1)  M = 3, one polynomial split 4 + 4, second half at B = 4
    and all q - 1 at (19, 1) per field: the largest values through 19 lazy stages;
  * one plan at (17, 4) driven from two streams at once."""
import functools

import numpy as np
import pytest

import ringo
from tests import synth_util as su

pytestmark = pytest.mark.gpu
FAST = pytest.mark.parametrize("name", ["jindo_zp", "zp220"])
KINDS = pytest.mark.parametrize("negacyclic", [False, True], ids=["cyclic", "cyclotomic"])
CASES = [(17, 1), (17, 4), (17, 5), (18, 1), (18, 3), (19, 1)]


def _transformer(name, logn, negacyclic):
    return (ringo.CyclotomicTransformer if negacyclic else ringo.CyclicTransformer)(ringo.Field(su.modulus(name)), 1 << logn)


# ---- routes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", [17, 18, 19])
@KINDS
@FAST
def test_route_is_fast256_in_three_passes(name, negacyclic, logn):
    T = _transformer(name, logn, negacyclic)
    assert T.route() == ("fast256", 3) and T.route(inverse=True) == ("fast256", 3)
    lib = ringo.lib()
    for d in (0, 1):
        assert lib.rg_ntt_route_name(T.h, d) == b"fast256" and lib.rg_ntt_passes(T.h, d) == 3


@FAST
def test_route_at_2e16_is_unchanged(name):
    T = _transformer(name, 16, True)
    assert T.route() == ("fast256", 2) and T.route(inverse=True) == ("fast256", 2)


@pytest.mark.parametrize("name", ["s256_top", "bfv_zp"])
def test_route_of_the_other_four_limb_moduli_is_tiled(name):
    T = _transformer(name, 17, True)
    assert T.route() == ("tiled", 2) and T.route(inverse=True) == ("tiled", 2)


@FAST
def test_table_built_plan_with_another_rank_inv(name):
    """rank_inv = 1 instead of N^-1: forward on the long route, inverse on the tiled passes, which
    multiply by the caller's rank_inv -- the oracle's inverse with that rank_inv.  Both directions
    read the same uploaded tables."""
    cf = su.cfield(name)
    tw, twi, ninv = su.oracle_tables(name, 17, True)  # cyclic
    F = ringo.Field(su.modulus(name))
    mont_one = np.ascontiguousarray(F.constants()[2], np.uint64).reshape(ninv.shape)  # 1 in Montgomery form
    assert not (mont_one == ninv).all()
    T = ringo.CyclicTransformer(F, 1 << 17, tables=(tw, twi, mont_one))
    assert T.route() == ("fast256", 3) and T.route(inverse=True) == ("tiled", 2)
    a = _inputs(name, 17, 1)[:1]
    assert (T.FwdNTTTo(None, a) == _oracle(name, 17, 1, False)["fwd"][:1]).all()
    assert (T.InvNTTTo(None, a) == cf.ntt_inv(a, twi, mont_one)).all()


# ---- parity ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _inputs(name, logn, batch):
    """[2 * batch, N, 4]: `batch` uniform polynomials, then `batch` whose first is q - 1 in its first
    half and zero in its second (the rest uniform again)."""
    q = su.modulus(name)
    N = 1 << logn
    rng = np.random.default_rng(100 * logn + batch)
    a = su.rand_residues(q, 4, 2 * batch * N, rng).reshape(2 * batch, N, 4)
    a[batch, :N // 2] = su.limbs_of(q - 1, 4)
    a[batch, N // 2:] = 0
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=2)
def _oracle(name, logn, batch, negacyclic):
    """The oracle's forward and inverse of _inputs(): computed once, shared by the tests of one case
    (which run next to each other), read-only."""
    cf = su.cfield(name)
    tw, twi, ninv = su.oracle_tables(name, logn, not negacyclic)
    a = _inputs(name, logn, batch)
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


# the decorators from the top vary fastest: the four tests of one (field, kind, case) run together
@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("inp", ["uniform", "half_qm1"])
@pytest.mark.parametrize("case", CASES, ids=["2e%d_x%d" % c for c in CASES])
@KINDS
@FAST
def test_parity(name, negacyclic, case, inp, in_place):
    logn, b = case
    T = _transformer(name, logn, negacyclic)
    assert T.route() == ("fast256", 3) and T.route(inverse=True) == ("fast256", 3)
    otw, otwi, oninv = su.oracle_tables(name, logn, not negacyclic)
    tw, twi, ninv = T.tables()
    assert (tw == otw).all() and (twi == otwi).all() and (ninv == oninv).all(), "tables"
    sl = slice(0, b) if inp == "uniform" else slice(b, 2 * b)
    a, want = _inputs(name, logn, b)[sl], _oracle(name, logn, b, negacyclic)
    fwd = _dev(T.fwd_dev, a, b, in_place)
    assert (fwd == want["fwd"][sl]).all(), "fwd"
    assert (_dev(T.inv_dev, a, b, in_place) == want["inv"][sl]).all(), "inv"
    assert (_dev(T.inv_dev, fwd, b, in_place) == a).all(), "inv(fwd(x)) != x"


@FAST
def test_all_qm1_at_2e19(name):
    """Every coefficient q - 1: the largest canonical value into every butterfly of the first stage."""
    q, logn = su.modulus(name), 19
    cf = su.cfield(name)
    T = _transformer(name, logn, True)
    tw, twi, ninv = su.oracle_tables(name, logn, False)
    a = np.broadcast_to(su.limbs_of(q - 1, 4), (1, 1 << logn, 4)).copy()
    fwd = _dev(T.fwd_dev, a, 1, True)
    assert (fwd == cf.ntt_fwd(a, tw)).all(), "fwd"
    assert (_dev(T.inv_dev, a, 1, False) == cf.ntt_inv(a, twi, ninv)).all(), "inv"
    assert (_dev(T.inv_dev, fwd, 1, True) == a).all(), "inv(fwd(x)) != x"


# ---- two streams -------------------------------------------------------------------------------------
@FAST
def test_two_streams_share_one_plan(name):
    """One plan at (17, 4): every call splits over the caller's stream and the plan's helper stream.
    Two caller streams queue forward and inverse transforms of their own buffers before either
    finishes (the fork / join events are per plan); every result equals the oracle."""
    import torch
    logn, b = 17, 4
    T = _transformer(name, logn, True)
    a, want = _inputs(name, logn, b), _oracle(name, logn, b, True)
    sl = [slice(0, b), slice(b, 2 * b)]
    xs = [torch.from_numpy(a[s].view(np.int64).reshape(-1).copy()).cuda() for s in sl]
    fs, vs = [torch.empty_like(x) for x in xs], [torch.empty_like(x) for x in xs]
    sts = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for _ in range(2):
        for i in range(2):
            T.fwd_dev(fs[i], xs[i], b, stream=sts[i])
        for i in range(2):
            T.inv_dev(vs[i], xs[i], b, stream=sts[i])
    for i in range(2):  # and back in place, ordered on the stream behind the forward's helper half
        T.inv_dev(fs[i], fs[i], b, stream=sts[i])
        T.fwd_dev(fs[i], fs[i], b, stream=sts[i])
    torch.cuda.synchronize()
    for i in range(2):
        shape = a[sl[i]].shape
        assert (fs[i].cpu().numpy().view(np.uint64).reshape(shape) == want["fwd"][sl[i]]).all(), ("fwd", i)
        assert (vs[i].cpu().numpy().view(np.uint64).reshape(shape) == want["inv"][sl[i]]).all(), ("inv", i)
