"""GPU parity of the 2^16 lazy MONT passes on the tile of 16 points per thread (ntt64.hpp
ntt16x_tile: ROW forward on RP tiles, COL inverse) and with rank_inv folded into the last inverse
round (ntt_tile.hpp; both tile shapes), bit for bit against the C oracle (oracle/oracle.c).

Moduli: p63 = 47104^4 + 1 (the headline prime) and 0x47e0f66500000001 (the largest prime == 1 mod
2^32 under the Montgomery gate).  N = 2^16, negacyclic and cyclic.  Batches 1 and 17 (ROW tiles of
16 rows of one polynomial, on the 8-point tile, beside the 16-point COL inverse) and 16, 32 and 48
(the RP ROW tiles: one row of 16 polynomials, forward on 16 points; 48 is three tile rows, so the
reversed second pass starts on another polynomial group than the first).  Every case runs out of
place and in place.

Inputs are synth_util.structured_batch, checked three ways as in test_gpu_ntt_mont.py: forward
against the oracle, inverse of the forward == the input, inverse of the input against the oracle.

Plans built from tables carry the caller's rank_inv, and the fold must scale by that value and not
by N^-1: rank_inv = 1 (the raw word), the Montgomery one (an unscaled inverse) and a random residue,
batch 16, the inverse against cf.ntt_inv(a, twi, rank_inv).

What this does not see: which kernels ran (see test_gpu_ntt_mont.py's note)."""
import functools

import numpy as np
import pytest

import ringo
from tests import synth_util as su

pytestmark = pytest.mark.gpu

NS = len(su.STRUCTURED)
LOGN = 16
N = 1 << LOGN
MODULI = {"p63": 47104 ** 4 + 1, "mont_tight": 0x47E0F66500000001}


@functools.lru_cache(maxsize=None)
def _cfield(name):
    import coracle as co
    return co.CField(MODULI[name])


@functools.lru_cache(maxsize=2)
def _tables(name, cyclic):
    tabs = _cfield(name).tables(N, cyclic=cyclic)
    for t in tabs:
        t.setflags(write=False)
    return tabs


def _dev(a):
    import torch
    return torch.from_numpy(a.view(np.int64).reshape(-1).copy()).cuda()


def _host(x, batch):
    return x.cpu().numpy().view(np.uint64).reshape(batch, N, 1)


def _same(what, got, want, ctx):
    bad = [i for i in range(want.shape[0]) if not (got[i] == want[i]).all()]
    labels = [su.STRUCTURED[i] if i < NS else f"random{i - NS}" for i in bad]
    assert not bad, ctx + (what, labels)


@pytest.mark.parametrize("batch", [1, 16, 17, 32, 48])
@pytest.mark.parametrize("negacyclic", [True, False], ids=["negacyclic", "cyclic"])
@pytest.mark.parametrize("name", list(MODULI))
def test_ntt_2e16_folded_inverse(name, negacyclic, batch):
    import torch
    q = MODULI[name]
    cf = _cfield(name)
    T = (ringo.CyclotomicTransformer if negacyclic else ringo.CyclicTransformer)(ringo.Field(q), N)
    otw, otwi, oninv = tabs = _tables(name, not negacyclic)
    tw, twi, ninv = T.tables()
    assert (tw == otw).all() and (twi == otwi).all() and (ninv == oninv).all(), "tables"
    rng = np.random.default_rng(1600 + batch)
    a = su.structured_batch(cf, q, N, tabs, batch, rng)
    want = cf.ntt_fwd(a, otw)
    want_inv = cf.ntt_inv(a, otwi, oninv)
    ctx = (name, "negacyclic" if negacyclic else "cyclic", batch)
    # out of place
    x = _dev(a)
    y, z = torch.empty_like(x), torch.empty_like(x)
    T.fwd_dev(y, x, batch)
    T.inv_dev(z, y, batch)
    torch.cuda.synchronize()
    _same("fwd, out of place", _host(y, batch), want, ctx)
    _same("inv roundtrip, out of place", _host(z, batch), a, ctx)
    T.inv_dev(z, x, batch)
    torch.cuda.synchronize()
    _same("inv, out of place", _host(z, batch), want_inv, ctx)
    _same("input untouched", _host(x, batch), a, ctx)
    # in place
    T.inv_dev(y, y, batch)
    z.copy_(x)
    T.fwd_dev(z, z, batch)
    T.inv_dev(x, x, batch)
    torch.cuda.synchronize()
    _same("inv roundtrip, in place", _host(y, batch), a, ctx)
    _same("fwd, in place", _host(z, batch), want, ctx)
    _same("inv, in place", _host(x, batch), want_inv, ctx)


@pytest.mark.parametrize("rank_inv", ["one", "mont_one", "random"])
@pytest.mark.parametrize("negacyclic", [True, False], ids=["negacyclic", "cyclic"])
@pytest.mark.parametrize("name", list(MODULI))
def test_table_built_plan_folds_its_own_rank_inv(name, negacyclic, rank_inv):
    import torch
    q = MODULI[name]
    cf = _cfield(name)
    batch = 16
    otw, otwi, oninv = tabs = _tables(name, not negacyclic)
    rng = np.random.default_rng(1616)
    S = {"one": 1, "mont_one": (1 << 64) % q, "random": int(rng.integers(2, q, dtype=np.uint64))}[rank_inv]
    assert S != int(oninv[0])
    sv = np.array([S], np.uint64)
    T = (ringo.CyclotomicTransformer if negacyclic else ringo.CyclicTransformer)(ringo.Field(q), N, tables=(otw, otwi, sv))
    assert (T.tables()[2] == sv).all()
    a = su.structured_batch(cf, q, N, tabs, batch, rng)
    want_inv = cf.ntt_inv(a, otwi, sv)
    ctx = (name, "negacyclic" if negacyclic else "cyclic", rank_inv)
    x = _dev(a)
    y = torch.empty_like(x)
    T.inv_dev(y, x, batch)
    T.inv_dev(x, x, batch)
    torch.cuda.synchronize()
    _same("inv, out of place", _host(y, batch), want_inv, ctx)
    _same("inv, in place", _host(x, batch), want_inv, ctx)
    T.fwd_dev(y, y, batch)  # the forward transform undoes all but the scale: it is unaffected by rank_inv
    torch.cuda.synchronize()
    _same("fwd of the scaled inverse", _host(y, batch), cf.ntt_fwd(want_inv, otw), ctx)
