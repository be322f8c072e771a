"""GPU parity of the 2^16 lazy NTT passes on both sides of the Montgomery-product gate
(ntt64.hpp ntt64_mont_ok, ntt_l1_lazy.hip), bit-exact against the C oracle (oracle/oracle.c).

Moduli: p63 = 47104^4 + 1 (the headline prime, MONT kernels), 0x47e0f66500000001 (the largest
prime == 1 mod 2^32 under the gate: the MONT kernels at their tightest headroom) and
0x47e0f67200000001 (the first such prime above the gate, which must stay correct on the Shoup
kernels).  N = 2^16, negacyclic and cyclic.  Batches 7 and 17 (16 rows of one polynomial per ROW
tile) and 16 (the same row of 16 polynomials, the RP tiles with the staged LDS twiddles).

Inputs are synth_util.structured_batch (all q - 1, the pre-images that put every output on q - 1,
alternating 0 / q - 1, zero, lone q - 1, ones, then random polynomials), checked three ways as in
test_gpu_ntt_synthetic.py: forward against the oracle, inverse of the forward == the input,
inverse of the input against the oracle.

What this does not see: which kernels ran.  Both products give the same canonical residues, so
a dispatch that fell back to the Shoup kernels for a modulus under the gate would still pass;
that the MONT instantiations run for p63 is shown by the kernel names in the traces under
profiles/ (r07_mont_ab.txt), not here."""
import functools

import numpy as np
import pytest

import ringo
from tests import synth_util as su

pytestmark = pytest.mark.gpu

NS = len(su.STRUCTURED)
LOGN = 16
MODULI = {"p63": 47104 ** 4 + 1, "mont_tight": 0x47E0F66500000001, "shoup_above": 0x47E0F67200000001}


@functools.lru_cache(maxsize=None)
def _cfield(name):
    import coracle as co
    return co.CField(MODULI[name])


@functools.lru_cache(maxsize=2)
def _tables(name, cyclic):
    tabs = _cfield(name).tables(1 << LOGN, cyclic=cyclic)
    for t in tabs:
        t.setflags(write=False)
    return tabs


@pytest.mark.parametrize("batch", [7, 16, 17])
@pytest.mark.parametrize("negacyclic", [True, False], ids=["negacyclic", "cyclic"])
@pytest.mark.parametrize("name", list(MODULI))
def test_ntt_2e16_both_sides_of_the_mont_gate(name, negacyclic, batch):
    q = MODULI[name]
    N = 1 << LOGN
    F = ringo.Field(q)
    cf = _cfield(name)
    T = (ringo.CyclotomicTransformer if negacyclic else ringo.CyclicTransformer)(F, N)
    otw, otwi, oninv = tabs = _tables(name, not negacyclic)
    tw, twi, ninv = T.tables()
    assert (tw == otw).all() and (twi == otwi).all() and (ninv == oninv).all(), "tables"
    rng = np.random.default_rng(1000 * LOGN + batch)
    a = su.structured_batch(cf, q, N, tabs, batch, rng)
    want = cf.ntt_fwd(a, otw)
    want_inv = cf.ntt_inv(a, otwi, oninv)
    got = T.FwdNTTTo(None, a)
    back = T.InvNTTTo(None, got)
    got_inv = T.InvNTTTo(None, a)
    for what, g, w in (("fwd", got, want), ("inv roundtrip", back, a), ("inv", got_inv, want_inv)):
        bad = [i for i in range(batch) if not (g[i] == w[i]).all()]
        labels = [su.STRUCTURED[i] if i < NS else f"random{i - NS}" for i in bad]
        assert not bad, (name, "negacyclic" if negacyclic else "cyclic", batch, what, labels)
