"""GPU parity on the kernel variants the reference's eight fields never reach, and structured
extremal inputs on the ones they do: libringo's bigpoly NTT and vec ops vs the C oracle
(oracle/oracle.c), bit-exact.  The oracle is pinned on these moduli by test_oracle_synthetic.py.

Moduli: tests/golden/synthetic_fields.json (single-word primes off the q = 1 mod 2^32 shortcut,
a 63-bit prime with 3q > 2^64 for the lazy kernels, 64-bit primes that get no Shoup tables,
256 / 448 / 896-bit primes without a spare top bit) plus the reference's fields at the ranks
their special kernels start at.  Ranks are the smallest at which each dispatch branch can go
wrong ("Which modulus takes which NTT kernel"), not a sweep.

Every case compares the table triple first, then checks every polynomial of the batch three
ways: forward vs the oracle, inverse of the forward == the input, inverse of the (arbitrary)
input vs the oracle; cyclic and negacyclic.  The batch is synth_util.structured_batch: all
q - 1, the pre-images that put every output of the forward / inverse on q - 1, alternating
0 / q - 1, zero, a lone q - 1 at either end, all 1, then random polynomials."""
import numpy as np
import pytest

import ringo
from tests import synth_util as su

pytestmark = pytest.mark.gpu

NS = len(su.STRUCTURED)  # 8


def _case(name, logn, batch):
    return pytest.param(name, logn, batch, id=f"{name}-2e{logn}-b{batch}")


def _ntt_case(name, logn, negacyclic, batch, stream=False):
    q = su.modulus(name)
    N = 1 << logn
    F = ringo.Field(q)
    cf = su.cfield(name)
    T = (ringo.CyclotomicTransformer if negacyclic else ringo.CyclicTransformer)(F, N)
    otw, otwi, oninv = tabs = su.oracle_tables(name, logn, not negacyclic)
    tw, twi, ninv = T.tables()
    assert (tw == otw).all() and (twi == otwi).all() and (ninv == oninv).all(), "tables"
    rng = np.random.default_rng(1000 * logn + batch)
    a = su.structured_batch(cf, q, N, tabs, batch, rng)
    want = cf.ntt_fwd(a, otw)
    want_inv = cf.ntt_inv(a, otwi, oninv)
    if stream:  # device-resident entry points on a side stream, out of place then in place
        import torch
        side = torch.cuda.Stream()
        x = torch.from_numpy(a.view(np.int64).reshape(-1).copy()).cuda()
        y = torch.empty_like(x)
        torch.cuda.synchronize()
        T.fwd_dev(y, x, batch, stream=side)
        T.inv_dev(x, y, batch, stream=side)
        side.synchronize()
        got = y.cpu().numpy().view(np.uint64).reshape(a.shape)
        back = x.cpu().numpy().view(np.uint64).reshape(a.shape)
        x.copy_(torch.from_numpy(a.view(np.int64).reshape(-1)))
        torch.cuda.synchronize()
        T.inv_dev(x, x, batch, stream=side)
        side.synchronize()
        got_inv = x.cpu().numpy().view(np.uint64).reshape(a.shape)
    else:
        got = T.FwdNTTTo(None, a)
        back = T.InvNTTTo(None, got)
        got_inv = T.InvNTTTo(None, a)
    for what, g, w in (("fwd", got, want), ("inv roundtrip", back, a), ("inv", got_inv, want_inv)):
        bad = [i for i in range(batch) if not (g[i] == w[i]).all()]
        labels = [su.STRUCTURED[i] if i < NS else f"random{i - NS}" for i in bad]
        assert not bad, (name, logn, "negacyclic" if negacyclic else "cyclic", what, labels)


# ---- L = 1 -------------------------------------------------------------------------------------
# logN 1, 5: per-stage kernels; 6, 12: the smallest and largest single tiled pass (pmax_of(1) =
# 12); 13: the first two-pass plan (6 + 7); 16: 8 + 8 -- ntt_r8 (Shoup fields; QLO1 = false for
# s30 / s62_lo), ntt_r2 with the register prefetch (the 64-bit Montgomery fields), and for
# s63_top the lazy ntt16_pass, at batches 7 and 17 (16 rows of one polynomial per ROW tile), 16
# (the same row of 16 polynomials) -- 17 also being the first batch past the polys % 16 boundary.
L1 = ["s30", "s62_lo", "s63_top", "s64_gold", "s64_lo"]
L1_CASES = [_case(n, lg, NS + 2) for n in L1 for lg in (1, 5, 6, 12, 13)]
L1_CASES += [_case(n, 16, NS + 1) for n in L1 if n != "s63_top"]
L1_CASES += [_case("s63_top", 16, b) for b in (7, 16, 17)]


@pytest.mark.parametrize("negacyclic", [True, False], ids=["negacyclic", "cyclic"])
@pytest.mark.parametrize("name,logn,batch", L1_CASES)
def test_ntt_single_word_fields(name, logn, batch, negacyclic):
    _ntt_case(name, logn, negacyclic, batch)


# ---- L = 2: the 8 + 8 plan (ntt_r2 without prefetch), with and without a spare bit --------------
@pytest.mark.parametrize("negacyclic", [True, False], ids=["negacyclic", "cyclic"])
@pytest.mark.parametrize("name,logn,batch", [_case("mult_zp", 16, NS + 1), _case("zp110", 16, NS + 1)])
def test_ntt_two_limb_fields_2e16(name, logn, batch, negacyclic):
    _ntt_case(name, logn, negacyclic, batch)


# ---- L = 1, 2 at 2^8 with batch % 16 == 0 -------------------------------------------------------
# run_tiled sends a P = 8 pass with 16 | sub-transforms to the 8-stage kernels: at N = 2^8 that is
# the whole transform in one ROW pass, the only shape where ntt_r8 / ntt_r2 run ROW with G0 = 0 and
# so fuse the N^-1 scaling (SCALE) -- any other batch takes ntt_pass_kernel<L, 8>.
@pytest.mark.parametrize("negacyclic", [True, False], ids=["negacyclic", "cyclic"])
@pytest.mark.parametrize("name,logn,batch", [_case(n, 8, 16) for n in ("p63", "s62_lo", "s64_lo", "zp110", "mult_zp")])
def test_ntt_2e8_batch16_single_row_pass(name, logn, batch, negacyclic):
    _ntt_case(name, logn, negacyclic, batch)


# ---- L = 4: generic CIOS plan -------------------------------------------------------------------
# pmax_of(4) = 11: logN 5 stage kernels, 6 and 11 single pass, 12 the first two-pass plan, 15 and
# 16 the ranks ntt256_run takes for q255 and must decline here (top bit set, or q[0] != 1).
L4_CASES = [_case(n, lg, NS + 2 if lg <= 12 else NS + 1) for n in ("s256_top", "s256_lo") for lg in (5, 6, 11, 12, 15, 16)]
L4_CASES += [_case("bfv_zp", lg, NS + 1) for lg in (15, 16)]


@pytest.mark.parametrize("negacyclic", [True, False], ids=["negacyclic", "cyclic"])
@pytest.mark.parametrize("name,logn,batch", L4_CASES)
def test_ntt_four_limb_generic_plan(name, logn, batch, negacyclic):
    _ntt_case(name, logn, negacyclic, batch)


# ---- L = 4: the ntt256 fast path with a modulus other than q255 ---------------------------------
# zp220 (q[0] == 1, 220 bits): batches 3 (4-rows-of-one-poly ROW tiling), 4 (same row of 4
# polys), 8 (two-stream split 4 + 4) and 9 (4 + 5: an uneven second half on the other tiling).
@pytest.mark.parametrize("negacyclic", [True, False], ids=["negacyclic", "cyclic"])
@pytest.mark.parametrize("name,logn,batch", [_case("zp220", lg, b) for lg in (15, 16) for b in (3, 4, 8, 9)])
def test_ntt_zp220_fast_path(name, logn, batch, negacyclic):
    _ntt_case(name, logn, negacyclic, batch)


@pytest.mark.parametrize("negacyclic", [True, False], ids=["negacyclic", "cyclic"])
@pytest.mark.parametrize("name,logn,batch", [_case("zp220", lg, 9) for lg in (15, 16)])
def test_ntt_zp220_fast_path_side_stream(name, logn, batch, negacyclic):
    _ntt_case(name, logn, negacyclic, batch, stream=True)


# ---- L = 7, 14 without a spare bit: run_stages<L, false> at every rank --------------------------
WIDE_CASES = [_case("s448_top", lg, NS + (2 if lg < 16 else 0)) for lg in (3, 9, 16)]
WIDE_CASES += [_case("s896_top", lg, NS + 2) for lg in (3, 9, 13)]


@pytest.mark.parametrize("negacyclic", [True, False], ids=["negacyclic", "cyclic"])
@pytest.mark.parametrize("name,logn,batch", WIDE_CASES)
def test_ntt_wide_fields_without_spare_bit(name, logn, batch, negacyclic):
    _ntt_case(name, logn, negacyclic, batch)


# ---- the existing special kernels, on the structured batch, at the smallest batch reaching them -
# p63 at 2^16: ntt16_pass, batch 16 (same row of 16 polys) and 9 (16 rows of one poly);
# jindo_zp: ntt256_pass at 2^15 / 2^16, batch 8 (split 4 + 4); zp440 / zp880: ntt_wide_pass, one
# pass below 2^9, two from 2^9 up to 2^16.
SPECIAL_CASES = [_case("p63", 16, 16), _case("p63", 16, NS + 1), _case("jindo_zp", 15, 8), _case("jindo_zp", 16, 8),
                 _case("zp440", 9, NS + 2), _case("zp440", 16, NS), _case("zp880", 9, NS + 2), _case("zp880", 16, NS)]


@pytest.mark.parametrize("negacyclic", [True, False], ids=["negacyclic", "cyclic"])
@pytest.mark.parametrize("name,logn,batch", SPECIAL_CASES)
def test_ntt_special_kernels_structured_inputs(name, logn, batch, negacyclic):
    _ntt_case(name, logn, negacyclic, batch)


# ---- vec ops ------------------------------------------------------------------------------------
OPS = ["add", "sub", "neg", "mul", "smul", "mul_add", "mul_sub", "smul_add", "smul_sub"]


@pytest.mark.parametrize("name", sorted(su.SYNTH))
def test_vec_ops_match_oracle_synthetic(name):
    """All nine ops over every synthetic prime, n = 4099 as test_vec_ops_match_oracle.  The
    front block holds every ordered TRIPLE (out, x, y) of synth_util.edge_values (at most 11^3 =
    1331 elements), so the *_add / *_sub forms see every edge value in `out` against every edge
    product; the smul* forms run once per edge value as the scalar.  The rest is random."""
    q = su.modulus(name)
    F = ringo.Field(q)
    cf = su.cfield(name)
    L = F.L
    rng = np.random.default_rng(7)
    n = 4099
    E = np.stack([su.limbs_of(v, L) for v in su.edge_values(q, L)])
    k = len(E)
    assert k ** 3 <= n
    idx = np.arange(k ** 3)
    a = su.rand_residues(q, L, n, rng)
    b = su.rand_residues(q, L, n, rng)
    base0 = su.rand_residues(q, L, n, rng)
    base0[:k ** 3] = E[idx // (k * k)]
    a[:k ** 3] = E[(idx // k) % k]
    b[:k ** 3] = E[idx % k]
    for op in OPS:
        scalars = [np.ascontiguousarray(e) for e in E] if op.startswith("smul") else [None]
        for c in scalars:
            bb = b if c is None else c
            want = base0.copy()
            got = base0.copy()
            cf.vec(op, want, a, bb)
            ringo._lib.check(ringo.lib().rg_vec(F.h, ringo.bigpoly._OPS[op], ringo._lib.ptr(got), ringo._lib.ptr(a),
                                                ringo._lib.ptr(bb), n))
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, (name, op, None if c is None else [hex(int(w)) for w in c], bad[:8])
