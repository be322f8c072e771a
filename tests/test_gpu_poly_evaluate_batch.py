"""GPU: the batched Poly.Evaluate (rg_poly_evaluate_batch_dev / rg_poly_evaluate_batch,
math/bigpoly/poly.go:64-76 for every polynomial of a batch at one point) against the C oracle's
single Horner pass (oracle.c of_poly_evaluate) per polynomial, bit-exact, for every limb count, at
the sizes where a partial lane row, a partial tile and the one-tile / several-tile fold can each go
wrong, with a gap of non-elements between the polynomials that must never be read."""
import numpy as np
import pytest

import coracle as co
import ringo
from ringo import _lib, bigpoly

pytestmark = pytest.mark.gpu

T = 4096  # kEvalTile (csrc/poly_eval.hip): 256 lanes x kEvalK = 16 coefficients
FIELDS = ["p63", "mult_zp", "jindo_zp", "zp440", "zp880"]  # L = 1, 2, 4, 7, 14
SIZES = [0, 1, 2, 255, 256, 257, T - 1, T, T + 1, 2 * T + 3]
BIG = {"p63": (1 << 16) + 1, "mult_zp": (1 << 16) + 1, "jindo_zp": (1 << 16) + 1, "zp440": 1 << 16, "zp880": 1 << 16}
NPOLY, GAP = 5, 7
POISON = 0x5a5a5a5a5a5a5a5a


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to("cuda")


def _h(t):
    return t.cpu().numpy().view(np.uint64)


def _limbs(v, L):
    return np.array([(v >> (64 * j)) & ((1 << 64) - 1) for j in range(L)], np.uint64)


def _elements(q, L, shape, rng):
    """Uniform words below q: the top limb below q's top limb, the others free."""
    out = rng.integers(0, 1 << 63, size=shape + (L,), dtype=np.int64).astype(np.uint64) * np.uint64(2)
    out += rng.integers(0, 2, size=shape + (L,), dtype=np.int64).astype(np.uint64)
    top = q >> (64 * (L - 1))
    out[..., L - 1] = rng.integers(0, top, size=shape, dtype=np.uint64) if top > 1 else 0
    return out


_F, _CASE = {}, {}


def _field(name, fields):
    if name not in _F:
        q = fields[name]
        _F[name] = (q, ringo.Field(q), co.CField(q))
    return _F[name]


def _case(name, n, fields):
    """(points [5][L], buffer [NPOLY][n + GAP][L] with 0xFF.. gaps, want [5][NPOLY][L]), computed once:
    polynomial 1 has every coefficient q - 1, the others are random; the points are 0, 1, q - 1 and
    two random elements."""
    if (name, n) not in _CASE:
        q, F, cf = _field(name, fields)
        L = F.L
        rng = np.random.default_rng(1000 + n)
        buf = np.full((NPOLY, n + GAP, L), 0xFFFFFFFFFFFFFFFF, np.uint64)
        buf[:, :n] = _elements(q, L, (NPOLY, n), rng)
        buf[1, :n] = _limbs(q - 1, L)
        pts = np.stack([_limbs(0, L), _limbs(1, L), _limbs(q - 1, L)] + list(_elements(q, L, (2,), rng)))
        want = np.stack([np.stack([cf.evaluate(buf[b, :n], x) for b in range(NPOLY)]) for x in pts])
        _CASE[(name, n)] = (pts, buf, want)
    return _CASE[(name, n)]


def _run(name, n, fields, batches=(1, 3, 5)):
    import torch
    q, F, _ = _field(name, fields)
    L = F.L
    pts, buf, want = _case(name, n, fields)
    d_p, d_x = _t(buf), _t(pts)
    for batch in batches:
        scr = torch.full(((bigpoly.evaluate_batch_scratch_bytes(F, n, batch) + 7) // 8,), POISON, dtype=torch.int64,
                         device="cuda")
        for i in range(len(pts)):
            out = torch.full((batch + 1, L), POISON, dtype=torch.int64, device="cuda")
            bigpoly.evaluate_batch_dev(F, d_p, n, n + GAP, batch, d_x[i], out, scr)
            torch.cuda.synchronize()
            got = _h(out)
            assert (got[:batch] == want[i, :batch]).all(), (name, n, batch, i)
            assert (got[batch] == np.uint64(POISON)).all(), (name, n, batch, i, "wrote past d_out")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", FIELDS)
def test_evaluate_batch_matches_oracle(name, n, fields):
    _run(name, n, fields)


@pytest.mark.parametrize("name", FIELDS)
def test_evaluate_batch_2e16_matches_oracle(name, fields):
    """17 tiles with a one-coefficient last tile (L <= 4), 16 full tiles (the two largest fields)."""
    _run(name, BIG[name], fields, batches=(3,))


@pytest.mark.parametrize("name", FIELDS)
def test_evaluate_batch_host_form(name, fields):
    q, F, _ = _field(name, fields)
    n = T + 1
    pts, buf, want = _case(name, n, fields)
    polys = [bigpoly.Poly(F, n, coeffs=buf[b, :n]) for b in range(NPOLY)]
    assert (bigpoly.EvaluateBatch(polys, pts[3]) == want[3]).all()
    out = np.full((3, F.L), POISON, np.uint64)  # the strided host form: the gap is not read
    x = np.ascontiguousarray(pts[4])
    _lib.check(_lib.lib().rg_poly_evaluate_batch(F.h, _lib.ptr(buf), n, n + GAP, 3, _lib.ptr(x), _lib.ptr(out)))
    assert (out == want[4, :3]).all()
    z = np.full((2, F.L), POISON, np.uint64)  # n = 0 gives 0
    _lib.check(_lib.lib().rg_poly_evaluate_batch(F.h, None, 0, 0, 2, _lib.ptr(x), _lib.ptr(z)))
    assert (z == 0).all()


@pytest.mark.parametrize("name", FIELDS)
def test_evaluate_batch_equals_single_entry(name, fields):
    """rg_poly_evaluate_dev, one polynomial per call on the same device data, gives the same words."""
    import torch
    q, F, _ = _field(name, fields)
    L, n = F.L, 2 * T + 3
    pts, buf, want = _case(name, n, fields)
    d_p, d_x = _t(buf), _t(pts)
    scr = torch.zeros(((bigpoly.evaluate_batch_scratch_bytes(F, n, NPOLY) + 7) // 8,), dtype=torch.int64, device="cuda")
    out = torch.full((NPOLY, L), POISON, dtype=torch.int64, device="cuda")
    bigpoly.evaluate_batch_dev(F, d_p, n, n + GAP, NPOLY, d_x[4], out, scr)
    one = torch.full((NPOLY, L), POISON, dtype=torch.int64, device="cuda")
    s1 = torch.zeros((_lib.lib().rg_poly_evaluate_scratch_bytes(F.h, n) // 8 + 1,), dtype=torch.int64, device="cuda")
    for b in range(NPOLY):
        _lib.check(_lib.lib().rg_poly_evaluate_dev(F.h, d_p[b].data_ptr(), n, d_x[4].data_ptr(), one[b].data_ptr(),
                                                   s1.data_ptr(), None))
    torch.cuda.synchronize()
    assert (_h(out) == _h(one)).all() and (_h(out) == want[4]).all()
