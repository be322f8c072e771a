"""GPU: the batched Poly.Evaluate with a point per group of polynomials (rg_poly_evaluate_multi_dev /
rg_poly_evaluate_multi) and the power tables of several bases (rg_buckler_powers_batch*), against Python
integers: polynomial b at point (b // group) % n_points equals sum(p_i x^i) % q, bit for bit, at the
sizes where a partial lane row, a partial tile and the one-tile / several-tile fold can each go wrong,
with a gap of -1 words between the polynomials and between the points that must never be read."""
import numpy as np
import pytest

import coracle as co
import ringo
from ringo import _lib, bigpoly, buckler
from ringo.bigpoly import RingoPanic

pytestmark = pytest.mark.gpu

FIELDS = ["p63", "jindo_zp", "zp880"]  # L = 1, 4, 14
SIZES = [0, 1, 255, 256, 257, 4096, 4097, 8193]
# (batch, group, n_points): (6, 1, 3) wraps round the points, (5, 2, 3) ends in a short group
SHAPES = [(6, 2, 3), (6, 1, 3), (5, 2, 3), (4, 4, 1), (3, 1, 3)]
NPOLY, NPTS, GAP = 6, 3, 5
FF = 0xFFFFFFFFFFFFFFFF

_F, _CASE = {}, {}


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to("cuda")


def _h(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def _field(name, fields):
    if name not in _F:
        q = fields[name]
        _F[name] = (q, ringo.Field(q))
    return _F[name]


def _rand(q, n, rng):
    nb = (q.bit_length() + 7) // 8 + 8
    return [int.from_bytes(rng.bytes(nb), "little") % q for _ in range(n)]


def _horner(p, x, q, Rinv):
    """sum p_i x^i in the Montgomery domain: every product carries one R^-1, as Poly.Evaluate's does."""
    z = 0
    for c in reversed(p):
        z = (z * x * Rinv + c) % q
    return z


def _case(name, n, fields):
    """Six polynomials of n coefficients and the point sets, as Montgomery-form integers, with every
    polynomial's value at every point, computed once.  Point set 0 is (0, 1, q - 1) as residues,
    point set 1 three random, pairwise different elements."""
    if (name, n) not in _CASE:
        q, F = _field(name, fields)
        rng = np.random.default_rng(7000 + n)
        Rinv = pow(1 << (64 * F.L), -1, q)
        polys = [_rand(q, n, rng) for _ in range(NPOLY)]
        if n:
            polys[1] = [q - 1] * n
        one = (1 << (64 * F.L)) % q
        sets = [[0, one, q - 1], _rand(q, NPTS, rng)]
        assert len(set(sets[0] + sets[1])) == 2 * NPTS
        want = [[[_horner(p, x, q, Rinv) for x in pts] for p in polys] for pts in sets]
        _CASE[(name, n)] = (polys, sets, want)
    return _CASE[(name, n)]


def _buffers(F, polys, pts, n, x_stride):
    L = F.L
    buf = np.full((NPOLY, n + GAP, L), FF, np.uint64)
    if n:
        buf[:, :n] = np.stack([co.to_limbs(p, L) for p in polys])
    xs = np.full((NPTS, x_stride, L), FF, np.uint64)
    xs[:, 0] = co.to_limbs(pts, L)
    return buf, xs


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", FIELDS)
def test_evaluate_multi_matches_python_integers(name, n, fields):
    import torch
    q, F = _field(name, fields)
    L = F.L
    polys, sets, want = _case(name, n, fields)
    for s, pts in enumerate(sets):
        for x_stride in (1, 5):
            buf, xs = _buffers(F, polys, pts, n, x_stride)
            d_p, d_x = _t(buf), _t(xs)
            for batch, group, n_points in SHAPES:
                scr = torch.full(((bigpoly.evaluate_multi_scratch_bytes(F, n, batch, n_points) + 7) // 8,), -1,
                                 dtype=torch.int64, device="cuda")
                out = torch.full((batch + 1, L), -1, dtype=torch.int64, device="cuda")
                bigpoly.evaluate_multi_dev(F, d_p, n, n + GAP, batch, d_x, x_stride, n_points, group, out, scr)
                got = _h(out)
                exp = co.to_limbs([want[s][b][(b // group) % n_points] for b in range(batch)], L)
                assert (got[:batch] == exp).all(), (name, n, s, x_stride, batch, group, n_points)
                assert (got[batch] == np.uint64(FF)).all(), "wrote past d_out"


@pytest.mark.parametrize("name", FIELDS)
def test_one_point_equals_the_batch_entry(name, fields):
    """n_points = 1 gives the limbs of rg_poly_evaluate_batch_dev, whatever the group."""
    import torch
    q, F = _field(name, fields)
    L = F.L
    for n in (257, 8193):
        polys, sets, want = _case(name, n, fields)
        buf, xs = _buffers(F, polys, sets[1], n, 1)
        d_p, d_x = _t(buf), _t(xs)
        scr = torch.zeros(((bigpoly.evaluate_batch_scratch_bytes(F, n, NPOLY) + 7) // 8,), dtype=torch.int64,
                          device="cuda")
        assert bigpoly.evaluate_multi_scratch_bytes(F, n, NPOLY, 1) == bigpoly.evaluate_batch_scratch_bytes(F, n, NPOLY)
        ref = torch.full((NPOLY, L), -1, dtype=torch.int64, device="cuda")
        bigpoly.evaluate_batch_dev(F, d_p, n, n + GAP, NPOLY, d_x[0], ref, scr)
        for group in (1, 4, NPOLY, 100):
            out = torch.full((NPOLY, L), -1, dtype=torch.int64, device="cuda")
            bigpoly.evaluate_multi_dev(F, d_p, n, n + GAP, NPOLY, d_x, 1, 1, group, out, scr)
            assert (_h(out) == _h(ref)).all(), (name, n, group)
        assert (_h(ref) == co.to_limbs([want[1][b][0] for b in range(NPOLY)], L)).all()


@pytest.mark.parametrize("name", FIELDS)
def test_host_form_and_mirror(name, fields):
    q, F = _field(name, fields)
    L, n = F.L, 4097
    polys, sets, want = _case(name, n, fields)
    P = [bigpoly.Poly(F, n, coeffs=co.to_limbs(p, L)) for p in polys]
    got = bigpoly.EvaluateMulti(P, co.to_limbs(sets[1], L), 2)
    assert (got == co.to_limbs([want[1][b][(b // 2) % NPTS] for b in range(NPOLY)], L)).all()
    buf, xs = _buffers(F, polys, sets[0], n, 5)  # the strided host form: the gaps are not read
    out = np.full((5, L), FF, np.uint64)
    _lib.check(_lib.lib().rg_poly_evaluate_multi(F.h, _lib.ptr(buf), n, n + GAP, 5, _lib.ptr(xs), 5, 3, 2,
                                                 _lib.ptr(out)))
    assert (out == co.to_limbs([want[0][b][(b // 2) % 3] for b in range(5)], L)).all()


def test_refusals(fields):
    """group, n_points or x_stride of 0, and what the batch entry refuses; the addresses are made up."""
    q, F = _field("p63", fields)
    lib = _lib.lib()
    A = [0x10000 * (i + 1) for i in range(4)]
    call = lambda **kw: lib.rg_poly_evaluate_multi_dev(  # noqa: E731
        F.h, A[0], kw.get("n", 8), kw.get("stride", 8), kw.get("batch", 4), A[1], kw.get("x_stride", 1),
        kw.get("n_points", 2), kw.get("group", 2), A[2], kw.get("scratch", A[3]), None)
    for kw in (dict(group=0), dict(n_points=0), dict(x_stride=0), dict(stride=7), dict(scratch=None),
               dict(n_points=1 << 20, group=1, batch=1 << 20), dict(group=0, batch=0)):
        assert call(**kw) == -1, kw
    assert call(batch=0) == 0
    assert lib.rg_poly_evaluate_multi_dev(None, A[0], 8, 8, 4, A[1], 1, 2, 2, A[2], A[3], None) == -1
    with pytest.raises(RingoPanic):
        bigpoly.evaluate_multi_dev(F, A[0], 8, 8, 4, A[1], 1, 2, 0, A[2], A[3])
    for args in ((A[0], 0, 3, 4, A[1]), (A[0], 1, 1 << 16, 4, A[1]), (A[0], 1, 3, 4, A[0]), (None, 1, 3, 4, A[1])):
        assert lib.rg_buckler_powers_batch_dev(F.h, *args, None) == -1, args
    assert lib.rg_buckler_powers_batch_dev(F.h, A[0], 1, 0, 4, A[1], None) == 0


@pytest.mark.parametrize("name", FIELDS)
def test_powers_batch_matches_pow(name, fields):
    """out[k][i] = c_k^i against pow(c, i, q) for three bases, 0 and 1 among them, c_stride 1 and 5."""
    import torch
    q, F = _field(name, fields)
    L = F.L
    R = 1 << (64 * L)
    rng = np.random.default_rng(11)
    plain = [0, 1, _rand(q, 1, rng)[0]]  # the bases as residues
    mont = [c * R % q for c in plain]
    for n in (1, 16, 17, 257):
        exp = np.stack([co.to_limbs([pow(c, i, q) * R % q for i in range(n)], L) for c in plain])
        for c_stride in (1, 5):
            cs = np.full((3, c_stride, L), FF, np.uint64)
            cs[:, 0] = co.to_limbs(mont, L)
            got = buckler.PowersBatch(F, cs.reshape(-1, L)[:2 * c_stride + 1], n, c_stride)
            assert got.shape == (3, n, L) and (got == exp).all(), (name, n, c_stride, "host")
            out = torch.full((3 * n + 1, L), -1, dtype=torch.int64, device="cuda")
            buckler.powers_batch_dev(F, _t(cs), c_stride, 3, n, out)
            h = _h(out)
            assert (h[:3 * n].reshape(3, n, L) == exp).all(), (name, n, c_stride, "dev")
            assert (h[3 * n] == np.uint64(FF)).all(), "wrote past d_out"
        one = buckler.Powers(F, co.to_limbs(mont[2:], L)[0], n)
        assert (one == exp[2]).all()
