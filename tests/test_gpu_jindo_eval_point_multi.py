"""GPU: the evaluation points of a batch of proofs in one call (rg_jindo_eval_point_multi_dev:
encode(leftVec(x_k)) and rightVec(x_k) for n_points points, jindo/utils.go:63-82 with
encoder.go:105-146), bit-exact against the C oracle (tests/jindo_proto.left_right, CJindo.encode) and,
word for word, against the single entry rg_jindo_eval_point_dev on each point alone, over the
parameter sets of test_gpu_jindo_eval_point.py (d 8 to 1024, one to four ring primes, L 1 to 14, an
odd exp, rows 3 to 65).

Every output and the scratch are poison words before a call and poison words follow every output,
so a word nobody wrote and a write past an end both show; the points lie in a poisoned buffer too, so
a wrong stride reads poison, not a neighbour."""
import numpy as np
import pytest

import coracle as co
from ringo import _lib, jindo
from tests import jindo_synth_util as su
from tests.jindo_proto import left_right, mont, random_ck

pytestmark = pytest.mark.gpu

NAMES = ["syn_d8_p63", "syn_d128_mixed4", "syn_b7000_e5_p63", "syn_d1024_mult", "syn_d256_q62top", "t10_b8",
         "p63_t10_b2", "zp880_t10_b1"]
POISON = 0x5a5a5a5a5a5a5a5a
GUARD = 8
INVALID = _lib.STATUS["RG_ERR_INVALID"]


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to("cuda")


def _h(t):
    return t.cpu().numpy().view(np.uint64)


_SET = {}


def _setup(name):
    if name not in _SET:
        P, fq = su.params(name)
        params = jindo.Parameters.from_dict(P, fq)
        _SET[name] = (P, fq, params, jindo.Verifier(params, ck=random_ck(P, 7)), co.CJindo(P, fq), co.CField(fq))
    return _SET[name]


def _oracle(name, xs):
    """(left [n][rows][nq][d], right [n][cs][L]) of the Montgomery ints xs, by the oracle."""
    P, fq, params, vrf, cj, F = _setup(name)
    L = params.L
    lefts, rights = [], []
    for x in xs:
        left_e, right_e = left_right(P, F, x)
        lefts.append(np.stack([cj.encode(co.to_limbs([e], L)) for e in left_e]))
        rights.append(co.to_limbs(right_e, L))
    return np.stack(lefts), np.stack(rights)


_CASE = {}


def _case(name):
    """The set's five points 0, 1, q - 1 and two random elements, with the oracle's vectors; computed once."""
    if name not in _CASE:
        P, fq, params, vrf, cj, F = _setup(name)
        rng = np.random.default_rng(91)
        xs = [0, mont(F, 1), mont(F, fq - 1)] + [mont(F, int.from_bytes(rng.bytes(120), "little")) for _ in range(2)]
        _CASE[name] = (xs,) + _oracle(name, xs)
    return _CASE[name]


def _points(params, xs, stride):
    """The points at element k * stride of a poisoned device buffer of len(xs) * stride elements."""
    buf = np.full((len(xs) * stride, params.L), POISON, np.uint64)
    buf[::stride] = co.to_limbs(xs, params.L)
    return _t(buf)


class _Out:
    """left | guard | right | guard | scratch | guard in one poisoned buffer."""

    def __init__(self, P, params, vrf, n):
        import torch
        self.lw, self.rw = n * P["rows"] * params.nq * P["d"], n * P["cols"] * P["slots"] * params.L
        nbytes = vrf.eval_point_multi_scratch_bytes(n)
        assert nbytes > 0 and nbytes % 8 == 0
        self.sw = nbytes // 8
        self.buf = torch.full((self.lw + self.rw + self.sw + 3 * GUARD,), POISON, dtype=torch.int64, device="cuda")
        a = self.lw + GUARD
        b = a + self.rw + GUARD
        self.left, self.right, self.scratch = self.buf[:self.lw], self.buf[a:a + self.rw], self.buf[b:b + self.sw]
        self.guards = [self.buf[self.lw:a], self.buf[a + self.rw:b], self.buf[b + self.sw:]]

    def guards_intact(self):
        return all((_h(g) == np.uint64(POISON)).all() for g in self.guards)

    def all_poison(self):
        return bool((_h(self.buf) == np.uint64(POISON)).all())


def _run(name, xs, stride, right=True, stream=None):
    """One eval_point_multi_dev on the points; returns the buffers without synchronising."""
    P, fq, params, vrf, cj, F = _setup(name)
    o = _Out(P, params, vrf, len(xs))
    d_x = _points(params, xs, stride)
    assert vrf.eval_point_multi_dev(len(xs), d_x, stride, o.left, o.right if right else None, o.scratch,
                                    stream=stream) is None
    return o, d_x


_SINGLE = {}


def _single(name):
    """rg_jindo_eval_point_dev on each of the set's five points alone: (left [5][...], right [5][...])."""
    if name not in _SINGLE:
        import torch
        P, fq, params, vrf, cj, F = _setup(name)
        xs, want_left, want_right = _case(name)
        ls, rs = [], []
        for x in xs:
            left = torch.full(want_left[0].shape, POISON, dtype=torch.int64, device="cuda")
            right = torch.full(want_right[0].shape, POISON, dtype=torch.int64, device="cuda")
            vrf.eval_point_dev(_t(co.to_limbs([x], params.L)[0]), left, right)
            torch.cuda.synchronize()
            ls.append(_h(left))
            rs.append(_h(right))
        _SINGLE[name] = (np.stack(ls), np.stack(rs))
    return _SINGLE[name]


@pytest.mark.parametrize("stride", [1, 5])
@pytest.mark.parametrize("name", NAMES)
def test_points_match_oracle_and_single_entry(name, stride):
    import torch
    xs, want_left, want_right = _case(name)
    one_left, one_right = _single(name)
    assert (one_left == want_left).all() and (one_right == want_right).all()
    o, _ = _run(name, xs, stride)
    torch.cuda.synchronize()
    got_left, got_right = _h(o.left).reshape(want_left.shape), _h(o.right).reshape(want_right.shape)
    for k in range(len(xs)):
        assert (got_left[k] == want_left[k]).all(), (name, stride, k, "left")
        assert (got_right[k] == want_right[k]).all(), (name, stride, k, "right")
        assert (got_left[k] == one_left[k]).all() and (got_right[k] == one_right[k]).all(), (name, stride, k)
        assert (got_left[k, -1] == want_left[k, -1]).all()  # left[rows - 1] = encode(x)
    assert o.guards_intact(), (name, stride, "wrote past an output")


@pytest.mark.parametrize("name", NAMES)
def test_right_null_leaves_right_untouched(name):
    import torch
    xs, want_left, _ = _case(name)
    o, _ = _run(name, xs, 5, right=False)
    torch.cuda.synchronize()
    assert (_h(o.left).reshape(want_left.shape) == want_left).all(), name
    assert (_h(o.right) == np.uint64(POISON)).all(), (name, "d_right = NULL was written")
    assert o.guards_intact(), name


@pytest.mark.parametrize("name", NAMES)
def test_one_point_equals_the_single_entry(name):
    import torch
    xs, _, _ = _case(name)
    one_left, one_right = _single(name)
    o, _ = _run(name, xs[4:], 1)
    torch.cuda.synchronize()
    assert (_h(o.left).reshape(one_left[4].shape) == one_left[4]).all(), name
    assert (_h(o.right).reshape(one_right[4].shape) == one_right[4]).all(), name
    assert o.guards_intact(), name


def test_three_hundred_points():
    """A point index above 255 (rows 3, d 8): every point against the oracle."""
    import torch
    name = "syn_d8_p63"
    P, fq, params, vrf, cj, F = _setup(name)
    rng = np.random.default_rng(300)
    xs = [mont(F, int.from_bytes(rng.bytes(16), "little")) for _ in range(300)]
    assert len(set(xs)) == 300
    want_left, want_right = _oracle(name, xs)
    o, _ = _run(name, xs, 1)
    torch.cuda.synchronize()
    got_left, got_right = _h(o.left).reshape(want_left.shape), _h(o.right).reshape(want_right.shape)
    bad = [k for k in range(300) if not ((got_left[k] == want_left[k]).all() and (got_right[k] == want_right[k]).all())]
    assert not bad, bad[:8]
    assert o.guards_intact()


def test_two_streams_with_separate_scratch():
    import torch
    name = "syn_d128_mixed4"
    xs, want_left, want_right = _case(name)
    P, fq, params, vrf, cj, F = _setup(name)
    oa, ob = _Out(P, params, vrf, 5), _Out(P, params, vrf, 5)
    xa, xb = _points(params, xs, 1), _points(params, xs[::-1], 5)
    torch.cuda.synchronize()  # the uploads and the poison fills ran on the null stream
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    vrf.eval_point_multi_dev(5, xa, 1, oa.left, oa.right, oa.scratch, stream=s1)
    vrf.eval_point_multi_dev(5, xb, 5, ob.left, ob.right, ob.scratch, stream=s2)
    torch.cuda.synchronize()
    for o, wl, wr in ((oa, want_left, want_right), (ob, want_left[::-1], want_right[::-1])):
        assert (_h(o.left).reshape(wl.shape) == wl).all() and (_h(o.right).reshape(wr.shape) == wr).all()
        assert o.guards_intact()


def test_refusals_leave_every_buffer_untouched():
    import torch
    name = "t10_b8"
    P, fq, params, vrf, cj, F = _setup(name)
    xs, want_left, want_right = _case(name)
    lib = _lib.lib()
    o = _Out(P, params, vrf, 5)
    d_x = _points(params, xs, 5)
    ptr = dict(n=5, x=d_x.data_ptr(), stride=5, left=o.left.data_ptr(), right=o.right.data_ptr(),
               scratch=o.scratch.data_ptr())

    def call(**kw):
        a = dict(ptr, **kw)
        return lib.rg_jindo_eval_point_multi_dev(vrf.h, a["n"], a["x"], a["stride"], a["left"], a["right"], a["scratch"],
                                                 None)

    cases = [dict(stride=0), dict(n=65536), dict(scratch=ptr["left"]), dict(scratch=None), dict(left=None), dict(x=None),
             dict(right=ptr["left"] + 8), dict(left=ptr["x"]), dict(scratch=ptr["x"] + 8 * 5 * params.L)]
    for kw in cases:
        assert call(**kw) == INVALID, kw
        assert "jindo eval point multi" in lib.rg_last_error().decode(), kw
    assert call(n=0) == 0  # nothing to do, nothing touched
    assert vrf.eval_point_multi_scratch_bytes(0) == 0
    assert vrf.eval_point_multi_scratch_bytes(65536) == 0
    assert vrf.eval_point_multi_scratch_bytes(65535) > 0
    torch.cuda.synchronize()
    assert o.all_poison()
    assert call() == 0  # the same arguments, unchanged, are accepted
    torch.cuda.synchronize()
    assert (_h(o.left).reshape(want_left.shape) == want_left).all()
    assert (_h(o.right).reshape(want_right.shape) == want_right).all()
    assert o.guards_intact()
