"""GPU parity: the Buckler norm decomposition on the device (rg_buckler_dcmp_*; buckler/utils.go:34-56,
buckler/prover.go:77-111, 182-192), bit-exact against tests/buckler_dcmp_ref.py (pinned on the CPU by
test_buckler_dcmp_ref.py), through the `_dev` entry points into buffers pre-filled with -1 and through
the host forms of the Python mirror."""
import ctypes
import functools
import math

import numpy as np
import pytest

import ringo
from ringo import _lib, buckler
from ringo.bigpoly import RingoPanic
from tests import buckler_dcmp_ref as D
from tests import buckler_lin_ref as R
from tests import synth_util as su
from tests.buckler_lin_util import rand_ints

pytestmark = pytest.mark.gpu

GOLD = ["p63", "mult_zp", "jindo_zp", "zp440", "zp880"]
# synthetic moduli with no spare top bit and a supported limb count: where q - x and the compare
# with q >> 1 use every bit of the top limb
NOSPARE = sorted(k for k, v in su.SYNTH.items() if v["bits"] == 64 * v["limbs"] and v["limbs"] in (1, 2, 4, 7, 14))
FIELDS = GOLD + NOSPARE
INVALID = -1


@functools.lru_cache(maxsize=None)
def _ctx(key):
    q = su.modulus(key)
    return ringo.Field(q), R.Ref(q)


@functools.lru_cache(maxsize=None)
def _base(bound):
    """Bound 1 stands for the base [1] (decomposeBase(1) panics in the reference)."""
    return tuple([1] if bound == 1 else D.decomposeBase(bound))


def _bounds(L):
    b = [1, 2, 3, 8, 1000, (1 << 20) - 1]
    if L >= 2:
        b += [1 << 64, (1 << 64) + 1, (1 << 65) - 1]  # the compare and the borrow cross a limb
    return b


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


def _filled(*shape):
    import torch
    return torch.full(shape, -1, dtype=torch.int64, device="cuda")


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def _scratch(nbytes):
    import torch
    return torch.empty(max(1, nbytes // 8), dtype=torch.int64, device="cuda")


def _plain_inputs(q, base, n, rng):
    """n plain values: 0, 1, q - 1, q >> 1 and its successor, +-b_j and +-(b_j - 1) for every j,
    +-sum(base) and one beyond, then seeded random values within the bound and over the whole
    field.  When the edge values alone outnumber n, a seeded choice of them."""
    S = sum(base)
    edges = [0, 1, q - 1, q >> 1, (q >> 1) + 1, S, -S, S + 1, -S - 1]
    for b in base:
        edges += [b, -b, b - 1, 1 - b]
    if len(edges) >= n:
        return [edges[i] % q for i in rng.choice(len(edges), size=n, replace=False)]
    nr = n - len(edges)
    nbytes = (q.bit_length() + 7) // 8 + 8
    inb = [int.from_bytes(rng.bytes(nbytes), "little") % (2 * S + 1) - S for _ in range(nr // 2)]
    return [v % q for v in edges + inb + rand_ints(q, nr - len(inb), rng)]


def _limbs_of_digits(ref, vecs):
    """The restated digit witnesses (lists of Montgomery ints, each 0, R or q - R) as limbs,
    through a three-entry table instead of a big-int conversion per element."""
    vals = [0, D.set_int64(ref, 1), D.set_int64(ref, -1)]
    lut = {v: i for i, v in enumerate(vals)}
    idx = np.array([[lut[x] for x in v] for v in vecs], np.int64)
    return ref.arr(vals)[idx]


def _inf_case(F, ref, dc, base, rank, rng):
    """Batch 3 and batch 1 through inf_dev, against infDcmp of each witness; returns (w ints, want)."""
    q = ref.q
    plain = _plain_inputs(q, base, 3 * rank, rng)
    w = [p * ref.R % q for p in plain]
    want = np.stack([_limbs_of_digits(ref, D.infDcmp(ref, w[k * rank:(k + 1) * rank], base)) for k in range(3)])
    dw = _dev(ref.arr(w).reshape(3, rank, F.L))
    for batch in (3, 1):
        out = _filled(batch, len(base), rank, F.L)
        dc.inf_dev(out, dw, batch, rank)
        assert (_host(out) == want[:batch]).all(), (rank, batch, base[:2])
    return w, want


@pytest.mark.parametrize("key", FIELDS)
@pytest.mark.parametrize("rank", [8, 128, 200, 4096])
def test_inf_matches_restatement(key, rank):
    """Rank 8: less than a wave; 200: a partial workgroup; 4096: 16 workgroups per witness.  Every
    bound runs at the three small ranks; the code has one path for every rank, so at 4096 (where
    the restatement costs seconds) three bounds do: base [1], 1000 and, for L >= 2, 2^64 + 1."""
    F, ref = _ctx(key)
    rng = np.random.default_rng(rank)
    bounds = _bounds(F.L) if rank < 4096 else [1, 1000] + ([(1 << 64) + 1] if F.L >= 2 else [])
    for bound in bounds:
        base = list(_base(bound))
        dc = buckler.Decomposer(F, base)
        w, want = _inf_case(F, ref, dc, base, rank, rng)
        if rank == 200:  # the host form, one witness and a batch
            assert (dc.DecomposeInf(ref.arr(w[:rank])) == want[0]).all()
            assert (dc.DecomposeInf(ref.arr(w).reshape(3, rank, F.L)) == want).all()


@pytest.mark.parametrize("key", ["p63", "jindo_zp"])
def test_inf_bound_q_minus_1(key):
    """decomposeBase(q - 1): nb = the bit length of q, the first base element about q / 2."""
    F, ref = _ctx(key)
    base = list(_base(ref.q - 1))
    assert len(base) == ref.q.bit_length() and base[0] == ref.q >> 1
    dc = buckler.Decomposer(F, ref.q - 1)
    assert dc.dcmpBase == base
    for rank in (8, 200):
        _inf_case(F, ref, dc, base, rank, np.random.default_rng(rank))


def test_inf_unaligned_output_and_saturated_base():
    """An output at an odd word offset takes the one-word stores; a base element of 2^(64L) or more
    is stored saturated and never reached."""
    F, ref = _ctx("mult_zp")
    rank, rng = 200, np.random.default_rng(2)
    base = [1 << 130, (ref.q >> 1) + 1, ref.q >> 1, 5, 1]
    dc = buckler.Decomposer(F, base)
    plain = _plain_inputs(ref.q, base, rank, rng)
    w = [p * ref.R % ref.q for p in plain]
    want = _limbs_of_digits(ref, D.infDcmp(ref, w, base))
    buf = _filled(1 + len(base) * rank * F.L)
    dc.inf_dev(buf[1:].data_ptr(), _dev(ref.arr(w)), 1, rank)
    got = _host(buf)
    assert got[0] == np.uint64(0xFFFFFFFFFFFFFFFF) and (got[1:].reshape(want.shape) == want).all()


PROJ_CASES = [(128, 2), (512, 8), (4096, (1 << 20) - 1)]  # nb = 1 (no zero tail), 3, 20


@pytest.mark.parametrize("key", FIELDS)
@pytest.mark.parametrize("rank,bound", PROJ_CASES)
def test_proj_matches_restatement(key, rank, bound):
    F, ref = _ctx(key)
    rng = np.random.default_rng(rank)
    base = list(_base(bound))
    assert len(base) == {128: 1, 512: 3, 4096: 20}[rank]
    dc = buckler.Decomposer(F, bound)
    w = [p * ref.R % ref.q for p in _plain_inputs(ref.q, base, 128, rng)] + rand_ints(ref.q, rank - 128, rng)
    want = ref.arr(D.projDcmp(ref, w, base, rank))
    out = _filled(rank, F.L)
    dc.proj_dev(out, _dev(ref.arr(w)), rank)
    assert (_host(out) == want).all()
    assert (dc.DecomposeProj(ref.arr(w)) == want).all()


def _above_half(q):
    """The least a with a^2 > q / 2; a^2 < q for every modulus here, so a^2 mod q lies above q / 2."""
    a = math.isqrt(q >> 1) + 1
    assert q >> 1 < a * a < q
    return a


@pytest.mark.parametrize("key", FIELDS)
@pytest.mark.parametrize("rank", [1, 200, 4096])
def test_two_norm_matches_restatement(key, rank):
    """Rank 1: one coefficient, base [1]; 200: one partial sum; 4096: four partial sums, and with
    decomposeBase(q - 1) up to 896 digits, so several workgroups walk the base.  Inputs: all q - 1
    (the sum is the rank), all q >> 1, the whole field at random, and one whose sum lies above q / 2
    (the digits are -1)."""
    F, ref = _ctx(key)
    q, L = ref.q, F.L
    rng = np.random.default_rng(rank)
    bounds = {1: [2], 200: [(1 << 20) - 1] + ([(1 << 64) + 1] if L >= 2 else []), 4096: [q - 1, 1000]}[rank]
    a = _above_half(q)
    plain = [[q - 1] * rank, [q >> 1] * rank, rand_ints(q, rank, rng), [0] * (rank - 1) + [a]]
    w = [[p * ref.R % q for p in v] for v in plain]
    dw = _dev(np.stack([ref.arr(v) for v in w]))
    for bound in bounds:
        base = list(_base(bound))
        dc = buckler.Decomposer(F, bound)
        res = [D.twoDcmp(ref, v, base) for v in w]
        assert res[0][1] == rank % q and res[3][1] == a * a % q > q >> 1
        want = np.stack([ref.arr(r[0]) for r in res])
        want_sq = ref.arr([r[1] * ref.R % q for r in res])
        if bound == q - 1:  # in reach of the base: -(q - a^2 mod q) recomposes from -1 digits alone
            neg = D.set_int64(ref, -1)
            assert set(res[3][0][:len(base)]) <= {0, neg} and neg in res[3][0][:len(base)]
        for batch in (4, 1):
            for with_sq in (True, False):
                out = _filled(batch, rank, L)
                sq = _filled(batch, L) if with_sq else None
                dc.two_dev(out, dw, batch, rank, d_sq=sq, d_scratch=_scratch(dc.scratch_bytes(batch, rank)))
                assert (_host(out) == want[:batch]).all(), (bound, batch, with_sq)
                if with_sq:
                    assert (_host(sq) == want_sq[:batch]).all(), (bound, batch)
        digits, sq = dc.DecomposeTwoNorm(np.stack([ref.arr(v) for v in w]))
        assert (digits == want).all() and (sq == want_sq).all()
        d1, s1 = dc.DecomposeTwoNorm(ref.arr(w[3]))
        assert (d1 == want[3]).all() and (s1 == want_sq[3]).all()


def test_inf_digits_feed_the_encoder_unchanged():
    """prover.go:77-86 then :149: the output of inf_dev is a batch of batch * nb witnesses for
    Encoder.encode_dev as it stands."""
    F, ref = _ctx("jindo_zp")
    q, L = ref.q, F.L
    rank, emb, batch, bound = 128, 256, 2, 1000
    base = list(_base(bound))
    nb, S = len(base), sum(base)
    rng = np.random.default_rng(17)
    centred = [int(v) for v in rng.integers(-S, S + 1, size=batch * rank)]
    centred[:4] = [S, -S, 0, -1]
    w = [c % q * ref.R % q for c in centred]
    dc = buckler.Decomposer(F, bound)
    enc = buckler.NewEncoder(F, rank, emb)
    digits = _filled(batch, nb, rank, L)
    dc.inf_dev(digits, _dev(ref.arr(w)), batch, rank)
    ecd = _filled(batch * nb, emb, L)
    enc.encode_dev(ecd, digits, batch * nb, d_scratch=_scratch(enc.scratch_bytes(batch * nb)))
    got = _host(ecd)
    got_digits = _host(digits)
    code = {0: 0, D.set_int64(ref, 1): 1, D.set_int64(ref, -1): -1}
    for k in range(batch):
        restated = D.infDcmp(ref, w[k * rank:(k + 1) * rank], base)
        for j in range(nb):
            assert (got[k * nb + j] == ref.arr(ref.encode(restated[j], emb))).all(), (k, j)
        dig = [[code[x] for x in ref.ints(got_digits[k, j])] for j in range(nb)]
        for i in range(rank):  # in-bound inputs recompose: sum_j base_j digit_j = w
            assert sum(base[j] * dig[j][i] for j in range(nb)) == centred[k * rank + i]


def test_live_handle_argument_errors():
    """The checks of a handle that has run kernels, with real buffers: nothing is written."""
    import torch
    F, ref = _ctx("p63")
    dc = buckler.Decomposer(F, 8)  # nb = 3
    rank = 384
    w = _dev(ref.arr(rand_ints(ref.q, rank, np.random.default_rng(1))))
    out = _filled(3 * rank)
    dc.inf_dev(out, w, 1, rank)  # the handle is live
    torch.cuda.synchronize()
    L = _lib.lib()
    keep = _filled(rank)
    scr = _scratch(dc.scratch_bytes(1, rank))
    assert L.rg_buckler_dcmp_inf_dev(dc.h, w.data_ptr(), 1, rank, w.data_ptr(), None) == INVALID
    assert L.rg_buckler_dcmp_proj_dev(dc.h, w.data_ptr(), rank - 1, keep.data_ptr(), None) == INVALID
    assert L.rg_buckler_dcmp_proj_dev(dc.h, w.data_ptr(), rank, w.data_ptr(), None) == INVALID
    assert L.rg_buckler_dcmp_two_dev(dc.h, w.data_ptr(), 1, 2, keep.data_ptr(), None, scr.data_ptr(), None) == INVALID
    assert L.rg_buckler_dcmp_two_dev(dc.h, w.data_ptr(), 1, rank, keep.data_ptr(), None, None, None) == INVALID
    assert L.rg_buckler_dcmp_two_dev(dc.h, w.data_ptr(), 1, rank, keep.data_ptr(), keep.data_ptr(), scr.data_ptr(),
                                     None) == INVALID
    assert (_host(keep) == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    with pytest.raises(RingoPanic):  # a buffer too small for [nb][rank][L]
        dc.inf_dev(_filled(rank), w, 1, rank)
    with pytest.raises(RingoPanic):
        dc.proj_dev(keep, w, 256)
    h = ctypes.c_void_p()
    assert L.rg_buckler_dcmp_create(F.h, None, 3, ctypes.byref(h)) == INVALID


def test_two_streams_share_one_handle():
    import torch
    F, ref = _ctx("jindo_zp")
    rank, bound = 4096, (1 << 20) - 1
    base = list(_base(bound))
    dc = buckler.Decomposer(F, bound)  # first used by both streams below
    rng = np.random.default_rng(23)
    ws = [[p * ref.R % ref.q for p in _plain_inputs(ref.q, base, rank, rng)] for _ in range(2)]
    dws = [_dev(ref.arr(w)) for w in ws]
    outs = [_filled(len(base), rank, F.L) for _ in range(2)]
    two = [_filled(rank, F.L) for _ in range(2)]
    scr = [_scratch(dc.scratch_bytes(1, rank)) for _ in range(2)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for _ in range(3):
        for s in range(2):
            dc.inf_dev(outs[s], dws[s], 1, rank, stream=streams[s])
            dc.two_dev(two[s], dws[s], 1, rank, d_scratch=scr[s], stream=streams[s])
    for s in range(2):
        streams[s].synchronize()
        assert (_host(outs[s]) == _limbs_of_digits(ref, D.infDcmp(ref, ws[s], base))).all()
        assert (_host(two[s]) == ref.arr(D.twoDcmp(ref, ws[s], base)[0])).all()
