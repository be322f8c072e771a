"""GPU: the projection checker's TransposeTo with a matrix per vector
(rg_buckler_checker_transpose_xof_dev), against tests/buckler_lin_ref.ProjChecker set to each vector's
XOF bytes, bit for bit; the checker's own matrix is neither read nor changed."""
import numpy as np
import pytest

import ringo
from ringo import buckler
from ringo.bigpoly import RingoPanic
from tests import buckler_lin_ref as R
from tests.buckler_lin_util import rand_ints, xof_bytes

pytestmark = pytest.mark.gpu

FIELDS = ["p63", "jindo_zp", "zp880"]
RANKS = [128, 384]  # 384: three chunks of columns, not a power of two


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


def _bytes(b):
    import torch
    return torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda()


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("rank", RANKS)
@pytest.mark.parametrize("name", FIELDS)
def test_transpose_xof_matches_reference(name, rank, fields):
    """Three vectors, three matrices: random, all-zero XOF bytes (every entry true) and all-0xFF (the
    zero matrix).  The handle's own matrix, a fourth one, gives the same transpose before and after."""
    import torch
    q = fields[name]
    F, ref = ringo.Field(q), R.Ref(q)
    L = F.L
    rng = np.random.default_rng(rank + L)
    xofs = [xof_bytes(k, rank, rng) for k in ("random", "zeros", "ones")]
    vs = [rand_ints(q, rank, rng) for _ in range(3)]
    want = np.stack([ref.arr(R.ProjChecker(ref, rank).set_xof(x).transpose(v)) for x, v in zip(xofs, vs)])
    assert (want[2] == 0).all() and (want[1] != 0).any()
    own = xof_bytes("random", rank, rng)
    chk = buckler.ProjChecker(F, rank).SetXOF(own)
    d_v = _dev(np.stack([ref.arr(v) for v in vs]))
    before = torch.full((3, rank, L), -1, dtype=torch.int64, device="cuda")
    chk.transpose_dev(before, d_v, 3)
    out = torch.full((4, rank, L), -1, dtype=torch.int64, device="cuda")
    bits = torch.full((chk.transpose_xof_scratch_bytes(3) // 8,), -1, dtype=torch.int64, device="cuda")
    assert chk.transpose_xof_scratch_bytes(3) == 3 * rank * 16
    chk.transpose_xof_dev(out, d_v, 3, _bytes(b"".join(xofs)), bits)
    got = _host(out)
    assert (got[:3] == want).all()
    assert (got[3] == np.uint64(2 ** 64 - 1)).all(), "wrote past d_out"
    after = torch.full((3, rank, L), -1, dtype=torch.int64, device="cuda")
    chk.transpose_dev(after, d_v, 3)
    own_want = np.stack([ref.arr(R.ProjChecker(ref, rank).set_xof(own).transpose(v)) for v in vs])
    assert (_host(before) == own_want).all() and (_host(after) == own_want).all()


def test_a_checker_never_set_is_accepted_and_other_kinds_are_refused(fields):
    import torch
    q = fields["p63"]
    F, ref = ringo.Field(q), R.Ref(q)
    rank = 128
    rng = np.random.default_rng(3)
    x, v = xof_bytes("random", rank, rng), rand_ints(q, rank, rng)
    chk = buckler.ProjChecker(F, rank)  # no SetXOF
    out = torch.full((1, rank, 1), -1, dtype=torch.int64, device="cuda")
    bits = torch.empty(rank * 2, dtype=torch.int64, device="cuda")
    d_v = _dev(ref.arr(v))
    chk.transpose_xof_dev(out, d_v, 1, _bytes(x), bits)
    assert (_host(out)[0] == ref.arr(R.ProjChecker(ref, rank).set_xof(x).transpose(v))).all()
    with pytest.raises(RingoPanic):  # its own matrix is still unset
        chk.transpose_dev(out, d_v, 1)
    lib = buckler.lib()
    A = [0x10000 * (i + 1) for i in range(4)]
    ntt = buckler.NewNTTChecker(F, rank)
    assert lib.rg_buckler_checker_transpose_xof_dev(ntt.h, A[0], A[1], 1, A[2], A[3], None) == -1
    assert lib.rg_buckler_checker_transpose_xof_scratch_bytes(ntt.h, 4) == 0
    for args in ((A[0], A[0], 1, A[2], A[3]), (A[0], A[1], 1, None, A[3]), (A[0], A[1], 1, A[2], None),
                 (A[0], A[1], 65536, A[2], A[3]), (A[0], A[1], 1, A[2], A[0])):
        assert lib.rg_buckler_checker_transpose_xof_dev(chk.h, *args, None) == -1, args
    assert lib.rg_buckler_checker_transpose_xof_dev(chk.h, A[0], A[1], 0, A[2], A[3], None) == 0
