"""GPU parity: Prover.sumCheckMask of a batch of proofs in one launch (rg_buckler_sumcheck_mask_batch*;
prover.go:381-397), bit for bit against buckler_lin_ref.sumCheckMask per proof and against the single
entry rg_buckler_sumcheck_mask_dev: the mask [n][emb][L], mask.Coeffs[:maskRank] contiguous
[n][maskRank][L] and the mask sums [n][L], into buffers pre-filled with -1 that carry one guard
element past their end."""
import numpy as np
import pytest

from ringo import _lib, buckler
from tests import buckler_proj_util as P

pytestmark = pytest.mark.gpu

FF = np.uint64(2 ** 64 - 1)
# mask_rank as a function of (rank, emb): no subtraction at all, one, every entry below rank, and up to emb
MASK_RANKS = {"rank": lambda r, e: r, "rank+1": lambda r, e: r + 1, "2rank": lambda r, e: 2 * r, "emb": lambda r, e: e}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


def _filled(words):
    import torch
    return torch.full((words,), -1, dtype=torch.int64, device="cuda")


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def _case(key, rank, mask_rank, emb, n):
    cs = [P.mask_case(key, rank, mask_rank, emb, i) for i in range(n)]
    return (np.stack([c[0] for c in cs]), np.stack([c[1] for c in cs]), np.stack([c[2] for c in cs]))


def _run(F, rank, mask_rank, emb, rand, com=True, stream=None):
    """-> (mask [n][emb][L], maskCom [n][mask_rank][L] or None, maskSum [n][L]); the guards are checked."""
    n, L = rand.shape[0], F.L
    sizes = (n * emb * L, n * mask_rank * L, n * L)
    d_mask, d_com, d_sum = (_filled(s + L) for s in sizes)
    buckler.sumcheck_mask_batch_dev(F, rank, mask_rank, emb, n, _dev(rand), d_mask, d_sum,
                                    d_mask_com=d_com if com else None, stream=stream)
    if stream is not None:
        stream.synchronize()
    out = []
    for t, s, shape in zip((d_mask, d_com, d_sum), sizes, ((n, emb, L), (n, mask_rank, L), (n, L))):
        h = _host(t)
        assert (h[s:] == FF).all(), "guard element overwritten"
        out.append(h[:s].reshape(shape))
    if not com:
        assert (out[1] == FF).all()  # never touched
        out[1] = None
    return out


@pytest.mark.parametrize("key", P.FIELDS)
@pytest.mark.parametrize("rank", [128, 256])
@pytest.mark.parametrize("kind", list(MASK_RANKS))
def test_parity(key, rank, kind):
    F, _ = P.ctx(key)
    emb = 4 * rank
    mask_rank = MASK_RANKS[kind](rank, emb)
    for n in (1, 3, 5):
        rand, want_mask, want_sum = _case(key, rank, mask_rank, emb, n)
        mask, com, msum = _run(F, rank, mask_rank, emb, rand)
        assert (mask == want_mask).all() and (msum == want_sum).all(), n
        assert (com == want_mask[:, :mask_rank]).all(), n
        assert (mask[:, mask_rank:] == 0).all()


@pytest.mark.parametrize("key", ["p63", "mult_zp", "jindo_zp", "zp440", "zp880"])
@pytest.mark.parametrize("kind", list(MASK_RANKS))
def test_equal_to_the_single_entry_bit_for_bit(key, kind):
    F, _ = P.ctx(key)
    rank, emb, n, L = 128, 512, 5, P.ctx(key)[0].L
    mask_rank = MASK_RANKS[kind](rank, emb)
    rand, _, _ = _case(key, rank, mask_rank, emb, n)
    mask, com, msum = _run(F, rank, mask_rank, emb, rand)
    for i in range(n):
        d_mask, d_sum = _filled(emb * L), _filled(L)
        buckler.sumcheck_mask_dev(F, rank, mask_rank, emb, _dev(rand[i]), d_mask, d_sum)
        single = _host(d_mask).reshape(emb, L)
        assert (single == mask[i]).all() and (single[:mask_rank] == com[i]).all(), i
        assert (_host(d_sum) == msum[i]).all(), i


def test_without_the_commit_layout():
    """d_mask_com = NULL: the other two outputs are the same and nothing else is written."""
    key, rank, emb = "jindo_zp", 256, 1024
    F, _ = P.ctx(key)
    for mask_rank in (rank + 1, emb):
        rand, want_mask, want_sum = _case(key, rank, mask_rank, emb, 3)
        mask, com, msum = _run(F, rank, mask_rank, emb, rand, com=False)
        assert com is None and (mask == want_mask).all() and (msum == want_sum).all()


def test_host_form_streams_and_nothing_to_do():
    import torch
    key, rank, emb = "zp440", 128, 512
    F, _ = P.ctx(key)
    mask_rank = 2 * rank
    rand, want_mask, want_sum = _case(key, rank, mask_rank, emb, 3)
    mask, com, msum = buckler.SumCheckMaskBatch(F, rank, mask_rank, emb, rand)
    assert (mask == want_mask).all() and (com == want_mask[:, :mask_rank]).all() and (msum == want_sum).all()
    st = torch.cuda.Stream()
    mask, com, msum = _run(F, rank, mask_rank, emb, rand, stream=st)
    assert (mask == want_mask).all() and (com == want_mask[:, :mask_rank]).all() and (msum == want_sum).all()
    L = _lib.lib()
    assert L.rg_buckler_sumcheck_mask_batch_dev(F.h, rank, mask_rank, emb, 0, None, None, None, None, None) == 0
    # refused before the device is touched: real buffers stay -1
    d_mask, d_sum, d_rand = _filled(3 * emb * F.L), _filled(3 * F.L), _dev(rand)
    assert L.rg_buckler_sumcheck_mask_batch_dev(F.h, rank, rank - 1, emb, 3, d_rand.data_ptr(), d_mask.data_ptr(),
                                                None, d_sum.data_ptr(), None) == -1
    assert L.rg_buckler_sumcheck_mask_batch_dev(F.h, rank, mask_rank, emb, 3, d_rand.data_ptr(), d_mask.data_ptr(),
                                                d_mask.data_ptr(), d_sum.data_ptr(), None) == -1
    assert (_host(d_mask) == FF).all() and (_host(d_sum) == FF).all()
