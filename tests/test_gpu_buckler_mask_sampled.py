"""GPU parity: Prover.sumCheckMask of a batch of proofs with its MustSetRandom draws made inside the
mask kernel (rg_buckler_sumcheck_mask_batch_sampled*; prover.go:381-397 over element.go:299-343), bit
for bit against buckler_lin_ref.sumCheckMask fed the draws of tests/set_random_ref.py (draw k of
proof p = the element of instance first + p * mask_rank + k), and against the composition the entry
is defined by: rg_field_sampler_elems_dev into a buffer, then rg_buckler_sumcheck_mask_batch_dev.
q255 takes the whole-word route, zp110 the byte-serial one.  Outputs go into buffers pre-filled with
-1 that carry one guard element past their end; first = 2^32 - 100, so the proofs' instances straddle
2^32."""
import functools

import numpy as np
import pytest

import ringo
from ringo import buckler
from tests import buckler_lin_ref as R
from tests import set_random_ref as sr

pytestmark = pytest.mark.gpu

FF = np.uint64(2 ** 64 - 1)
N_PROOFS = 3
FIRST = 2 ** 32 - 100
# (rank, mask_rank, emb_rank): no subtraction; no zero tail; a partial second block; a chain of four
# draws per lane (and lanes of three); more than one workgroup per proof
SHAPES = [(128, 128, 256), (128, 256, 256), (128, 300, 512), (64, 200, 256)]
CASES = [(k, s) for k in (sr.Q255, "zp110") for s in SHAPES] + [(sr.Q255, (1024, 2048, 2048))]


def _filled(words):
    import torch
    return torch.full((words,), -1, dtype=torch.int64, device="cuda")


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


@functools.lru_cache(maxsize=None)
def _ctx(key):
    F = ringo.Field(sr.modulus(key))
    return F, buckler.FieldSampler(F, sr.SEED), R.Ref(sr.modulus(key))


@functools.lru_cache(maxsize=None)
def _want(key, rank, mask_rank, emb):
    """(draws [n][mask_rank][L], mask [n][emb][L], maskSum [n][L]) of the restatement."""
    _, _, ref = _ctx(key)
    vals, _ = sr.draws(sr.SEED, ref.q, FIRST, N_PROOFS * mask_rank)
    masks, sums = [], []
    for p in range(N_PROOFS):
        rand = list(vals[p * mask_rank:(p + 1) * mask_rank])
        mask, msum = R.sumCheckMask(ref, rank, mask_rank, emb, rand)
        masks.append(ref.arr(mask))
        sums.append(ref.arr([msum])[0])
    return ref.arr(vals).reshape(N_PROOFS, mask_rank, ref.L), np.stack(masks), np.stack(sums)


def _run(key, rank, mask_rank, emb, com=True, stream=None):
    """-> (mask [n][emb][L], maskCom [n][mask_rank][L] or None, maskSum [n][L]); the guards are checked."""
    F, S, _ = _ctx(key)
    n, L = N_PROOFS, F.L
    sizes = (n * emb * L, n * mask_rank * L, n * L)
    d_mask, d_com, d_sum = (_filled(s + L) for s in sizes)
    buckler.sumcheck_mask_batch_sampled_dev(S, rank, mask_rank, emb, n, FIRST, d_mask, d_sum,
                                            _filled(S.scratch_bytes() // 8), d_mask_com=d_com if com else None,
                                            stream=stream)
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


@pytest.mark.parametrize("key,shape", CASES)
@pytest.mark.parametrize("com", [True, False])
def test_parity_with_the_restatement(key, shape, com):
    rank, mask_rank, emb = shape
    draws, want_mask, want_sum = _want(key, rank, mask_rank, emb)
    mask, mcom, msum = _run(key, rank, mask_rank, emb, com=com)
    assert (mask == want_mask).all(), np.flatnonzero((mask != want_mask).any(axis=2).reshape(-1))[:8]
    assert (msum == want_sum).all() and (msum == draws[:, 0]).all()  # draw 0, before the subtraction
    assert (mask[:, mask_rank:] == 0).all()  # every word written: none of the -1 is left
    if com:
        assert (mcom == want_mask[:, :mask_rank]).all()


@pytest.mark.parametrize("key,shape", CASES)
def test_equal_to_the_composition_bit_for_bit(key, shape):
    rank, mask_rank, emb = shape
    F, S, _ = _ctx(key)
    n, L = N_PROOFS, F.L
    d_rand = _filled(n * mask_rank * L)
    S.elems_dev(FIRST, n * mask_rank, d_rand, _filled(S.scratch_bytes() // 8))
    d_mask, d_com, d_sum = _filled(n * emb * L), _filled(n * mask_rank * L), _filled(n * L)
    buckler.sumcheck_mask_batch_dev(F, rank, mask_rank, emb, n, d_rand, d_mask, d_sum, d_mask_com=d_com)
    mask, mcom, msum = _run(key, rank, mask_rank, emb)
    assert (_host(d_mask).reshape(n, emb, L) == mask).all()
    assert (_host(d_com).reshape(n, mask_rank, L) == mcom).all()
    assert (_host(d_sum).reshape(n, L) == msum).all()


def test_host_form_streams_and_nothing_to_do():
    import torch
    key, (rank, mask_rank, emb) = "zp110", SHAPES[2]
    F, S, _ = _ctx(key)
    _, want_mask, want_sum = _want(key, rank, mask_rank, emb)
    mask, mcom, msum = buckler.SumCheckMaskBatchSampled(S, rank, mask_rank, emb, N_PROOFS, FIRST)
    assert (mask == want_mask).all() and (mcom == want_mask[:, :mask_rank]).all() and (msum == want_sum).all()
    mask, mcom, msum = _run(key, rank, mask_rank, emb, stream=torch.cuda.Stream())
    assert (mask == want_mask).all() and (mcom == want_mask[:, :mask_rank]).all() and (msum == want_sum).all()
    from ringo import _lib
    L = _lib.lib()
    assert L.rg_buckler_sumcheck_mask_batch_sampled_dev(S.h, rank, mask_rank, emb, 0, 0, None, None, None, None,
                                                        None) == 0
    # refused before the device is touched: real buffers stay -1
    d_mask, d_sum, sc = _filled(N_PROOFS * emb * F.L), _filled(N_PROOFS * F.L), _filled(32)
    for a in ((rank, rank - 1, emb, N_PROOFS, FIRST, d_mask.data_ptr(), None, d_sum.data_ptr(), sc.data_ptr()),
              (rank, mask_rank, emb, N_PROOFS, FIRST, d_mask.data_ptr(), d_mask.data_ptr(), d_sum.data_ptr(),
               sc.data_ptr()),
              (rank, mask_rank, emb, N_PROOFS, 2 ** 64 - 1 - 3 * mask_rank + 1, d_mask.data_ptr(), None,
               d_sum.data_ptr(), sc.data_ptr())):
        assert L.rg_buckler_sumcheck_mask_batch_sampled_dev(S.h, *a, None) == -1
    assert (_host(d_mask) == FF).all() and (_host(d_sum) == FF).all() and (_host(sc) == FF).all()
