"""CPU: the refusals of the field-element sampler and of the sampled mask (include/ringo.h:
rg_field_sampler_*, rg_buckler_sumcheck_mask_batch_sampled*).  Creating an rg_fsampler touches no
device, so every refusal runs here with a live handle; each returns its status with a reason in
rg_last_error before the device is touched.  The device addresses below are made-up numbers: a call
that read them would crash, not fail."""
import ctypes
import re

import numpy as np
import pytest

import ringo
from ringo import _lib, buckler
from ringo.bigpoly import RingoPanic

INVALID, UNSUPPORTED = -1, -3
A, B, C, D = 0x10000000, 0x20000000, 0x30000000, 0x40000000  # distinct fake device addresses, far apart
TOP = 2 ** 64 - 1


def _why():
    return _lib.lib().rg_last_error().decode()


@pytest.fixture(scope="module")
def F(fields):
    return ringo.Field(fields["jindo_zp"])


@pytest.fixture(scope="module")
def S(F):
    return buckler.FieldSampler(F, b"seed")


def _create(f, seed=b"seed", out=True, seed_len=None):
    h = ctypes.c_void_p(1)
    st = _lib.lib().rg_field_sampler_create(f, seed, len(seed or b"") if seed_len is None else seed_len,
                                            ctypes.byref(h) if out else None)
    return st, h


def test_handle_is_created_and_destroyed_with_no_device(F, fields):
    L = _lib.lib()
    for key in ("p63", "zp110", "jindo_zp", "zp220", "zp440", "zp880", "mult_zp"):
        G = ringo.Field(fields[key])
        st, h = _create(G.h)
        assert st == 0 and h.value, key
        assert L.rg_field_sampler_scratch_bytes(h) == 256
        L.rg_field_sampler_destroy(h)
    L.rg_field_sampler_destroy(None)  # as free(NULL)
    assert L.rg_field_sampler_scratch_bytes(None) == 0
    st, h = _create(F.h, seed=b"")  # an empty seed is a seed
    assert st == 0 and h.value
    L.rg_field_sampler_destroy(h)


def test_create_refusals(F):
    st, h = _create(None)
    assert st == INVALID and h.value is None and _why().startswith("field sampler") and "NULL field" in _why()
    st, _ = _create(F.h, out=False)
    assert st == INVALID and _why().startswith("field sampler") and "NULL out" in _why()
    st, h = _create(F.h, seed=None, seed_len=4)
    assert st == INVALID and h.value is None and "NULL seed" in _why()
    G = ringo.Field((1 << 130) + 5 | 1, limbs=3)  # a limb count with no kernel
    st, h = _create(G.h)
    assert st == UNSUPPORTED and h.value is None and _why().startswith("field sampler") and "3 limbs" in _why()


def test_elems_refusals_with_a_live_handle(S):
    L = _lib.lib()
    dev, host = L.rg_field_sampler_elems_dev, L.rg_field_sampler_elems

    def refused(why, *a):
        assert dev(*a, None) == INVALID and _why().startswith("field sampler") and why in _why(), (a, _why())

    refused("NULL handle", None, 0, 4, A, B)
    assert dev(None, 0, 0, A, B, None) == INVALID  # refused even where nothing would run
    refused("NULL output", S.h, 0, 4, None, B)
    refused("NULL scratch", S.h, 0, 4, A, None)
    # instances first .. first + n - 1 must stay below 2^64 - 1
    refused("2^64 - 1", S.h, TOP, 1, A, B)
    refused("2^64 - 1", S.h, TOP - 1, 2, A, B)
    refused("2^64 - 1", S.h, TOP - 69, 71, A, B)
    refused("2^64 - 1", S.h, 2 ** 63, 2 ** 63, A, B)
    refused("2^64 - 1", S.h, 1, TOP, A, B)
    # d_out [n][4] words against the 256 bytes of scratch
    refused("overlaps", S.h, 0, 4, A, A)
    refused("overlaps", S.h, 0, 4, A, A + 4 * 32 - 8)
    refused("overlaps", S.h, 0, 4, A, A - 248)
    assert dev(S.h, 5, 0, None, None, None) == 0  # nothing to do
    assert dev(S.h, TOP, 0, None, None, None) == 0
    one = np.ones(4, np.uint64)
    assert host(None, 0, 1, _lib.ptr(one)) == INVALID and "NULL handle" in _why()
    assert host(S.h, 0, 1, None) == INVALID and _why().startswith("field sampler") and "NULL output" in _why()
    assert host(S.h, TOP, 1, _lib.ptr(one)) == INVALID and "2^64 - 1" in _why()
    assert host(S.h, 0, 0, None) == 0
    assert (one == 1).all()


def test_mask_sampled_refusals(S):
    L = _lib.lib()
    dev, host = L.rg_buckler_sumcheck_mask_batch_sampled_dev, L.rg_buckler_sumcheck_mask_batch_sampled
    E = 0x50000000  # the scratch

    def refused(why, *a):
        assert dev(*a, None) == INVALID and _why().startswith("buckler mask sampled") and why in _why(), (a, _why())

    refused("NULL handle", None, 128, 256, 512, 2, 0, A, B, C, E)
    # the constraints of rg_buckler_sumcheck_mask_batch_dev: rank >= 1, rank <= mask_rank <= emb_rank <= 2^40
    refused("rank", S.h, 0, 256, 512, 2, 0, A, B, C, E)
    refused("rank", S.h, 128, 127, 512, 2, 0, A, B, C, E)
    refused("rank", S.h, 128, 513, 512, 2, 0, A, B, C, E)
    refused("rank", S.h, 128, 256, (1 << 40) + 1, 2, 0, A, B, C, E)
    refused("n_proofs", S.h, 128, 256, 512, 65536, 0, A, B, C, E)
    refused("n_proofs", S.h, 128, 256, 512, 1 << 40, 0, A, B, C, E)
    refused("NULL buffer", S.h, 128, 256, 512, 2, 0, None, B, C, E)
    refused("NULL buffer", S.h, 128, 256, 512, 2, 0, A, B, None, E)
    refused("NULL scratch", S.h, 128, 256, 512, 2, 0, A, B, C, None)
    for a in ((A, A, C, E), (A, B, A, E), (A, B, B, E), (A, None, A, E), (A, B, C, A), (A, B, C, B), (A, B, C, C),
              (A, None, C, C), (A, A + 8, C, E), (A, B, A + 2 * 512 * 32 - 8, E), (A, B, C, C - 248)):
        refused("alias", S.h, 128, 256, 512, 2, 0, *a)
    # draw k of proof p reads instance first + p * mask_rank + k: all of them below 2^64 - 1
    refused("2^64 - 1", S.h, 128, 256, 512, 2, TOP - 511, A, B, C, E)
    refused("2^64 - 1", S.h, 128, 256, 512, 2, TOP, A, B, C, E)
    refused("2^64 - 1", S.h, 128, 1 << 40, 1 << 40, 65535, TOP - (65535 << 40) + 1, A, B, C, E)
    assert dev(S.h, 128, 256, 512, 0, TOP, None, None, None, None, None) == 0  # nothing to do
    assert dev(S.h, 128, 127, 512, 0, 0, None, None, None, None, None) == INVALID  # the shape is checked even then
    one = np.ones(4, np.uint64)
    p = _lib.ptr(one)
    assert host(None, 1, 2, 4, 1, 0, p, None, p) == INVALID and "NULL handle" in _why()
    assert host(S.h, 0, 2, 4, 1, 0, p, None, p) == INVALID and _why().startswith("buckler mask sampled")
    assert host(S.h, 1, 2, 4, 65536, 0, p, None, p) == INVALID and "n_proofs" in _why()
    assert host(S.h, 1, 2, 4, 1, 0, None, None, p) == INVALID and "NULL buffer" in _why()
    assert host(S.h, 1, 1, 1, 1, 0, p, None, p) == INVALID and "alias" in _why()
    assert host(S.h, 1, 2, 4, 1, TOP - 1, p, None, p) == INVALID and "2^64 - 1" in _why()
    assert host(S.h, 1, 2, 4, 0, 0, None, None, None) == 0
    assert (one == 1).all()


def test_the_header_states_the_calls_and_the_mirror_has_the_entries(F, S):
    src = open(_lib.HEADER).read()
    arity = {"rg_field_sampler_create": 4, "rg_field_sampler_destroy": 1, "rg_field_sampler_scratch_bytes": 1,
             "rg_field_sampler_elems_dev": 6, "rg_field_sampler_elems": 4,
             "rg_buckler_sumcheck_mask_batch_sampled_dev": 11, "rg_buckler_sumcheck_mask_batch_sampled": 9}
    for name, n in arity.items():
        assert name in _lib._SIGS and re.search(r"\b%s\(" % name, src), name
        assert len(_lib._SIGS[name][1]) == n, name
        assert hasattr(_lib.lib(), name), name
    assert "Stream items, whatever n: 3" in src  # the header states the count
    for name in ("elems", "elems_dev", "scratch_bytes"):
        assert hasattr(buckler.FieldSampler, name), name
    assert callable(buckler.SumCheckMaskBatchSampled) and callable(buckler.sumcheck_mask_batch_sampled_dev)
    assert S.scratch_bytes() == 256
    assert S.elems(0, 0).shape == (0, F.L)
    mask, com, msum = buckler.SumCheckMaskBatchSampled(S, 128, 256, 512, 0, 0)
    assert mask.shape == (0, 512, F.L) and com.shape == (0, 256, F.L) and msum.shape == (0, F.L)
    with pytest.raises(RingoPanic):
        buckler.SumCheckMaskBatchSampled(S, 128, 600, 512, 1, 0)
    with pytest.raises(RingoPanic):
        S.elems(TOP, 1)
