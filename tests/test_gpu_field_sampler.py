"""GPU parity of the field-element sampler (rg_field_sampler_elems*, csrc/buckler_sample.hip over
csprng.hpp's draw), bit for bit against tests/set_random_ref.py -- Uint.SetRandom restated over the C
oracle's UniformSampler words -- on one field per limb count: the byte-serial route (p63, zp110,
zp220, zp440, zp880) and the whole-word route with its fix-up launch (q255; mult_zp for L = 2).
tests/test_oracle_set_random.py asserts on the CPU that these draws hold elements of two, three and
more tries on both routes.  Outputs go into buffers pre-filled with -1 that carry a guard word past
their end."""
import numpy as np
import pytest

import ringo
from ringo import buckler
from tests import set_random_ref as sr

pytestmark = pytest.mark.gpu

FF = np.uint64(2 ** 64 - 1)


def _filled(words):
    import torch
    return torch.full((words,), -1, dtype=torch.int64, device="cuda")


def _scratch(S):
    return _filled(S.scratch_bytes() // 8)


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def _sampler(key):
    F = ringo.Field(sr.modulus(key))
    return F, buckler.FieldSampler(F, sr.SEED)


def _elems(S, L, first, n, stream=None):
    """elems_dev into a poisoned buffer -> [n][L]; the guard word is checked."""
    d_out = _filled(n * L + 1)
    S.elems_dev(first, n, d_out, _scratch(S), stream=stream)
    if stream is not None:
        stream.synchronize()
    h = _host(d_out)
    assert h[n * L] == FF, "guard word overwritten"
    return h[:n * L].reshape(n, L)


def _differ(got, want):
    bad = np.flatnonzero((got != want).any(axis=1))
    return bad.size, bad[:8]


@pytest.mark.parametrize("key", sr.FIELDS + ("mult_zp",))
@pytest.mark.parametrize("first", sr.FIRSTS)
def test_elems_match_set_random(key, first):
    """n = 1500: not a multiple of 512, more than one workgroup; 2^32 - 700 straddles 2^32."""
    F, S = _sampler(key)
    q = sr.modulus(key)
    vals, _ = sr.draws(sr.SEED, q, first, sr.N)
    got = _elems(S, F.L, first, sr.N)
    assert _differ(got, sr.limbs(vals, q, F.L))[0] == 0, (key, first, _differ(got, sr.limbs(vals, q, F.L)))


@pytest.mark.parametrize("key", sr.FIELDS)
def test_the_last_instances(key):
    """n = 70 ending exactly at instance 2^64 - 2, the last one the entry takes."""
    F, S = _sampler(key)
    q = sr.modulus(key)
    first = 2 ** 64 - 1 - 70
    vals, _ = sr.draws(sr.SEED, q, first, 70)
    got = _elems(S, F.L, first, 70)
    assert _differ(got, sr.limbs(vals, q, F.L))[0] == 0, (key, _differ(got, sr.limbs(vals, q, F.L)))


@pytest.mark.parametrize("key", [sr.Q255, "zp110"])
def test_two_streams_with_their_own_scratch_equal_one_call(key):
    import torch
    F, S = _sampler(key)
    L, n, first = F.L, sr.N, sr.FIRSTS[1]
    whole = _elems(S, L, first, n)
    half = 700
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    d_a, d_b = _filled(half * L + 1), _filled((n - half) * L + 1)
    sc_a, sc_b = _scratch(S), _scratch(S)
    torch.cuda.synchronize()
    S.elems_dev(first, half, d_a, sc_a, stream=s0)
    S.elems_dev(first + half, n - half, d_b, sc_b, stream=s1)
    s0.synchronize()
    s1.synchronize()
    a, b = _host(d_a), _host(d_b)
    assert a[half * L] == FF and b[(n - half) * L] == FF
    assert (a[:half * L].reshape(half, L) == whole[:half]).all()
    assert (b[:(n - half) * L].reshape(n - half, L) == whole[half:]).all()


@pytest.mark.parametrize("key", [sr.Q255, "p63", "zp440"])
def test_host_form_agrees(key):
    F, S = _sampler(key)
    got = S.elems(sr.FIRSTS[2], 600)
    assert got.shape == (600, F.L) and (got == _elems(S, F.L, sr.FIRSTS[2], 600)).all()
    vals, _ = sr.draws(sr.SEED, sr.modulus(key), sr.FIRSTS[2], sr.N)
    assert (got == sr.limbs(vals[:600], sr.modulus(key), F.L)).all()
    assert S.elems(5, 0).shape == (0, F.L)


def test_refused_before_the_device_is_touched():
    import torch
    from ringo.bigpoly import RingoPanic
    F, S = _sampler(sr.Q255)
    d_out, sc = _filled(8 * F.L), _scratch(S)
    with pytest.raises(RingoPanic):
        S.elems_dev(2 ** 64 - 8, 8, d_out, sc)
    with pytest.raises(RingoPanic):
        S.elems_dev(0, 8, d_out, d_out)
    torch.cuda.synchronize()
    assert (_host(d_out) == FF).all() and (_host(sc) == FF).all()
