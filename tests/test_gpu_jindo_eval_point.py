"""GPU: the inputs Evaluate and Verify derive from the transcript, built on the device:
rg_jindo_eval_point_dev (encode(leftVec(x)) and rightVec(x), jindo/utils.go:63-82 with
encoder.go:105-146) and rg_jindo_encode_challenges_dev (encodeChallengeTo, utils.go:20-46), bit-exact
against the C oracle (CJindo.encode, CJindo.encode_challenge, tests/jindo_proto.left_right) on the
fixture and synthetic parameter sets: the smallest ring, four unequal primes, an odd exp with
slots * exp < d, d = 1024, a prime below 2^62, nqo = 2, three primes, and ChallengeBound = 1."""
import numpy as np
import pytest

import coracle as co
from ringo import _lib, jindo
from ringo._lib import RingoError
from tests import jindo_synth_util as su
from tests.jindo_proto import left_right, mont, random_ck

pytestmark = pytest.mark.gpu

NAMES = ["syn_d8_p63", "syn_d128_mixed4", "syn_b7000_e5_p63", "syn_d1024_mult", "syn_d256_q62top", "t10_b8",
         "p63_t10_b2", "zp880_t10_b1"]
POISON = 0x5a5a5a5a5a5a5a5a


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


def _points(F, fq):
    rng = np.random.default_rng(77)
    return [("0", 0), ("1", mont(F, 1)), ("random", mont(F, int.from_bytes(rng.bytes(120), "little")))]


@pytest.mark.parametrize("name", NAMES)
def test_eval_point_matches_oracle(name):
    import torch
    P, fq, params, vrf, cj, F = _setup(name)
    L, cs = params.L, P["cols"] * P["slots"]
    lw, rw = P["rows"] * params.nq * P["d"], cs * L
    for label, x in _points(F, fq):
        left_e, right_e = left_right(P, F, x)
        want_left = np.stack([cj.encode(co.to_limbs([e], L)) for e in left_e])
        want_right = co.to_limbs(right_e, L)
        d_x = _t(co.to_limbs([x], L)[0])
        buf = torch.full((lw + rw + 8,), POISON, dtype=torch.int64, device="cuda")
        left, right = buf[:lw], buf[lw:lw + rw]
        vrf.eval_point_dev(d_x, left, right)
        torch.cuda.synchronize()
        assert (_h(left).reshape(want_left.shape) == want_left).all(), (name, label, "left")
        assert (_h(right).reshape(want_right.shape) == want_right).all(), (name, label, "right")
        assert (_h(buf[lw + rw:]) == np.uint64(POISON)).all(), (name, label, "wrote past right")
        # right = None: left alone is written, the words after it stay as they were
        buf.fill_(POISON)
        vrf._p.eval_point_dev(d_x, left)
        torch.cuda.synchronize()
        assert (_h(left).reshape(want_left.shape) == want_left).all(), (name, label, "left, right = None")
        assert (_h(buf[lw:]) == np.uint64(POISON)).all(), (name, label, "right = None was written")


def _bytes_of(v):
    """The 16 bytes encodeChallengeTo reads as v: two big-endian words, the low word first."""
    return (v & ((1 << 64) - 1)).to_bytes(8, "big") + (v >> 64).to_bytes(8, "big")


def _challenge_strings(P):
    bound = min(P["base"], 1 << (120 // P["exp"])) // 2
    rng = np.random.default_rng(5)
    out = [bytes(16), b"\xff" * 16] + [rng.bytes(16) for _ in range(16)]
    if bound >= 2:  # digits at the sign boundary: 0, bound/2 (kept), bound/2 + 1 (negated), bound - 1
        edges = [0, bound // 2, min(bound // 2 + 1, bound - 1), bound - 1]
        e = P["exp"]
        for pat in ([edges[0]] * e, [edges[1]] * e, [edges[2]] * e, [edges[3]] * e, [edges[i % 4] for i in range(e)],
                    [edges[(i + 2) % 4] for i in range(e)]):
            v = sum(r * bound ** i for i, r in enumerate(pat))
            assert v < 1 << 128
            out.append(_bytes_of(v))
    return bound, out


@pytest.mark.parametrize("ring", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_encode_challenges_matches_oracle(name, ring):
    import torch
    P, fq, params, vrf, cj, F = _setup(name)
    bound, strs = _challenge_strings(P)
    assert vrf._p.challenge_bound() == bound
    n, nl = len(strs), params.nqo if ring else params.nq
    want = np.stack([cj.encode_challenge(ring, b) for b in strs])
    d_b = torch.from_numpy(np.frombuffer(b"".join(strs), np.uint8).copy()).to("cuda")
    out = torch.full((n + 1, nl, P["d"]), POISON, dtype=torch.int64, device="cuda")
    vrf.encode_challenges_dev(ring, d_b, n, out)
    torch.cuda.synchronize()
    got = _h(out)
    assert (got[:n] == want).all(), (name, ring)
    assert (got[n] == np.uint64(POISON)).all(), (name, ring, "wrote past d_out")
    if bound == 1:  # every remainder by 1 is 0 (zp880, exp 64)
        assert (got[:n] == 0).all()
    else:
        assert got[:n].any()


def test_encode_challenges_refusals():
    """A live handle: another ring, and a parameter set whose ChallengeBound is 0 (exp > 120)."""
    import torch
    P, fq, params, vrf, cj, F = _setup("syn_d128_mixed4")
    d_b = torch.zeros(16, dtype=torch.uint8, device="cuda")
    out = torch.full((params.nq, P["d"]), POISON, dtype=torch.int64, device="cuda")
    L = _lib.lib()
    assert L.rg_jindo_encode_challenges_dev(vrf.h, 2, d_b.data_ptr(), 1, out.data_ptr(), None) == -1
    assert "ring 2" in L.rg_last_error().decode()
    Q = dict(P, exp=121, slots=1)  # slots * exp <= d = 128
    big = jindo.Prover(jindo.Parameters.from_dict(Q, fq), ck=random_ck(Q, 7))
    with pytest.raises(RingoError) as e:
        big.encode_challenges_dev(0, d_b, 1, out)
    assert e.value.status == -1 and "exp = 121" in str(e.value)
    torch.cuda.synchronize()
    assert (_h(out) == np.uint64(POISON)).all()
    with pytest.raises(RingoError):
        big.challenge_bound()
