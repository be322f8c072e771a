"""The device-sponge cases of test_gpu_xof.py, as functions of n_states that return (label, got, want)
triples: bytes the rg_xof_* calls produced against hashlib.shake_128 over the same bytes, every state on
its own data.  Shared with tests/exp_child_xof.py, which runs them on the experiments build's
lane-per-state kernels."""
import hashlib

import numpy as np
import torch

from ringo import xof

LENGTHS = [0, 1, 7, 8, 166, 167, 168, 169, 335, 336, 337, 1000]
POISON = 0xA5
GUARD = 64  # 8 guard words after every output


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def rand_bytes(rng, *shape):
    return rng.integers(0, 256, shape, dtype=np.uint8)


def shake(msg, n):
    return np.frombuffer(hashlib.shake_128(bytes(msg)).digest(n), np.uint8)


def state_bytes(buf, s, offset, stride, length):
    """What state s reads from the flat host copy `buf` of a device buffer."""
    return buf[offset + s * stride: offset + s * stride + length].tobytes()


class Out:
    """A poisoned device output [n][len + gap + GUARD]: state s writes at s * stride; rows() checks that
    everything past len is still poison."""

    def __init__(self, n, length, gap=0):
        self.n, self.len, self.stride = n, length, length + gap + GUARD
        self.t = torch.full((n * self.stride,), POISON, dtype=torch.uint8, device="cuda")

    def rows(self):
        h = self.t.cpu().numpy().reshape(self.n, self.stride)
        assert (h[:, self.len:] == POISON).all(), "bytes past len were written"
        return h[:, :self.len]


def absorb_lengths(n):
    """absorb_dev: every length, the source offset by 0..7 bytes, strides that are no multiple of 8, stride 0."""
    rng = np.random.default_rng(11 + n)
    h = xof.Shake128(n)
    outs = []
    for length in LENGTHS:
        for off in range(8):
            stride = 0 if off == 3 else length + 1 + 2 * (off % 4)
            if stride % 8 == 0 and stride:
                stride += 1
            buf = rand_bytes(rng, off + (n - 1) * stride + length + 8)
            d = dev(buf)
            o = Out(n, 32, gap=off)
            h.reset()
            h.absorb(d.data_ptr() + off, length, stride)
            h.squeeze(o.t, 32, o.stride)
            outs.append((f"len {length} off {off} stride {stride}", o, d,
                         [shake(state_bytes(buf, s, off, stride, length), 32) for s in range(n)]))
    torch.cuda.synchronize()
    return [(label, o.rows(), np.stack(want)) for label, o, _, want in outs]


def absorb_sequences(n):
    """Sequences of absorbs that leave the position at 0, 1 and 167 (the 0x9F case) before the squeeze."""
    rng = np.random.default_rng(12 + n)
    h = xof.Shake128(n)
    outs = []
    for chunks in ([100, 68], [168], [168, 1], [1], [50, 117], [167], [335], [5, 163, 167], [0, 336, 0], [7, 8, 9, 143]):
        bufs = [rand_bytes(rng, n, max(c, 1)) for c in chunks]
        ds = [dev(b) for b in bufs]
        o = Out(n, 40)
        h.reset()
        for c, d in zip(chunks, ds):
            h.absorb(d, c, max(c, 1))
        h.squeeze(o.t, 40, o.stride)
        want = [shake(b"".join(b[s, :c].tobytes() for b, c in zip(bufs, chunks)), 40) for s in range(n)]
        outs.append((f"chunks {chunks} end {sum(chunks) % 168}", o, ds, want))
    torch.cuda.synchronize()
    return [(label, o.rows(), np.stack(want)) for label, o, _, want in outs]


def plans(n):
    """absorb_plan_dev over literals and two device buffers."""
    rng = np.random.default_rng(13 + n)
    sa, sb = 9001, 613  # state strides, no multiple of 8
    A = rand_bytes(rng, (n - 1) * sa + 10000)
    B = rand_bytes(rng, (n - 1) * sb + 700)
    lit = rand_bytes(rng, 64).tobytes()
    dA, dB = dev(A), dev(B)
    LIT = xof.LITERAL
    cases = {
        "literal, device, literal": [(LIT, 0, 0, 5), (0, 3, sa, 300), (LIT, 5, 0, 7)],
        "a zero-length segment": [(LIT, 0, 0, 9), (0, 17, sa, 0), (LIT, 9, 0, 0), (0, 40, sa, 200)],
        "1-byte segments": [(LIT, i, 0, 1) if i % 2 else (0, 7 * i, sa, 1) for i in range(20)],
        "only 1-byte segments over two blocks": [(0, 3 * i, sa, 1) for i in range(340)],
        "straddling one and two block boundaries": [(0, 0, sa, 100), (0, 1000, sa, 100), (0, 2001, sa, 400), (LIT, 0, 0, 3)],
        "two bases": [(0, 8, sa, 168), (1, 5, sb, 333), (0, 500, sa, 64), (1, 0, sb, 2)],
        "a stride-0 device segment": [(0, 11, 0, 250), (1, 0, sb, 90), (0, 1, 0, 1)],
        "1,000 8-byte segments": [(0, 8 * i if i % 3 else 9 * i + 1, sa, 8) for i in range(1000)],
        "aligned rows after an 8-byte prefix": [(LIT, 0, 0, 8), (0, 2048, sa, 2048), (LIT, 8, 0, 8), (0, 4096, sa, 2048)],
    }
    h = xof.Shake128(n)
    outs = []
    for label, segs in cases.items():
        p = xof.Plan(segs, lit)
        want = []
        for s in range(n):
            msg = b""
            for base, off, stride, length in segs:
                msg += lit[off:off + length] if base == LIT else state_bytes((A, B)[base], s, off, stride, length)
            want.append(shake(msg, 48))
        assert len(p) == sum(x[3] for x in segs)
        o = Out(n, 48)
        h.reset()
        h.absorb_plan(p, [dA, dB][:p.n_bases])
        h.squeeze(o.t, 48, o.stride)
        outs.append((label, o, p, want))
    torch.cuda.synchronize()
    return [(label, o.rows(), np.stack(want)) for label, o, _, want in outs]


def squeeze_stream(n):
    """Successive squeezes continue one stream across block boundaries; out_stride > len leaves the gap alone."""
    rng = np.random.default_rng(14 + n)
    msg = rand_bytes(rng, n, 77)
    d = dev(msg)
    res = []
    for reads in ([100, 100, 200], [16] * 12, [168, 168, 1], [167, 1, 1, 500], [0, 1, 0, 169], [1]):
        h = xof.Shake128(n)
        h.absorb(d, 77)
        outs = [Out(n, r, gap=5) for r in reads]
        for o, r in zip(outs, reads):
            h.squeeze(o.t, r, o.stride)
        torch.cuda.synchronize()
        got = np.concatenate([o.rows() for o in outs], axis=1)
        res.append((f"reads {reads}", got, np.stack([shake(msg[s].tobytes(), sum(reads)) for s in range(n)])))
    return res


def copy_fork(n):
    """copy mid-absorb (position 100), the two forks continued differently; copy of a squeezing handle."""
    rng = np.random.default_rng(15 + n)
    m0, m1, m2 = rand_bytes(rng, n, 100), rand_bytes(rng, n, 70), rand_bytes(rng, n, 300)
    d0, d1, d2 = dev(m0), dev(m1), dev(m2)
    a, b, c = xof.Shake128(n), xof.Shake128(n), xof.Shake128(n)
    a.absorb(d0, 100)
    b.absorb(d2, 300)  # overwritten by the copy
    b.copy_from(a)
    a.absorb(d1, 70)
    b.absorb(d2, 300)
    oa, ob, oc1, oc2 = Out(n, 64), Out(n, 64), Out(n, 200), Out(n, 200)
    a.squeeze(oa.t, 64, oa.stride)
    b.squeeze(ob.t, 30, ob.stride)
    c.copy_from(b)  # a fork of the output stream
    b.squeeze(oc1.t, 200, oc1.stride)
    c.squeeze(oc2.t, 200, oc2.stride)
    torch.cuda.synchronize()
    cat = lambda s, *ms: b"".join(m[s].tobytes() for m in ms)
    wb = np.stack([shake(cat(s, m0, m2), 230) for s in range(n)])
    return [("fork a", oa.rows(), np.stack([shake(cat(s, m0, m1), 64) for s in range(n)])),
            ("fork b", ob.rows()[:, :30], wb[:, :30]),
            ("stream of b", oc1.rows(), wb[:, 30:]), ("stream of b's copy", oc2.rows(), wb[:, 30:])]


def reset_after_squeeze(n):
    rng = np.random.default_rng(16 + n)
    m0, m1 = rand_bytes(rng, n, 200), rand_bytes(rng, n, 31)
    d0, d1 = dev(m0), dev(m1)
    h = xof.Shake128(n)
    o0, o1 = Out(n, 20), Out(n, 20)
    h.absorb(d0, 200)
    h.squeeze(o0.t, 20, o0.stride)
    h.reset()
    h.absorb(d1, 31)
    h.squeeze(o1.t, 20, o1.stride)
    torch.cuda.synchronize()
    return [("before", o0.rows(), np.stack([shake(m0[s].tobytes(), 20) for s in range(n)])),
            ("after", o1.rows(), np.stack([shake(m1[s].tobytes(), 20) for s in range(n)]))]


def long_chain(n):
    """64 KiB in, 32 * 256 bytes out: a few hundred permutations through the block loop and the prefetch."""
    rng = np.random.default_rng(17 + n)
    m = rand_bytes(rng, n, 65536)
    d = dev(m)
    h = xof.Shake128(n)
    o = Out(n, 32 * 256)
    h.absorb(d, 65536)
    h.squeeze(o.t, 32 * 256, o.stride)
    torch.cuda.synchronize()
    return [("64 KiB", o.rows(), np.stack([shake(m[s].tobytes(), 32 * 256) for s in range(n)]))]


CASES = {f.__name__: f for f in (absorb_lengths, absorb_sequences, plans, squeeze_stream, copy_fork, reset_after_squeeze)}


def mismatches(triples):
    return [label for label, got, want in triples if got.shape != want.shape or not (got == want).all()]


def check_null_out(h):
    """A squeeze of 16 bytes into a NULL buffer (refused)."""
    h.squeeze(None, 16, 16)
