"""SHAKE128 sponges on the device (include/ringo.h rg_xof_*): the Jindo transcript and the projection XOF.

    plan = Plan([(LITERAL, 0, 0, 6), (0, 0, 2048, 2048)], b"Jindo!")   # (base, offset, state_stride, len)
    h = Shake128(n_states)
    h.absorb_plan(plan, [com])        # every state: the literal, then its own 2 KiB of `com`
    h.squeeze(out, 16, out_stride=16)  # [n_states][16] bytes

n_states sponges move in lockstep: every call absorbs (squeezes) the same number of bytes in every
state, each state its own.  Every call is one asynchronous stream item; nothing is copied to the host.
Buffers are tensors of any dtype on the current GPU, or raw int addresses, as in the rest of the mirror.
A handle is not safe for concurrent calls.
"""
import ctypes

from ._lib import XofSegC, check, lib, vp
from .bigpoly import RingoPanic, _stream

LITERAL = -1     # include/ringo.h RG_XOF_LITERAL
MAX_BASES = 8    # include/ringo.h RG_XOF_MAX_BASES
RATE = 168


def _bytes_addr(x, nbytes=None):
    """Device address of a buffer read or written as bytes: a contiguous tensor of any dtype on the
    current GPU holding at least nbytes, or a raw int address."""
    if x is None or isinstance(x, int):
        return x
    if not hasattr(x, "data_ptr"):
        raise TypeError("device buffer must be a tensor or an int address")
    import torch
    if not x.is_contiguous() or x.device.type != "cuda" or x.device.index != torch.cuda.current_device():
        raise RingoPanic("device buffer must be contiguous and on the current GPU")
    if nbytes is not None and x.numel() * x.element_size() < nbytes:
        raise RingoPanic(f"device buffer holds {x.numel() * x.element_size()} bytes, need {nbytes}")
    return x.data_ptr()


class Plan:
    """The serialisation of one message as segments absorbed in order (rg_xof_plan_create): each segment
    (base, offset, state_stride, len) reads, for state s, len bytes at bases[base] + offset +
    s * state_stride, or, with base == LITERAL, len bytes at `offset` of `literals` for every state."""

    def __init__(self, segments, literals=b""):
        segments = list(segments)
        arr = (XofSegC * max(1, len(segments)))()
        for i, (base, offset, stride, length) in enumerate(segments):
            arr[i] = XofSegC(int(base), int(offset), int(stride), int(length))
        literals = bytes(literals)
        h = vp()
        check(lib().rg_xof_plan_create(ctypes.cast(arr, vp) if segments else None, len(segments), literals or None,
                                       len(literals), ctypes.byref(h)))
        self.h = h
        self._L = lib()
        self.segments = segments
        self.n_bases = 1 + max([s[0] for s in segments if s[3]] + [-1])

    def __del__(self):
        if getattr(self, "h", None) and getattr(self, "_L", None):
            self._L.rg_xof_plan_destroy(self.h)
            self.h = None

    def __len__(self):
        """Bytes each state absorbs."""
        return lib().rg_xof_plan_bytes(self.h)


class Shake128:
    """n_states SHAKE128 sponges (sha3.NewShake128), zeroed and absorbing."""

    def __init__(self, n_states):
        h = vp()
        check(lib().rg_xof_create(n_states, ctypes.byref(h)))
        self.h = h
        self._L = lib()
        self.n_states = n_states

    def __del__(self):
        if getattr(self, "h", None) and getattr(self, "_L", None):
            self._L.rg_xof_destroy(self.h)
            self.h = None

    def reset(self, stream=None):
        """Reset(): zeroed and absorbing again."""
        check(lib().rg_xof_reset_dev(self.h, _stream(stream)))

    def copy_from(self, src, stream=None):
        """Clone(): this handle takes src's words, position and phase."""
        check(lib().rg_xof_copy_dev(self.h, src.h, _stream(stream)))

    def absorb(self, data, length, state_stride=None, stream=None):
        """State s absorbs `length` bytes at data + s * state_stride (default: length; 0: the same
        bytes for every state)."""
        stride = length if state_stride is None else state_stride
        need = (self.n_states - 1) * stride + length if length else 0
        check(lib().rg_xof_absorb_dev(self.h, _bytes_addr(data, need), length, stride, _stream(stream)))

    def absorb_plan(self, plan, bases=(), stream=None):
        """Every state absorbs the message `plan` describes over the device buffers `bases`."""
        bases = list(bases)
        arr = (vp * max(1, len(bases)))(*[_bytes_addr(b) for b in bases])
        check(lib().rg_xof_absorb_plan_dev(self.h, plan.h, arr if bases else None, len(bases), _stream(stream)))

    def squeeze(self, out, length, out_stride=None, stream=None):
        """State s writes the next `length` bytes of its output at out + s * out_stride (default:
        length).  The first squeeze pads; later ones continue the stream."""
        stride = length if out_stride is None else out_stride
        need = (self.n_states - 1) * stride + length if length else 0
        check(lib().rg_xof_squeeze_dev(self.h, _bytes_addr(out, need), length, stride, _stream(stream)))


def marshal_dev(field, x, n, x_stride, out, out_stride=None, stream=None):
    """Uint.Marshal() of n Montgomery elements (rg_field_marshal_dev): element k at x + k * x_stride
    elements, its 8 * L big-endian bytes at out + k * out_stride (default 8 * L)."""
    stride = 8 * field.L if out_stride is None else out_stride
    check(lib().rg_field_marshal_dev(field.h, _bytes_addr(x, ((n - 1) * x_stride + 1) * 8 * field.L if n else 0), n,
                                     x_stride, _bytes_addr(out, (n - 1) * stride + 8 * field.L if n else 0), stride,
                                     _stream(stream)))
