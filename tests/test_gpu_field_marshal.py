"""GPU: rg_field_marshal_dev (Uint.Marshal(), element.go: out of Montgomery form, 8 * L big-endian bytes)
against Python integers on every golden and synthetic field, for the values 0, 1, q - 1, R mod q and
random ones, read with element strides 1 and 5 and written with the natural and a padded byte stride,
with the bytes around every output still poison."""
import json
import os

import numpy as np
import pytest
import torch

import ringo
from ringo import xof

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = {}
for _f in ("fields.json", "synthetic_fields.json"):
    FIELDS.update({k: int(v["q_hex"], 16) for k, v in json.load(open(os.path.join(GOLDEN, _f))).items()})
POISON = 0xA5


@pytest.mark.parametrize("x_stride", [1, 5])
@pytest.mark.parametrize("name", sorted(FIELDS))
def test_marshal_is_the_big_endian_value(name, x_stride):
    q = FIELDS[name]
    F = ringo.Field(q)
    L = F.L
    rng = np.random.default_rng(L * 100 + x_stride)
    R = 1 << (64 * L)
    vals = [0, 1, q - 1, R % q] + [int.from_bytes(rng.bytes(8 * L + 8), "big") % q for _ in range(300)]
    n = len(vals)
    x = np.full(((n - 1) * x_stride + 1, L), 0xDEADBEEFDEADBEEF, np.uint64)  # the elements between are never read
    x[::x_stride] = F.mont(vals)
    dx = torch.from_numpy(x.view(np.int64)).to("cuda")
    for out_stride in (8 * L, 8 * L + 13):
        guard = 64
        out = torch.full((guard + n * out_stride + guard,), POISON, dtype=torch.uint8, device="cuda")
        xof.marshal_dev(F, dx, n, x_stride, out.data_ptr() + guard, out_stride)
        torch.cuda.synchronize()
        h = out.cpu().numpy()
        assert (h[:guard] == POISON).all() and (h[guard + (n - 1) * out_stride + 8 * L:] == POISON).all()
        body = h[guard:guard + n * out_stride].reshape(n, out_stride)
        assert (body[:, 8 * L:] == POISON).all()
        want = np.stack([np.frombuffer(v.to_bytes(8 * L, "big"), np.uint8) for v in vals])
        assert (body[:, :8 * L] == want).all()
