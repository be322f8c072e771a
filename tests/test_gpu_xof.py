"""GPU: the device SHAKE128 sponges (rg_xof_*, ringo.xof) against hashlib.shake_128, every state on its own
data, for 1, 3 and 65 states (65 is more than one wave holds in either kernel layout).  The cases are in
tests/xof_cases.py; the experiments build's lane-per-state kernels run the same cases in a child process
(tests/exp_child_xof.py), since they are what tools/time_transcript.py measures the product against."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ringo import RingoError, _lib, xof
from tests import xof_cases as xc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
INV = _lib.STATUS["RG_ERR_INVALID"]


@pytest.mark.parametrize("n_states", [1, 3, 65])
@pytest.mark.parametrize("case", sorted(xc.CASES))
def test_parity_with_hashlib(case, n_states):
    triples = xc.CASES[case](n_states)
    assert triples
    assert xc.mismatches(triples) == []


def test_one_long_chain():
    assert xc.mismatches(xc.long_chain(1)) == []


def _refused(fn):
    with pytest.raises(RingoError) as e:
        fn()
    assert e.value.status == INV
    assert _lib.lib().rg_last_error().decode().startswith("xof:")


@pytest.mark.parametrize("n_states", [1, 3])
def test_refusals_leave_the_state_alone(n_states):
    """Each refused call changes neither the words nor the position or phase: the handle goes on to give
    the stream of the accepted calls alone."""
    n = n_states
    rng = np.random.default_rng(18)
    m = xc.rand_bytes(rng, n, 10)
    d = xc.dev(m)
    h, other = xof.Shake128(n), xof.Shake128(n + 1)
    h.absorb(d, 10)
    two_bases = xof.Plan([(0, 0, 10, 4), (1, 0, 10, 4)])
    _refused(lambda: h.absorb_plan(two_bases, [d]))                         # base 1 outside [-1, 1)
    _refused(lambda: h.absorb_plan(two_bases, [d] * (xof.MAX_BASES + 1)))   # n_bases above the limit
    _refused(lambda: h.absorb_plan(two_bases, [d, 0]))                      # a NULL base
    _refused(lambda: xof.Plan([(xof.LITERAL, 2, 0, 3)], b"abcd"))           # a literal run past the blob
    _refused(lambda: h.copy_from(other))
    _refused(lambda: other.copy_from(h))
    _refused(lambda: xc.check_null_out(h))
    o1, o2 = xc.Out(n, 16), xc.Out(n, 16)
    if n > 1:
        _refused(lambda: h.squeeze(o1.t, 16, out_stride=15))                # out_stride < len: still absorbing
        h.absorb(d, 0)
    h.squeeze(o1.t, 16, o1.stride)
    _refused(lambda: h.absorb(d, 10))                                       # absorb after squeeze
    _refused(lambda: h.absorb_plan(two_bases, [d, d]))
    if n > 1:
        _refused(lambda: h.squeeze(o2.t, 16, out_stride=15))
    h.squeeze(o2.t, 16, o2.stride)
    torch.cuda.synchronize()
    got = np.concatenate([o1.rows(), o2.rows()], axis=1)
    assert (got == np.stack([xc.shake(m[s].tobytes(), 32) for s in range(n)])).all()
    h.reset()                                                              # reset returns it to absorbing
    h.absorb(d, 10)


def test_lane_per_state_kernels_of_the_experiments_build():
    r = subprocess.run([sys.executable, os.path.join(HERE, "exp_child_xof.py")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "xof lane layout ok" in r.stdout
