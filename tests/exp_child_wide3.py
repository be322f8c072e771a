"""Test helper run as a child process on the experiments build (libringo_exp.so), as tests/exp_child.py
is: RINGO_NTT_KERNEL=w3, which forces the wide fields' three-pass split (ntt_route.hpp ntt_wide_long)
onto ranks from 2^3 up, is honoured only there, and one process loads one libringo.  Never imported by
the product.

  python tests/exp_child_wide3.py <out.npz>
      for every case of CASES: the plan's route in both directions, and on the input inputs(case)
      fwd / inv out of place (fo, io: into a buffer pre-filled with -1) and in place (fi, ii), keys
      "<field>-<logN>-<batch>-<c|n>-<what>"
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (field, logN, batch, negacyclic): the middle pass at the smallest ranks; batch 3 leaves the last
# row tile partly past the batch
CASES = [(f, lg, b, neg) for f in ("zp440", "zp880") for lg in (3, 7, 9, 12) for b in (1, 3) for neg in (False, True)]


def key(case, what):
    f, lg, b, neg = case
    return f"{f}-{lg}-{b}-{'n' if neg else 'c'}-{what}"


def inputs(case):
    """[batch, N, L] residues: polynomial 0 is q - 1 in its first half and zero in its second, the
    rest uniform."""
    from tests import synth_util as su
    f, lg, b, neg = case
    q = su.modulus(f)
    L = (q.bit_length() + 63) // 64
    N = 1 << lg
    rng = np.random.default_rng(7000 + 100 * lg + 10 * b + neg + (L == 14) * 5)
    a = su.rand_residues(q, L, b * N, rng).reshape(b, N, L)
    a[0, :N // 2] = su.limbs_of(q - 1, L)
    a[0, N // 2:] = 0
    return a


def main(out):
    import torch

    import ringo
    from tests import synth_util as su
    os.environ["RINGO_NTT_KERNEL"] = "w3"  # read when a plan is created
    res = {}
    fields = {}
    for case in CASES:
        f, lg, b, neg = case
        F = fields.setdefault(f, ringo.Field(su.modulus(f)))
        T = (ringo.CyclotomicTransformer if neg else ringo.CyclicTransformer)(F, 1 << lg)
        routes = [T.route(False), T.route(True)]
        res[key(case, "route")] = np.array([r[0] == "wide" and r[1] for r in routes], np.int64)
        a = inputs(case)
        x = torch.from_numpy(a.view(np.int64).reshape(-1).copy()).cuda()
        for what, fn in (("f", T.fwd_dev), ("i", T.inv_dev)):
            y = torch.full_like(x, -1)
            fn(y, x, b)  # out of place
            z = x.clone()
            fn(z, z, b)  # in place
            torch.cuda.synchronize()
            res[key(case, what + "o")] = y.cpu().numpy()
            res[key(case, what + "i")] = z.cpu().numpy()
        assert (x.cpu().numpy().view(np.uint64).reshape(a.shape) == a).all(), "out-of-place call wrote its input"
    np.savez(out, **res)


if __name__ == "__main__":  # (the GPU test imports CASES, key and inputs: nothing above touches the process)
    sys.path[:0] = [os.path.join(ROOT, "ringo-snark_amd"), os.path.join(ROOT, "oracle"), ROOT]
    os.environ["RINGO_LIB"] = os.path.join(ROOT, "ringo-snark_amd", "lib", "libringo_exp.so")
    main(sys.argv[1])
