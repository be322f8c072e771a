"""Test helper run as a child process on the experiments build (libringo_exp.so), as tests/exp_child.py
is: with RINGO_XOF_LAYOUT=lane every rg_xof_* call runs the lane-per-state kernels of xof.hip
(keccak.hpp's scalar permutation, one state per lane), on the cases of tests/xof_cases.py.

  python tests/exp_child_xof.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ringo-snark_amd"), os.path.join(ROOT, "oracle"), ROOT]
os.environ["RINGO_LIB"] = os.path.join(ROOT, "ringo-snark_amd", "lib", "libringo_exp.so")
os.environ["RINGO_XOF_LAYOUT"] = "lane"  # read when a handle is created

if __name__ == "__main__":
    from tests import xof_cases as xc
    bad = []
    for n in (1, 3, 65):
        for name, fn in sorted(xc.CASES.items()):
            bad += [f"{name}[{n}]: {label}" for label in xc.mismatches(fn(n))]
    bad += [f"long_chain: {label}" for label in xc.mismatches(xc.long_chain(1))]
    if bad:
        print("\n".join(bad))
        raise SystemExit(1)
    print("xof lane layout ok")
