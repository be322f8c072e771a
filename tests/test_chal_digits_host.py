"""CPU: the challenge digit routine and ChallengeBound (ringo-snark_amd/csrc/chal_digits.hpp, what
encode_chal_kernel runs per challenge on the device) compiled for the host from the same source into
the stand-alone program tools/san_chal_digits.cpp with the address and undefined-behaviour
sanitizers, and run: the program compares every digit with 128-bit integer division (utils.go:12-46)
and exits non-zero on a mismatch or a sanitizer report.  The GPU parity tests
(test_gpu_jindo_eval_point.py) pin the device build of the same code."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_chal_digits_under_sanitizers(tmp_path):
    exe = tmp_path / "san_chal_digits"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "ringo-snark_amd", "csrc"), os.path.join(ROOT, "tools", "san_chal_digits.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "chal_digits ok" in r.stdout
