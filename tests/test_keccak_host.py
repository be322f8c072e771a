"""CPU: Keccak-f[1600] and the SHAKE128 sponge index algebra of ringo-snark_amd/csrc/keccak.hpp (what the
rg_xof_* kernels run on the device) compiled for the host from the same source into the stand-alone
program tools/san_keccak.cpp with the address and undefined-behaviour sanitizers, and run on a case
file written here with hashlib.shake_128: the program exits non-zero on a mismatch or a sanitizer
report.  The GPU parity tests (test_gpu_xof.py) pin the device build of the same code."""
import hashlib
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

LENGTHS = [0, 1, 7, 8, 166, 167, 168, 169, 335, 336, 337, 1000]
READS = [1, 16, 167, 168, 169, 500]


def _hex(b):
    return b.hex() if b else "-"


def _case(chunks, reads):
    want = hashlib.shake_128(b"".join(chunks)).digest(sum(reads))
    return f"{','.join(_hex(c) for c in chunks)} {','.join(str(r) for r in reads)} {want.hex()}"


def _sixteens(n):
    return [16] * (n // 16) + ([n % 16] if n % 16 else [])


def cases():
    rng = np.random.default_rng(1600)
    msg = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    out = []
    for n in LENGTHS:  # each absorbed whole, squeezed whole and as successive 16-byte reads
        m = msg(n)
        for r in READS:
            out.append(_case([m], [r]))
            out.append(_case([m], _sixteens(r)))
    m = msg(200)
    for cut in range(201):  # two absorbs at every cut
        out.append(_case([m[:cut], m[cut:]], [32]))
    return out


def test_keccak_under_sanitizers(tmp_path):
    exe = tmp_path / "san_keccak"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "ringo-snark_amd", "csrc"), os.path.join(ROOT, "tools", "san_keccak.cpp"),
                    "-o", str(exe)], check=True)
    lines = cases()
    assert len(lines) == len(LENGTHS) * len(READS) * 2 + 201
    case_file = tmp_path / "cases.txt"
    case_file.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(case_file)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"keccak ok: {len(lines)} cases" in r.stdout
