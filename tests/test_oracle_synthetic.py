"""CPU: pin the oracle on the synthetic fields (tests/golden/synthetic_fields.json).

The GPU parity tests of test_gpu_ntt_synthetic.py compare the library bit-exactly with
oracle/oracle.c on moduli the reference never generated a package for, so nothing but this
file says the C oracle is right there.  As test_oracle.py does for the reference's fields:
  * the fixture is internally consistent (prime, bits, limbs, q mod 2^32, 2-adicity) and the
    generator reproduces it byte for byte;
  * C field ops == big-int ops == the word-level CIOS restatement, on the reference's static
    edge values, the vec tests' edge set and random values;
  * C tables == pyref tables, C forward / inverse NTT == pyref, at logN 3, 5, 7, cyclic and
    negacyclic, on random input and on the structured extremal batch the GPU tests feed.
"""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import coracle as co
import pyref
from tests import synth_util as su
from tests.test_oracle import static_values

NAMES = sorted(su.SYNTH)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_is_consistent(name):
    f = su.SYNTH[name]
    q = int(f["q_hex"], 16)
    assert pyref.is_prime(q)
    assert q.bit_length() == f["bits"]
    assert (f["bits"] + 63) // 64 == f["limbs"] and f["limbs"] in (1, 2, 4, 7, 14)
    assert q % (1 << 32) == f["q_mod_2_32"]
    k = f["two_adicity"]
    assert (q - 1) % (1 << k) == 0 and (q - 1) % (1 << (k + 1)) != 0
    assert k >= 17  # negacyclic rank 2^16 exists


def test_fixture_covers_the_intended_classes():
    q = {n: su.modulus(n) for n in NAMES}
    assert len(NAMES) == 9
    for n in ("s30", "s62_lo"):  # single-word Shoup fields off the q = 1 mod 2^32 shortcut
        assert q[n] < 1 << 63 and q[n] % (1 << 32) != 1
    assert q["s63_top"] < 1 << 63 and q["s63_top"] % (1 << 32) == 1 and 3 * q["s63_top"] > 1 << 64
    assert q["s64_gold"] >> 63 and q["s64_gold"] % (1 << 32) == 1  # no Shoup tables from 2^63 up
    assert q["s64_lo"] >> 63 and q["s64_lo"] % (1 << 32) != 1
    assert q["s256_top"] >> 255 and q["s256_top"] % (1 << 64) == 1
    assert q["s256_lo"] >> 255 and q["s256_lo"] % (1 << 64) != 1
    assert q["s448_top"] >> 447 and q["s896_top"] >> 895


def test_generator_reproduces_fixture(tmp_path):
    out = tmp_path / "synthetic_fields.json"
    gen = os.path.join(su.HERE, "golden", "make_synthetic_fields.py")
    subprocess.run([sys.executable, gen, str(out)], check=True, capture_output=True)
    assert out.read_bytes() == open(os.path.join(su.HERE, "golden", "synthetic_fields.json"), "rb").read()


@pytest.mark.parametrize("name", NAMES)
def test_field_ops_c_vs_bigint(name):
    q = su.modulus(name)
    F = pyref.Field(q)
    cf = co.CField(q)
    assert F.L == su.SYNTH[name]["limbs"] == cf.L
    qinv, r2, one = cf.consts()
    assert qinv == F.qInvNeg and r2 == F.rSquare and one == F.R % q
    rng = random.Random(99)
    vals = static_values(F) + su.edge_values(q, F.L) + [rng.randrange(q) for _ in range(48)]
    for x in vals:
        assert cf.neg(x) == F.neg(x) == (q - x) % q
        for y in vals[::3] + [q - x if x else 0, q - 1 - x]:  # x + y = q and x + y = q - 1
            m = F.mul(x, y)
            assert F.mont_cios(x, y) == m
            assert cf.mul(x, y) == m
            assert cf.add(x, y) == F.add(x, y) == (x + y) % q
            assert cf.sub(x, y) == F.sub(x, y) == (x - y) % q


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("cyclic", [False, True])
def test_transforms_c_vs_bigint(name, cyclic):
    q = su.modulus(name)
    F = pyref.Field(q)
    cf = co.CField(q)
    rng = np.random.default_rng(5)
    for logn in [3, 5, 7]:
        N = 1 << logn
        tw, twi, ninv, _ = (pyref.cyclic_tables if cyclic else pyref.cyclotomic_tables)(F, N)
        ctabs = cf.tables(N, cyclic=cyclic)
        assert co.from_limbs(ctabs[0]) == tw and co.from_limbs(ctabs[1]) == twi
        assert co.from_limbs(ctabs[2][None]) == [ninv]
        batch = su.structured_batch(cf, q, N, ctabs, len(su.STRUCTURED) + 2, rng)
        cfwd = cf.ntt_fwd(batch, ctabs[0])
        cinv = cf.ntt_inv(batch, ctabs[1], ctabs[2])
        for i in range(batch.shape[0]):
            a = co.from_limbs(batch[i])
            assert co.from_limbs(cfwd[i]) == pyref.ntt_fwd(F, a, tw), (logn, i)
            assert co.from_limbs(cinv[i]) == pyref.ntt_inv(F, a, twi, ninv), (logn, i)
        # the two pre-images do what they are for: every output lands on q - 1
        assert co.from_limbs(cfwd[su.STRUCTURED.index("pre_fwd_qm1")]) == [q - 1] * N
        assert co.from_limbs(cinv[su.STRUCTURED.index("pre_inv_qm1")]) == [q - 1] * N


@pytest.mark.parametrize("name", NAMES)
def test_rand_residues_are_canonical(name):
    q = su.modulus(name)
    L = su.SYNTH[name]["limbs"]
    v = co.from_limbs(su.rand_residues(q, L, 512, np.random.default_rng(0)))
    assert max(v) < q and len(set(v)) > 500
