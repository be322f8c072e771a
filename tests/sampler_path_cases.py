"""The sampler-path cases shared by tests/test_oracle_sampler_paths.py (CPU: the oracle's path
census shows that each case reaches the branch it is there for, and bounds the words any COSAC
group draws) and tests/test_gpu_sampler_paths.py (GPU: the device's draws equal the oracle's).

The device samplers (csrc/jindo_sample.hip) are mostly data-dependent branches, and random `v` at
NewParameters' widths never takes several of them: the v1 side of a TwinCDT tail, the COSAC
streams' refill past 1024 words, the table-size thresholds.  The caller-settable stddevs
(rg_jindo_set_stddevs accepts any finite width above 0) reach them through the product library.

A case: the parameter set (golden/jindo_params.json), B commits of nv elements from first_commit,
the seed tag, the six stddevs (NewParameters' with `sd` overrides) and the pattern of v.

No case sets a COSAC width (ecd_blind, mask, mask_blind) below MIN_COSAC_SD: the sampler's loops
lengthen fast as the width shrinks (a plain simulation's median group draws ~6,800 words at 0.15),
and the device's lane loop is exactly as long as the oracle's.  WORD_CAP is what the CPU test
holds every case to before the GPU test may run it."""
import functools
import hashlib
import json
import os
from dataclasses import dataclass, field

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PARAMS = json.load(open(os.path.join(HERE, "golden", "jindo_params.json")))
SD_KEYS = ("ecd_sd", "ecd_blind_sd", "mask_sd", "mask_blind_sd", "mlwe_sd", "mask_mlwe_sd")
SEED_NAMES = ("enc_cdt", "enc_cosac", "enc_cosac_round", "mlwe_cdt", "mlwe_round", "uniform")  # rg_jindo_seeds
COSAC_SD_KEYS = ("ecd_blind_sd", "mask_sd", "mask_blind_sd")
MIN_COSAC_SD = 0.18
WORD_CAP = 16384


@dataclass(frozen=True)
class Case:
    id: str
    params: str            # key of golden/jindo_params.json
    B: int
    nv: int
    first: int             # first_commit
    tag: bytes             # the six seeds are SHA-256(tag || name), as ringo.jindo.Seeds.derive
    sd: tuple = ()         # ((key, width), ...) overriding NewParameters' stddevs
    v: str = "random"      # random | zero | qm1 | digits
    refused: bool = False  # the device refuses the shape (RG_ERR_UNSUPPORTED); the oracle still draws
    sizes: tuple = None    # (encode, MLWE) TwinCDT table entries the case is there for, None: any
    expect: dict = field(default_factory=dict, hash=False, compare=False)  # census minima (CPU test)

    @property
    def P(self):
        return PARAMS[self.params]

    @property
    def q(self):
        return int(self.P["field_q_hex"], 16)

    def stddevs(self):
        o = dict(self.sd)
        assert set(o) <= set(SD_KEYS)
        return tuple(float(o.get(k, self.P[k])) for k in SD_KEYS)

    def seeds_raw(self):
        return b"".join(hashlib.sha256(self.tag + k.encode()).digest() for k in SEED_NAMES)

    def make_v(self):
        """[B][nv][L] Montgomery words"""
        from tests.jindo_util import make_v
        q, L = self.q, (self.q.bit_length() + 63) // 64
        if self.v == "random":
            return np.stack([make_v(q, self.nv, seed=1000 + b) for b in range(self.B)])
        if self.v == "zero":  # digits 0: the interior rows' deltaInv sums are +0, their centres -0.0
            x = 0
        elif self.v == "qm1":  # the largest representative in every word
            x = q - 1
        elif self.v == "digits":  # the value b^exp - 1: every base-b digit is b - 1 (baseEncodeTo reads fromMont(v))
            x = (self.P["base"] ** self.P["exp"] - 1) * (1 << (64 * L)) % q
        else:
            raise ValueError(self.v)
        row = np.array([(x >> (64 * j)) & ((1 << 64) - 1) for j in range(L)], np.uint64)
        return np.ascontiguousarray(np.broadcast_to(row, (self.B, self.nv, L)))


SMALL_ECD = (("ecd_sd", 0.2),)
LONG_COSAC = (("ecd_blind_sd", 0.18), ("mask_sd", 0.2), ("mask_blind_sd", 0.22))

CASES = [
    # small-ecd: the tables of neighbouring centres disagree often, and the reference's tail sum
    # (x from tailLo to the table INDEX v0) stops short of 1, so both tail outcomes occur.  At 0.2
    # the centre-0 tables saturate (cdf > 1: entries 2^64 - 1, repeated).
    Case("small_ecd_0.2", "t10_b1", 1, 1024, 0, b"paths-ecd02", SMALL_ECD, sizes=(5, 123),
         expect=dict(cdt_tail_v0=30, cdt_tail_v1=30)),
    Case("small_ecd_0.45", "t10_b8", 1, 700, 5, b"paths-ecd045", (("ecd_sd", 0.45),), sizes=(11, 123),
         expect=dict(cdt_tail_v0=1, cdt_tail_v1=1)),
    # long-cosac: groups of 8 samples that draw past the first 1024 words of either stream
    Case("long_cosac_b1", "t10_b1", 1, 1024, 0, b"paths-cosac", LONG_COSAC,
         expect=dict(cos_over_base=20, cos_over_rnd=5, cos_zig_tail=5)),
    Case("long_cosac_b8", "t10_b8", 1, 700, 2, b"paths-cosac8", LONG_COSAC,
         expect=dict(cos_over_base=20, cos_over_rnd=5)),
    # table edges: the last encode table the device accepts (kCdtLdsMaxSize = 96; sizes are odd) and
    # the first it refuses; the MLWE table on either side of kMlweLdsTab = 512; the smallest tables
    Case("ecd_table_95", "t10_b1", 1, 1024, 1, b"paths-t95", (("ecd_sd", 5.2),), sizes=(95, 123)),
    Case("ecd_table_97", "t10_b1", 1, 64, 1, b"paths-t97", (("ecd_sd", 5.3),), sizes=(97, 123), refused=True),
    Case("mlwe_table_511", "t10_b1", 1, 300, 0, b"paths-m511", (("mlwe_sd", 28.3),), sizes=(89, 511)),
    Case("mlwe_table_513", "t10_b1", 1, 300, 0, b"paths-m513", (("mlwe_sd", 28.4),), sizes=(89, 513)),
    Case("tables_5", "t10_b8", 1, 700, 0, b"paths-t5",
         (("ecd_sd", 0.12), ("mlwe_sd", 0.12), ("mask_mlwe_sd", 0.12)), sizes=(5, 5)),
    # structured v at the reference's widths
    Case("v_zero", "t10_b1", 1, 1024, 0, b"paths-v0", v="zero"),
    Case("v_qm1", "t10_b1", 1, 1024, 0, b"paths-vq", v="qm1"),
    Case("v_digits", "t10_b8", 1, 700, 0, b"paths-vd", v="digits"),
    Case("nv_1", "t10_b1", 2, 1, 3, b"paths-nv1", expect=dict(ml_zig_tail=5)),
    Case("nv_rank", "t10_b8", 2, 1024, 0, b"paths-nvr", expect=dict(ml_zig_tail=5)),
    # combined: small-ecd and long-cosac at once (also the sampled commit, end to end).  At ecd_sd =
    # mask_sd = 0.2 the mask column's rows >= 1 go to TwinCDT, as in the reference, which picks the
    # sampler by `stdDev == twinCDT.StdDev()` (encoder.go:168): 96 COSAC groups are left.  Then at 0.3
    # (no such collision) with instance numbers past 2^40 (the window start carries into the
    # counter's high word)
    Case("combined", "t10_b1", 1, 1024, 0, b"paths-comb", SMALL_ECD + LONG_COSAC, sizes=(5, 123),
         expect=dict(cdt_tail_v0=30, cdt_tail_v1=30, cos_over_base=20, cos_over_rnd=5)),
    Case("combined_2e40", "t10_b1", 1, 1024, (1 << 40) + 12345, b"paths-comb40",
         (("ecd_sd", 0.3),) + LONG_COSAC, sizes=(7, 123),
         expect=dict(cdt_tail_v0=30, cdt_tail_v1=30, cos_over_base=20, cos_over_rnd=5)),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
COMBINED = ("combined", "combined_2e40")


@functools.lru_cache(maxsize=None)
def oracle_draws(case_id):
    """(draws, census) of the C oracle for one case; computed once per process, read-only"""
    import coracle as co
    import pyref
    c = BY_ID[case_id]
    P = c.P
    draws, census = co.CJindo(P, c.q).sample(c.stddevs(), pyref.delta_inv(P["base"], P["exp"]), c.seeds_raw(),
                                             c.first, c.make_v(), census=True)
    for a in draws.values():
        a.setflags(write=False)
    return draws, census
