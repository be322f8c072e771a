"""CPU: the oracle's path census (oracle.c of_jindo_sample_census) over tests/sampler_path_cases.py.

The GPU test (test_gpu_sampler_paths.py) compares the device's draws with the oracle's; that only
tests a branch of the device samplers if the oracle's draws take it.  So every case is run here
with the census, and what the case is there for is asserted: both outcomes of a TwinCDT tail,
COSAC groups past the first 1024 words of either stream, the table sizes on both sides of the
kernels' thresholds, the ziggurat's tail in both rounded samplers.

Safety condition for the GPU: the device draws exactly the words the oracle draws, so the oracle's
largest per-group word count bounds cosac2_noise_kernel's longest lane loop.  Every case stays
under WORD_CAP words per group and stream, and no case sets a COSAC width below MIN_COSAC_SD.

The oracle itself is pinned at the new widths where the reference pins anything: TwinCDT draws at
sigma 0.2 and 0.3 against a direct Python restatement of gaussian_twin_cdt.go."""
import math

import numpy as np
import pytest

import coracle as co
import pyref
from tests import sampler_path_cases as spc

IDS = [c.id for c in spc.CASES]


@pytest.mark.parametrize("cid", IDS)
def test_case_reaches_its_paths(cid):
    c = spc.BY_ID[cid]
    _, cs = spc.oracle_draws(cid)
    print(cid, cs)
    # the words any COSAC group draws from either stream: the device's longest lane loop
    assert 0 < cs["cos_max_base"] <= spc.WORD_CAP and 0 < cs["cos_max_rnd"] <= spc.WORD_CAP
    sd = dict(zip(spc.SD_KEYS, c.stddevs()))
    assert all(sd[k] >= spc.MIN_COSAC_SD for k in spc.COSAC_SD_KEYS)
    assert c.B <= 3 and c.params in ("t10_b1", "t10_b8")
    if c.sizes is not None:
        assert (cs["cdt_enc_size"], cs["cdt_mlwe_size"]) == c.sizes
    for k, least in c.expect.items():
        assert cs[k] >= least, (k, cs[k], least)
    assert cs["cdt_tails"] == cs["cdt_tail_v0"] + cs["cdt_tail_v1"] <= cs["cdt_draws"]
    assert cs["cos_over_base"] <= cs["cos_groups"] and cs["cos_over_rnd"] <= cs["cos_groups"]


def test_cases_cover_what_the_issue_lists():
    """the conditions of the case table as a whole"""
    cen = {cid: spc.oracle_draws(cid)[1] for cid in IDS}
    c02 = cen["small_ecd_0.2"]
    assert c02["cdt_tail_v0"] >= 30 and c02["cdt_tail_v1"] >= 30
    for cid in ("long_cosac_b1", "long_cosac_b8"):
        assert cen[cid]["cos_over_base"] >= 20 and cen[cid]["cos_over_rnd"] >= 5, (cid, cen[cid])
    assert max(c["cos_zig_tail"] for c in cen.values()) >= 5 and max(c["ml_zig_tail"] for c in cen.values()) >= 5
    assert min(c["cos_zig_wedge"] for c in cen.values()) > 0 and min(c["ml_zig_wedge"] for c in cen.values()) > 0
    sizes = {(c["cdt_enc_size"], c["cdt_mlwe_size"]) for c in cen.values()}
    assert {(95, 123), (97, 123), (89, 511), (89, 513), (5, 5)} <= sizes
    # at the reference's widths the v1 side of a tail is never drawn: what the small-ecd cases are for
    for cid in ("v_zero", "v_qm1", "v_digits", "nv_1", "nv_rank"):
        assert cen[cid]["cdt_tail_v1"] == 0 and cen[cid]["cos_over_base"] == 0
    # the refused shape is the only one the GPU test does not draw
    assert [c.id for c in spc.CASES if c.refused] == ["ecd_table_97"]


def test_structured_v_centres():
    """v = 0: the interior TwinCDT rows' centres are -0.0, so every such row's draws are centred
    draws of table 0 with no tail (the few tails are the last row's, encoded from lastRow)."""
    c = spc.BY_ID["v_zero"]
    en = spc.oracle_draws("v_zero")[0]["enc_noise"]
    hi = math.ceil(9 * c.P["ecd_sd"])
    assert np.abs(en[0, :c.P["cols"], 1:-1]).max() <= hi + 1  # v0 = size: one past the table
    cs = spc.oracle_draws("v_zero")[1]
    assert cs["cdt_tails"] < 256 * c.P["cols"]


def test_census_leaves_the_draws_alone():
    for cid in ("small_ecd_0.2", "long_cosac_b8"):
        c = spc.BY_ID[cid]
        plain = co.CJindo(c.P, c.q).sample(c.stddevs(), pyref.delta_inv(c.P["base"], c.P["exp"]), c.seeds_raw(),
                                           c.first, c.make_v())
        got = spc.oracle_draws(cid)[0]
        for k in plain:
            assert plain[k].tobytes() == got[k].tobytes(), (cid, k)


# ---- gaussian_twin_cdt.go restated directly (Python floats are Go's float64; math.exp is this
# machine's libm, as in oracle.c: parity of libm with Go's math.Exp is unpinned, test_oracle_samplers.py)
def _go_u64(x):  # uint64(float64) on amd64 for the values computeCDT produces
    return int(x) if x < 2.0 ** 63 else (int(x - 2.0 ** 63) if x - 2.0 ** 63 < 2.0 ** 63 else 0) | (1 << 63)


def _go_round(x):  # math.Round for x >= 0
    return x if x >= 2.0 ** 52 else math.floor(x + 0.5)


def _compute_cdt(center, sigma):  # gaussian_twin_cdt.go:13-33
    hi = int(math.ceil(9 * sigma))
    cdf, norm, t = 0.0, math.sqrt(2 * math.pi) * sigma, []
    for x in range(-hi, hi + 1):
        xf = float(x)
        cdf += math.exp(-(xf - center) * (xf - center) / (2 * sigma * sigma)) / norm
        t.append((1 << 64) - 1 if cdf > 1 else _go_u64(_go_round(cdf * 2.0 ** 64)))
    return t


def _bsearch(t, u):  # slices.BinarySearch
    i, j = 0, len(t)
    while i < j:
        h = (i + j) >> 1
        if t[h] < u:
            i = h + 1
        else:
            j = h
    return i, i < len(t) and t[i] == u


def _twin_cdt_sample(tables, sigma, center, u):  # Sample, gaussian_twin_cdt.go:77-111
    tail_lo = -int(math.ceil(9 * sigma))
    c_floor = math.floor(center)
    c_frac = center - c_floor
    c0, c1 = int(math.floor(128 * c_frac)) % 128, int(math.ceil(128 * c_frac)) % 128
    v0, ok = _bsearch(tables[c0], u)
    v0 -= 1 if ok else 0
    v1, ok = _bsearch(tables[c1], u)
    v1 -= 1 if ok else 0
    if v0 == v1:
        return v0 + int(c_floor) + tail_lo, None
    cdf, norm = 0.0, math.sqrt(2 * math.pi) * sigma
    for x in range(tail_lo, v0 + 1):
        xf = float(x)
        cdf += math.exp(-(xf - c_frac) * (xf - c_frac) / (2 * sigma * sigma)) / norm
    p = float(u) / 2.0 ** 64
    return (v0 if p < cdf else v1) + tail_lo + int(c_floor), p < cdf


@pytest.mark.parametrize("sigma", [0.2, 0.3])
@pytest.mark.parametrize("center", [0.0, 37 / 128, -3 + 127 / 128, 0.3, -2.71, 0.999, 5.004])
def test_oracle_twin_cdt_matches_restatement(sigma, center):
    """of_sampler_draws' TwinCDT at the small widths, draw for draw, centres on the 1/128 grid
    (c0 == c1: no tail) and off it; off the grid both tail outcomes occur."""
    n = 4000
    seed = b"twin-%r-%r" % (sigma, center)
    got = co.sampler_draws("twin_cdt", seed.ljust(32, b".")[:32] + bytes(32), sigma, center, n, per_inst=n)
    u = pyref.UniformSampler(seed.ljust(32, b".")[:32])
    tables = [_compute_cdt(i / 128, sigma) for i in range(128)]
    want, sides = zip(*[_twin_cdt_sample(tables, sigma, center, u.sample()) for _ in range(n)])
    assert list(got) == list(want)
    on_grid = (128 * center) == math.floor(128 * center)
    if on_grid:
        assert all(s is None for s in sides)
    elif center in (0.3, -2.71):
        assert sides.count(True) >= 3 and sides.count(False) >= 3, (sides.count(True), sides.count(False))


@pytest.mark.parametrize("sigma", [0.12, 0.2, 0.3, 0.45, 0.7, 4.787466224214409, 5.2])
def test_tail_cdf_bounds_over_a_centre_interval(sigma):
    """What cdt2_noise_kernel's tail bounds rest on (rg_jindo_set_stddevs): over cFrac in
    [c, c + 1] / 128 the reference's tail cdf f_j(cFrac) = sum_{x = tailLo}^{j} rho(x - cFrac) / norm
    lies between min and max of its two end values widened by h^2 / 8 (2 + 1.14 / sigma) / sigma^2,
    h = 1/128 -- checked here at 8 points inside every interval for every j.  The simpler
    'f_j falls with the centre' (end values alone, upper end at c) holds at NewParameters' widths
    and fails at small ones: the lattice sum swings with the centre by 2 exp(-2 pi^2 sigma^2), which
    is below the kernel's 2^-40 band only from sigma ~ 1.2 up.  The small-ecd cases caught it."""
    T = math.ceil(9 * sigma)
    x = np.arange(-T, 2 * T + 2, dtype=np.float64)  # x = tailLo .. size: every j the kernel can index
    c = np.arange(0, 128 * 8 + 1, dtype=np.float64) / (128 * 8)
    f = np.cumsum(np.exp(-(x[None, :] - c[:, None]) ** 2 / (2 * sigma * sigma)) / (math.sqrt(2 * math.pi) * sigma), axis=1)
    a, b = f[0:-1:8], f[8::8]  # the ends of the 128 intervals, [128][j]
    chord = (2 + 1.14 / sigma) / (sigma * sigma) / (8 * 128 * 128)
    inner = np.stack([f[k:-1:8] for k in range(8)])  # [8][128][j]
    slack = 1e-12  # float sums
    assert (inner >= np.minimum(a, b) - chord - slack).all() and (inner <= np.maximum(a, b) + chord + slack).all()
    falls = (inner <= a + slack).all() and (inner >= b - slack).all()
    assert falls == (sigma > 1.2)
