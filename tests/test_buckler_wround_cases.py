"""CPU: the cases of tests/buckler_wround_util.py say what they claim, asserted on the reference's output
(buckler_dcmp_ref, the oracle's Encode), not the device's."""
import numpy as np
import pytest

from tests import buckler_wround_util as U


@pytest.mark.parametrize("key", U.FIELDS)
def test_the_dcmp_cases_hold_every_digit_a_residual_and_the_two_norm_extremes(key):
    _, ref = U.ctx(key)
    inf_digits, residuals, two_digits, sums = U.dcmp_census(key)
    assert inf_digits == {-1, 0, 1}
    assert residuals >= 1  # a coefficient beyond the sum of the base: no error
    assert any(s > ref.q >> 1 for s in sums) and -1 in two_digits  # a sum above q / 2: digits -1
    assert any(s == 0 for s in sums)  # the zero vector
    assert 1 in two_digits and 0 in two_digits


@pytest.mark.parametrize("key", U.LONG_KEYS)
def test_the_long_base_puts_digits_past_the_first_workgroup(key):
    """decomposeBase(2^300) has 300 digits, and the small sums land in its last few: the walk of the
    final kernel's second workgroup (entries 256 ..) has to pass through the first one's steps."""
    assert len(U.BASES[300]) == 300
    _, ref = U.ctx(key)
    for rank in (1024, 2500):
        assert "long_base" in U.tables_of(key, rank)
        row = U.two_want(key, rank, 2, 0, 300)[0]  # all q - 1: sqNm = rank
        nz = np.nonzero(row.any(axis=1))[0]
        assert len(nz) and nz.min() >= 256 and nz.max() < 300
    assert "long_base" not in U.tables_of(key, 200) and "long_base" not in U.tables_of("jindo_zp", 1024)


def test_the_tables_cover_the_shapes_the_issue_names():
    for name, (n_w, inf, two) in U.TABLES.items():
        rows = U.srcs_of(name) + U.outs_of(name)
        assert len(set(rows)) == len(rows) and len(rows) < n_w, name  # disjoint, and a bystander is left
    n_w, inf, two = U.TABLES["shared_src"]
    assert inf[0][0] == two[0][0]
    n_w, inf, two = U.TABLES["two_inf"]
    assert inf[0][1] != inf[1][1] and list(inf[1][2]) != list(range(inf[1][2][0], inf[1][2][0] + 3))
    assert not U.TABLES["only_two"][1] and not U.TABLES["only_inf"][2]
    assert {len(U.BASES[k]) for k in (1, 2, 3)} == {1, 2, 3} and sum(U.BASES[3]) == U.BOUND
    assert [200 % 256 != 0, 1024 % 1024 == 0, -(-2500 // 1024) == 3] == [True] * 3
    assert U.SELS["identity"][1] == tuple(range(U.SELS["identity"][0]))
    assert U.SELS["subset"] == (5, (3, 0)) and len(U.SELS["one_row"][1]) == 1


@pytest.mark.parametrize("key", ["p63", "zp880"])
def test_the_encode_cases_are_the_oracles(key):
    """RandEncode differs from Encode in coefficients 0 and rank only; zeros above."""
    rank, emb = 64, 128
    for i in range(U.N_PROOFS):
        plain, rnd = U.enc_want(key, rank, emb, i, 3, False), U.enc_want(key, rank, emb, i, 3, True)
        assert (plain[rank:] == 0).all() and (rnd[rank + 1:] == 0).all()
        assert (rnd[rank] == U.enc_draw(key, rank, i, 3)).all()
        assert (plain[1:rank] == rnd[1:rank]).all() and (plain[0] != rnd[0]).any()
