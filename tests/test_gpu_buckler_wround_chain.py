"""GPU: a witness table stays on the device, in one layout, from the assignment to the d_w of
rg_buckler_prove_checks_dev.  One chained case at rank 256 on jindo_zp with three proofs: the dcmp round,
the first encode round, rg_buckler_prove_proj_round_dev, the second encode round and ONE in-place forward
NTT of the whole table.  The final table must equal the oracle's Encode + NTT of each row of the
reference's final witness table (buckler_dcmp_ref, buckler_lin_ref.ProjChecker)."""
import numpy as np
import pytest

import ringo
from ringo import buckler
from tests import buckler_dcmp_ref as D
from tests import buckler_lin_ref as R
from tests import buckler_wround_util as U

pytestmark = pytest.mark.gpu

KEY, RANK, EMB, N_W = "jindo_zp", 256, 512, 7
A_ROW, INF_ROWS, TWO_ROW, B_ROW, PROJ_ROW, PDCMP_ROW = 0, (1, 2), 3, 4, 5, 6
FIRST, SECOND = (0, 1, 2, 3, 4), (5, 6)  # the rows of the two commit rounds (ctx.wSecond: proj and its digits)
IDX = (0, 3, 4)  # small signed entries, every entry bound + 1, random full-width entries


def _reference(ref, i, xof):
    """The reference's final plain table of proof i, as limbs [N_W][RANK][L]."""
    a, b = list(U.witness(KEY, RANK, i, A_ROW)), list(U.witness(KEY, RANK, i, B_ROW))
    digits = D.infDcmp(ref, a, list(U.BASES[2]))
    two, _ = D.twoDcmp(ref, a, list(U.BASES[3]))
    proj = R.ProjChecker(ref, RANK).set_xof(xof).transform(a)
    pdcmp = D.projDcmp(ref, proj, list(U.BASES[2]), RANK)
    return np.stack([ref.arr(r) for r in (a, digits[0], digits[1], two, b, proj, pdcmp)])


def test_the_table_stays_on_the_device_from_assignment_to_the_checks():
    import torch
    F, ref = U.ctx(KEY)
    L, n = F.L, len(IDX)
    rng = np.random.default_rng(2024)
    xofs = [rng.bytes(32 * RANK) for _ in IDX]
    draws = np.stack([np.stack([U.enc_draw(KEY, RANK, i, r) for r in range(N_W)]) for i in IDX])  # [n][N_W][L]
    plain = np.stack([_reference(ref, i, x) for i, x in zip(IDX, xofs)])
    tw = ref.cf.tables(EMB, cyclic=True)[0]
    want = np.stack([ref.cf.ntt_fwd(np.stack([ref.cf.buckler_encode(plain[k, r], EMB, rnd=draws[k, r])
                                              for r in range(N_W)]), tw) for k in range(n)])
    want_com = np.stack([np.stack([ref.cf.buckler_encode(plain[k, r], EMB, rnd=draws[k, r])[:RANK + 1]
                                   for r in range(N_W)]) for k in range(n)])

    dc2, dc3 = buckler.Decomposer(F, list(U.BASES[2])), buckler.Decomposer(F, list(U.BASES[3]))
    dcmp = buckler.DcmpRoundPlan(F, RANK, N_W, inf=[(A_ROW, dc2, INF_ROWS)], two=[(A_ROW, dc3, TWO_ROW)])
    enc1 = buckler.EncodeRoundPlan(F, RANK, EMB, N_W, FIRST)
    enc2 = buckler.EncodeRoundPlan(F, RANK, EMB, N_W, SECOND)
    proj = buckler.ProjRoundPlan(F, RANK, N_W, [(A_ROW, PROJ_ROW, PDCMP_ROW, dc2)])
    emb_plan = ringo.bigpoly.NewCyclicTransformer(F, EMB)

    start = np.full((n, N_W, RANK, L), U.FF, np.uint64)  # the assignment: only the free witnesses are set
    start[:, A_ROW], start[:, B_ROW] = plain[:, A_ROW], plain[:, B_ROW]
    d_w = U.dev_guarded(start, L)
    d_e = U.filled(n * N_W * EMB * L, L)
    d_c1, d_c2 = U.filled(n * len(FIRST) * (RANK + 1) * L, L), U.filled(n * len(SECOND) * (RANK + 1) * L, L)
    d_r1, d_r2 = U.dev(draws[:, list(FIRST)]), U.dev(draws[:, list(SECOND)])
    d_x = U.dev(np.frombuffer(b"".join(xofs), np.uint8).copy(), np.uint8)
    words = max(dcmp.scratch_bytes(n), enc1.scratch_bytes(n), proj.scratch_bytes(n), enc2.scratch_bytes(n)) // 8
    d_s = U.filled(words, L)  # one scratch: the calls follow each other on one stream

    dcmp.round_dev(n, d_w, None, d_s)
    enc1.round_dev(n, d_w, d_e, d_rand=d_r1, d_com=d_c1, d_scratch=d_s)
    proj.round_dev(n, d_w, d_x, d_s)
    enc2.round_dev(n, d_w, d_e, d_rand=d_r2, d_com=d_c2, d_scratch=d_s)
    emb_plan.fwd_dev(d_e, d_e, n * N_W)
    torch.cuda.synchronize()

    U.unguard(d_s, (words,), L, "the scratch")
    assert (U.unguard(d_w, plain.shape, L, "the plain table") == plain).all()
    got = U.unguard(d_e, want.shape, L, "the encoded table")
    for k in range(n):
        for r in range(N_W):
            assert (got[k, r] == want[k, r]).all(), (k, r)
    assert (U.unguard(d_c1, (n, len(FIRST), RANK + 1, L), L, "com 1") == want_com[:, list(FIRST)]).all()
    assert (U.unguard(d_c2, (n, len(SECOND), RANK + 1, L), L, "com 2") == want_com[:, list(SECOND)]).all()
