"""GPU: the long-draw fix-up of the field sampler's whole-word route and of the sampled mask.  A draw
needs more tries than the whole-word kernels make with probability 0.475^256 at q255, so the fix-up
launches (fs_fix_kernel, mask_sampled_chain_kernel<WHOLE>) are reached only on the experiments build
with the tries capped (RINGO_JINDO_UNI_TRIES, tests/exp_child_fsampler.py): at 0 every draw is left
to the fix-up, at 1 the ~47% rejected on their first try are -- and in the mask, chains whose first,
second or both draws are.  The outputs still equal tests/set_random_ref.py's draws, bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import buckler_lin_ref as R
from tests import set_random_ref as sr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("tries", [0, 1])
def test_long_draws_fixup(tmp_path, tries):
    out = tmp_path / f"fs_{tries}.npz"
    r = subprocess.run([sys.executable, os.path.join(HERE, "exp_child_fsampler.py"), str(tries), str(out)],
                       capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {k: v.view(np.uint64) for k, v in np.load(out).items()}
    q = sr.modulus(sr.Q255)
    ref = R.Ref(q)
    vals, t_el = sr.draws(sr.SEED, q, 0, sr.FIXUP_ELEMS)
    assert sum(t > 1 for t in t_el) >= 30  # (tries = 1: both kernels write elements)
    assert (got["elems"].reshape(-1, ref.L) == sr.limbs(vals, q, ref.L)).all()
    m = sr.FIXUP_MASK
    vals, t_mk = sr.draws(sr.SEED, q, m["first"], m["n_proofs"] * m["mask_rank"])
    # chains (k, k + rank) of every kind: neither draw long, the first, the second, both
    kinds = {(t_mk[p * m["mask_rank"] + c] > 1, t_mk[p * m["mask_rank"] + m["rank"] + c] > 1)
             for p in range(m["n_proofs"]) for c in range(m["rank"])}
    assert len(kinds) == 4
    for p in range(m["n_proofs"]):
        rand = list(vals[p * m["mask_rank"]:(p + 1) * m["mask_rank"]])
        mask, msum = R.sumCheckMask(ref, m["rank"], m["mask_rank"], m["emb"], rand)
        want = ref.arr(mask)
        assert (got["mask"].reshape(m["n_proofs"], m["emb"], ref.L)[p] == want).all(), p
        assert (got["com"].reshape(m["n_proofs"], m["mask_rank"], ref.L)[p] == want[:m["mask_rank"]]).all(), p
        assert (got["sum"].reshape(m["n_proofs"], ref.L)[p] == ref.arr([msum])[0]).all(), p
