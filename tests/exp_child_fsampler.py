"""Test helper run as a child process on the experiments build (libringo_exp.so), as tests/exp_child.py
is: the tries cap of the whole-word kernels (RINGO_JINDO_UNI_TRIES) is honoured only there, and one
process loads one libringo.  Never imported by the product.

  python tests/exp_child_fsampler.py <tries> <out.npz>
      with RINGO_JINDO_UNI_TRIES=<tries>, at q255 and the seed of tests/set_random_ref.py:
      elems    rg_field_sampler_elems_dev, instances 0 .. 599
      mask, com, sum   rg_buckler_sumcheck_mask_batch_sampled_dev, (rank, mask_rank, emb_rank) =
               (128, 256, 256), 2 proofs, first_instance 2^32 - 100
      every output into a buffer pre-filled with -1
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ringo-snark_amd"), os.path.join(ROOT, "oracle"), ROOT]
os.environ["RINGO_LIB"] = os.path.join(ROOT, "ringo-snark_amd", "lib", "libringo_exp.so")

import numpy as np  # noqa: E402


def main(tries, out):
    import torch

    import ringo
    from ringo import buckler
    from tests import set_random_ref as sr
    os.environ["RINGO_JINDO_UNI_TRIES"] = tries
    F = ringo.Field(sr.modulus(sr.Q255))
    S = buckler.FieldSampler(F, sr.SEED)
    L = F.L

    def filled(words):
        return torch.full((words,), -1, dtype=torch.int64, device="cuda")

    d_el = filled(sr.FIXUP_ELEMS * L)
    S.elems_dev(0, sr.FIXUP_ELEMS, d_el, filled(S.scratch_bytes() // 8))
    m = sr.FIXUP_MASK
    d_mask, d_com, d_sum = (filled(m["n_proofs"] * k * L) for k in (m["emb"], m["mask_rank"], 1))
    buckler.sumcheck_mask_batch_sampled_dev(S, m["rank"], m["mask_rank"], m["emb"], m["n_proofs"], m["first"], d_mask,
                                            d_sum, filled(S.scratch_bytes() // 8), d_mask_com=d_com)
    torch.cuda.synchronize()
    np.savez(out, elems=d_el.cpu().numpy(), mask=d_mask.cpu().numpy(), com=d_com.cpu().numpy(),
             sum=d_sum.cpu().numpy())


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
