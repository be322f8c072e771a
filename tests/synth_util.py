"""Shared by the synthetic-field tests (test_oracle_synthetic.py on the CPU,
test_gpu_ntt_synthetic.py on the GPU): the fixture loader, a vectorised sampler of canonical
residues, and the structured extremal input batch.

Everything here works on raw limb values, the domain the kernels work in: "q - 1" is the
residue whose limbs are those of q - 1 (the largest canonical value), whatever it means in
Montgomery form."""
import functools
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SYNTH = json.load(open(os.path.join(HERE, "golden", "synthetic_fields.json")))
_GOLDEN = json.load(open(os.path.join(HERE, "golden", "fields.json")))

M64 = (1 << 64) - 1


def modulus(name):
    """q of a synthetic field or of one of the reference's fields."""
    return int((SYNTH.get(name) or _GOLDEN[name])["q_hex"], 16)


def limbs_of(v, L):
    return np.array([(v >> (64 * i)) & M64 for i in range(L)], dtype=np.uint64)


def rand_residues(q, L, n, rng):
    """[n, L] canonical residues without per-element big-int work: low limbs uniform, the top
    limb uniform below q's top limb (for L = 1: uniform below q).  Every value is < q; the sliver
    of residues sharing q's top limb is left to the structured inputs."""
    top = q >> (64 * (L - 1))
    out = rng.integers(0, 1 << 64, size=(n, L), dtype=np.uint64)
    out[:, L - 1] = rng.integers(0, top, size=n, dtype=np.uint64)
    return out


# the structured polynomials, most telling first: a batch smaller than the list takes its head
STRUCTURED = ["all_qm1", "pre_fwd_qm1", "pre_inv_qm1", "alt_0_qm1", "zero", "qm1_first", "qm1_last", "ones"]


def structured_batch(cf, q, N, tabs, batch, rng):
    """[batch, N, L] input: the STRUCTURED polynomials (head of the list when batch is smaller),
    then random ones.
      all_qm1      every coefficient q - 1
      pre_fwd_qm1  the oracle's inverse transform of all_qm1: every OUTPUT of the forward
                   transform is q - 1, so the last stage's canonical reduction sits on its edge
                   in every lane
      pre_inv_qm1  the oracle's forward transform of all_qm1: the same for the inverse
      alt_0_qm1    0, q - 1, 0, q - 1, ...
      zero, qm1_first (q - 1 at index 0 only), qm1_last (at index N - 1 only), ones (raw 1)
    `tabs` = cf.tables(N, cyclic=...)."""
    L = cf.L
    tw, twi, ninv = tabs
    qm1 = limbs_of(q - 1, L)
    polys = {}
    polys["all_qm1"] = np.broadcast_to(qm1, (N, L)).copy()
    polys["pre_fwd_qm1"] = cf.ntt_inv(polys["all_qm1"][None], twi, ninv)[0]
    polys["pre_inv_qm1"] = cf.ntt_fwd(polys["all_qm1"][None], tw)[0]
    alt = np.zeros((N, L), np.uint64)
    alt[1::2] = qm1
    polys["alt_0_qm1"] = alt
    polys["zero"] = np.zeros((N, L), np.uint64)
    first = np.zeros((N, L), np.uint64)
    first[0] = qm1
    polys["qm1_first"] = first
    last = np.zeros((N, L), np.uint64)
    last[N - 1] = qm1
    polys["qm1_last"] = last
    ones = np.zeros((N, L), np.uint64)
    ones[:, 0] = 1
    polys["ones"] = ones
    names = STRUCTURED[:batch]
    a = np.empty((batch, N, L), np.uint64)
    for i, k in enumerate(names):
        a[i] = polys[k]
    nr = batch - len(names)
    if nr:
        a[len(names):] = rand_residues(q, L, nr * N, rng).reshape(nr, N, L)
    return a


def edge_values(q, L):
    """The vec-op edge set as raw values: 0, 1, 2, q-2, q-1, (q-1)/2, (q+1)/2, R mod q,
    R^2 mod q, q with its top limb zeroed, 2^64 (L > 1); canonical ones only, no repeats.
    Pairs from it hit x + y = q exactly, x + y = q - 1, x - x, 0 - (q-1), (q-1)(q-1), neg(0)."""
    R = 1 << (64 * L)
    vals = [0, 1, 2, q - 2, q - 1, (q - 1) // 2, (q + 1) // 2, R % q, R * R % q, q & ((1 << (64 * (L - 1))) - 1)]
    if L > 1:
        vals.append(1 << 64)
    out = []
    for v in vals:
        if 0 <= v < q and v not in out:
            out.append(v)
    return out


@functools.lru_cache(maxsize=None)
def cfield(name):
    import coracle as co
    return co.CField(modulus(name))


@functools.lru_cache(maxsize=4)
def oracle_tables(name, logn, cyclic):
    """The oracle's table triple, computed once per (field, rank, kind) and shared; read-only."""
    tabs = cfield(name).tables(1 << logn, cyclic=cyclic)
    for t in tabs:
        t.setflags(write=False)
    return tabs
