"""GPU: Verifier.Verify's checks called from C.  `abi_replay bverify` (tools/abi_replay.c) makes the call
sequence of INTEGRATION.md section 3 as a cgo caller would -- the handles from Compile's data, the
projection matrix from the XOF bytes, rg_buckler_verify_checks_dev on rg_malloc'd buffers, one word
read back -- and its verdicts, sides and pwEvals equal tests/buckler_verify_ref.py bit for bit.

The program runs once, as a fresh child process; the 110 s limit only ends a hung child."""
import os
import subprocess

import numpy as np
import pytest

import coracle as co
from tests import buckler_lin_ref as R
from tests import buckler_verify_ref as V
from tests.buckler_lin_util import RECOMPOSE_BOUND
from tests.buckler_verify_util import HonestProof, perturbations

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPLAY = os.path.join(os.path.dirname(HERE), "ringo-snark_amd", "lib", "abi_replay")


def _put(path, name, arr):
    np.ascontiguousarray(arr).tofile(os.path.join(path, name + ".bin"))


def _get(path, name, shape):
    a = np.fromfile(os.path.join(path, name + ".bin"), dtype=np.uint64)
    assert a.size == int(np.prod(shape)), (name, a.size, shape)
    return a.reshape(shape)


def _put_circuit(path, ref, prefix, cons):
    term_off, coeffs, pw_idx, wit_off, wit = [0], [], [], [0], []
    for c in cons:
        for coeff, pw, ws in c:
            coeffs.append(coeff)
            pw_idx.append(-1 if pw is None else pw)
            wit += ws
            wit_off.append(len(wit))
        term_off.append(len(pw_idx))
    _put(path, prefix + "_term_off", np.array(term_off, np.uint64))
    _put(path, prefix + "_coeffs", ref.arr(coeffs))
    _put(path, prefix + "_pw_idx", np.array(pw_idx, np.int64))
    _put(path, prefix + "_wit_off", np.array(wit_off, np.uint64))
    _put(path, prefix + "_wit", np.array(wit, np.uint64))
    return {prefix + "_nc": len(cons), prefix + "_nt": len(pw_idx), prefix + "_nwit": len(wit)}


def test_verifier_checks_from_c(fields, tmp_path):
    q, rank = fields["jindo_zp"], 128
    jr = 4 * rank + 3
    ref = R.Ref(q)
    L = ref.L
    hp = HonestProof(ref, rank, seed=7, two_pairs=True)
    path = str(tmp_path)
    off, pairs = [0], []
    for ps in hp.lin:
        pairs += [[wo, wi] for wo, wi in ps]
        off.append(len(pairs))
    rbase = R.decomposeBase(RECOMPOSE_BOUND)
    pert = perturbations(hp, jr)
    cases = [(hp.evals(jr), hp.mask_sums(), hp.chal())] + [(pert[n][0], pert[n][1], pert[n][3]) for n in
                                                          ("sum_remlo", "shared_witness", "lin_mask_sum", "eval_point")]
    kv = dict(limbs=L, rank=rank, jindo_rank=jr, w_cnt=hp.wCnt, n_pw=len(hp.pw), recompose_nb=len(rbase),
              n_pairs=len(pairs), aut_idx=5, ncases=len(cases))
    kv.update(_put_circuit(path, ref, "arith", hp.arith))
    kv.update(_put_circuit(path, ref, "sum", hp.sum))
    with open(os.path.join(path, "params.txt"), "w") as f:
        for k, v in kv.items():
            f.write(f"{k} {int(v)}\n")
    _put(path, "q", co.to_limbs([q], L))
    _put(path, "recompose_base", ref.arr([ref.set_uint64(b) for b in rbase]))
    with open(os.path.join(path, "xof.bin"), "wb") as f:
        f.write([s for s in hp.spec if s[0] == "proj"][0][1])
    _put(path, "pair_off", np.array(off, np.uint64))
    _put(path, "pairs", np.array(pairs, np.uint64))
    _put(path, "pw", np.stack([ref.arr(v) for v in hp.pw]))
    for i, (evals, ms, ch) in enumerate(cases):
        _put(path, f"evals_{i}", ref.arr(evals))
        _put(path, f"mask_sums_{i}", ref.arr(ms))
        _put(path, f"chal_{i}", ref.arr(ch))

    assert os.path.exists(REPLAY), f"{REPLAY} not built: run __graft_entry__.build()"
    r = subprocess.run([REPLAY, "bverify", path], capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, (r.returncode, r.stderr)

    n_evals = V.layout(hp.wCnt, True, True, True)["n"]
    assert int(_get(path, "info", (2,))[0]) == n_evals
    wants = [V.verify(ref, rank, jr, hp.wCnt, ch, ms, evals, hp.pw, hp.checkers, *hp.cons()) for evals, ms, ch in cases]
    assert [w[0] for w in wants] == [0, V.SUM_REM | V.SUM, V.ARITH | V.LIN | V.SUM, V.LIN, 31]
    assert r.stdout.splitlines() == [f"case {i} verdict {w[0]}" for i, w in enumerate(wants)]
    for i, (verdict, sides, pw_evals) in enumerate(wants):
        assert int(_get(path, f"verdict_{i}", (1,))[0]) == verdict, i
        assert (_get(path, f"sides_{i}", (8, L)) == ref.arr(sides)).all(), i
        assert (_get(path, f"pw_evals_{i}", (len(hp.pw), L)) == ref.arr(pw_evals)).all(), i
    assert int(_get(path, "host_verdict", (1,))[0]) == 0
    assert (_get(path, "host_sides", (8, L)) == ref.arr(wants[0][1])).all()
    assert (_get(path, "host_pw_evals", (len(hp.pw), L)) == ref.arr(wants[0][2])).all()
