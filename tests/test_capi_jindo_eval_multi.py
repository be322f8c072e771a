"""CPU: what the batch prover's two Evaluate calls (include/ringo.h rg_jindo_eval_open_multi_dev,
rg_jindo_eval_respond_multi_dev) decide on the host: the NULL handle's refusal and its reason whatever
the other arguments are; the refusals that need no shape (counts, strides, NULL buffers, the NULL rule
of batch 1), which are decided before the handle is read and so are made here with a made-up handle;
the scratch sizes of refused arguments; the header constant against the mirror; the mirror's methods.
The overlap checks and the ChallengeBound of 0 read the handle's shape, and an rg_jindo cannot be
created without a device (its ring tables and commit key are uploaded), so those run with real buffers
in test_gpu_jindo_eval_multi.py, where the whole list is issued again.  The addresses below are made-up
numbers: a call that read them would crash, not fail."""
import re

from ringo import _lib, jindo

INVALID = _lib.STATUS["RG_ERR_INVALID"]
A = [0x100000 * (i + 1) for i in range(12)]  # distinct fake device addresses
PREFIX = "jindo eval multi"


def _why():
    return _lib.lib().rg_last_error().decode()


def _open(h, n, batch, ps=1, cs=1, xs=1, incom=A[0], enc=A[1], mlwe=A[2], x=A[3], bb=A[4], ob_enc=A[5], ob_mlwe=A[6],
          pf_incom=A[7], pf_partial=A[8], scratch=A[9]):
    return _lib.lib().rg_jindo_eval_open_multi_dev(h, n, batch, incom, enc, mlwe, ps, cs, x, xs, bb, ob_enc, ob_mlwe,
                                                   pf_incom, pf_partial, scratch, None)


def _respond(h, n, stride=1, ob_enc=A[0], ob_mlwe=A[1], cb=A[2], pf_enc=A[3], pf_mlwe=A[4], scratch=A[5]):
    return _lib.lib().rg_jindo_eval_respond_multi_dev(h, n, ob_enc, ob_mlwe, stride, cb, pf_enc, pf_mlwe, scratch, None)


def test_null_handle_refused_whatever_else_is_wrong():
    # the handle is looked at first: no other defect is reported in its place, and nothing is read
    for kw in (dict(), dict(n=0), dict(n=65536), dict(batch=0), dict(ps=0), dict(cs=0), dict(xs=0), dict(enc=None),
               dict(scratch=None), dict(bb=None), dict(batch=1), dict(pf_incom=A[1])):
        a = dict(n=3, batch=2)
        a.update(kw)
        assert _open(None, **a) == INVALID, kw
        assert _why().startswith(PREFIX) and "NULL handle" in _why(), kw
    for kw in (dict(), dict(n=0), dict(n=65536), dict(stride=0), dict(ob_enc=None), dict(scratch=None),
               dict(pf_enc=A[0])):
        a = dict(n=3)
        a.update(kw)
        assert _respond(None, **a) == INVALID, kw
        assert _why().startswith(PREFIX) and "NULL handle" in _why(), kw


H = 0x7f0000000000  # a made-up handle: the refusals below are decided before the handle is read


def test_refusals_that_do_not_read_the_handle():
    spare = [0x900000 + 0x1000 * i for i in range(3)]
    open_cases = [dict(n=0), dict(n=65536), dict(batch=0), dict(batch=32769), dict(ps=0), dict(cs=0), dict(xs=0),
                  dict(ps=(1 << 31) + 1), dict(xs=(1 << 30) + 1), dict(incom=None), dict(enc=None), dict(mlwe=None),
                  dict(x=None), dict(pf_incom=None), dict(pf_partial=None), dict(scratch=None),
                  # the NULL rule, both ways
                  dict(bb=None), dict(ob_enc=None), dict(ob_mlwe=None), dict(bb=None, ob_enc=None, ob_mlwe=None),
                  dict(batch=1), dict(batch=1, bb=None), dict(batch=1, bb=None, ob_enc=None),
                  dict(batch=1, ob_enc=None, ob_mlwe=None), dict(batch=1, bb=spare[0], ob_enc=spare[1], ob_mlwe=spare[2])]
    for kw in open_cases:
        a = dict(n=3, batch=2)
        a.update(kw)
        assert _open(H, **a) == INVALID, kw
        assert _why().startswith(PREFIX) and "NULL handle" not in _why(), (kw, _why())
    for kw in (dict(n=0), dict(n=65536), dict(stride=0), dict(stride=(1 << 31) + 1), dict(ob_enc=None), dict(ob_mlwe=None),
               dict(cb=None), dict(pf_enc=None), dict(pf_mlwe=None), dict(scratch=None)):
        a = dict(n=3)
        a.update(kw)
        assert _respond(H, **a) == INVALID, kw
        assert _why().startswith(PREFIX) and "NULL handle" not in _why(), (kw, _why())


def test_scratch_bytes_of_refused_arguments():
    L = _lib.lib()
    for n in (0, 1, 64, 65535, 65536):
        for batch in (0, 1, 12):
            assert L.rg_jindo_eval_open_multi_scratch_bytes(None, n, batch) == 0
        assert L.rg_jindo_eval_respond_multi_scratch_bytes(None, n) == 0
    # with a handle that is never read: the arguments the calls refuse
    for n, batch in ((0, 2), (65536, 2), (3, 0), (3, 32769)):
        assert L.rg_jindo_eval_open_multi_scratch_bytes(H, n, batch) == 0
    for n in (0, 65536):
        assert L.rg_jindo_eval_respond_multi_scratch_bytes(H, n) == 0


def test_constant_is_in_the_header_and_the_mirror():
    m = re.search(r"#define RG_JINDO_EVAL_MAX_PROOFS (\d+)", open(_lib.HEADER).read())
    assert m and int(m.group(1)) == jindo.EVAL_MAX_PROOFS == 65535


def test_the_mirror_has_the_methods():
    for name in ("eval_open_multi_scratch_bytes", "eval_open_multi_dev", "eval_respond_multi_scratch_bytes",
                 "eval_respond_multi_dev"):
        assert callable(getattr(jindo.Prover, name)), name
