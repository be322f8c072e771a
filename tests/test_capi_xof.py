"""CPU: the host-side refusals of the rg_xof_* entries and rg_field_marshal_dev that need no device (each
returns RG_ERR_INVALID and leaves a reason in rg_last_error), and rg_xof_seg's layout as the C compiler
sees it against the ctypes mirror.  The refusals that need a handle are in test_gpu_xof.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np

from ringo import _lib, xof
from ringo._lib import XofSegC, vp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = _lib.STATUS["RG_ERR_INVALID"]


def _refused(status, starts):
    assert status == INV
    why = _lib.lib().rg_last_error().decode()
    assert why.startswith(starts) and len(why) > len(starts), why


def _segs(*rows):
    arr = (XofSegC * len(rows))(*[XofSegC(*r) for r in rows])
    return arr, ctypes.cast(arr, vp)


def test_null_arguments_are_refused():
    L = _lib.lib()
    h = vp()
    _refused(L.rg_xof_create(1, None), "xof:")
    _refused(L.rg_xof_create(0, ctypes.byref(h)), "xof:")
    assert not h.value
    _refused(L.rg_xof_reset_dev(None, None), "xof:")
    _refused(L.rg_xof_copy_dev(None, None, None), "xof:")
    _refused(L.rg_xof_absorb_dev(None, None, 0, 0, None), "xof:")
    _refused(L.rg_xof_absorb_plan_dev(None, None, None, 0, None), "xof:")
    _refused(L.rg_xof_squeeze_dev(None, None, 0, 0, None), "xof:")
    L.rg_xof_destroy(None)
    L.rg_xof_plan_destroy(None)
    assert L.rg_xof_plan_bytes(None) == 0


def test_plan_create_refusals():
    L = _lib.lib()
    h = vp()
    keep, one = _segs((xof.LITERAL, 0, 0, 4))
    _refused(L.rg_xof_plan_create(one, 1, b"abcd", 4, None), "xof:")
    _refused(L.rg_xof_plan_create(None, 1, b"abcd", 4, ctypes.byref(h)), "xof:")
    _refused(L.rg_xof_plan_create(one, 1, None, 4, ctypes.byref(h)), "xof:")
    _refused(L.rg_xof_plan_create(one, 65537, b"abcd", 4, ctypes.byref(h)), "xof:")
    for bad in ((xof.LITERAL, 1, 0, 4), (xof.LITERAL, 5, 0, 0), (xof.LITERAL, 0, 0, 5),  # a literal run past the blob
                (-2, 0, 0, 1), (xof.MAX_BASES, 0, 0, 1)):                                 # a base no call can name
        keep, p = _segs((xof.LITERAL, 0, 0, 4), bad)
        _refused(L.rg_xof_plan_create(p, 2, b"abcd", 4, ctypes.byref(h)), "xof: segment 1")
        assert not h.value


def test_field_marshal_refusals():
    L = _lib.lib()
    q = np.array([0xFFFFFFFF00000001], np.uint64)
    f = vp()
    assert L.rg_field_create(1, _lib.ptr(q), ctypes.byref(f)) == 0
    try:
        _refused(L.rg_field_marshal_dev(None, 8, 1, 1, 8, 8, None), "field marshal:")
        _refused(L.rg_field_marshal_dev(f, None, 1, 1, 8, 8, None), "field marshal:")
        _refused(L.rg_field_marshal_dev(f, 8, 1, 1, None, 8, None), "field marshal:")
        _refused(L.rg_field_marshal_dev(f, 8, 2, 0, 8, 8, None), "field marshal:")
        _refused(L.rg_field_marshal_dev(f, 8, 2, 1, 8, 7, None), "field marshal:")
        assert L.rg_field_marshal_dev(f, 8, 0, 1, 8, 8, None) == 0  # nothing to do
    finally:
        L.rg_field_destroy(f)


def test_xof_seg_layout_is_the_c_compilers(tmp_path):
    cc = shutil.which("cc")
    assert cc, "no cc on PATH"
    src = tmp_path / "seg_layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ringo.h"\n'
                   'int main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %d %d\\n", sizeof(rg_xof_seg), offsetof(rg_xof_seg, base),\n'
                   '         offsetof(rg_xof_seg, offset), offsetof(rg_xof_seg, state_stride), offsetof(rg_xof_seg, len),\n'
                   '         RG_XOF_LITERAL, RG_XOF_MAX_BASES);\n  return 0;\n}\n')
    exe = tmp_path / "seg_layout"
    subprocess.run([cc, "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(XofSegC), XofSegC.base.offset, XofSegC.offset.offset, XofSegC.state_stride.offset,
                   XofSegC.len.offset, xof.LITERAL, xof.MAX_BASES]
