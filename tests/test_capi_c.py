"""CPU: the C side of the drop-in boundary.  include/ringo.h compiles alone as C11 and as C++17;
tools/abi_replay.c, the C11 caller built beside the library, reports the struct layouts and the
enumerators as the C compiler sees them, and they equal the ctypes mirrors; every prototype of the
header is parsed and held against the hand-written ctypes table `_lib._SIGS` (arity, pointer or
scalar, and each scalar's width and signedness: a c_int where the header says size_t passes every
small-value test); the host-side refusals return the documented codes to a C caller."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from ringo import _lib, bigpoly, jindo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
REPLAY = os.path.join(ROOT, "ringo-snark_amd", "lib", "abi_replay")
WARN = ["-Wall", "-Wextra", "-Werror", "-pedantic"]


def _replay(*args):
    assert os.path.exists(REPLAY), f"{REPLAY} not built: run __graft_entry__.build()"
    r = subprocess.run([REPLAY, *args], capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, (r.returncode, r.stderr)
    return r.stdout


@pytest.mark.parametrize("compiler,flags,ext", [("cc", ["-std=c11"], "c"), ("c++", ["-std=c++17"], "cpp")])
def test_header_compiles_alone(compiler, flags, ext, tmp_path):
    cc = shutil.which(compiler)
    assert cc, f"no {compiler} on PATH"
    src = tmp_path / f"only_ringo_h.{ext}"
    src.write_text('#include "ringo.h"\n')
    r = subprocess.run([cc, *flags, *WARN, "-I", INCLUDE, "-c", str(src), "-o", str(tmp_path / "only_ringo_h.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_abi_replay_is_built():
    assert os.path.isfile(REPLAY) and os.access(REPLAY, os.X_OK), f"{REPLAY} missing: the build step makes it"


# ---- layout ------------------------------------------------------------------------------------------
MIRRORS = {"rg_jindo_params": _lib.JindoParamsC, "rg_jindo_stddevs": _lib.JindoStddevsC,
           "rg_jindo_seeds": _lib.JindoSeedsC, "rg_jindo_verify_result": jindo.VerifyResultC}


def _python_layout():
    """What the ctypes side believes, under the names `abi_replay layout` prints."""
    out = {}
    for cname, cls in MIRRORS.items():
        out[f"sizeof.{cname}"] = ctypes.sizeof(cls)
        for field, _ in cls._fields_:
            desc = getattr(cls, field)
            out[f"{cname}.{field}.offset"] = desc.offset
            out[f"{cname}.{field}.size"] = desc.size
    out["sizeof.rg_status"] = ctypes.sizeof(_lib._SIGS["rg_field_create"][0])  # how the mirror reads a status
    out.update(_lib.STATUS)
    out.update({"RG_VEC_" + k.upper(): v for k, v in bigpoly._OPS.items()})
    out.update({"RG_MAC_" + name.upper(): v for v, name in jindo.Prover.MAC_KINDS.items()})
    out["RG_SAMPLER_LAYOUT"] = _lib.SAMPLER_LAYOUT
    return out


def _c_layout():
    out = {}
    for line in _replay("layout").splitlines():
        name, value = line.split()
        assert name not in out, name
        out[name] = int(value)
    return out


def test_layout_equals_the_ctypes_mirrors():
    c, py = _c_layout(), _python_layout()
    assert sorted(c) == sorted(py), (sorted(set(c) - set(py)), sorted(set(py) - set(c)))
    wrong = {k: (c[k], py[k]) for k in c if c[k] != py[k]}
    assert not wrong, f"(C, ctypes) differ: {wrong}"


def test_layout_names_every_struct_field_and_enumerator_of_the_header():
    """`abi_replay layout` itself is hand-written: it prints every field of the four public structs and
    every enumerator the header defines, so a field added to the header cannot go unmirrored."""
    src = _strip_comments(open(_lib.HEADER).read())
    c = _c_layout()
    for body, name in re.findall(r"typedef struct \{(.*?)\}\s*(\w+);", src, flags=re.S):
        assert f"sizeof.{name}" in c, name
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                fields += [re.sub(r"\[.*?\]", "", d).split()[-1] for d in decl.split(",")]
        got = [k.split(".")[1] for k in c if k.startswith(name + ".") and k.endswith(".offset")]
        assert sorted(got) == sorted(fields), name
    enumerators = re.findall(r"\b(RG_[A-Z0-9_]+)\s*=", src)
    assert len(enumerators) == 7 + 9 + 3
    for e in enumerators + ["RG_SAMPLER_LAYOUT"]:
        assert e in c, e
    m = re.search(r"#define RG_SAMPLER_LAYOUT (\d+)", src)
    assert int(m.group(1)) == c["RG_SAMPLER_LAYOUT"]
    assert _lib.lib().rg_version().decode().endswith(f"sampler-layout {c['RG_SAMPLER_LAYOUT']}")


# ---- prototypes --------------------------------------------------------------------------------------
def _strip_comments(src):
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


# C scalar -> (kind, bytes, signed)
C_SCALARS = {"int": ("int", 4, True), "size_t": ("int", 8, False), "long long": ("int", 8, True),
             "unsigned long long": ("int", 8, False), "double": ("float", 8, None), "rg_status": ("int", 4, True)}
# what a typed ctypes pointer may point at, in bytes, per C pointee
C_POINTEES = {"uint64_t": 8, "int64_t": 8, "uint8_t": 1, "int": 4, "size_t": 8, "long long": 8, "double": 8,
              "rg_jindo_params": 264, "rg_jindo_stddevs": 48, "rg_jindo_seeds": 192}


def _c_type(decl, is_param):
    """`const uint64_t* d_p` -> ("ptr", pointee, depth); `size_t n` -> ("int", 8, False)."""
    decl = decl.strip()
    depth = decl.count("*")
    words = [w for w in decl.replace("*", " ").split() if w != "const"]
    if is_param:
        assert len(words) >= 2, decl  # the header names every parameter
        words = words[:-1]
    base = " ".join(words)
    if depth:
        return ("ptr", base, depth)
    if base == "void" and not is_param:
        return ("void",)
    assert base in C_SCALARS, f"unknown C type {decl!r}"
    return C_SCALARS[base]


def header_prototypes():
    """{name: (return type, [parameter types])} of every function include/ringo.h declares."""
    src = _strip_comments(open(_lib.HEADER).read())
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    src = re.sub(r'extern "C" \{', "", src)
    src = re.sub(r"typedef\s+(struct|enum)\s*\{.*?\}\s*\w+\s*;", "", src, flags=re.S)
    src = re.sub(r"enum\s*\{.*?\}\s*;", "", src, flags=re.S)
    src = re.sub(r"typedef\s+struct\s+\w+\s+\w+\s*;", "", src)
    protos = {}
    for stmt in src.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt or stmt == "}":
            continue
        m = re.fullmatch(r"(.+?)\b(rg_[a-z0-9_]+)\s*\((.*)\)", stmt)
        assert m, f"not a prototype: {stmt!r}"
        ret, name, params = m.groups()
        assert name not in protos, name
        params = [] if params.strip() == "void" else [_c_type(p, True) for p in params.split(",")]
        protos[name] = (_c_type(ret, False), params)
    return protos


def _ctypes_type(t):
    if t is None:
        return ("void",)
    if t in (ctypes.c_void_p, ctypes.c_char_p):
        return ("ptr", None)
    if isinstance(t, type) and issubclass(t, ctypes._Pointer):
        return ("ptr", ctypes.sizeof(t._type_))
    if t is ctypes.c_double:
        return ("float", 8, None)
    assert issubclass(t, ctypes._SimpleCData), t
    return ("int", ctypes.sizeof(t), t(-1).value < 0)


def _mismatch(c, py):
    """None when the ctypes type `py` can carry the C type `c`, else a description."""
    if c[0] == "ptr":
        if py[0] != "ptr":
            return f"header has a pointer ({c[1]}{'*' * c[2]}), _SIGS a scalar {py}"
        if py[1] is not None:  # a typed ctypes pointer: the pointee's size must be the C pointee's
            want = 8 if c[2] > 1 else C_POINTEES.get(c[1])
            if want is None:
                return f"typed ctypes pointer for {c[1]}*"
            if want != py[1]:
                return f"pointee of {c[1]}{'*' * c[2]} is {want} bytes, _SIGS points at {py[1]}"
        return None
    if py[0] == "ptr":
        return f"header has a scalar {c}, _SIGS a pointer"
    return None if c == py else f"header {c} != _SIGS {py} (kind, bytes, signed)"


def test_parser_reads_every_declared_function():
    protos = header_prototypes()
    assert sorted(protos) == _lib.header_symbols()
    assert protos["rg_last_error"] == (("ptr", "char", 1), [])
    assert protos["rg_field_destroy"] == (("void",), [("ptr", "rg_field", 1)])
    assert protos["rg_jindo_verify_dev"][1][13:15] == [("float", 8, None)] * 2
    assert protos["rg_buckler_lincheck_create"][1][3] == ("ptr", "rg_linchecker", 2)
    assert protos["rg_jindo_sample_dev"][1][5] == ("int", 8, False)  # unsigned long long first_commit


def test_every_header_symbol_has_a_binding():
    missing = sorted(set(header_prototypes()) - set(_lib._SIGS))
    assert not missing, f"declared in ringo.h, absent from _lib._SIGS: {missing}"


def test_sigs_match_the_header_prototypes():
    protos = header_prototypes()
    wrong = []
    for name, (res, args) in _lib._SIGS.items():
        assert name in protos, f"{name} is in _SIGS but not in ringo.h"
        c_ret, c_args = protos[name]
        if len(args) != len(c_args):
            wrong.append(f"{name}: header takes {len(c_args)} parameters, _SIGS {len(args)}")
            continue
        m = _mismatch(c_ret, _ctypes_type(res))
        if m:
            wrong.append(f"{name} return: {m}")
        for i, (c, py) in enumerate(zip(c_args, args)):
            m = _mismatch(c, _ctypes_type(py))
            if m:
                wrong.append(f"{name} parameter {i}: {m}")
    assert not wrong, "\n".join(wrong)


def test_pointee_sizes_are_the_compilers():
    """The struct sizes C_POINTEES assumes are the ones `abi_replay layout` prints."""
    c = _c_layout()
    for name in ("rg_jindo_params", "rg_jindo_stddevs", "rg_jindo_seeds"):
        assert C_POINTEES[name] == c[f"sizeof.{name}"], name


# ---- refusals ----------------------------------------------------------------------------------------
def test_host_side_refusals_from_c():
    """A NULL handle, stride < n, an even modulus, a rank that is no power of two and rg_set_probe(1)
    on the product library: each returns the documented code to a C caller before anything reaches a
    device (abi_replay exits 2 on any other status)."""
    lines = _replay("refuse").splitlines()
    got = {line.split(" ", 1)[1].split("(")[0]: int(line.split()[0]) for line in lines if "rg_set_probe" not in line}
    inv = _lib.STATUS["RG_ERR_INVALID"]
    assert got == {"rg_field_create": inv, "rg_ntt_fwd": inv, "rg_vec": inv, "rg_jindo_commit": inv,
                   "rg_jindo_mac_kinds": inv, "rg_poly_evaluate_batch": inv, "rg_poly_evaluate_batch_dev": inv,
                   "rg_ntt_create": _lib.STATUS["RG_ERR_NOT_POW2"]}
    assert f"{inv} rg_set_probe(1)" in lines and "0 rg_set_probe(0)" in lines
