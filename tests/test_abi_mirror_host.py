"""The ctypes mirror of the C ABI, derived from include/rover_step.h: every Structure's layout and field names, every entry point's
parameter kinds.  Header and Python only: no GPU, and the library is not loaded.

What this cannot see is a tandem edit of header and mirror: the literal field lists and sizes in the scaler, motion, bogie, occlusion,
obs-noise and track host tests pin those."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from isaac_rover_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(os.path.join(INCLUDE, "rover_step.h")).read(), flags=re.S)

# every Structure subclass any module of the binding defines: a new one is picked up without an edit here, and fails until _lib.TYPEDEFS
# names its typedef
STRUCTS = sorted((s for s in C.Structure.__subclasses__() if s.__module__.startswith(_lib.__package__ + "._")), key=lambda s: s.__name__)
C_NAME = {mirror: name for name, mirror in _lib.TYPEDEFS.items()}
DECLARED = {name: body for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", HEADER)}
PROTOTYPES = {name: (ret, params) for ret, name, params in re.findall(r"ROVER_API\s+([\w\s\*]+?)\b(rover_\w+)\s*\(([^()]*)\)\s*;", HEADER)}

SCALARS = {"int": "i32", "int32_t": "i32", "uint32_t": "u32", "int64_t": "i64", "uint64_t": "u64", "float": "f32", "double": "f64"}
CTYPES = {C.c_int: "i32", C.c_int32: "i32", C.c_uint32: "u32", C.c_int64: "i64", C.c_uint64: "u64", C.c_float: "f32", C.c_double: "f64"}
RETURNS = {C.c_int: "int", C.c_char_p: "const char*", None: "void"}


def c_name(field):
    """The C name of a mirrored field: a trailing underscore only keeps a Python keyword out of the way (``in_`` is ``in``)."""
    return field[:-1] if field.endswith("_") else field


def declared_fields(body):
    """The field names of a struct body in order: ``int32_t tensor, first, length;`` declares three, ``K[2]`` and ``*x`` are K and x."""
    names = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        for part in decl.split(","):
            names.append(re.search(r"(\w+)\s*(?:\[[^\]]*\]\s*)*$", part).group(1))
    return names


def c_param_kinds(params):
    """The kinds of a C parameter list in order: a ``*`` or an array declarator (it decays) is "ptr", a scalar its type."""
    params = params.strip()
    if params in ("", "void"):
        return []
    kinds = []
    for p in params.split(","):
        if "*" in p or "[" in p:
            kinds.append("ptr")
        else:
            kinds.append(SCALARS[[w for w in p.split() if w != "const"][0]])
    return kinds


def ctypes_kind(t):
    return "ptr" if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer) else CTYPES[t]


def host_c_compiler():
    """The host clang of the ROCm install csrc/build.sh compiles with, else cc.  None of them: the library could not have been built either."""
    build_sh = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "build.sh")).read()
    hipcc = os.environ.get("HIPCC") or re.search(r'HIPCC="\$\{HIPCC:-([^}]+)\}"', build_sh).group(1)
    rocm = os.path.dirname(os.path.dirname(hipcc))
    for cc in (os.path.join(rocm, "llvm", "bin", "clang"), os.path.join(rocm, "lib", "llvm", "bin", "clang"), shutil.which("cc")):
        if cc and os.path.exists(cc):
            return cc
    pytest.fail("no C compiler: neither the ROCm install's clang nor cc")


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    """{"rover_cfg": sizeof, "rover_cfg.num_envs": offsetof, ...} as one C program that includes the header prints them."""
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "rover_step.h"', "int main(void) {"]
    for s in STRUCTS:
        t = C_NAME[s]
        lines.append(f'    printf("{t} %zu\\n", sizeof({t}));')
        lines += [f'    printf("{t}.{f} %zu\\n", offsetof({t}, {c_name(f)}));' for f, *_ in s._fields_]
    lines += ["    return 0;", "}"]
    tmp = tmp_path_factory.mktemp("abi_probe")
    src, exe = tmp / "probe.c", tmp / "probe"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([host_c_compiler(), "-x", "c", "-std=c11", "-I", INCLUDE, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_the_header_and_the_binding_are_both_seen():
    assert len(STRUCTS) >= 28 and len(PROTOTYPES) >= 95
    assert set(STRUCTS) == set(C_NAME) and len(C_NAME) == len(_lib.TYPEDEFS), set(STRUCTS) ^ set(C_NAME)      # one typedef per mirror, none left out
    assert set(_lib.TYPEDEFS) == set(DECLARED), set(_lib.TYPEDEFS) ^ set(DECLARED)
    assert set(PROTOTYPES) == set(_lib.SYMBOLS), set(PROTOTYPES) ^ set(_lib.SYMBOLS)
    assert all(getattr(_lib, s.__name__) is s for s in STRUCTS)              # every mirror is importable from _lib


@pytest.mark.parametrize("struct", STRUCTS, ids=lambda s: s.__name__)
def test_struct_layout_matches_the_header(struct, c_layout):
    t = C_NAME[struct]
    assert C.sizeof(struct) == c_layout[t], (t, C.sizeof(struct), c_layout[t])
    for f, *_ in struct._fields_:
        assert getattr(struct, f).offset == c_layout[f"{t}.{f}"], (t, f, getattr(struct, f).offset, c_layout[f"{t}.{f}"])


@pytest.mark.parametrize("struct", STRUCTS, ids=lambda s: s.__name__)
def test_struct_fields_are_the_headers_in_order(struct):
    assert [c_name(f) for f, *_ in struct._fields_] == declared_fields(DECLARED[C_NAME[struct]])


@pytest.mark.parametrize("name", sorted(_lib.SYMBOLS))
def test_argtypes_match_the_prototype(name):
    ret, params = PROTOTYPES[name]
    restype, argtypes = _lib.SYMBOLS[name]
    assert [ctypes_kind(t) for t in argtypes] == c_param_kinds(params), (name, params)
    assert RETURNS[restype] == " ".join(ret.replace("*", " * ").split()).replace(" *", "*"), (name, ret)


def test_array_parameters_decay_to_pointers():
    for name in ("rover_build_heightfield", "rover_heightfield_limits", "rover_occlusion_order", "rover_motion_plane_fit", "rover_motion_bogie_fit"):
        assert PROTOTYPES[name][1].count("[") >= 1 and "ptr" in c_param_kinds(PROTOTYPES[name][1]), name


def test_no_stream_names_the_ctx_calls_without_a_stream():
    """Engine._call appends the current stream unless the symbol is in NO_STREAM: that set is the ctx entry points which return a code
    and whose prototype does not end in ``void *stream``."""
    without = set()
    for name, (ret, params) in PROTOTYPES.items():
        parts = [p.strip() for p in params.split(",")]
        if ret.split() == ["int"] and re.fullmatch(r"(const\s+)?rover_ctx\s*\*\s*\w+", parts[0]) and not re.fullmatch(r"void\s*\*\s*stream", parts[-1]):
            without.add(name)
    assert without == set(_lib.NO_STREAM), without ^ set(_lib.NO_STREAM)
