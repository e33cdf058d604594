"""The hand-written ctypes mirror (mitsuba3dopplertof_amd/_abi.py) against include/dtof.h, all of it: every prototype's return and parameter classes, every mirrored
structure's size and field offsets.  The checks are functions of the table / structure they are given, so the same file shows on mutated copies that they can fail.
Nothing here loads the library or needs a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from mitsuba3dopplertof_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dtof.h")
STRUCTURES = {"dtof_scene_info": _abi._Info, "dtof_render_stats": _abi._Stats, "dtof_modulation": _abi._Modulation, "dtof_denoise_params": _abi._DenoiseParams,
              "dtof_temporal_params": _abi._TemporalParams, "dtof_temporal_buffers": _abi._TemporalBuffers, "dtof_adaptive_params": _abi._AdaptiveParams}

C_SCALARS = {"int": "i32", "int32_t": "i32", "uint32_t": "u32", "int64_t": "i64", "uint64_t": "u64", "size_t": "u64", "float": "f32", "double": "f64"}
C_RETURNS = {"const char *": "const char *", "uint32_t": "uint32_t", "uint64_t": "uint64_t", "void": "void", "int": "int"}
CTYPES_SCALARS = {C.c_int: "i32", C.c_int32: "i32", C.c_uint32: "u32", C.c_int64: "i64", C.c_uint64: "u64", C.c_size_t: "u64", C.c_float: "f32", C.c_double: "f64"}
CTYPES_RETURNS = {C.c_char_p: "const char *", C.c_uint32: "uint32_t", C.c_uint64: "uint64_t", None: "void", C.c_int: "int"}


def header_code():
    """include/dtof.h without comments and preprocessor lines"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return "\n".join(line for line in text.split("\n") if not line.lstrip().startswith("#"))


def parse_prototypes(code):
    """{name: (return class, [parameter class, ...])} of every dtof_* prototype; a type outside the classes the binding knows is a KeyError"""
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w ]*?[\s*]+)(dtof_\w+)\s*\(([^()]*)\)\s*;", code):
        classes = []
        for p in (p.strip() for p in params.split(",")):
            if p == "void":
                continue
            classes.append("pointer" if "*" in p or "[" in p else C_SCALARS[[w for w in p.split() if w != "const"][0]])
        assert name not in out, name
        out[name] = (C_RETURNS[" ".join(ret.replace("*", " * ").split())], classes)
    return out


def ctypes_class(t):
    if t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer)):
        return "pointer"
    return CTYPES_SCALARS[t]


def table_problems(table, prototypes):
    """every way `table` (name -> (restype, argtypes)) disagrees with the parsed prototypes, as a list of strings"""
    problems = ["%s: no entry in the table" % n for n in sorted(set(prototypes) - set(table))]
    problems += ["%s: not declared in the header" % n for n in sorted(set(table) - set(prototypes))]
    for name in sorted(set(table) & set(prototypes)):
        (restype, argtypes), (ret, params) = table[name], prototypes[name]
        if CTYPES_RETURNS.get(restype, repr(restype)) != ret:
            problems.append("%s: returns %s, the table says %r" % (name, ret, restype))
        if len(argtypes) != len(params):
            problems.append("%s: %d parameters, the table has %d" % (name, len(params), len(argtypes)))
            continue
        problems += ["%s: parameter %d is %s, the table says %s" % (name, i, want, ctypes_class(got))
                     for i, (got, want) in enumerate(zip(argtypes, params)) if ctypes_class(got) != want]
    return problems


def struct_declarators(code, cname):
    """how many members the header's `typedef struct { ... } cname;` declares"""
    body = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*%s\s*;" % cname, code).group(1)
    return sum(len(stmt.split(",")) for stmt in body.split(";") if stmt.strip())


def struct_source(struct, cname):
    """a C file that holds the size of `cname` and the offset and size of every field to what ctypes computed for `struct`"""
    lines = ["#include <stddef.h>", '#include "dtof.h"', '_Static_assert(sizeof(%s) == %d, "sizeof %s");' % (cname, C.sizeof(struct), cname)]
    for name, _ in struct._fields_:
        field = getattr(struct, name)
        lines.append('_Static_assert(offsetof(%s, %s) == %d, "offset of %s");' % (cname, name, field.offset, name))
        lines.append('_Static_assert(sizeof(((%s *) 0)->%s) == %d, "size of %s");' % (cname, name, field.size, name))
    return "\n".join(lines) + "\n"


def struct_problems(struct, cname, code, tmp_path):
    """[] if the compiler agrees with ctypes about every field of `struct` and the header declares as many; else what it said"""
    n = struct_declarators(code, cname)
    if n != len(struct._fields_):
        return ["%s: the header declares %d members, the mirror %d" % (cname, n, len(struct._fields_))]
    src = tmp_path / (cname + ".c")
    src.write_text(struct_source(struct, cname))
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / (cname + ".o"))],
                       capture_output=True, text=True)
    return [r.stderr] if r.returncode != 0 else []


@pytest.fixture(scope="module")
def code():
    return header_code()


@pytest.fixture(scope="module")
def prototypes(code):
    return parse_prototypes(code)


needs_gcc = pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")


def test_the_parser_sees_every_declared_function(code, prototypes):
    """the name set test_capi_exports_every_declared_symbol derives (from the comment-stripped header): the prototype parser skips none of them"""
    names = set(re.findall(r"\b(dtof_[a-z0-9_]+)\s*\(", code))
    assert len(names) >= 28 and set(prototypes) == names
    assert prototypes["dtof_version"] == ("const char *", []) and prototypes["dtof_cancel"] == ("void", ["pointer"])
    assert prototypes["dtof_scene_export"] == ("int", ["pointer", "i32", "pointer", "u64", "pointer"])
    assert prototypes["dtof_scene_world_to_pixel"] == ("int", ["pointer", "pointer"])      # double out12[12]


def test_the_table_matches_every_prototype(prototypes):
    assert table_problems(_abi.SIGNATURES, prototypes) == []


@needs_gcc
@pytest.mark.parametrize("cname", sorted(STRUCTURES))
def test_every_mirrored_structure_has_the_headers_layout(cname, code, tmp_path):
    assert struct_problems(STRUCTURES[cname], cname, code, tmp_path) == []


def test_the_mirrored_structures_are_all_of_the_headers(code):
    assert set(re.findall(r"typedef\s+struct\s*\{[^{}]*\}\s*(\w+)\s*;", code)) == set(STRUCTURES)


def test_declare_sets_what_a_partial_library_has_and_skips_the_rest():
    class Entry:
        restype, argtypes = "unset", "unset"

    class Partial:
        pass

    have = ("dtof_version", "dtof_render_rows_async", "dtof_scene_destroy", "dtof_scene_plan_facts_launches")
    lib = Partial()
    for name in have + ("not_of_the_table",):
        setattr(lib, name, Entry())
    assert _abi.declare(lib) is lib
    assert sorted(vars(lib)) == sorted(have + ("not_of_the_table",))      # nothing it lacks was added
    for name in have:
        assert (getattr(lib, name).restype, getattr(lib, name).argtypes) == (_abi.SIGNATURES[name][0], list(_abi.SIGNATURES[name][1])), name
    assert (lib.not_of_the_table.restype, lib.not_of_the_table.argtypes) == ("unset", "unset")
    assert lib.dtof_version.restype is C.c_char_p and lib.dtof_scene_destroy.restype is None and lib.dtof_scene_plan_facts_launches.restype is C.c_uint64


def test_the_prototype_check_flags_a_mutated_table(prototypes):
    def mutated(name, restype=..., argtypes=...):
        table = dict(_abi.SIGNATURES)
        table[name] = (table[name][0] if restype is ... else restype, table[name][1] if argtypes is ... else argtypes)
        return table_problems(table, prototypes)

    rows = _abi.SIGNATURES["dtof_render_rows_async"][1]
    assert mutated("dtof_render_rows_async", argtypes=rows[:-1]) == ["dtof_render_rows_async: 8 parameters, the table has 7"]      # a dropped parameter
    layout = _abi.SIGNATURES["dtof_scene_set_film_layout"][1]
    assert layout[2] is C.c_uint64
    assert mutated("dtof_scene_set_film_layout", argtypes=layout[:2] + [C.c_uint32]) == ["dtof_scene_set_film_layout: parameter 2 is u64, the table says u32"]
    assert mutated("dtof_scene_plan_facts_launches", restype=C.c_uint32) == ["dtof_scene_plan_facts_launches: returns uint64_t, the table says %r" % C.c_uint32]
    assert mutated("dtof_version", restype=C.c_int) != [] and mutated("dtof_render", argtypes=[C.c_uint32] + _abi.SIGNATURES["dtof_render"][1][1:]) != []
    table = dict(_abi.SIGNATURES)
    del table["dtof_last_error"]
    table["dtof_no_such_entry"] = (C.c_int, [])
    assert table_problems(table, prototypes) == ["dtof_last_error: no entry in the table", "dtof_no_such_entry: not declared in the header"]


@needs_gcc
def test_the_structure_check_flags_a_mutated_structure(code, tmp_path):
    def mirror(fields):
        return type("Mutated", (C.Structure,), {"_fields_": fields})

    fields = list(_abi._Stats._fields_)
    assert struct_problems(mirror(fields), "dtof_render_stats", code, tmp_path) == []      # the copy itself is sound
    i, j = [n for n, _ in fields].index("n_batches"), [n for n, _ in fields].index("ms_first")
    swapped = list(fields)
    swapped[i], swapped[j] = swapped[j], swapped[i]      # two swapped fields of different size
    out = struct_problems(mirror(swapped), "dtof_render_stats", code, tmp_path)
    assert len(out) == 1 and "offset of n_batches" in out[0] and "offset of ms_first" in out[0]
    a, b = [n for n, _ in fields].index("n_launches_trace"), [n for n, _ in fields].index("n_launches_shade")
    swapped = list(fields)
    swapped[a], swapped[b] = swapped[b], swapped[a]      # ... and of the same size
    out = struct_problems(mirror(swapped), "dtof_render_stats", code, tmp_path)
    assert len(out) == 1 and "offset of n_launches_trace" in out[0] and "offset of n_launches_shade" in out[0]
    retyped = [(n, C.c_uint32 if n == "n_bounces_inline" else t) for n, t in fields]      # c_uint32 where the header says uint64_t
    out = struct_problems(mirror(retyped), "dtof_render_stats", code, tmp_path)
    assert len(out) == 1 and "size of n_bounces_inline" in out[0]
    renamed = [("n_lanes" if n == "n_paths" else n, t) for n, t in fields]      # a field name the header lacks does not compile
    out = struct_problems(mirror(renamed), "dtof_render_stats", code, tmp_path)
    assert len(out) == 1 and "n_lanes" in out[0]
    assert struct_problems(mirror(fields[:-1]), "dtof_render_stats", code, tmp_path) == ["dtof_render_stats: the header declares 19 members, the mirror 18"]
