"""CPU: the binding's statement of the ABI -- the prototype table, the struct mirrors and the constants of
libfsm_amd/capi.py -- against include/fsm_hip.h and include/fsm_hip_plan.h as the compiler reads them.  A small C++17
program instantiates a template on decltype(&name) for every declared function and prints one code per return and
parameter type (v void, p pointer, f8 double, i4 / u4 / u8 integers); it links nothing."""
import ast
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_abi import ROOT, declared_symbols

from libfsm_amd import capi

STRUCTS = {"fsm_hip_range": capi.RANGE_DTYPE, "fsm_hip_dfa_desc": capi._Desc, "fsm_hip_dfa_info": capi._Info,
           "fsm_hip_multi_batch": capi.MultiBatch, "fsm_hip_multi_batch_ids": capi.MultiBatchIds,
           "fsm_hip_multi_batch_eager": capi.MultiBatchEager, "fsm_hip_node_batch": capi.NodeBatch, "fsm_hip_pos_batch": capi.PosBatch}

PROGRAM_HEAD = r"""
#include <cstddef>
#include <cstdio>
#include <type_traits>
#include "fsm_hip.h"
#include "fsm_hip_plan.h"
template <class T> void code()
{
	if constexpr (std::is_void_v<T>) std::printf("v");
	else if constexpr (std::is_pointer_v<T>) std::printf("p");
	else if constexpr (std::is_floating_point_v<T>) std::printf("f%zu", sizeof(T));
	else std::printf("%c%zu", std::is_signed_v<T> ? 'i' : 'u', sizeof(T));
}
template <class F> struct sig;
template <class R, class... A> struct sig<R (*)(A...)> {
	static void print(const char *name)
	{
		std::printf("F %s ", name);
		code<R>();
		std::printf(":");
		((code<A>(), std::printf(",")), ...);
		std::printf("\n");
	}
};
int main()
{
"""


def header_text():
    txt = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("fsm_hip.h", "fsm_hip_plan.h"))
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def header_constants():
    """the names of the headers' enumerators and value macros (the include guards have no value)"""
    txt = header_text()
    return sorted(set(re.findall(r"#\s*define\s+(FSM_HIP_[A-Z0-9_]+)[ \t]+\S", txt)) | set(re.findall(r"\b(FSM_HIP_[A-Z0-9_]+)\s*=[^=]", txt)))


def header_fields(struct):
    """the field names of a struct of the headers, in order"""
    body = re.search(r"struct\s+%s\s*\{(.*?)\}" % struct, header_text(), re.S).group(1)
    names = []
    for decl in body.split(";"):
        names += [re.search(r"(\w+)\s*$", part).group(1) for part in decl.split(",") if part.strip()]
    return names


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """what the compiler makes of the headers: (signature by function, (sizeof, offsetof by field) by struct, value by constant)"""
    td = tmp_path_factory.mktemp("capi_prototypes")
    lines = [PROGRAM_HEAD]
    lines += ['\tsig<decltype(&%s)>::print("%s");\n' % (s, s) for s in sorted(declared_symbols())]
    for s in STRUCTS:
        lines.append('\tstd::printf("S %s %%zu", sizeof(struct %s));\n' % (s, s))
        lines += ['\tstd::printf(" %s=%%zu", offsetof(struct %s, %s));\n' % (f, s, f) for f in header_fields(s)]
        lines.append('\tstd::printf("\\n");\n')
    lines += ['\tstd::printf("C %s %%llu\\n", (unsigned long long)(%s));\n' % (c, c) for c in header_constants()]
    lines.append("\treturn 0;\n}\n")
    src, exe = str(td / "protos.cpp"), str(td / "protos")
    open(src, "w").write("".join(lines))
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    funcs, structs, consts = {}, {}, {}
    for line in subprocess.check_output([exe], text=True).splitlines():
        kind, name, rest = line.split(" ", 2)
        if kind == "F":
            funcs[name] = rest
        elif kind == "S":
            size, *fields = rest.split()
            structs[name] = (int(size), {f.split("=")[0]: int(f.split("=")[1]) for f in fields})
        else:
            consts[name] = int(rest)
    return funcs, structs, consts


def type_code(t):
    """a ctypes type of the table -> the code the program prints for the C type"""
    if t is None:
        return "v"
    if not issubclass(t, C._SimpleCData):
        assert issubclass(t, (C._Pointer, C.Array)), t
        return "p"
    if t._type_ in "PzZ":
        return "p"
    if t._type_ in "fdg":
        return "f%d" % C.sizeof(t)
    return "%s%d" % ("i" if t(-1).value < 0 else "u", C.sizeof(t))


def table_signature(proto):
    restype, argtypes = proto
    return type_code(restype) + ":" + "".join(type_code(a) + "," for a in argtypes)


def test_table_is_the_header(compiled):
    funcs = compiled[0]
    assert len(funcs) >= 173 and set(funcs) == declared_symbols()
    table = capi.PROTOTYPES
    assert sorted(set(funcs) - set(table)) == [], "declared, not in the table"
    assert sorted(set(table) - set(funcs)) == [], "in the table, not declared"
    wrong = {name: (table_signature(table[name]), funcs[name]) for name in funcs if table_signature(table[name]) != funcs[name]}
    assert not wrong, wrong     # name: (the table's, the header's)


def test_table_is_applied_on_every_load(built):
    for lib in (capi.load_library(), capi.load_library(capi.LIB_PATH)):
        for name, (restype, argtypes) in capi.PROTOTYPES.items():
            fn = getattr(lib, name)
            assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_struct_mirrors(compiled):
    structs = compiled[1]
    for name, mirror in STRUCTS.items():
        size, offsets = structs[name]
        if isinstance(mirror, np.dtype):
            got = (mirror.itemsize, {f: mirror.fields[f][1] for f in mirror.names})
        else:   # a Python keyword as a field name carries a trailing underscore
            got = (C.sizeof(mirror), {f.rstrip("_"): getattr(mirror, f).offset for f, _ in mirror._fields_})
        assert list(got[1]) == header_fields(name), name
        assert got == (size, offsets), name


def test_constants(compiled):
    consts = compiled[2]
    mirrored = {name: getattr(capi, name[len("FSM_HIP_"):]) for name in consts if hasattr(capi, name[len("FSM_HIP_"):])}
    mirrored.update({"FSM_HIP_PLAN_" + what.upper(): index for what, (index, _) in capi.Plan._WHAT.items()})
    wrong = {name: (value, consts.get(name)) for name, value in mirrored.items() if consts.get(name) != value}
    assert not wrong, wrong     # name: (the binding's, the header's)
    # ... and no integer constant of the binding is without its enumerator or macro (IN_*: the values of KNOB_INPUT_MODE, which
    # the header gives in a comment only)
    own = {k for k, v in vars(capi).items() if k.isupper() and not k.startswith(("_", "IN_")) and isinstance(v, int)}
    assert sorted(k for k in own if "FSM_HIP_" + k not in mirrored) == [] and len(own) > 40


def test_prototypes_are_set_in_one_place():
    """no .py file but the table's module assigns .restype or .argtypes on an fsm_hip_* attribute"""
    found = []
    for top in ("libfsm_amd", "tests", "tools"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            for f in sorted(files):
                path = os.path.join(d, f)
                if not f.endswith(".py") or os.path.samefile(path, capi.__file__):
                    continue
                for node in ast.walk(ast.parse(open(path).read(), path)):
                    if (isinstance(node, ast.Attribute) and isinstance(node.ctx, ast.Store) and node.attr in ("restype", "argtypes")
                            and isinstance(node.value, ast.Attribute) and node.value.attr.startswith("fsm_hip_")):
                        found.append("%s:%d" % (os.path.relpath(path, ROOT), node.lineno))
    assert not found, found
