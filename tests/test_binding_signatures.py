"""The Python binding against include/tmpc_hip.h (no GPU): solver._SIGNATURES against every prototype, the ctypes / numpy struct mirrors
against every struct, and BatchedSolver._call's conversions on a stub library.  A row with one pointer too few, a prototype that gained an
argument or two swapped struct fields fail here instead of corrupting a call on the device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_CLASS = {"int32_t": "i32", "uint32_t": "u32", "int64_t": "i64", "uint64_t": "u64", "double": "f64", "float": "f32", "void": "void",
           "int": "i32", "uint8_t": "u8"}      # `int` is the 4-byte int of every platform this library builds for: one class with int32_t, as in ctypes
C_TYPE = {"i32": C.c_int32, "u32": C.c_uint32, "i64": C.c_int64, "u64": C.c_uint64, "f64": C.c_double, "f32": C.c_float, "u8": C.c_uint8}
PROTOTYPE = re.compile(r"^[ \t]*((?:const[ \t]+)?\w+[ \t*]+)(tmpc_\w+)[ \t]*\(([^()]*)\)[ \t]*;", re.M)
STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;")

# header struct -> its Python mirror; a struct of the header that is missing here fails test_struct_mirrors unless NO_MIRROR names it with a reason
NO_MIRROR = {}


def header_text():
    with open(os.path.join(ROOT, "include", "tmpc_hip.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def c_class(decl):
    """'const void *d_x' / 'int32_t N' / 'int' (a return type) -> pointer, i32, ... ."""
    if "*" in decl:
        return "pointer"
    words = decl.replace("const", " ").split()
    return C_CLASS[words[0]]


def py_class(t):
    if t is None:
        return "void"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return "pointer"
    kind = "f" if t in (C.c_float, C.c_double) else "u" if t(-1).value > 0 else "i"
    return f"{kind}{8 * C.sizeof(t)}"


def header_prototypes(text):
    out = {}
    for ret, name, args in PROTOTYPE.findall(text):
        args = [a.strip() for a in args.split(",")]
        out[name] = (c_class(ret), [] if args == ["void"] else [c_class(a) for a in args])
    return out


def prototype_mismatches(text, signatures):
    """Every disagreement between the header's prototypes and a signature table, as text."""
    protos, bad = header_prototypes(text), []
    for name in sorted(set(protos) ^ set(signatures)):
        bad.append(f"{name}: only in the {'header' if name in protos else 'table'}")
    for name in sorted(set(protos) & set(signatures)):
        ret, args = protos[name]
        restype, argtypes = signatures[name]
        if py_class(restype) != ret:
            bad.append(f"{name}: returns {ret} in the header, {py_class(restype)} in the table")
        if len(argtypes) != len(args):
            bad.append(f"{name}: {len(args)} arguments in the header, {len(argtypes)} in the table")
            continue
        for i, (a, t) in enumerate(zip(args, argtypes)):
            if py_class(t) != a:
                bad.append(f"{name}: argument {i} is {a} in the header, {py_class(t)} in the table")
    return bad


def header_structs(text):
    """name -> ctypes.Structure built from the header's own field list."""
    defines = {k: int(v) for k, v in re.findall(r"#define\s+(\w+)\s+(-?\d+)\s*$", text, re.M)}
    out = {}
    for tag, body, name in STRUCT.findall(text):
        assert tag == name
        fields = []
        for decl in [d.strip() for d in body.split(";") if d.strip()]:
            m = re.fullmatch(r"(\w+)\s+(\w+)(?:\[(\w+)\])?", decl)
            assert m, decl
            t = C_TYPE[C_CLASS[m.group(1)]]
            if m.group(3):
                t = t * (defines[m.group(3)] if m.group(3) in defines else int(m.group(3)))
            fields.append((m.group(2), t))
        out[name] = type(name, (C.Structure,), {"_fields_": fields})
    return out


def layout(struct):
    return [(n, getattr(struct, n).offset, getattr(struct, n).size) for n, _ in struct._fields_], C.sizeof(struct)


def mirrors():
    from mpc_planner_amd import distributed, solver
    rec = distributed.RECORD_DTYPE
    rec_layout = [(n, rec.fields[n][1], rec.fields[n][0].itemsize) for n in rec.names], rec.itemsize
    return {"tmpc_dims": layout(solver.TmpcDims), "tmpc_obstacle_options": layout(solver.TmpcObstacleOptions),
            "tmpc_path_options": layout(solver.TmpcPathOptions), "tmpc_guidance_options": layout(solver.TmpcGuidanceOptions),
            "tmpc_record": rec_layout}


def struct_mismatches(text, mirror_layouts):
    bad = []
    for name, struct in header_structs(text).items():
        if name in NO_MIRROR:
            continue
        if name not in mirror_layouts:
            bad.append(f"{name}: no Python mirror")
        elif layout(struct) != mirror_layouts[name]:
            bad.append(f"{name}: header {layout(struct)} != mirror {mirror_layouts[name]}")
    return bad + [f"{name}: a mirror without a struct in the header" for name in set(mirror_layouts) - set(header_structs(text))]


def test_signature_table_matches_every_prototype():
    from mpc_planner_amd import solver
    text = header_text()
    protos = header_prototypes(text)
    assert len(protos) >= 63
    assert sorted(protos) == sorted(set(re.findall(r"\b(tmpc_[a-z0-9_]+)\s*\(", text)))      # the expression misses no function the header names
    assert prototype_mismatches(text, solver._SIGNATURES) == []
    assert solver.EXPORTS == list(solver._SIGNATURES)
    assert solver._SIGNATURES["tmpc_last_error"][0] is C.c_char_p


def test_struct_mirrors():
    text = header_text()
    assert len(header_structs(text)) >= 5
    assert struct_mismatches(text, mirrors()) == []
    assert mirrors()["tmpc_dims"][1] == 208 and mirrors()["tmpc_record"][1] == 16


def test_the_checks_see_a_wrong_row_prototype_or_field():
    """The three mistakes this file is there for, made on copies: each one has to be reported."""
    from mpc_planner_amd import solver
    text = header_text()
    table = dict(solver._SIGNATURES)
    ret, args = table["tmpc_fit_path"]
    table["tmpc_fit_path"] = (ret, args[:-1])                                                 # a table row with one pointer too few
    assert prototype_mismatches(text, table) == ["tmpc_fit_path: 17 arguments in the header, 16 in the table"]
    grown = text.replace("int tmpc_clear_slot(tmpc_handle *h, int32_t slot);", "int tmpc_clear_slot(tmpc_handle *h, int32_t slot, int32_t flags);")
    assert grown != text                                                                      # a prototype that gained an argument
    assert prototype_mismatches(grown, solver._SIGNATURES) == ["tmpc_clear_slot: 3 arguments in the header, 2 in the table"]
    table["tmpc_fit_path"] = (ret, args[:4] + [C.c_int32] + args[5:])                         # a count where the header has a pointer
    assert prototype_mismatches(text, table) == ["tmpc_fit_path: argument 4 is pointer in the header, i32 in the table"]

    class Swapped(C.Structure):                                                               # two fields of TmpcPathOptions swapped
        _fields_ = [("size", C.c_uint32), ("window_segments", C.c_int32), ("search_range", C.c_int32)]
    wrong = dict(mirrors(), tmpc_path_options=layout(Swapped))
    assert len(struct_mismatches(text, wrong)) == 1 and struct_mismatches(text, wrong)[0].startswith("tmpc_path_options:")
    assert struct_mismatches(text + "\ntypedef struct tmpc_new { int32_t a; } tmpc_new;", mirrors()) == ["tmpc_new: no Python mirror"]


# ---- BatchedSolver._call on a stub library ----------------------------------------------------------------------------------------------
class StubLibrary:
    """tmpc_* functions that record what they are given; `missing` names are absent, `codes` are returned instead of 0."""

    def __init__(self, missing=(), codes=None):
        self.calls, self.missing, self.codes = [], set(missing), codes or {}

    def __getattr__(self, name):
        if not name.startswith("tmpc_") or name in self.missing:
            raise AttributeError(name)

        def fn(*args):
            if name == "tmpc_last_error":
                return b"the stub's message"
            self.calls.append((name, args))
            if name == "tmpc_create":
                args[0]._obj.value = 0x1234
            return self.codes.get(name, 0)
        return fn


@pytest.fixture
def stub_solver():
    from mpc_planner_amd import solver

    def make(**kw):
        path = os.path.abspath("/nonexistent/libtmpc_hip_stub.so")
        solver._libs[path] = StubLibrary(**kw)
        try:
            s = solver.BatchedSolver(solver.TmpcDims(), 4, lib_path=path)
        finally:
            del solver._libs[path]
        del s.lib.calls[:]
        return s
    return make


def test_call_converts_by_the_table(stub_solver):
    s = stub_solver()
    s.scenario_halfspaces(0x7000, np.int64(6), np.int32(3), None, 0, 1, disc_offset=np.float32(0.5))
    (name, args), = s.lib.calls
    assert name == "tmpc_scenario_halfspaces" and args[0] is s._h and s._h.value == 0x1234
    assert args[1:] == (0x7000, 6, 3, None, None, 1.0, 0.5)
    assert [type(a) for a in args[1:]] == [int, int, int, type(None), type(None), float, float]
    keep = C.c_void_p(0x7100)
    opt = C.c_int32(5)
    del s.lib.calls[:]
    s._call("tmpc_select_best", True, np.uint8(2), keep, np.int64(0x7200), C.byref(opt))      # ctypes objects pass through untouched
    args = s.lib.calls[0][1]
    assert args[1:3] == (1, 2) and type(args[1]) is int and args[3] is keep and args[4] == 0x7200 and type(args[4]) is int
    assert args[5]._obj is opt


def test_call_refuses_a_missing_symbol_and_raises_on_a_code(stub_solver):
    from mpc_planner_amd import solver
    s = stub_solver(missing=["tmpc_fit_path"], codes={"tmpc_solve": -2, "tmpc_latency_mode_capacity": 7, "tmpc_set_latency_mode": 1})
    with pytest.raises(solver.TmpcError) as e:
        s.fit_path(1, 2, 3, 4, 5, 6, 7, 8)
    assert str(e.value) == "this library has no tmpc_fit_path (a missing kernel is an error, there is no host fallback)"
    with pytest.raises(solver.TmpcError) as e:
        s.solve()
    assert str(e.value) == "tmpc_solve failed (-2): the stub's message"
    assert s.latency_mode_capacity(3) == 7 and s.set_latency_mode(3) is False                 # a non-negative return that is a value, not an error
    s.lib.codes["tmpc_latency_mode_capacity"] = -1
    with pytest.raises(solver.TmpcError):
        s.latency_mode_capacity(3)
    s.lib.codes["tmpc_synchronize"] = 1                                                       # any other entry: non-zero is an error
    with pytest.raises(solver.TmpcError):
        s.synchronize()
