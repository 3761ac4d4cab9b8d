"""Records the C call every wrapper of StackWriters, StackEnvironment and StackScenario makes -> tests/golden/stack_binding_calls.json
(tests/test_stack_binding_calls.py replays it), in the manner of make_binding_calls.py.

Run on the commit whose calls are to be pinned:  python tests/golden/make_stack_binding_calls.py  (no library, no GPU).  The committed file was
recorded BEFORE the three classes got their common base and the one binding path, and the rewrite was held to it; after adding a wrapper, add
its call to CALLS, run this again and check that the diff of the JSON holds the new wrapper and nothing else.
The StubLibrary of tests/test_binding_signatures.py stands in for the library, so nothing is launched.  Per call: the entry's name, whether
the first argument is the solver's handle, and behind it the Python type and the value of every argument as the library would receive it --
the cols array as its values and its length, the options struct as its fields.  The inputs are the awkward ones on purpose: numpy scalars for
counts and reals, None and 0 for pointers, a ctypes object that has to pass through untouched."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "stack_binding_calls.json")
STUB_PATH = os.path.abspath("/nonexistent/libtmpc_hip_stack_stub.so")

KEEP = C.c_void_p(0x7100)                       # a ctypes object: passed through as it is
i64, i32, f32, f64 = np.int64, np.int32, np.float32, np.float64

# (module, class, method) -> variants of (positional arguments, keyword arguments).  StackScenario.support allocates a CUDA tensor before it
# calls support_async: tests/test_gpu_stack_scenario.py runs it on the device.
LEFT_OUT = {"StackScenario.support": "torch.empty(device=cuda) before tmpc_stack_scenario_support"}
CALLS = {
    ("stack_writers", "StackWriters", "prepare_obstacles"): [
        ((i64(2), i32(12), np.int16(5), 0x7001, 0x7002, KEEP, 0x7004, 0x7005, 0x7006, 0x7007, 0x7008, 0x7009), {}),
        ((2, 12, 5, 0x7001, 0x7002, 0x7003, 0x7004, 0x7005, 0x7006, 0x7007, 0x7008, 0x7009),
         dict(d_raw_vel=0, d_raw_pred=i64(0x700A), probabilistic=True, noise=f32(0.25), propagate_passes=i64(2), max_obstacle_distance=f64(7.5))),
    ],
    ("stack_writers", "StackWriters", "set_obstacle_columns"): [
        (([3, 7, 11, 12, 13, 14, 15, 16], i64(1), i32(1), 0x7001, 0x7002, 0x7003, KEEP, 0, None, f32(0.5)), {}),
        ((np.arange(9, dtype=np.int64), 0, 1, 0x7001, 0x7002, 0x7003, 0x7004, 0x7005, 0x7006, 0.325),
         dict(disc_offset=f32(0.125), risk=0.02, obstacle_radius=i32(1))),
        ((None, 1, 1, 0x7001, 0x7002, 0x7003, 0x7004, 0x7005, 0x7006, 0.325), {}),
    ],
    ("stack_writers", "StackWriters", "linearize_topology_columns"): [
        (([4, 5, 6, 8, 9, 10], 0x7001, i64(2), KEEP, 0x7003, f32(0.75)), {}),
        (([4, 5, 6], 0, i32(0), 0x7002, 0x7003, 0.325), dict(d_obstacle_radius=0x7004, d_static_halfspaces=0x7005, n_static=i64(1), d_is_original=KEEP)),
        ((None, None, 0, 0x7002, 0x7003, 0.325), {}),
        (([], None, 0, 0x7002, 0x7003, 0.325), {}),
    ],
    ("stack_env", "StackEnvironment", "set_path_columns"): [
        ((list(range(20, 38)), 0x7001, KEEP, i64(3)), {}),
        ((list(range(9)), 0x7001, 0x7002, i32(1)), dict(d_closest_s=0x7003, d_state=i64(0x7004))),
        ((None, 0, None, 1), {}),
    ],
    ("stack_env", "StackEnvironment", "road_halfspaces"): [
        ((list(range(9)), 0x7001, i64(2), f32(1.5), i32(2), KEEP, i64(3)), {}),
        ((list(range(18)), 0x7001, 2, 1.25, 1.75, 0x7002, 3), dict(first_row=i32(1), d_bound_segments=0x7003)),
        (([], 0x7001, 2, 1.25, 1.75, 0x7002, 3), {}),
    ],
    ("stack_env", "StackEnvironment", "decomp_halfspaces"): [
        ((0x7001, i64(2), i32(16), 0x7002, 0x7003, 0x7004, 0x7005, KEEP, 0x7007, 0, i64(400), f32(2.5), i32(4), 0x7009, None, 0x700B), {}),
    ],
    ("stack_env", "StackEnvironment", "set_halfspace_columns"): [
        (([30, 31, 32, 33, 34, 35, 36], 0x7001, KEEP, i64(2)), {}),
        (([30, 31, 32, 33], 0x7001, 0x7002, 2), dict(disc_offset=f32(0.0625))),
        (([30], 0x7001, 0x7002, 2), {}),
        ((None, 0x7001, 0x7002, 2), {}),
    ],
    ("stack_scenario", "StackScenario", "halfspaces"): [
        (([40, 41, 42, 43, 44, 45, 46], 0x7001, i64(300), KEEP, 0, f32(0.75)), {}),
        (([40, 41, 42, 43], 0x7001, 300, 0x7002, 0x7003, 0.725), dict(disc_offset=i32(1))),
        ((None, 0x7001, 300, 0x7002, 0x7003, 0.725), {}),
    ],
    ("stack_scenario", "StackScenario", "support_async"): [
        (([40, 41, 42, 43], i64(50), f32(0.5), KEEP, None), {}),
        (([], 50, 1e-6, 0x7001, 0), {}),
    ],
}
# a cols length that is not a whole number of entries: refused in Python, with the text the GPU tests match
VALUE_ERRORS = [
    (("stack_writers", "StackWriters", "linearize_topology_columns"), (([4, 5], 0x7001, 2, 0x7002, 0x7003, 0.325), {}), "multiple of 3"),
    (("stack_env", "StackEnvironment", "set_path_columns"), ((list(range(8)), 0x7001, 0x7002, 1), {}), "per entry"),
    (("stack_scenario", "StackScenario", "halfspaces"), (([40, 41, 42], 0x7001, 300, 0x7002, 0x7003, 0.725), {}), "per row"),
]
# per class: an entry the library lacks, an entry that returns a code
FAILURES = [(("stack_writers", "StackWriters", "prepare_obstacles"), "tmpc_stack_prepare_obstacles", -1),
            (("stack_env", "StackEnvironment", "decomp_halfspaces"), "tmpc_stack_decomp_halfspaces", -2),
            (("stack_scenario", "StackScenario", "support_async"), "tmpc_stack_scenario_support", 3)]


def _norm(a):
    """One argument as the stub received it: [type, value]."""
    if type(a).__name__ == "CArgObject":                          # C.byref(options)
        return ["byref", type(a._obj).__name__, {f: getattr(a._obj, f) for f, _ in a._obj._fields_}]
    if isinstance(a, C.Array):
        return ["array", a._type_.__name__, list(a), len(a)]
    if isinstance(a, C._SimpleCData):
        return [type(a).__name__, a.value, a is KEEP]
    return [type(a).__name__, a]


def _stub_solver(**kw):
    """A BatchedSolver on the StubLibrary of tests/test_binding_signatures.py (its handle: 0x1234)."""
    sys.path.insert(0, os.path.dirname(HERE))
    from test_binding_signatures import StubLibrary
    from mpc_planner_amd import solver
    solver._libs[STUB_PATH] = StubLibrary(**kw)
    try:
        s = solver.BatchedSolver(solver.TmpcDims(), 4, lib_path=STUB_PATH)
    finally:
        del solver._libs[STUB_PATH]
    del s.lib.calls[:]
    return s


def _method(s, key):
    import importlib
    module, cls, method = key
    return getattr(getattr(importlib.import_module("mpc_planner_amd." + module), cls)(s), method)


def wrappers():
    """The public methods of the three classes, as "Class.method"."""
    import importlib
    import inspect
    out = set()
    for module, cls in (("stack_writers", "StackWriters"), ("stack_env", "StackEnvironment"), ("stack_scenario", "StackScenario")):
        c = getattr(importlib.import_module("mpc_planner_amd." + module), cls)
        out |= {f"{cls}.{n}" for n, _ in inspect.getmembers(c, inspect.isfunction) if not n.startswith("_")}
    return out


def record():
    calls = {}
    for key, variants in CALLS.items():
        got = []
        for args, kwargs in variants:
            s = _stub_solver()
            assert _method(s, key)(*args, **kwargs) is None
            (name, c_args), = s.lib.calls
            got.append({"entry": name, "handle_first": c_args[0] is s._h and s._h.value == 0x1234, "args": [_norm(a) for a in c_args[1:]]})
            s.close()
        calls[f"{key[1]}.{key[2]}"] = got
    value_errors = {}
    for key, (args, kwargs), pattern in VALUE_ERRORS:
        s = _stub_solver()
        try:
            _method(s, key)(*args, **kwargs)
            seen = ["no error"]
        except ValueError as e:
            seen = ["ValueError", pattern, bool(re.search(pattern, str(e)))]
        value_errors[f"{key[1]}.{key[2]}"] = seen + [len(s.lib.calls)]         # nothing reached the library
        s.close()
    failures = {}
    for key, entry, code in FAILURES:
        args, kwargs = CALLS[key][0]
        texts = []
        for kw in (dict(missing=[entry]), dict(codes={entry: code})):
            s = _stub_solver(**kw)
            from mpc_planner_amd import solver
            try:
                _method(s, key)(*args, **kwargs)
                texts.append(["no error"])
            except solver.TmpcError as e:
                texts.append(["TmpcError", str(e)])
            s.close()
        failures[entry] = {"missing": texts[0], "code": texts[1]}
    return {"calls": calls, "value_errors": value_errors, "failures": failures, "left_out": LEFT_OUT}


def main():
    sys.path.insert(0, ROOT)
    data = record()
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {OUT}: {len(data['calls'])} wrappers")


if __name__ == "__main__":
    main()
