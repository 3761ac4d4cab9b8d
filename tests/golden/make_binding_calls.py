"""Records the C call every public BatchedSolver method makes -> tests/golden/binding_calls.json (tests/test_binding_calls.py replays it).

Run on the commit whose calls are to be pinned:  python tests/golden/make_binding_calls.py  (needs the built library for the argtypes, no
GPU).  The committed file was recorded on solver.py as it stood BEFORE the binding got its signature table and one call path, and the rewrite
was held to it; after adding a wrapper, run it again and check that the diff of the JSON holds the new method and nothing else.
A recording stub stands in for the library, so nothing is launched: `record()` finds the methods by introspection, gives every parameter a
sentinel chosen from its name and default, and calls each method with every parameter set, with the required ones only, and with the
variants of EXTRA.  A parameter the rules below cannot classify is an error, so a new wrapper cannot be skipped silently."""
import ctypes as C
import hashlib
import inspect
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "binding_calls.json")
FAKE_PATH = "/nonexistent/libtmpc_hip_recording_stub.so"
B = 3

# Methods that allocate a CUDA tensor before they call the library: not recordable without a GPU; tests/test_gpu_shmpc_loop.py runs them on the device.
NEEDS_CUDA_TENSOR = {"scenario_support": "torch.empty(device=cuda) before tmpc_scenario_support",
                     "scenario_discarded": "torch.zeros(device=cuda) before tmpc_scenario_discarded",
                     "scenario_empty_stages": "torch.zeros(device=cuda) before tmpc_scenario_empty_stages"}
# required parameters that are reals / counts (those with defaults are classified by the default's type)
REALS = {"robot_radius", "offset_first", "offset_second", "resolution", "decomp_range", "radius", "tol"}
# further variants: the required parameters plus these -- the None / 0 / False paths that neither of the two standard calls reaches
EXTRA = {"set_slots": [dict(slots=None)], "set_param_sharing": [dict(base_of=None)], "scatter_parameters": [dict(cols=None)],
         "guidance_plan": [dict(options=None)], "guidance_decide": [dict(options=None, enable_output=False)],
         "solve": [dict(sync=False)], "solve_iterations": [dict(keep_iterate=True, complete=False, sync=False), dict(keep_multipliers=True, new_solve=True)],
         "set_latency_mode": [dict(on=False), dict(on=2), dict(on=3)], "set_throughput_mode": [dict(on=False)],
         "pack_records": [dict(d_guidance_id=0, d_weight=0)], "set_batch_device": [dict(d_xinit=0)], "warmstart": [dict(d_mode=0)],
         "prepare_obstacles": [dict(d_raw_vel=0x7700, probabilistic=True, propagate_passes=2)]}
COUNTS = {"B", "S", "n_iter", "slot", "mode", "reps", "max_records", "first", "size_x", "size_y", "pos_stride", "per_rank", "set_size", "seed", "max_obstacles"}


def _norm(a):
    """One argument as the stub received it, in a form that does not depend on addresses of host memory."""
    if a is None:
        return None
    if isinstance(a, C.c_void_p):
        arr = getattr(a, "_arr", None)                           # numpy's data_as keeps the array alive here: a host array
        if arr is not None:
            return ["host", str(arr.dtype), int(arr.nbytes)]
        return None if a.value is None else ["int", a.value]      # a pointer that came from an integer: the integer, wrapped or not; NULL: None
    if type(a).__name__ == "CArgObject":                          # C.byref(x)
        return ["byref", type(a._obj).__name__, bytes(a._obj).hex()]
    if isinstance(a, C.Array):
        raw = bytes(a)
        return ["array", type(a).__name__, raw.hex() if len(raw) <= 256 else "sha256:" + hashlib.sha256(raw).hexdigest()]
    if isinstance(a, C._SimpleCData):                             # e.g. c_uint64(seed): its value
        a = a.value
    if isinstance(a, (bool, int, float, bytes, str)):
        return [type(a).__name__, a.decode() if isinstance(a, bytes) else a]
    return ["?", type(a).__module__ + "." + type(a).__name__, repr(a)]


def _norm_return(r):
    if isinstance(r, np.ndarray):
        return ["ndarray", str(r.dtype), list(r.shape)]
    if isinstance(r, dict):
        return {k: _norm_return(v) for k, v in r.items()}
    if isinstance(r, (tuple, list)):
        return [_norm_return(v) for v in r]
    if r is None or isinstance(r, (bool, int, float, str)):
        return [type(r).__name__, r]
    return ["?", type(r).__name__, repr(r)]


class RecordingStub:
    """Any tmpc_* attribute is a function that records (name, normalised arguments) and returns 0; the few entries with out-parameters or a
    value as their return give fixed ones, so that what the wrappers return is pinned too."""

    def __init__(self):
        self.calls = []
        self._handles = 0

    def __getattr__(self, name):
        if not name.startswith("tmpc_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append([name, [_norm(a) for a in args]])
            return self._answer(name, args)
        fn.__name__ = name
        return fn

    def _answer(self, name, args):
        if name == "tmpc_create":
            self._handles += 1
            args[0]._obj.value = 0x5000 + self._handles
        elif name == "tmpc_last_error":
            return b"stub error text"
        elif name in ("tmpc_set_latency_mode", "tmpc_has_lane_kernels"):
            return 1
        elif name == "tmpc_latency_mode_capacity":
            return 5
        elif name == "tmpc_kernel_info":
            args[1].value = b"stub kernel"
            return 11
        elif name == "tmpc_select_best":
            args[5]._obj.value = 2
        elif name == "tmpc_get_timings":
            args[3]._obj.value = 2
        elif name == "tmpc_get_stream":
            args[1]._obj.value = 0xABC0
        elif name == "tmpc_result_device_ptrs":
            args[1]._obj.value, args[2]._obj.value = 0xD100, 0xD200
        return 0


def _dims(solver):
    d = solver.TmpcDims()
    d.N, d.S, d.n_lin, d.M, d.npar, d.n_slk, d.slack = 4, 1, 2, 1, 21, 1, 0
    return d


def _value(solver, s, name, default, k):
    """The sentinel of parameter `name` (k-th parameter of its method): distinct per position."""
    d, rng = s.dims, np.random.RandomState(k)
    host = {"xinit": lambda: rng.rand(B, d.nx), "x0": lambda: rng.rand(B, d.N + 1, d.nvar), "params": lambda: rng.rand(B, d.N, d.npar),
            "slots": lambda: [2, 0, 1], "base_of": lambda: [0, 0, 2], "weight": lambda: [1.5, 0.5, 2.5], "disabled": lambda: [0, 1, 0],
            "z": lambda: rng.rand(2, d.nvar), "p": lambda: rng.rand(2, d.npar), "pi": lambda: rng.rand(2, solver.NX), "lamh": lambda: rng.rand(2, d.nh),
            "cols": lambda: [3, 7, 11], "options": lambda: solver.guidance_options(3, selection_weight_consistency=0.75)}
    if name in host:
        return host[name]()
    if name == "other":
        return solver.BatchedSolver(_dims(solver), B, lib_path=FAKE_PATH)
    if name.startswith("d_"):
        return 0x7F0000000000 + 0x1000 * (k + 1)
    if isinstance(default, bool):
        return True
    if isinstance(default, float) or name in REALS:
        return 0.25 + k + 0.0625 * k
    if isinstance(default, int) or name.startswith("n_") or name in COUNTS or (default is None and name in ("count",)):
        return 2 + k
    raise SystemExit(f"make_binding_calls: cannot classify parameter {name!r} (default {default!r}): add a rule")


def record(solver):
    """-> {"calls": {method: {"all": ..., "required": ...}}, "left_out": {...}} on whatever mpc_planner_amd.solver is given."""
    stub = RecordingStub()
    solver._libs[FAKE_PATH] = stub
    try:
        out = {}
        methods = [(n, f) for n, f in inspect.getmembers(solver.BatchedSolver, inspect.isfunction) if not n.startswith("_")]
        for name, fn in methods:
            if name in NEEDS_CUDA_TENSOR:
                continue
            out[name] = {}
            for variant in ["all", "required"] + [f"extra{i}" for i in range(len(EXTRA.get(name, [])))]:
                stub._handles = 0
                s = solver.BatchedSolver(_dims(solver), B, lib_path=FAKE_PATH)
                s.B = B
                kwargs = {}
                for k, (pname, par) in enumerate(list(inspect.signature(fn).parameters.items())[1:]):
                    required = par.default is inspect.Parameter.empty
                    if required or variant == "all":
                        kwargs[pname] = _value(solver, s, pname, None if required else par.default, k)
                if variant.startswith("extra"):
                    kwargs.update(EXTRA[name][int(variant[5:])])
                del stub.calls[:]
                ret = fn(s, **kwargs)
                out[name][variant] = {"calls": [list(c) for c in stub.calls], "returns": _norm_return(ret)}
                for v in [s] + list(kwargs.values()):            # no handle is left for a later __del__ to destroy in the middle of another recording
                    if isinstance(v, solver.BatchedSolver):
                        v.close()
        return {"calls": out, "left_out": NEEDS_CUDA_TENSOR}
    finally:
        del solver._libs[FAKE_PATH]


def bound_types(solver):
    """argtypes / restype of every exported function as load_library left them on the real library (None: never set)."""
    lib = solver.load_library()
    out = {}
    for name in sorted(solver.EXPORTS):
        f = getattr(lib, name)
        out[name] = {"argtypes": None if f.argtypes is None else [t.__name__ for t in f.argtypes],
                     "restype": None if f.restype is None else f.restype.__name__}
    return out


def main():
    sys.path.insert(0, ROOT)
    from mpc_planner_amd import solver
    data = record(solver)
    data["bound"] = bound_types(solver)
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {OUT}: {len(data['calls'])} methods, {len(data['bound'])} functions")


if __name__ == "__main__":
    main()
