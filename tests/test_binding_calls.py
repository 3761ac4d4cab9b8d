"""Every BatchedSolver wrapper still makes the C call it made when tests/golden/binding_calls.json was recorded (on the commit before the
binding got its signature table): same function, same arguments in the same order, same return value -- replayed on a recording stub, no GPU.
tests/golden/make_binding_calls.py is both the recorder and the replayer; it finds the methods by introspection."""
import inspect
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_binding_calls as recorder  # noqa: E402

# The only methods that may be missing from the recording: they allocate a CUDA tensor before they call the library.
# tests/test_gpu_shmpc_loop.py runs all three on the device.
LEFT_OUT = {"scenario_support", "scenario_discarded", "scenario_empty_stages"}
# Declared `void` in the header: the recorded commit left ctypes' default restype (c_int) on them, the table says None.
VOID = {"tmpc_default_dims", "tmpc_default_dims_ex", "tmpc_destroy"}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "binding_calls.json")) as f:
        return json.load(f)


def test_recording_covers_every_public_method(golden):
    from mpc_planner_amd import solver
    public = {n for n, _ in inspect.getmembers(solver.BatchedSolver, inspect.isfunction) if not n.startswith("_")}
    assert set(golden["left_out"]) == LEFT_OUT == set(recorder.NEEDS_CUDA_TENSOR)
    assert public - LEFT_OUT == set(golden["calls"]), "a wrapper without a recorded call (or a recorded wrapper that is gone): extend tests/golden/binding_calls.json"


def test_every_wrapper_makes_the_recorded_call(golden):
    from mpc_planner_amd import solver
    now = json.loads(json.dumps(recorder.record(solver)))["calls"]           # through JSON: tuples and lists compare equal
    for method in sorted(golden["calls"]):
        assert now[method] == golden["calls"][method], method


def test_argtypes_are_the_recorded_ones(golden):
    import __graft_entry__ as g
    g.build()
    from mpc_planner_amd import solver
    now = recorder.bound_types(solver)
    assert set(now) == set(golden["bound"])
    for name, was in golden["bound"].items():
        if was["argtypes"] is not None:                                      # None: never bound on the recorded commit (tests/test_binding_signatures.py holds them to the header)
            assert now[name]["argtypes"] == was["argtypes"], name
        if name not in VOID:
            assert now[name]["restype"] == was["restype"], name
        else:
            assert now[name]["restype"] is None, name
