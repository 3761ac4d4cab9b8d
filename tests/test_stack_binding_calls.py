"""Every wrapper of StackWriters, StackEnvironment and StackScenario still makes the C call it made when tests/golden/stack_binding_calls.json
was recorded (on the commit before the three classes got their common base and the one binding path): same entry, the handle first, the same
arguments of the same Python types behind it -- the cols array by value and length, the options struct by field, chi as it is evaluated on the
host --, the same two TmpcError texts and the same refusals of a cols length that is no whole number of entries.  Replayed on the
StubLibrary of tests/test_binding_signatures.py, no GPU.  tests/golden/make_stack_binding_calls.py is both the recorder and the replayer."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_stack_binding_calls as recorder  # noqa: E402

ENTRIES = ["tmpc_stack_prepare_obstacles", "tmpc_stack_set_obstacle_columns", "tmpc_stack_linearize_topology_columns", "tmpc_stack_set_path_columns",
           "tmpc_stack_road_halfspaces", "tmpc_stack_decomp_halfspaces", "tmpc_stack_set_halfspace_columns", "tmpc_stack_scenario_halfspaces",
           "tmpc_stack_scenario_support"]


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "stack_binding_calls.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def now():
    return json.loads(json.dumps(recorder.record()))                         # through JSON: tuples and lists compare equal


def test_recording_covers_every_wrapper_and_entry(golden):
    assert recorder.wrappers() - set(golden["left_out"]) == set(golden["calls"]), "a wrapper without a recorded call: extend make_stack_binding_calls.CALLS"
    assert set(golden["left_out"]) == {"StackScenario.support"}
    assert sorted({c["entry"] for calls in golden["calls"].values() for c in calls}) == sorted(ENTRIES)
    assert all(c["handle_first"] for calls in golden["calls"].values() for c in calls)


def test_every_wrapper_makes_the_recorded_call(golden, now):
    for wrapper in sorted(golden["calls"]):
        assert now["calls"][wrapper] == golden["calls"][wrapper], wrapper


def test_missing_symbol_and_return_code_raise_the_recorded_text(golden, now):
    assert now["failures"] == golden["failures"]
    for entry, texts in golden["failures"].items():
        assert texts["missing"] == ["TmpcError", f"this library has no {entry} (a missing kernel is an error, there is no host fallback)"]
        assert texts["code"][0] == "TmpcError" and texts["code"][1].startswith(f"{entry} failed (") and texts["code"][1].endswith("): the stub's message")


def test_cols_that_are_no_whole_number_of_entries_are_refused_in_python(golden, now):
    assert now["value_errors"] == golden["value_errors"]
    assert sorted(v[:3] for v in golden["value_errors"].values()) == [["ValueError", "multiple of 3", True], ["ValueError", "per entry", True],
                                                                      ["ValueError", "per row", True]]
    assert all(v[3] == 0 for v in golden["value_errors"].values())           # nothing reached the library


def test_one_base_holds_call_and_one_function_reaches_the_library(monkeypatch):
    from mpc_planner_amd import _binding, solver, stack_env, stack_scenario, stack_writers
    classes = (stack_writers.StackWriters, stack_env.StackEnvironment, stack_scenario.StackScenario)
    bases = {c.__mro__[1] for c in classes}
    assert len(bases) == 1 and bases != {object}
    base, = bases
    assert "_call" in vars(base) and "__init__" in vars(base)
    assert not any("_call" in vars(c) or "__init__" in vars(c) for c in classes)
    assert solver._pointer is _binding._pointer
    # BatchedSolver._invoke and the base's _call go through the same function of the binding module
    seen = []
    real = _binding.invoke
    monkeypatch.setattr(_binding, "invoke", lambda *a, **kw: (seen.append(a[2] if len(a) > 2 else kw.get("name")), real(*a, **kw))[1])
    s = recorder._stub_solver()
    s.synchronize()
    stack_env.StackEnvironment(s).set_halfspace_columns([30, 31, 32, 33], 0x7001, 0x7002, 2)
    assert seen == ["tmpc_synchronize", "tmpc_stack_set_halfspace_columns"]
    assert [name for name, _ in s.lib.calls] == seen
    s.close()
