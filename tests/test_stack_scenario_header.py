"""The fourth C header, include/tmpc_hip_stack_scenario.h (the scenario rows and the support of generated solvers' module stacks), without a
GPU: every library build exports its two entry points, the generated safe_horizon library among them; mpc_planner_amd/stack_scenario.py's
signature table agrees with its prototypes; the three older headers and their tables know nothing of them; scenario_columns reads a stack's
parameter map in the documented order, and the generated Safe-Horizon map is the hand-written cfg 5 map."""
import ctypes as C
import glob
import json
import os
import re
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from test_binding_signatures import header_prototypes, header_text, prototype_mismatches  # noqa: E402

NAMES = ["tmpc_stack_scenario_halfspaces", "tmpc_stack_scenario_support"]
GENERATED = ("tmpc_cfg2", "goal_gaussian", "jackal_tmpc", "goal_so_unicycle", "path_velocity", "road_decomp", "safe_horizon")


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def _meta(name):
    with open(os.path.join(ROOT, "build", "generated", f"{name}_meta.json")) as fh:
        return json.load(fh)


def test_every_library_exports_both_entry_points():
    import __graft_entry__ as g
    g.build()
    from mpc_planner_amd import solver
    text = _header("tmpc_hip_stack_scenario.h")
    protos = header_prototypes(text)
    assert sorted(protos) == sorted(NAMES)
    assert sorted(protos) == sorted(set(re.findall(r"\b(tmpc_[a-z0-9_]+)\s*\(", text)))              # the expression misses no function the header names
    generated = sorted(glob.glob(os.path.join(ROOT, "build", "generated", "libtmpc_hip_*.so")))
    assert {f"libtmpc_hip_{n}.so" for n in GENERATED} <= {os.path.basename(p) for p in generated}
    for path in [solver.LIB_PATH, solver.LAB_LIB_PATH] + generated:
        lib = C.CDLL(path)
        for n in NAMES:
            assert hasattr(lib, n), f"{os.path.basename(path)} does not export {n}"


def test_signature_table_matches_the_prototypes():
    from mpc_planner_amd import stack_scenario
    text = _header("tmpc_hip_stack_scenario.h")
    assert prototype_mismatches(text, stack_scenario._SIGNATURES) == []
    assert stack_scenario.EXPORTS == list(stack_scenario._SIGNATURES) == NAMES
    assert list(header_prototypes(text)) == NAMES                                                   # the header's order
    # and the check sees a wrong row
    table = dict(stack_scenario._SIGNATURES)
    ret, args = table["tmpc_stack_scenario_support"]
    table["tmpc_stack_scenario_support"] = (ret, args[:-1])
    assert prototype_mismatches(text, table) == ["tmpc_stack_scenario_support: 7 arguments in the header, 6 in the table"]


def test_the_older_headers_and_their_tables_are_unchanged():
    from mpc_planner_amd import solver, stack_env, stack_writers
    older = [header_text(), _header("tmpc_hip_stack.h"), _header("tmpc_hip_stack_env.h")]
    for n in NAMES:
        assert not any(n in text for text in older)
        for module in (solver, stack_writers, stack_env):
            assert n not in module.EXPORTS and n not in module._SIGNATURES
    with open(os.path.join(HERE, "golden", "binding_calls.json")) as fh:
        assert sorted(solver.EXPORTS) == sorted(json.load(fh)["bound"])
    assert len(stack_writers.EXPORTS) == 3 and len(stack_env.EXPORTS) == 4
    assert '#include "tmpc_hip.h"' in open(os.path.join(ROOT, "include", "tmpc_hip_stack_scenario.h")).read()


def test_scenario_columns_on_the_safe_horizon_stack():
    """The generated Safe-Horizon library: five path segments, the slack model, 24 scenario rows -- the hand-written cfg 5 map, spill-free."""
    import __graft_entry__ as g
    g.build()
    from mpc_planner_amd.parameters import define_parameters
    from mpc_planner_amd.stack_scenario import scenario_columns
    meta = _meta("safe_horizon")
    pm = meta["parameter_map"]
    assert pm == dict(define_parameters(5, 0, guidance=False, ellipsoids=False, slack=True, n_scenario=24)._params)
    assert meta["npar"] == len(pm) == 127 and meta["nh"] == 24 and meta["slack"]
    assert meta["spill_free"] and meta["wave_kernel_scratch"] == {}
    cols = scenario_columns(pm, 24)
    assert len(cols) == 73 == len(set(cols)) and all(0 <= c < meta["npar"] for c in cols)
    assert cols[0] == pm["ego_disc_0_offset"]
    for r in range(24):
        assert cols[1 + 3 * r:4 + 3 * r] == [pm[f"disc_0_scenario_constraint_{r}_{f}"] for f in ("a1", "a2", "b")]
    assert scenario_columns(pm, 3) == cols[:10]
    # a missing name raises: no 25th row, no second disc, a stack without scenario rows
    for call in (lambda: scenario_columns(pm, 25), lambda: scenario_columns(pm, 24, disc=1),
                 lambda: scenario_columns(_meta("road_decomp")["parameter_map"], 1)):
        with pytest.raises(KeyError, match="the parameter map has no"):
            call()


def test_scenario_columns_on_the_hand_written_layout():
    """cfg 5 (N = 20, S = 5, no topology rows, no ellipsoids, 24 slack rows): the helper on the hand-written map gives the layout's own offsets
    (csrc/tmpc_stage.hpp ip_disc_offset, ip_slk) -- the last 72 columns, as solver.own_parameter_columns states them."""
    from mpc_planner_amd import solver
    from mpc_planner_amd.parameters import define_parameters
    from mpc_planner_amd.stack_scenario import scenario_columns
    ps = define_parameters(5, 8, guidance=False, ellipsoids=False, slack=True, n_scenario=24)._params
    d5 = solver.default_dims(N=20, S=5, n_lin=0, M=0, n_slk=24, slack=1)
    assert len(ps) == d5.npar == 127
    cols = scenario_columns(ps, 24)
    assert cols == [54] + list(range(55, 127))                                # ip_disc_offset = 8 + slack + 9 S, then ip_slk
    assert cols[1:] == solver.own_parameter_columns(d5).tolist()
    with pytest.raises(KeyError, match="the parameter map has no"):
        scenario_columns(define_parameters(5, 8)._params, 1)                  # the T-MPC map has no scenario rows
