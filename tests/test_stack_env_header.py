"""The third C header, include/tmpc_hip_stack_env.h (the path window, the road rows and the decomp rows of generated solvers' module stacks),
without a GPU: every library build exports its entry points, mpc_planner_amd/stack_env.py's signature table agrees with its prototypes, the two
older headers and their tables know nothing of them, the two column helpers read a stack's parameter map in the documented order, and the
scenes of the closed-loop test (tests/stack_env_cases.py) hold what they were chosen for on the mirrors."""
import ctypes as C
import glob
import json
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from test_binding_signatures import header_prototypes, header_text, prototype_mismatches  # noqa: E402

NAMES = ["tmpc_stack_set_path_columns", "tmpc_stack_road_halfspaces", "tmpc_stack_decomp_halfspaces", "tmpc_stack_set_halfspace_columns"]
GENERATED = ("tmpc_cfg2", "goal_gaussian", "jackal_tmpc", "goal_so_unicycle", "path_velocity", "road_decomp")


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def _meta(name):
    with open(os.path.join(ROOT, "build", "generated", f"{name}_meta.json")) as fh:
        return json.load(fh)


def test_every_library_exports_every_prototype():
    import __graft_entry__ as g
    g.build()
    from mpc_planner_amd import solver
    text = _header("tmpc_hip_stack_env.h")
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
    from mpc_planner_amd import solver, stack_env
    text = _header("tmpc_hip_stack_env.h")
    assert prototype_mismatches(text, stack_env._SIGNATURES) == []
    assert stack_env.EXPORTS == list(stack_env._SIGNATURES) == NAMES
    assert list(header_prototypes(text)) == NAMES                                                   # the header's order
    # the decomposition has the argument list of tmpc_decomp_halfspaces, as the header says
    assert header_prototypes(text)["tmpc_stack_decomp_halfspaces"] == header_prototypes(header_text())["tmpc_decomp_halfspaces"]
    assert stack_env._SIGNATURES["tmpc_stack_decomp_halfspaces"] == solver._SIGNATURES["tmpc_decomp_halfspaces"]
    # and the check sees a wrong row
    table = dict(stack_env._SIGNATURES)
    ret, args = table["tmpc_stack_road_halfspaces"]
    table["tmpc_stack_road_halfspaces"] = (ret, args[:-1])
    assert prototype_mismatches(text, table) == ["tmpc_stack_road_halfspaces: 11 arguments in the header, 10 in the table"]


def test_the_older_headers_and_their_tables_are_unchanged():
    from mpc_planner_amd import solver, stack_writers
    first, second = header_text(), _header("tmpc_hip_stack.h")
    for n in NAMES:
        assert n not in first and n not in second
        assert n not in solver.EXPORTS and n not in solver._SIGNATURES and n not in stack_writers.EXPORTS and n not in stack_writers._SIGNATURES
    with open(os.path.join(HERE, "golden", "binding_calls.json")) as fh:
        assert sorted(solver.EXPORTS) == sorted(json.load(fh)["bound"])
    assert len(stack_writers.EXPORTS) == 3
    assert '#include "tmpc_hip.h"' in open(os.path.join(ROOT, "include", "tmpc_hip_stack_env.h")).read()


def test_column_helpers_on_the_road_decomp_stack():
    import __graft_entry__ as g
    g.build()
    from mpc_planner_amd.parameters import define_parameters
    from mpc_planner_amd.stack_env import decomp_columns, path_columns
    from mpc_planner_amd.stack_writers import obstacle_columns, topology_columns
    meta = _meta("road_decomp")
    pm = meta["parameter_map"]
    assert meta["npar"] == 76 and meta["nh"] == 10 and meta["slack"] and meta["spill_free"]
    assert pm == dict(define_parameters(3, 2, add_halfspaces=2, slack=True, n_decomp=4)._params)
    pcols, dcols, tcols, ocols = path_columns(pm, 3), decomp_columns(pm, 4), topology_columns(pm, 4), obstacle_columns(pm, 2, 0)
    assert len(pcols) == 27 == len(set(pcols)) and len(dcols) == 13 == len(set(dcols))
    # disjoint from each other and from the topology and collision columns -- but for ego_disc_0_offset, which EllipsoidConstraints and
    # DecompConstraints both set (ellipsoid_constraints.cpp, decomp_constraints.cpp: setParameters) and both helpers therefore name
    assert not set(pcols) & set(dcols) and not set(pcols + dcols) & set(tcols) and not set(pcols) & set(ocols)
    assert set(dcols) & set(ocols) == {pm["ego_disc_0_offset"]} and dcols[0] == pm["ego_disc_0_offset"]
    for i in range(3):
        names = [f"spline_{a}{i}_{c}" for a in "xy" for c in "abcd"] + [f"spline{i}_start"]
        assert pcols[9 * i:9 * i + 9] == [pm[n] for n in names]
    for r in range(4):
        assert dcols[1 + 3 * r:4 + 3 * r] == [pm[f"disc_0_decomp_{r}_{f}"] for f in ("a1", "a2", "b")]
    assert all(0 <= c < 76 for c in pcols + dcols)
    # a missing name raises: no fourth segment, no fifth decomp row, no second disc; a stack without decomp rows or without a path
    for call in (lambda: path_columns(pm, 4), lambda: decomp_columns(pm, 5), lambda: decomp_columns(pm, 4, disc=1),
                 lambda: decomp_columns(_meta("jackal_tmpc")["parameter_map"], 1), lambda: path_columns(_meta("goal_so_unicycle")["parameter_map"], 1)):
        with pytest.raises(KeyError, match="the parameter map has no"):
            call()


def test_column_helpers_on_the_hand_written_layout():
    """The slack model with 12 decomp rows (N = 20, S = 5, 8 topology rows, 8 ellipsoids): the helpers on the hand-written map give the layout's
    own contiguous offsets (csrc/tmpc_stage.hpp ip_spline, ip_disc_offset, ip_slk)."""
    from mpc_planner_amd import solver
    from mpc_planner_amd.parameters import define_parameters
    from mpc_planner_amd.stack_env import decomp_columns, path_columns
    ps = define_parameters(5, 8, slack=True, n_decomp=12)._params
    dims = solver.default_dims(N=20, S=5, n_lin=8, M=8, n_slk=12, slack=1)
    assert len(ps) == dims.npar == 172
    assert path_columns(ps, 5) == list(range(9, 54))                          # ip_spline: 8 + slack + 9 seg + which
    assert decomp_columns(ps, 12) == [79] + list(range(136, 172))             # ip_disc_offset, then ip_slk: the last 36 columns
    # without the slack weight the window starts one column earlier
    pn = define_parameters(5, 8)._params
    assert path_columns(pn, 5) == list(range(8, 53))
    with pytest.raises(KeyError, match="the parameter map has no"):
        decomp_columns(pn, 1)


def test_the_closed_loop_scenes_hold_their_conditions_on_the_mirrors():
    """tests/stack_env_cases.py at tick 0: in every scene the decomposition has complete stages (rows, status 0) and truncated ones, the road rows
    are real rows, every column of the stack but the nine weights is written, and nothing is NaN."""
    import __graft_entry__ as g
    g.build()
    import stack_env_cases as cases
    from mpc_planner_amd.stack_env import decomp_columns, path_columns
    from mpc_planner_amd.stack_writers import obstacle_columns, topology_columns
    pm = _meta("road_decomp")["parameter_map"]
    pb = cases.problem()
    pcols = path_columns(pm, cases.S)
    base = cases.base_rows(pm)
    blank = base.copy()
    written = sorted(set(pcols + decomp_columns(pm, cases.N_ROWS) + obstacle_columns(pm, cases.M, 0) + topology_columns(pm, cases.N_TOPO)))
    assert len(written) == 76 - 9
    blank[:, :, written] = np.nan
    t = cases.host_tick(pm, pcols, blank, pb["xinit"][::cases.P].copy(), pb["x0"], np.full(cases.Q, -1), 0)
    assert not np.isnan(t["rows"]).any()
    for q in range(cases.Q):
        dc = t["decomp"][q]
        assert ((dc["count"] > 0) & (dc["status"] == 0)).any() and (dc["status"] == 1).any() and not (dc["status"] == 2).any()
        assert np.isfinite(t["road"][q, 1:]).all() and (np.abs(t["road"][q, 1:, :, :2]).max(axis=2) > 0.1).all()
    assert (t["obstacles"][1]["selected"] < 0).any() and not (t["obstacles"][0]["selected"] < 0).any()
