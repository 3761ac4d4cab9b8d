"""The second C header, include/tmpc_hip_stack.h (the row writers of generated solvers' module stacks), without a GPU: every library build
exports its entry points, mpc_planner_amd/stack_writers.py's signature table agrees with its prototypes, tmpc_hip.h and solver.EXPORTS know
nothing of them, and the two column helpers read a stack's parameter map in the documented order."""
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

NAMES = ["tmpc_stack_prepare_obstacles", "tmpc_stack_set_obstacle_columns", "tmpc_stack_linearize_topology_columns"]
GENERATED = ("tmpc_cfg2", "goal_gaussian", "jackal_tmpc", "goal_so_unicycle", "path_velocity")


def stack_header_text():
    with open(os.path.join(ROOT, "include", "tmpc_hip_stack.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def _meta(name):
    with open(os.path.join(ROOT, "build", "generated", f"{name}_meta.json")) as fh:
        return json.load(fh)


def test_every_library_exports_every_prototype():
    import __graft_entry__ as g
    g.build()
    from mpc_planner_amd import solver
    protos = header_prototypes(stack_header_text())
    assert sorted(protos) == sorted(NAMES)
    assert sorted(protos) == sorted(set(re.findall(r"\b(tmpc_[a-z0-9_]+)\s*\(", stack_header_text())))   # the expression misses no function the header names
    generated = sorted(glob.glob(os.path.join(ROOT, "build", "generated", "libtmpc_hip_*.so")))
    assert {f"libtmpc_hip_{n}.so" for n in GENERATED} <= {os.path.basename(p) for p in generated}
    for path in [solver.LIB_PATH, solver.LAB_LIB_PATH] + generated:
        lib = C.CDLL(path)
        for n in NAMES:
            assert hasattr(lib, n), f"{os.path.basename(path)} does not export {n}"


def test_signature_table_matches_the_prototypes():
    from mpc_planner_amd import solver, stack_writers
    text = stack_header_text()
    assert prototype_mismatches(text, stack_writers._SIGNATURES) == []
    assert stack_writers.EXPORTS == list(stack_writers._SIGNATURES) == NAMES
    # the first entry point has the argument list of tmpc_prepare_obstacles, as the header says
    assert header_prototypes(text)["tmpc_stack_prepare_obstacles"] == header_prototypes(header_text())["tmpc_prepare_obstacles"]
    ret, args = stack_writers._SIGNATURES["tmpc_stack_prepare_obstacles"]
    assert (ret, args) == solver._SIGNATURES["tmpc_prepare_obstacles"]
    # and the check sees a wrong row
    table = dict(stack_writers._SIGNATURES)
    ret, args = table["tmpc_stack_set_obstacle_columns"]
    table["tmpc_stack_set_obstacle_columns"] = (ret, args[:-1])
    assert prototype_mismatches(text, table) == ["tmpc_stack_set_obstacle_columns: 16 arguments in the header, 15 in the table"]


def test_first_header_and_its_table_are_unchanged():
    from mpc_planner_amd import solver
    text = header_text()
    assert "tmpc_stack_" not in text
    assert not any(n.startswith("tmpc_stack_") for n in solver.EXPORTS) and not any(n.startswith("tmpc_stack_") for n in solver._SIGNATURES)
    with open(os.path.join(HERE, "golden", "binding_calls.json")) as fh:
        golden = json.load(fh)
    assert sorted(solver.EXPORTS) == sorted(golden["bound"])
    assert '#include "tmpc_hip.h"' in open(os.path.join(ROOT, "include", "tmpc_hip_stack.h")).read()


def test_column_helpers_on_the_jackal_stack():
    import __graft_entry__ as g
    g.build()
    from mpc_planner_amd.stack_writers import obstacle_columns, topology_columns
    from mpc_planner_amd.parameters import define_parameters
    pm = _meta("jackal_tmpc")["parameter_map"]
    assert pm == dict(define_parameters(3, 5, ellipsoids=False, gaussian=True)._params)
    ocols, tcols = obstacle_columns(pm, 5, 1), topology_columns(pm, 5)
    assert len(ocols) == 32 == len(set(ocols)) and len(tcols) == 15 == len(set(tcols)) and not set(ocols) & set(tcols)
    assert ocols[:2] == [pm["ego_disc_radius"], pm["ego_disc_0_offset"]]
    for j in range(5):
        assert ocols[2 + 6 * j:8 + 6 * j] == [pm[f"gaussian_obst_{j}_{f}"] for f in ("x", "y", "major", "minor", "risk", "r")]
        assert tcols[3 * j:3 * j + 3] == [pm[f"lin_constraint_{j}_{f}"] for f in ("a1", "a2", "b")]
    assert all(0 <= c < 82 for c in ocols + tcols)
    # a missing name raises: the Gaussian stack has no ellipsoid columns, and no sixth obstacle or topology row
    for call in (lambda: obstacle_columns(pm, 5, 0), lambda: obstacle_columns(pm, 6, 1), lambda: topology_columns(pm, 6)):
        with pytest.raises(KeyError, match="parameter map has no"):
            call()
    with pytest.raises(ValueError, match="row_model"):
        obstacle_columns(pm, 5, 2)


def test_column_helpers_on_the_hand_written_layout():
    """cfg 2 (N = 20, S = 5, 8 topology rows, 8 ellipsoids): the helpers on the hand-written map give the layout's own offsets (csrc/tmpc_stage.hpp
    ip_lin, ip_disc_radius, ip_ellipsoid) -- the topology part of solver.own_parameter_columns and the contiguous ellipsoid block behind it."""
    from mpc_planner_amd import solver
    from mpc_planner_amd.parameters import define_parameters
    from mpc_planner_amd.stack_writers import obstacle_columns, topology_columns
    pm = define_parameters(5, 8)._params
    dims = solver.default_dims(N=20, S=5, n_lin=8, M=8)
    assert len(pm) == dims.npar == 135
    tcols, ocols = topology_columns(pm, 8), obstacle_columns(pm, 8, 0)
    assert tcols == solver.own_parameter_columns(dims)[:24].tolist() == list(range(53, 77))
    assert ocols == list(range(77, 77 + 2 + 7 * 8))
    # the Gaussian layout (row_model 1): 6 per obstacle behind the two disc entries
    pg = define_parameters(5, 8, ellipsoids=False, gaussian=True)._params
    assert obstacle_columns(pg, 8, 1) == list(range(77, 77 + 2 + 6 * 8))
    # the slack model's stride: one more weight in front
    ps = define_parameters(5, 8, slack=True, n_decomp=12)._params
    assert topology_columns(ps, 8) == list(range(54, 78)) and obstacle_columns(ps, 8, 0) == list(range(78, 78 + 58))
    assert np.array_equal(solver.own_parameter_columns(solver.default_dims(N=20, S=5, n_lin=8, M=8, n_slk=12, slack=1))[:24], topology_columns(ps, 8))
