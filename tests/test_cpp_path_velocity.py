"""C++ PathReferenceVelocity (mpc_planner_modules/modules_hip.h; PathVelocityProfile of mpc_planner_modules/reference_path.h) against the
numpy mirror (mpc_planner_amd/modules.py fit_path / path_velocity_window / path_velocity_at): onDataReceived fits the profile on the
centreline's knots, update publishes it in ModuleData, setParameters writes the spline_v columns through the generated
setSolverParameterSplineV{A..D} -- values bitwise (%.17g round-trips a double), nothing else written.  CPU: built against the host side of the
`path_velocity` stack of build(); no Solver object is made."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "mpc_planner_amd", "cpp")
SRC = os.path.join(ROOT, "tests", "cpp", "test_path_velocity.cpp")
GEN = os.path.join(ROOT, "build", "generated_path_velocity")
BIN = os.path.join(ROOT, "build", "test_path_velocity")
N, S = 20, 3


def _build():
    """The host side of the stack (parameter map, setSolverParameter* functions, dims header) and the program; the library is linked for
    the Solver class the headers declare, none is constructed.  n_lin = M = 0: the stack's rows are the generated library's, none of the
    hand-written row modules of modules_hip.h is compiled."""
    import __graft_entry__ as g
    g.build()
    from mpc_planner_amd import generate_solver as gs
    from mpc_planner_amd.codegen import plugin as P, stacks
    st = stacks.settings(N=N, max_obstacles=2, num_segments=S); st["contouring"]["dynamic_velocity_reference"] = True
    model, mm = stacks.contouring_path_velocity_ellipsoids(st)
    pm = P.define_parameters(mm, P.Parameters(), st)
    gs._write_host_side(GEN, pm, N, False, 10, 0.2, n_lin=0, M=0, n_slk=0, num_segments=S, max_obstacles=2, model=model)
    assert "#define SOLVER_PATH_VELOCITY 1" in open(os.path.join(GEN, "include", "mpc_planner_solver", "hip_solver_dims.h")).read()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(CPP, "include"),
                           "-I", os.path.join(GEN, "include"), "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include", SRC, os.path.join(CPP, "src", "solver_interface.cpp"),
                           os.path.join(GEN, "src", "mpc_planner_parameters.cpp"), "-L", os.path.join(ROOT, "mpc_planner_amd"), "-ltmpc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "mpc_planner_amd"), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-o", BIN])
    return pm


def test_stacks_without_the_columns_do_not_get_the_module(tmp_path):
    from mpc_planner_amd.generate_solver import generate_solver
    generate_solver(str(tmp_path), N=N, max_obstacles=2, num_segments=S)
    assert "SOLVER_PATH_VELOCITY" not in open(tmp_path / "include" / "mpc_planner_solver" / "hip_solver_dims.h").read()


@pytest.mark.parametrize("given_s", [False, True])
def test_host_module_writes_the_mirrors_columns(tmp_path, given_s):
    """Seven waypoints (six segments) with a velocity, S = 3.  Ticks: the segment in the middle; count - 2 (one zero slot); count - 1 (two);
    -1 (before the first track: clamped to 0); closest_s inside a segment, ON a knot, at the length, below the first knot.  Rows 0 and
    N - 1 of a block prefilled with -3: the twelve spline_v columns equal the mirror's window, every other column keeps the prefill; v_ref
    equals path_velocity_at.  With given s the knots are the path's own (stretched and moved), else chord lengths.  A path without
    velocities: nothing is published and every slot is (0, 0, 0, reference_velocity)."""
    import path_fit_cases as pf
    from mpc_planner_amd import modules as md
    pm = _build()
    ref_v = 1.7
    xy = pf.waypoints(np.random.default_rng(31), 7)
    v = np.random.default_rng(32).uniform(0.5, 2.5, 7)
    s_in = 1.25 * md.path_knots(xy) + 3.5
    fit = md.fit_path(xy, s=s_in if given_s else None, v=v)
    knots = fit["path"][:, 8]
    ticks = [(2, 0.5 * (knots[2] + knots[3])), (4, knots[4]), (5, fit["length"]), (-1, knots[0] - 0.5)]
    vals = [S, ref_v, int(given_s), 7]
    for i in range(7):
        vals += [xy[i, 0], xy[i, 1], s_in[i], v[i]]
    vals += [len(ticks)] + [x for t in ticks for x in t]
    f = str(tmp_path / "scene.bin")
    np.array(vals, float).tofile(f)
    out = subprocess.run([BIN, os.path.join(GEN, "config"), f], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l.split() for l in out.stdout.splitlines()]
    assert [l[1] for l in lines if l[0] == "published"] == ["1", "0"]
    profile = [l for l in lines if l[0] == "profile"][0]
    assert int(profile[1]) == 6 and float(profile[2]) == fit["length"]
    cols = [pm.index(f"spline_v{i}_{k}") for i in range(S) for k in "abcd"]
    rest = np.setdiff1d(np.arange(pm.length()), cols)
    rows = {(int(l[1]), int(l[2])): np.array([float(x) for x in l[3:]]) for l in lines if l[0] == "p"}
    v_ref = {int(l[1]): float(l[2]) for l in lines if l[0] == "tick"}
    for t, (seg, s) in enumerate(ticks):
        want = md.path_velocity_window(fit["velocity"], fit["count"], max(seg, 0), S, ref_v)
        for k in (0, N - 1):
            assert len(rows[(t, k)]) == pm.length()
            assert np.array_equal(rows[(t, k)][cols], want.ravel()), (t, k)
            assert (rows[(t, k)][rest] == -3.0).all()
        assert v_ref[t] == md.path_velocity_at(fit["velocity"], fit["path"], fit["count"], fit["length"], s, ref_v), t
    assert (md.path_velocity_window(fit["velocity"], 6, 4, S, ref_v)[2] == 0.0).all() and v_ref[1] == v[4]      # (what the cases are meant to reach)
    plain = np.array([float(x) for x in [l for l in lines if l[0] == "noprofile"][0][2:]])
    assert np.array_equal(plain[cols], md.path_velocity_window(None, 0, 1, S, ref_v).ravel()) and (plain[rest] == -3.0).all()
