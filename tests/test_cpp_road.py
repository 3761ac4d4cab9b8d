"""C++ drop-in with road constraints: Contouring::update -> constructRoadConstraints (contouring.cpp:181-262 restated in
mpc_planner_amd/cpp/include/mpc_planner_modules/modules_hip.h) fills ModuleData::static_obstacles, LinearizedConstraints appends the two rows
behind the obstacle rows of every local planner, ONE batched optimize() -- for a solver generated with add_halfspaces=2 (own directory
build/generated_road: SOLVER_NLIN 10, SOLVER_MAX_OBSTACLES 8) -- against the numpy mirrors and the Python path on the same tick."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "build", "generated_road")
BIN = os.path.join(ROOT, "build", "test_road_constraints")
N, M, B, S = 20, 8, 12, 5
WIDTH = 4.0


def _build():
    import __graft_entry__ as g
    g.build()
    from mpc_planner_amd.generate_solver import generate_solver
    generate_solver(GEN, N=N, max_obstacles=M, num_segments=S, guidance=True, add_halfspaces=2)
    cpp = os.path.join(ROOT, "mpc_planner_amd", "cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(cpp, "include"), "-I", os.path.join(GEN, "include"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_road_constraints.cpp"),
                           os.path.join(cpp, "src", "solver_interface.cpp"), os.path.join(GEN, "src", "mpc_planner_parameters.cpp"),
                           "-L", os.path.join(ROOT, "mpc_planner_amd"), "-ltmpc_hip", "-Wl,-rpath," + os.path.join(ROOT, "mpc_planner_amd"),
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-o", BIN])


def test_cpp_road_modules_compile():
    """The C++ Contouring with road constraints, RealTimeData's bounds and the modules sized by max_obstacles + n_other_halfspaces compile
    against a solver generated with add_halfspaces=2 (CPU)."""
    _build()
    assert os.path.exists(BIN)
    hdr = open(os.path.join(GEN, "include", "mpc_planner_solver", "hip_solver_dims.h")).read()
    assert "#define SOLVER_NLIN 10\n" in hdr and "#define SOLVER_MAX_OBSTACLES 8\n" in hdr


def _scene_file(sc, path, selected, road_mode, two_way=False, left=None, right=None):
    from mpc_planner_amd import scenes
    W = scenes.WEIGHTS
    vals = [N, M, B, S, 1]
    vals += [W[k] for k in ("acceleration", "angular_velocity", "velocity", "reference_velocity", "contour", "lag", "terminal_angle", "terminal_contouring")]
    vals += [scenes.ROBOT_RADIUS, scenes.OBSTACLE_RADIUS]
    vals += list(sc["xinit"][0])
    for j in range(M):
        vals += list(sc["obstacles"]["pos"][j].ravel())
    vals += list(sc["segments"].ravel())
    for b in range(B):
        vals += list(sc["guidance_pos"][b].ravel()) + list(sc["guidance_vel"][b].ravel())
    vals += [selected, road_mode, WIDTH, float(two_way)]
    if road_mode == 2:
        vals += list(np.asarray(left).ravel()) + list(np.asarray(right).ravel())
    np.array(vals, float).tofile(path)


def _bounds(sc):
    """Bound cubics on the path's knots: the path shifted 2.2 m to the left and 1.9 m to the right in y (the scenes' paths run along +x)."""
    left, right = sc["segments"][:, :8].copy(), sc["segments"][:, :8].copy()
    left[:, 7] += 2.2; right[:, 7] -= 1.9
    return left, right


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["centreline", "two_way", "bounds", "off"])
def test_cpp_road_optimize_matches_python_path(tmp_path, mode):
    from mpc_planner_amd import scenes, solver, modules as md
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < os.path.getmtime(os.path.join(ROOT, "mpc_planner_amd", "libtmpc_hip.so")):
        _build()
    sc = scenes.make_scene(21, N=N, M=M, B=B, tmpc_pp=True)
    selected = 3
    left, right = _bounds(sc)
    f = str(tmp_path / "scene.bin")
    _scene_file(sc, f, selected, {"off": 0, "bounds": 2}.get(mode, 1), two_way=mode == "two_way", left=left, right=right)
    out = subprocess.run([BIN, os.path.join(GEN, "config"), f], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.splitlines()
    head = [l for l in lines if l.startswith("exit_code")][0].split()
    exit_code, best = int(head[1]), int(head[3])
    planners = [l.split() for l in lines if l.startswith("planner")]
    xs = np.array([[float(v) for v in l.split()[2:]] for l in lines if l.startswith("x ")])
    ps = np.array([[float(v) for v in l.split()[2:]] for l in lines if l.startswith("p ")])
    qs = np.array([[float(v) for v in l.split()[3:]] for l in lines if l.startswith("q ")]).reshape(B + 1, N, -1)
    road = [[float(v) for v in l.split()[2:]] for l in lines if l.startswith("road ")]
    assert [l for l in lines if l.startswith("reset")][0].split()[1:] == ["0", "0", "1"]
    # ---- the Python path on the same tick ----
    if mode == "bounds":
        rd = scenes.add_road_constraints(sc, WIDTH, left=left, right=right)
    else:
        rd = scenes.add_road_constraints(sc, WIDTH, two_way=mode == "two_way")
    pm = rd["pm"]
    road_cols = [pm.index(f"lin_constraint_{j}_{f}") for j in (M, M + 1) for f in ("a1", "a2", "b")]
    params = rd["params"].copy()
    if mode == "off":                                                   # add_road_constraints = false: the two extra rows are the dummies (1, 0, x + 100)
        assert road == []
        params[:, :, road_cols] = np.tile([1.0, 0.0, sc["xinit"][0, 0] + 100.0], 2)
        i0 = [pm.index(f"lin_constraint_{j}_{f}") for j in (0, 1) for f in ("a1", "a2", "b")]
        params[B][:, i0] = np.tile([1.0, 0.0, sc["xinit"][0, 0] + 100.0], 2)        # the non-guided planner: dummies only
    else:                                                               # Contouring::update's halfspaces == the numpy mirror
        assert len(road) == N and road[0] == []
        np.testing.assert_allclose(np.array(road[1:]).reshape(N - 1, 2, 3), rd["road_rows"][1:], rtol=0, atol=1e-12)
        assert np.abs(rd["road_rows"][1:, :, 2]).min() > 0.5 and np.ptp(rd["road_rows"][1:, 0, 2]) > 1e-3       # real, stage-dependent rows
    np.testing.assert_allclose(qs[:, :, road_cols], params[:, :, road_cols], rtol=0, atol=1e-12)   # road-row parameters of EVERY planner
    np.testing.assert_allclose(qs, params, rtol=0, atol=1e-12)
    s = solver.BatchedSolver(solver.default_dims(N=N, S=S, n_lin=M + 2, M=M), B_max=B + 1)
    s.set_latency_mode(True)                                            # the C++ Solver mirror serves ticks with a latency variant where the shape has one
    s.set_batch(sc["xinit"], sc["x0"], params); s.solve(); g = s.get()
    w = np.ones(B + 1); w[selected] = 0.75
    py_best = s.select_best(weight=w)
    s.close()
    assert len(planners) == B + 1
    for b, pl in enumerate(planners):
        assert int(pl[3]) == 0 and int(pl[5]) == g["exit_code"][b], (b, pl)
        if g["exit_code"][b] == 1:
            assert abs(float(pl[7]) - g["pobj"][b] * w[b]) <= 1e-7 * max(1.0, abs(g["pobj"][b]))
    assert (g["exit_code"] == 1).sum() >= 2
    assert best == py_best and exit_code == g["exit_code"][py_best]
    np.testing.assert_allclose(ps, params[py_best], rtol=0, atol=1e-12)
    np.testing.assert_allclose(xs, g["xtraj"][py_best], rtol=0, atol=1e-7)
    if mode != "off":                                                   # the winner respects the road rows (linear rows: the last QP's bound carries over)
        k = np.arange(1, N)
        for j in range(2):
            val = rd["road_rows"][k, j, 0] * g["xtraj"][py_best][k, 0] + rd["road_rows"][k, j, 1] * g["xtraj"][py_best][k, 1] - rd["road_rows"][k, j, 2]
            assert val.max() <= 1e-5
