"""C++ reference path: the Solver-free header mpc_planner_modules/reference_path.h (g++ only, CPU) on the scenes of the bitwise device test
(tests/path_cases.py) against the numpy mirror (mpc_planner_amd/modules.py track_path) -- segments equal, values bitwise (%.17g round-trips a
double) --, and Contouring::update in path mode (modules_hip.h, RealTimeData::reference_path) on a generated solver over three ticks and a
new path: current_path_segment, state["spline"] and the spline rows of the solver against the mirror; in the same program the batched device
twin (mpc_planner_modules/reference_path_batch.h) against the header.  The window mode (an empty
reference_path) is what tests/test_cpp_road.py and tests/test_cpp_optimize.py cover."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "mpc_planner_amd", "cpp")
SRC = os.path.join(ROOT, "tests", "cpp", "test_reference_path.cpp")
BIN = os.path.join(ROOT, "build", "test_reference_path")
GEN = os.path.join(ROOT, "build", "generated_path")
BIN_SOLVER = os.path.join(ROOT, "build", "test_reference_path_solver")
N, M, S = 20, 8, 5


def _build_header_only():
    """No generated header, no HIP, no library: the header stands alone."""
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(CPP, "include"), SRC, "-o", BIN])


@pytest.mark.parametrize("with_bounds", [False, True])
def test_header_equals_the_mirror_bitwise(tmp_path, with_bounds):
    import path_cases as pc
    _build_header_only()
    case = pc.bitwise_scenes()
    want = pc.mirror(case, with_bounds)
    n_sc = len(case["count"])
    vals = [n_sc, pc.N_SEG_MAX, pc.S, pc.SEARCH_RANGE, int(with_bounds)]
    for q in range(n_sc):
        vals += [case["count"][q], case["length"][q], case["segment"][q], case["pos"][q, 0], case["pos"][q, 1]]
        vals += list(case["path"][q].ravel()) + list(case["bounds"][q].ravel())
    f = str(tmp_path / "scenes.bin")
    np.array(vals, float).tofile(f)
    out = subprocess.run([BIN, f], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l.split() for l in out.stdout.splitlines()]
    scenes_out = {int(l[1]): l for l in lines if l[0] == "scene"}
    assert sorted(scenes_out) == [q for q in range(n_sc) if case["count"][q] > 0]          # the count-0 scene: nothing
    for q, l in scenes_out.items():
        assert int(l[2]) == want["segment"][q] and float(l[3]) == want["s"][q] and int(l[4]) == want["reached"][q], (q, l)
    win = np.array([[float(v) for v in l[3:]] for l in lines if l[0] == "w"]).reshape(len(scenes_out), pc.S, 9)
    assert np.array_equal(win, want["window"][sorted(scenes_out)])
    if with_bounds:
        for side, tag in enumerate("lr"):
            bw = np.array([[float(v) for v in l[3:]] for l in lines if l[0] == tag]).reshape(len(scenes_out), pc.S, 8)
            assert np.array_equal(bw, want["bound_window"][sorted(scenes_out), side])
    else:
        assert not [l for l in lines if l[0] in "lr"]


def _build_solver():
    import __graft_entry__ as g
    g.build()
    from mpc_planner_amd.generate_solver import generate_solver
    generate_solver(GEN, N=N, max_obstacles=M, num_segments=S, guidance=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-DWITH_SOLVER", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(CPP, "include"),
                           "-I", os.path.join(GEN, "include"), "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include", SRC, os.path.join(CPP, "src", "solver_interface.cpp"),
                           os.path.join(GEN, "src", "mpc_planner_parameters.cpp"), "-L", os.path.join(ROOT, "mpc_planner_amd"), "-ltmpc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "mpc_planner_amd"), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-o", BIN_SOLVER])


def test_cpp_contouring_path_mode_compiles():
    """Contouring with RealTimeData::reference_path, onDataReceived, reset and isObjectiveReached compiles against a generated solver (CPU)."""
    _build_solver()
    assert os.path.exists(BIN_SOLVER)


@pytest.mark.gpu
def test_cpp_contouring_update_in_path_mode(tmp_path):
    """Three ticks along a 12 x 2 m path -- a reset (global search), one step across the first knot, a jump the local search (range 2) cannot
    follow -- then the same position after a new path arrived (global again): current_path_segment, state["spline"] and the spline columns of
    the solver's parameter rows (stages 0 and N - 1) equal the mirror's, bit for bit; the weights are written, nothing else is."""
    from mpc_planner_amd import scenes, modules as md
    from mpc_planner_amd.parameters import define_parameters
    if not os.path.exists(BIN_SOLVER) or os.path.getmtime(BIN_SOLVER) < os.path.getmtime(os.path.join(ROOT, "mpc_planner_amd", "libtmpc_hip.so")):
        _build_solver()
    path = scenes.reference_path_segments(np.random.default_rng(5), S=12, seg_len=2.0)
    length = 24.0
    ticks = [(1.7, 0.1, 0), (2.3, 0.1, 0), (21.9, 0.2, 0), (21.9, 0.2, 1)]
    W = scenes.WEIGHTS
    vals = [N, S] + [W[k] for k in ("acceleration", "angular_velocity", "velocity", "reference_velocity", "contour", "lag", "terminal_angle", "terminal_contouring")]
    vals += [scenes.ROBOT_RADIUS, 0.0, 0.0, 0.0, 1.0, -5.0]
    vals += [len(path)] + list(path.ravel()) + [length, len(ticks)] + [v for t in ticks for v in t]
    f = str(tmp_path / "scene.bin")
    np.array(vals, float).tofile(f)
    out = subprocess.run([BIN_SOLVER, os.path.join(GEN, "config"), f], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l.split() for l in out.stdout.splitlines()]
    got_ticks = [l for l in lines if l[0] == "tick"]
    rows = {(int(l[1]), int(l[2])): np.array([float(v) for v in l[3:]]) for l in lines if l[0] == "p"}
    pm = define_parameters(S, M, guidance=True)
    spl = [pm.index(n.format(i)) for i in range(S) for n in ("spline_x{}_a", "spline_x{}_b", "spline_x{}_c", "spline_x{}_d",
                                                              "spline_y{}_a", "spline_y{}_b", "spline_y{}_c", "spline_y{}_d", "spline{}_start")]
    seg, segs = -1, []
    for t, (x, y, new_path) in enumerate(ticks):
        want = md.track_path(path, length, (x, y), S, segment=-1 if new_path else seg, search_range=2)
        seg = want["segment"]; segs.append(seg)
        l = got_ticks[t]
        assert int(l[2]) == seg and float(l[3]) == want["s"] and int(l[4]) == int(want["reached"]) and int(l[5]) == S, (t, l)
        for k in (0, N - 1):
            assert np.array_equal(rows[(t, k)][spl], want["window"].ravel()), (t, k)
            assert rows[(t, k)][pm.index("contour")] == W["contour"]
    assert segs == [0, 1, 3, 10]
    assert [l for l in lines if l[0] == "reset"][0][1] == "10"          # reset(): the global search again
    # the batched device twin (reference_path_batch.h) in the same program: two scenes (12 segments; 3 < S), six entries of which one names no
    # scene, a global then a local tick -- parameter rows, state, bound windows, segments and closest_s equal the host's, bit for bit
    batch = [l for l in lines if l[0] == "batch"][0]
    assert batch[1:] == ["differ", "0", "written", str(5 * N * 9 * S), "state_differ", "0", "bound_differ", "0", "segment_differ", "0"], batch
    assert [l[3:] for l in lines if l[0] == "batch_tick"] == [["4", "2"], ["4", "2"]]
