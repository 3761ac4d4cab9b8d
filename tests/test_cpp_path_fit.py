"""C++ path fit: the Solver-free header mpc_planner_modules/reference_path.h (fit / fitBounds / fitCubic; g++ only, CPU) on the launches of the
bitwise device test (tests/path_fit_cases.py) against the numpy mirror (mpc_planner_amd/modules.py fit_path) -- counts equal, values bitwise
(%.17g round-trips a double) --, Contouring::onDataReceived with waypoints (modules_hip.h, RealTimeData::reference_path_points) followed by
update against fit followed by window, and on the GPU the batched twin's setWaypoints (mpc_planner_modules/reference_path_batch.h, one
tmpc_fit_path launch) against setPaths with host-fitted cubics."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "mpc_planner_amd", "cpp")
SRC = os.path.join(ROOT, "tests", "cpp", "test_path_fit.cpp")
BIN = os.path.join(ROOT, "build", "test_path_fit")
GEN = os.path.join(ROOT, "build", "generated_path_fit")
BIN_SOLVER = os.path.join(ROOT, "build", "test_path_fit_solver")
N, M, S = 20, 8, 5


def _build_header_only():
    """No generated header, no HIP, no library: the header stands alone."""
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    headers = [os.path.join(CPP, "include", "mpc_planner_modules", "reference_path.h"), os.path.join(CPP, "include", "mpc_planner_types", "prep_arithmetic.h")]
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(f) for f in [SRC] + headers):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(CPP, "include"), SRC, "-o", BIN])


@pytest.mark.parametrize("given_s, extras, which", [(False, True, "bitwise"), (True, False, "bitwise"), (True, True, "small")])
def test_header_equals_the_mirror_bitwise(tmp_path, given_s, extras, which):
    import path_fit_cases as pf
    _build_header_only()
    case = pf.bitwise_launch() if which == "bitwise" else pf.small_launch()
    Q, P = len(case["count"]), case["n_pts_max"]
    want = pf.mirror(case, P - 1, given_s, extras)
    vals = [Q, P, int(given_s), int(extras)]
    for q in range(Q):
        vals += [case["count"][q]] + list(case["xy"][q].ravel()) + list(case["s"][q]) + list(case["left"][q].ravel()) + list(case["right"][q].ravel()) + list(case["v"][q])
    f = str(tmp_path / "scenes.bin")
    np.array(vals, float).tofile(f)
    out = subprocess.run([BIN, f], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l.split() for l in out.stdout.splitlines()]
    head = {int(l[1]): l for l in lines if l[0] == "scene"}
    assert sorted(head) == list(range(Q))
    rows = {tag: {} for tag in "plrv"}
    for l in lines:
        if l[0] in rows:
            rows[l[0]].setdefault(int(l[1]), []).append([float(v) for v in l[3:]])
    for q in range(Q):
        assert int(head[q][2]) == want["status"][q] and int(head[q][3]) == want["count"][q], (q, head[q])
        m = int(want["count"][q])
        if want["status"][q]:
            assert all(q not in rows[tag] for tag in "plrv")
            continue
        assert float(head[q][4]) == want["length"][q]
        assert np.array_equal(np.array(rows["p"][q]), want["path"][q, :m]), q
        if extras:
            assert float(head[q][5]) == want["road_width"][q]
            assert np.array_equal(np.array(rows["l"][q]), want["bounds"][q, 0, :m]) and np.array_equal(np.array(rows["r"][q]), want["bounds"][q, 1, :m]), q
            assert np.array_equal(np.array(rows["v"][q]), want["velocity"][q, :m]), q
        else:
            assert all(q not in rows[tag] for tag in "lrv")
    assert want["status"].tolist() == [1 if (min(c, P) < 2 or q == case["duplicate"]) else 0 for q, c in enumerate(case["count"])]


def _build_solver():
    import __graft_entry__ as g
    g.build()
    from mpc_planner_amd.generate_solver import generate_solver
    generate_solver(GEN, N=N, max_obstacles=M, num_segments=S, guidance=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-DWITH_SOLVER", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(CPP, "include"),
                           "-I", os.path.join(GEN, "include"), "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include", SRC, os.path.join(CPP, "src", "solver_interface.cpp"),
                           os.path.join(GEN, "src", "mpc_planner_parameters.cpp"), "-L", os.path.join(ROOT, "mpc_planner_amd"), "-ltmpc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "mpc_planner_amd"), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-o", BIN_SOLVER])


def _scene_file(tmp_path):
    import path_fit_cases as pf
    xy = pf.waypoints(np.random.default_rng(21), 14)
    left, right = xy + [0.3, 2.0], xy - [0.2, 1.5]
    left[0], right[0] = xy[0] + [1.5, 2.0], xy[0] - [1.5, 2.0]           # road width |(3, 4)| = 5
    pos = xy[6] + [0.2, -0.3]
    f = str(tmp_path / "scene.bin")
    np.array([S, pos[0], pos[1], len(xy)] + list(xy.ravel()) + list(left.ravel()) + list(right.ravel()), float).tofile(f)
    return f, xy, left, right, pos


def test_cpp_contouring_fits_waypoints_on_data_received(tmp_path):
    """Contouring::onDataReceived with waypoints followed by update gives the window of fit followed by window, segment and state["spline"]
    included; with road constraints on, the bound cubics are fitBounds' and road/width is 5; without waypoints data is left untouched.  CPU: no
    Solver object is made.  The mirror's own answer pins the segment."""
    from mpc_planner_amd import modules as md
    _build_solver()
    f, xy, left, right, pos = _scene_file(tmp_path)
    out = subprocess.run([BIN_SOLVER, "contouring", os.path.join(GEN, "config"), f], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = {l.split()[0]: l.split() for l in out.stdout.splitlines()}
    fit = md.fit_path(xy)
    seg, _ = md.find_closest_point(fit["path"], fit["length"], pos)
    assert lines["contouring"][1:] == ["differ", "0", "path_differ", "0", "segment", str(seg), str(seg), "spline_same", "1", "length_same", "1", "bounds", "0", "0",
                                       "width_same", "1"], lines["contouring"]
    assert lines["bounds"][1:7] == ["differ", "0", "0", "width_same", "1", "width"] and float(lines["bounds"][7]) == 5.0, lines["bounds"]
    assert lines["untouched"] == ["untouched", "1"]


@pytest.mark.gpu
def test_cpp_batched_twin_set_waypoints_equals_set_paths(tmp_path):
    """BatchedPathTracking::setWaypoints (one upload, one tmpc_fit_path launch into the twin's own buffers) followed by two ticks equals setPaths
    with host-fitted cubics followed by the same ticks, bitwise: windows, bound windows, segments, closest_s; and the fitted cubics, counts,
    lengths, status and road widths on the device equal ReferencePathSpline::fit / fitBounds on the host.  Three scenes: 13 segments, 3 (fewer
    than S), and a repeated waypoint (count 0: both twins leave it alone)."""
    if not os.path.exists(BIN_SOLVER) or os.path.getmtime(BIN_SOLVER) < os.path.getmtime(os.path.join(ROOT, "mpc_planner_amd", "libtmpc_hip.so")):
        _build_solver()
    f, xy, *_ = _scene_file(tmp_path)
    out = subprocess.run([BIN_SOLVER, "batch", os.path.join(GEN, "config"), f], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    batch = [l.split() for l in out.stdout.splitlines() if l.startswith("batch")][0]
    assert batch[1:10] == ["differ", "0", "segment_differ", "0", "fit_differ", "0", "counts", "13", "3"] and batch[10] == "0", batch
    assert batch[11] == "segments" and batch[12] in ("5", "6") and batch[13] in ("1", "2") and batch[14] == "-1", batch
