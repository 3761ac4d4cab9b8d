"""C++ free space: the Solver-free headers mpc_planner_modules/free_space.h and mpc_planner_types/costmap.h (g++ only, CPU) as a stand-alone
program on the launches of the bitwise device test (tests/free_space_cases.py) against the numpy mirror (mpc_planner_amd/modules.py
costmap_points, decomp_halfspaces) -- counts and statuses equal, values bitwise (%.17g round-trips a double); once more under
-fsanitize=address,undefined."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "mpc_planner_amd", "cpp")
SRC = os.path.join(ROOT, "tests", "cpp", "test_free_space.cpp")
BIN = os.path.join(ROOT, "build", "test_free_space")
BIN_SAN = os.path.join(ROOT, "build", "test_free_space_san")


def _build(sanitize=False):
    """No generated header, no HIP, no library: the headers stand alone."""
    out = BIN_SAN if sanitize else BIN
    os.makedirs(os.path.dirname(out), exist_ok=True)
    inc = os.path.join(CPP, "include")
    headers = [os.path.join(inc, "mpc_planner_modules", f) for f in ("free_space.h", "reference_path.h")] + \
              [os.path.join(inc, "mpc_planner_types", f) for f in ("prep_arithmetic.h", "costmap.h", "path_segment.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in [SRC] + headers):
        extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", *extra, "-I", inc, SRC, "-o", out])
    return out


def _run_decomp(tmp_path, binary, case, want):
    keep = [q for q in range(len(case["count"])) if case["main_of"][q] >= 0 and case["path_count"][q] > 0]      # the header has no scenes to skip
    Nn, n_rows = case["N"], case["n_rows"]
    vals = [len(keep), Nn, case["n_pts_max"], n_rows, case["n_seg_max"], case["range"], case["dt"]]
    for q in keep:
        vals += [case["path_count"][q]] + list(case["path"][q].ravel()) + [case["path_length"][q], case["s0"][q], case["state_x"][q]] \
            + list(case["v"][q, :Nn]) + [case["count"][q]] + list(case["points"][q].ravel())
    f = str(tmp_path / "launch.bin")
    np.array(vals, float).tofile(f)
    out = subprocess.run([binary, "decomp", f], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rows = np.full((len(keep), Nn, n_rows, 3), np.nan); count = np.full((len(keep), Nn), -1); status = np.full((len(keep), Nn), -1)
    for l in out.stdout.splitlines():
        w = l.split()
        if w[0] == "stage":
            count[int(w[1]), int(w[2])] = int(w[3]); status[int(w[1]), int(w[2])] = int(w[4])
        elif w[0] == "row":
            rows[int(w[1]), int(w[2]), int(w[3])] = [float(v) for v in w[4:]]
    assert np.array_equal(count, want["count"][keep]) and np.array_equal(status, want["status"][keep])
    assert np.array_equal(rows, want["rows"][keep])
    return len(keep)


@pytest.mark.parametrize("sanitize", [False, True])
def test_header_equals_the_mirror_bitwise(tmp_path, sanitize):
    import free_space_cases as fs
    binary = _build(sanitize)
    assert _run_decomp(tmp_path, binary, fs.bitwise_launch(), fs.bitwise_mirror()) == 12
    assert _run_decomp(tmp_path, binary, fs.scattered_launch(8), fs.scattered_mirror(8)) == 8


@pytest.mark.parametrize("max_points", [0, 100])
def test_costmap_header_equals_the_mirror(tmp_path, max_points):
    from mpc_planner_amd import modules as md
    binary = _build()
    rng = np.random.default_rng(3)
    cost = np.where(rng.uniform(size=(37, 53)) < 0.2, rng.integers(1, 256, (37, 53)), 0).astype(np.uint8)
    origin, res = (-3.25, 7.5), 0.05
    f = str(tmp_path / "map.bin")
    np.array([53, 37, origin[0], origin[1], res, max_points] + list(cost.ravel()), float).tofile(f)
    out = subprocess.run([binary, "costmap", f], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l.split() for l in out.stdout.splitlines()]
    want, count, overflow = md.costmap_points(cost, origin, res, max_points or None)
    assert lines[0] == ["points", str(count), str(int(overflow))]
    assert np.array_equal(np.array([[float(v) for v in l[1:]] for l in lines[1:]]).reshape(-1, 2), want)
    assert overflow == bool(max_points)


GEN = os.path.join(ROOT, "build", "generated_free_space")
BIN_SOLVER = os.path.join(ROOT, "build", "test_free_space_solver")
N, M, S = 20, 8, 5


def _build_solver():
    import __graft_entry__ as g
    g.build()
    from mpc_planner_amd.generate_solver import generate_solver
    generate_solver(GEN, N=N, max_obstacles=M, num_segments=S, guidance=True, slack=True, n_decomp=12)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-DWITH_SOLVER", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(CPP, "include"),
                           "-I", os.path.join(GEN, "include"), "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include", SRC, os.path.join(CPP, "src", "solver_interface.cpp"),
                           os.path.join(GEN, "src", "mpc_planner_parameters.cpp"), "-L", os.path.join(ROOT, "mpc_planner_amd"), "-ltmpc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "mpc_planner_amd"), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-o", BIN_SOLVER])


def _scene_file(tmp_path):
    """A corridor scene (scenes.with_costmap) on the fitted path of its own reference cubics; two sets of speeds for the two ticks."""
    import free_space_cases as fs
    from mpc_planner_amd import modules as md
    sc = fs.corridor_scene(5)
    seg = sc["segments"]
    xy = np.array([md._road_segment_eval(seg[:, :8], seg[:, 8], float(v))[:2] for v in np.linspace(-3.0, 30.0, 25)])
    fit = md.fit_path(xy)
    v = np.stack([sc["x0"][0, :N, md.IDX["v"]], np.random.default_rng(4).uniform(0.5, 2.5, N)])
    cm = sc["costmap"]
    vals = [12, fs.RANGE, fit["count"]] + list(fit["path"].ravel()) + [fit["length"], 0.0, 0.0, 3.0] + list(v.ravel()) + [0.125, cm.shape[1], cm.shape[0]] \
        + list(sc["costmap_origin"]) + [sc["costmap_resolution"]] + list(cm.ravel())
    f = str(tmp_path / "scene.bin")
    np.array(vals, float).tofile(f)
    return f, sc, fit, v


def test_cpp_decomp_constraints_equal_the_mirror(tmp_path):
    """DecompConstraints::isDataReady, update and setParameters (modules_hip.h) on one corridor scene: "Costmap " is reported missing without a
    costmap; the decomp columns and ego_disc_0_offset the generated setters wrote equal the mirror's rows bitwise, counts and statuses too.  CPU."""
    import free_space_cases as fs
    from mpc_planner_amd import modules as md
    _build_solver()
    assert "#define SOLVER_NDECOMP 12" in open(os.path.join(GEN, "include", "mpc_planner_solver", "hip_solver_dims.h")).read()
    f, sc, fit, v = _scene_file(tmp_path)
    out = subprocess.run([BIN_SOLVER, "module", os.path.join(GEN, "config"), f], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l.split() for l in out.stdout.splitlines()]
    assert out.stdout.splitlines()[0] == "ready 0 [Costmap ] 1 []"
    pts, count, _ = md.costmap_points(sc["costmap"], sc["costmap_origin"], sc["costmap_resolution"])
    assert lines[1] == ["points", str(count), "exceeded", "0"]
    want = md.decomp_halfspaces(fit["path"], fit["length"], 3.0, v[0], fs.DT, pts, fs.RANGE, 12, 0.0)
    stages = [l for l in lines if l[0] == "stage"]
    assert [int(l[2]) for l in stages] == want["count"].tolist() and [int(l[3]) for l in stages] == want["status"].tolist()
    assert all(float(l[4]) == 0.125 for l in stages) and len(stages) == N
    rows = np.array([[float(x) for x in l[3:]] for l in lines if l[0] == "row"]).reshape(N, 12, 3)
    assert np.array_equal(rows, want["rows"]) and want["count"][1:].min() >= 4 and want["count"].max() > 6


@pytest.mark.gpu
def test_cpp_batched_twin_equals_the_host_header(tmp_path):
    """BatchedFreeSpace (mpc_planner_modules/free_space_batch.h): costmaps uploaded once, then two ticks of tmpc_decomp_halfspaces +
    tmpc_set_halfspace_rows -- the points extracted in the first only -- against FreeSpace::occupiedCells / decomposePath on the host, bitwise:
    rows, counts, statuses, point counts, and the parameters read back (every other column keeps its prefill)."""
    if not os.path.exists(BIN_SOLVER) or os.path.getmtime(BIN_SOLVER) < os.path.getmtime(os.path.join(ROOT, "mpc_planner_amd", "libtmpc_hip.so")):
        _build_solver()
    f, sc, *_ = _scene_file(tmp_path)
    out = subprocess.run([BIN_SOLVER, "batch", os.path.join(GEN, "config"), f], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    batch = [l.split() for l in out.stdout.splitlines() if l.startswith("batch")][0]
    n = int((sc["costmap"] != 0).sum())
    assert batch[1:] == ["differ", "0", "params_differ", "0", "points", str(n), str(n)], batch
