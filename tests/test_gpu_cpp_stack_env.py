"""GPU: the column mode of the C++ batched path and free-space twins (mpc_planner_modules/reference_path_batch.h BatchedPathTracking::setColumns
and roadHalfspaces, mpc_planner_modules/free_space_batch.h BatchedFreeSpace::setColumns -> include/tmpc_hip_stack_env.h).
tests/cpp/test_stack_env.cpp is linked twice: against libtmpc_hip.so, where it runs setPaths() -> track() -> setParameters() -> roadHalfspaces()
(centreline, bounds) -> setCostmaps() -> update() -> setParameters() through tmpc_hip.h, and against the generated libtmpc_hip_road_decomp.so
(its parameter map is the hand-written one of that shape: N = 20, 3 segments, 4 topology rows, 2 ellipsoids, 4 decomp rows, slack model), where
the same calls go through the tmpc_stack_* entries with the columns read from the stack's map.  The parameter rows, the road buffers and the
state the two programs leave are equal bit for bit, and equal to the numpy mirrors."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
GEN = os.path.join(ROOT, "build", "generated_stack_env")
N, M, S, N_ROWS, Q, B, NPAR = 20, 2, 3, 4, 2, 5, 76
DT = 0.2


def _build(name, libdir, lib):
    from mpc_planner_amd.generate_solver import generate_solver
    out = os.path.join(ROOT, "build", name)
    src = os.path.join(ROOT, "tests", "cpp", "test_stack_env.cpp")
    inc = os.path.join(ROOT, "mpc_planner_amd", "cpp", "include", "mpc_planner_modules")
    deps = [src, os.path.join(libdir, f"lib{lib}.so"), os.path.join(inc, "reference_path_batch.h"), os.path.join(inc, "free_space_batch.h")]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    generate_solver(GEN, N=N, max_obstacles=M, num_segments=S, guidance=True, slack=True, n_decomp=N_ROWS, add_halfspaces=2)
    cpp = os.path.join(ROOT, "mpc_planner_amd", "cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(cpp, "include"), "-I", os.path.join(GEN, "include"),
                           "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include", src, os.path.join(cpp, "src", "solver_interface.cpp"),
                           os.path.join(GEN, "src", "mpc_planner_parameters.cpp"), "-L", libdir, "-l" + lib, "-Wl,-rpath," + libdir,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-o", out])
    return out


def test_cpp_twins_in_column_mode_on_the_generated_library_equal_the_layout_mode():
    import free_space_cases as fs
    from mpc_planner_amd import modules as md, scenes
    from mpc_planner_amd.stack_env import decomp_columns, path_columns
    from test_gpu_parity import _generated_lib
    path, meta = _generated_lib("road_decomp")
    pmap = meta["parameter_map"]
    assert meta["npar"] == NPAR
    pcols, dcols = path_columns(pmap, S), decomp_columns(pmap, N_ROWS)
    layout_bin = _build("test_stack_env_layout", os.path.join(ROOT, "mpc_planner_amd"), "tmpc_hip")
    columns_bin = _build("test_stack_env_generated", os.path.dirname(path), "tmpc_hip_road_decomp")
    rng = np.random.default_rng(78)
    fit = fs.fitted_path()
    n_seg = fit["count"]
    left, right = fit["path"][:, :8].copy(), fit["path"][:, :8].copy()
    left[:, 7] += 2.0; right[:, 7] -= 1.5
    way = fs.waypoints()
    pos = np.stack([way[2] + [0.1, -0.2], way[4] + [-0.15, 0.25]])
    sc = fs.corridor_scene(5)
    cost = sc["costmap"]
    size_y, size_x = cost.shape
    resolution = sc["costmap_resolution"]
    origin = np.stack([pos[q] - [2.0, size_y * resolution / 2.0] for q in range(Q)])
    decomp_range, disc_offset, r = 1.0, 0.04, scenes.ROBOT_RADIUS
    offsets = md.road_offsets(4.0, r)
    scene_of, main_of = np.array([0, 1, 0, 9, 1]), np.array([2, 1])
    tracked = [md.track_path(fit["path"], fit["length"], pos[q], S, segment=-1, left=left, right=right) for q in range(Q)]
    x0 = rng.normal(size=(B, N + 1, 8))
    for b in range(B):
        q = scene_of[b] % Q
        x0[b, :, md.IDX["v"]] = rng.uniform(0.5, 2.5, N + 1)
        x0[b, :, md.IDX["spline"]] = tracked[q]["s"] - 0.3 + 0.25 * np.arange(N + 1) + 0.02 * b
    vals = [Q, B, n_seg, len(pcols), len(dcols), size_x, size_y, resolution, decomp_range, disc_offset, offsets[0], offsets[1]] + pcols + dcols
    for i in range(n_seg):
        vals += list(fit["path"][i]) + list(left[i]) + list(right[i])
    vals.append(fit["length"])
    for q in range(Q):
        vals += list(pos[q]) + list(origin[q])
    vals += list(cost.ravel().astype(float)) + list(scene_of) + list(main_of) + list(x0.ravel())
    tmp = os.path.join(ROOT, "build", "stack_env_case")
    os.makedirs(tmp, exist_ok=True)
    np.array(vals, float).tofile(os.path.join(tmp, "in.bin"))
    out = {}
    n_road = Q * N * 3 * 3
    for mode, binary in (("layout", layout_bin), ("columns", columns_bin)):
        run = subprocess.run([binary, os.path.join(GEN, "config"), os.path.join(tmp, "in.bin"), os.path.join(tmp, mode + ".bin"), mode],
                             capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        print(run.stdout.strip())
        flat = np.fromfile(os.path.join(tmp, mode + ".bin"))
        assert len(flat) == B * N * NPAR + 2 * n_road + B * 6
        out[mode] = dict(rows=flat[:B * N * NPAR].reshape(B, N, NPAR), centre=flat[B * N * NPAR:][:n_road].reshape(Q, N, 3, 3),
                         bounds=flat[B * N * NPAR + n_road:][:n_road].reshape(Q, N, 3, 3), state=flat[-B * 6:].reshape(B, 6))
    lay, col = out["layout"], out["columns"]
    for key in lay:
        assert np.array_equal(col[key], lay[key]), key
    named = pcols + dcols
    rest = np.setdiff1d(np.arange(NPAR), named)
    valid = [b for b in range(B) if 0 <= scene_of[b] < Q]
    assert (col["rows"][:, :, rest] == -7.0).all() and not (col["rows"][valid][:, :, named] == -7.0).any() and (col["rows"][3] == -7.0).all()
    # against the mirrors
    for q in range(Q):
        pts, _, overflow = md.costmap_points(cost, origin[q], resolution, 4096)
        assert not overflow
        dc = md.decomp_halfspaces(fit["path"], fit["length"], tracked[q]["s"], x0[main_of[q], :N, md.IDX["v"]], DT, pts, decomp_range, N_ROWS, pos[q, 0])
        assert (dc["count"][1:] > 0).all()
        s_of_k = x0[main_of[q], :N, md.IDX["spline"]]
        centre = md.road_halfspaces(tracked[q]["window"], s_of_k, *offsets)
        bounds = md.road_halfspaces_from_bounds(tracked[q]["window"], tracked[q]["left"], tracked[q]["right"], s_of_k, 0.325)
        assert np.array_equal(col["centre"][q, 1:, 1:3], centre[1:]) and (col["centre"][q, :, 0] == -5.0).all() and (col["centre"][q, 0] == -5.0).all()
        assert np.array_equal(col["bounds"][q, 1:, 0:2], bounds[1:]) and (col["bounds"][q, :, 2] == -5.0).all()
        for b in valid:
            if scene_of[b] != q:
                continue
            assert np.array_equal(col["rows"][b][:, pcols], np.tile(tracked[q]["window"].reshape(-1), (N, 1)))
            assert np.array_equal(col["rows"][b][:, dcols[1:]], dc["rows"].reshape(N, 3 * N_ROWS)) and (col["rows"][b][:, dcols[0]] == disc_offset).all()
            assert col["state"][b, 4] == tracked[q]["s"] and (np.delete(col["state"][b], 4) == -9.0).all()
    assert (col["state"][3] == -9.0).all()
