"""GPU: the column mode of the C++ batched obstacle twin (mpc_planner/data_preparation_batch.h, BatchedObstaclePreparation::setColumns ->
include/tmpc_hip_stack.h).  tests/cpp/test_stack_columns.cpp is linked twice: against libtmpc_hip.so, where it runs prepare() ->
setParameters() -> linearizeTopology() through tmpc_hip.h, and against the generated libtmpc_hip_tmpc_cfg2.so (its parameter map is the
hand-written cfg 2 map), where the same calls go through the tmpc_stack_* entries with the columns read from the stack's map.  The parameter
rows the two programs leave are equal bit for bit, and equal to the numpy mirrors in the collision columns."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
GEN = os.path.join(ROOT, "build", "generated_stack_columns")
N, M, S, Q, R, B = 20, 8, 5, 3, 10, 7
DT = 0.2


def _build(name, libdir, lib):
    from mpc_planner_amd.generate_solver import generate_solver
    out = os.path.join(ROOT, "build", name)
    src = os.path.join(ROOT, "tests", "cpp", "test_stack_columns.cpp")
    deps = [src, os.path.join(libdir, f"lib{lib}.so"), os.path.join(ROOT, "mpc_planner_amd", "cpp", "include", "mpc_planner", "data_preparation_batch.h")]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    generate_solver(GEN, N=N, max_obstacles=M, num_segments=S, guidance=True)
    cpp = os.path.join(ROOT, "mpc_planner_amd", "cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(cpp, "include"), "-I", os.path.join(GEN, "include"),
                           "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include", src, os.path.join(cpp, "src", "solver_interface.cpp"),
                           os.path.join(GEN, "src", "mpc_planner_parameters.cpp"), "-L", libdir, "-l" + lib, "-Wl,-rpath," + libdir,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-o", out])
    return out


def test_cpp_twin_in_column_mode_on_the_generated_library_equals_the_layout_mode():
    from mpc_planner_amd import modules as md, scenes
    from mpc_planner_amd.stack_writers import obstacle_columns, topology_columns
    from test_gpu_parity import _generated_lib
    path, meta = _generated_lib("tmpc_cfg2")
    pmap = meta["parameter_map"]
    ocols, tcols = obstacle_columns(pmap, M, 0), topology_columns(pmap, M)
    layout_bin = _build("test_stack_columns_layout", os.path.join(ROOT, "mpc_planner_amd"), "tmpc_hip")
    columns_bin = _build("test_stack_columns_generated", os.path.dirname(path), "tmpc_hip_tmpc_cfg2")
    rng = np.random.default_rng(77)
    counts = [R, 5, M]                                                       # more than M (selection), fewer (dummies), exactly M
    state = np.stack([np.array([0.4 * q, -0.3 * q, 0.2 * q - 0.1, rng.uniform(0.5, 2.0)]) for q in range(Q)])
    pos = state[:, None, :2] + np.stack([rng.uniform(1.0, 9.0, (Q, R)), rng.uniform(-3.0, 3.0, (Q, R))], 2)
    speed, heading = rng.uniform(0.3, 1.4, (Q, R)), rng.uniform(-np.pi, np.pi, (Q, R))
    vel = np.stack([speed * np.cos(heading), speed * np.sin(heading)], 2)
    radius = rng.uniform(0.3, 0.6, (Q, R))
    scene_of = np.arange(B) % Q
    is_original = np.zeros(B); is_original[B - 1] = 1
    x0 = rng.normal(size=(B, N + 1, 7))
    for b in range(B):
        x0[b, :, 2] = state[scene_of[b], 0] + np.linspace(0.0, 6.0, N + 1)
        x0[b, :, 3] = state[scene_of[b], 1] + rng.normal(0.0, 1.5, N + 1)
    x0[0, 3, 2:4] = pos[0, 0] + vel[0, 0] * DT * 2 + np.array([0.1, -0.05])  # inside obstacle 0's disc at stage 3, if the selection keeps it first
    vals = [Q, R, B, len(ocols), len(tcols)] + ocols + tcols
    for q in range(Q):
        vals += list(state[q]) + [counts[q]]
        for i in range(R):
            vals += list(pos[q, i]) + list(vel[q, i]) + [radius[q, i]]
    vals += list(scene_of) + list(is_original) + list(x0.ravel())
    tmp = os.path.join(ROOT, "build", "stack_columns_case")
    os.makedirs(tmp, exist_ok=True)
    np.array(vals, float).tofile(os.path.join(tmp, "in.bin"))
    rows = {}
    for mode, binary in (("layout", layout_bin), ("columns", columns_bin)):
        out = subprocess.run([binary, os.path.join(GEN, "config"), os.path.join(tmp, "in.bin"), os.path.join(tmp, mode + ".bin"), mode],
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        print(out.stdout.strip())
        rows[mode] = np.fromfile(os.path.join(tmp, mode + ".bin")).reshape(B, N, 135)
    assert np.array_equal(rows["columns"], rows["layout"])
    named = ocols + tcols
    rest = np.setdiff1d(np.arange(135), named)
    assert (rows["columns"][:, :, rest] == -7.0).all() and not (rows["columns"][:, :, named] == -7.0).any()
    # the collision columns against the mirror where no ranking takes place (scenes 1 and 2: at most M raw obstacles)
    pm = scenes.make_scene(0, N=N, M=M, B=1)["pm"]
    assert dict(pm._params) == pmap
    for b in range(B):
        q = scene_of[b]
        if counts[q] > M:
            continue
        obs = md.prepare_obstacles(state[q], pos[q, :counts[q]], radius[q, :counts[q]], M, N, DT, raw_vel=vel[q, :counts[q]], probabilistic=True,
                                   propagate_passes=2, risk=0.05)
        # chi as the C++ twin evaluates it on the host, ExponentialQuantile(0.5, 1 - risk) = -log(1 - (1 - risk)) / 0.5 (modules_hip.h) with libm's
        # log: one bit from the mirror's -log(risk) / 0.5, because 1 - 0.95 is not 0.05
        obs["chi"] = np.where(obs["gaussian"], -math.log(1.0 - (1.0 - 0.05)) / 0.5, 1.0)
        want = np.full((N, 135), -7.0)
        md.ellipsoid_set_parameters(pm, want, state[q, :2], obs, scenes.ROBOT_RADIUS, disc_offset=0.03)
        assert np.array_equal(rows["columns"][b][:, ocols], want[:, ocols]), b
    assert np.array_equal(rows["columns"][B - 1][:, tcols], np.tile([1.0, 0.0, state[scene_of[B - 1], 0] + 100.0], (N, M)))
