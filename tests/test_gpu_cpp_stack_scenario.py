"""GPU: the C++ batched scenario rows (mpc_planner_modules/scenario_rows_batch.h BatchedScenarioRows) in both modes.
tests/cpp/test_stack_scenario.cpp is linked twice: against libtmpc_hip.so, where update() and support() go through tmpc_hip.h
(tmpc_scenario_halfspaces, tmpc_scenario_support), and against the generated libtmpc_hip_safe_horizon.so, where after setColumns() the same
calls go through include/tmpc_hip_stack_scenario.h with the columns read from the stack's map.  One tick of tests/stack_scenario_cases.py's
2 scenes x 2 solvers: sample -> discard -> halfspaces, a solve, support and empty stages.  Each program compares its rows and counts with the
file this test writes from the numpy mirrors (the counts: the mirror's support on the same library's solution of the mirror-built batch) and
writes them out; the two programs' rows are equal bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import stack_scenario_cases as cases  # noqa: E402

NPAR = 127


def _build(name, libdir, lib):
    out = os.path.join(ROOT, "build", name)
    src = os.path.join(ROOT, "tests", "cpp", "test_stack_scenario.cpp")
    cpp = os.path.join(ROOT, "mpc_planner_amd", "cpp", "include")
    deps = [src, os.path.join(libdir, f"lib{lib}.so"), os.path.join(cpp, "mpc_planner_modules", "scenario_rows_batch.h"),
            os.path.join(cpp, "mpc_planner_solver", "device_plumbing.h"), os.path.join(ROOT, "include", "tmpc_hip_stack_scenario.h")]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", cpp, "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include", src,
                           "-L", libdir, "-l" + lib, "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-o", out])
    return out


def test_cpp_scenario_rows_in_both_modes_equal_the_mirrors():
    from mpc_planner_amd import solver
    from mpc_planner_amd.stack_scenario import scenario_columns
    from test_gpu_parity import _generated_lib
    path, meta = _generated_lib("safe_horizon")
    pmap = meta["parameter_map"]
    pb = cases.loop_problem()
    assert meta["npar"] == NPAR and pmap == dict(pb["pm"]._params)
    cols = scenario_columns(pmap, cases.R)
    layout_bin = _build("test_stack_scenario_layout", os.path.join(ROOT, "mpc_planner_amd"), "tmpc_hip")
    columns_bin = _build("test_stack_scenario_generated", os.path.dirname(path), "tmpc_hip_safe_horizon")
    B, N, seed, off = cases.B, cases.N, 4242, 0.03
    pred = cases.prediction(pb, 0)
    start = pb["params"].copy(); start[:, :, cols] = -7.0
    rows, which, _, empty = cases.host_rows(cases.Map(pmap), pb["params"], pb["xinit"], pb["x0"], pred, pb["prob"], seed, disc_offset=off)
    assert not (rows[:, :, cols] == -7.0).any()
    vals = [B, cases.M, cases.MODES, cases.S_CEN, cases.N_DISCARD, N, cases.R, B, NPAR, seed, cases.RADIUS, off, cases.TOL] + cols
    vals += list(pred.ravel()) + list(pb["prob"].ravel()) + list(pb["xinit"][:, 0]) + list(pb["scene_of"]) + list(pb["xinit"].ravel())
    vals += list(pb["x0"].ravel()) + list(start.ravel())
    tmp = os.path.join(ROOT, "build", "stack_scenario_case")
    os.makedirs(tmp, exist_ok=True)
    np.array(vals, float).tofile(os.path.join(tmp, "in.bin"))
    out = {}
    for mode, binary, lib_path, dims in (("layout", layout_bin, None, solver.default_dims(**cases.CFG5_DIMS)),
                                         ("columns", columns_bin, path, solver.default_dims(N=N, lib_path=path))):
        # the counts this library's solve of the mirror-built batch gives on the mirrors
        s = solver.BatchedSolver(dims, B_max=B, lib_path=lib_path)
        s.set_batch(pb["xinit"], pb["x0"], rows); s.solve(); sol = s.get()
        s.close()
        sup, act = cases.host_support(cases.Map(pmap), sol["xtraj"], rows, which)
        np.concatenate([rows.ravel(), sup, act, empty]).astype(float).tofile(os.path.join(tmp, f"expect_{mode}.bin"))
        run = subprocess.run([binary, os.path.join(tmp, "in.bin"), os.path.join(tmp, f"expect_{mode}.bin"), os.path.join(tmp, mode + ".bin"), mode],
                             capture_output=True, text=True, timeout=120)
        print(run.stdout.strip())
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
        flat = np.fromfile(os.path.join(tmp, mode + ".bin"))
        assert len(flat) == B * N * NPAR + 3 * B
        out[mode] = dict(rows=flat[:B * N * NPAR].reshape(B, N, NPAR), counts=flat[B * N * NPAR:].reshape(3, B).astype(np.int32))
        assert np.array_equal(out[mode]["rows"], rows)
        assert np.array_equal(out[mode]["counts"], np.stack([sup, act, empty]))
        assert (sol["exit_code"] == 1).any() and sup.sum() > 0
    assert np.array_equal(out["columns"]["rows"], out["layout"]["rows"])
    rest = np.setdiff1d(np.arange(NPAR), cols)
    assert np.array_equal(out["columns"]["rows"][:, :, rest], start[:, :, rest])
