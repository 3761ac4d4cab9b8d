"""C++ obstacle preparation: mpc_planner/data_preparation.h (the reference's six functions on the Eigen-free types, reading ModuleConfig) against
the numpy mirror (mpc_planner_amd/modules.py prepare_obstacles) on a 12-obstacle list written to a file -- selection indices equal, values
bitwise (%.17g round-trips a double) --, and the batched device twin (mpc_planner/data_preparation_batch.h: one upload, tmpc_prepare_obstacles,
tmpc_set_obstacle_parameters) against the host path through the parameter rows.  Built like tests/test_cpp_road.py builds its binary."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "build", "generated_prep")
BIN = os.path.join(ROOT, "build", "test_data_preparation")
N, M, S = 20, 8, 5
DT = 0.2


def _build():
    import __graft_entry__ as g
    g.build()
    from mpc_planner_amd.generate_solver import generate_solver
    generate_solver(GEN, N=N, max_obstacles=M, num_segments=S, guidance=True)
    cpp = os.path.join(ROOT, "mpc_planner_amd", "cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(cpp, "include"), "-I", os.path.join(GEN, "include"),
                           "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "test_data_preparation.cpp"),
                           os.path.join(cpp, "src", "solver_interface.cpp"), os.path.join(GEN, "src", "mpc_planner_parameters.cpp"),
                           "-L", os.path.join(ROOT, "mpc_planner_amd"), "-ltmpc_hip", "-Wl,-rpath," + os.path.join(ROOT, "mpc_planner_amd"),
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-o", BIN])


def _raw(n=12):
    rng = np.random.Generator(np.random.PCG64(4300))
    pos = np.stack([rng.uniform(1.0, 15.0, n), rng.uniform(-5.0, 5.0, n)], 1)
    speed = rng.uniform(0.3, 1.6, n); heading = rng.uniform(-np.pi, np.pi, n)
    vel = np.stack([speed * np.cos(heading), speed * np.sin(heading)], 1)
    radius = rng.uniform(0.3, 0.6, n)
    state = np.array([0.4, -0.3, 0.25, 1.3])
    k = np.arange(N, dtype=float)
    pred = np.zeros((n, N, 5))
    pred[:, :, 0:2] = pos[:, None, :] + (vel[:, None, :] * DT) * k[None, :, None]
    pred[:, :, 1] += 0.04 * np.sin(0.6 * k)[None, :]
    pred[:, :, 2] = heading[:, None]
    pred[:, :, 3] = rng.uniform(0.05, 0.3, n)[:, None] * (1.0 + 0.1 * k[None, :]); pred[:, :, 4] = 0.5 * pred[:, :, 3]
    pred[1::4, N - 1, 3] = 0.0                                         # a zero last step: a DETERMINISTIC prediction
    return dict(pos=pos, vel=vel, radius=radius, state=state, pred=pred)


# (given, probabilistic, propagate_uncertainty, max_obstacle_distance): the two wrappers, deterministic and probabilistic, with and without the filter
CASES = [(0, 0, 0, 0.0), (0, 1, 0, 0.0), (0, 1, 0, 7.0), (1, 0, 0, 0.0), (1, 0, 0, 7.0), (1, 1, 1, 0.0), (1, 1, 0, 7.0)]


def _reference_dummy_has_one_pass_more(case):
    """Given predictions in probabilistic mode: the reference's dummy is built by getConstantVelocityPrediction INSIDE ensureObstacleSize
    (data_preparation.cpp:160-163), which already runs one uncertainty pass (:75-76) that the given predictions never see.  The device and the
    mirror count the passes alike for every obstacle (include/tmpc_hip.h); the C++ functions are the reference's, so there -- and only there
    -- a dummy's radii are one pass further.  A dummy sits 141 m away: the radii never reach a constraint."""
    return case[0] == 1 and case[1] == 1


def _write(path, raw, case, copies=3, drop=5):
    given, prob, prop, max_dist = case
    n = len(raw["radius"])
    vals = [n, given, prob, prop, max_dist, copies, drop] + list(raw["state"])
    for i in range(n):
        vals += list(raw["pos"][i]) + list(raw["vel"][i]) + [raw["radius"][i]]
    if given:
        vals += list(raw["pred"].ravel())
    np.array(vals, float).tofile(path)


def _mirror(raw, case, n=None):
    from mpc_planner_amd import modules as md
    given, prob, prop, max_dist = case
    n = len(raw["radius"]) if n is None else n
    kw = dict(raw_pred=raw["pred"][:n]) if given else dict(raw_vel=raw["vel"][:n])
    passes = (1 if prop else 0) if given else (2 if prob else 0)        # what the wrappers amount to (ros1_jackalsimulator.cpp:345-346, ros1_jackal.cpp:324-332)
    return md.prepare_obstacles(raw["state"], raw["pos"][:n], raw["radius"][:n], M, N, DT, probabilistic=bool(prob), propagate_passes=passes,
                                max_obstacle_distance=max_dist, **kw)


def test_cpp_host_functions_reproduce_the_mirror(tmp_path):
    """The header compiles against a generated solver and the host functions, run the way the two wrappers' obstacle callbacks run them,
    reproduce the numpy mirror on a 12-obstacle list: selection indices equal, every value bitwise; defineRobotArea's discs (CPU)."""
    from mpc_planner_amd import modules as md
    _build()
    raw = _raw()
    for case in CASES:
        f = str(tmp_path / "scene.bin")
        _write(f, raw, case)
        out = subprocess.run([BIN, os.path.join(GEN, "config"), f], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        lines = out.stdout.splitlines()
        sel = [int(v) for v in [l for l in lines if l.startswith("sel")][0].split()[1:]]
        obs = [l.split() for l in lines if l.startswith("ob ")]
        want = _mirror(raw, case)
        keys = np.sort(md.obstacle_selection_distance(raw["pred"][:, :, :2], raw["state"]))
        assert np.diff(keys).min() > 1e-9                               # no two keys within the reach of a last-bit difference in cos / sin
        assert sel == want["selected"].tolist(), case
        assert len(obs) == M
        for j, l in enumerate(obs):
            assert int(l[2]) == int(want["gaussian"][j]) and float(l[3]) == want["radius"][j], (case, j)
            steps = np.array([float(v) for v in l[4:]]).reshape(N, 5)
            np.testing.assert_array_equal(steps[:, 0:2], want["pos"][j], err_msg=str((case, j)))
            shape = want["shape"][j]
            if sel[j] < 0 and _reference_dummy_has_one_pass_more(case):
                shape = shape.copy()
                shape[:, 1], shape[:, 2] = md.propagate_prediction_uncertainty(shape[:, 1], shape[:, 2], DT)
            np.testing.assert_array_equal(steps[:, 2:5], shape, err_msg=str((case, j)))
        if case[2] == 0 and case[0] == 0 and case[3] == 0.0 and case[1] == 0:
            assert sorted(sel) != list(range(M)) and min(sel) >= 0        # 12 > 8: a real selection
        area = {int(l.split()[1]): [float(v) for v in l.split()[2:]] for l in lines if l.startswith("area")}
        assert area[1] == [0.0, 0.25] and area[3] == [-0.25, 0.25, 0.0, 0.25, 0.25, 0.25]
    want = _mirror(raw, CASES[2])
    assert (want["selected"] < 0).any() and want["gaussian"].all()    # the filter leaves fewer than M: dummies, GAUSSIAN in probabilistic mode


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if not (_reference_dummy_has_one_pass_more(c) and c[3] > 0.0)])     # (there the filter leaves dummies)
def test_cpp_batched_twin_rows_equal_the_host_path(tmp_path, case):
    """Three scenes (12, 7 and 2 obstacles of the list; 12, 10 and 8 -- no dummies -- where the reference's dummies carry a pass the device
    does not count, _reference_dummy_has_one_pass_more) x two batch entries each: the collision columns tmpc_set_obstacle_parameters writes
    from the twin's buffers equal, bit for bit, what EllipsoidConstraints::setParameters writes from the host-prepared obstacles; every
    other column keeps its -7; the selections are equal."""
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < os.path.getmtime(os.path.join(ROOT, "mpc_planner_amd", "libtmpc_hip.so")):
        _build()
    raw = _raw()
    f = str(tmp_path / "scene.bin")
    _write(f, raw, case, drop=2 if _reference_dummy_has_one_pass_more(case) else 5)
    out = subprocess.run([BIN, os.path.join(GEN, "config"), f, "gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rows = [l for l in out.stdout.splitlines() if l.startswith("rows")][0].split()
    print(" ".join(rows))
    got = dict(zip(rows[1::2], [int(v) for v in rows[2::2]]))
    assert got["scenes"] == 3 and got["entries"] == 6
    assert got["written"] == 6 * N * (2 + 7 * M)                       # ego_disc_radius, ego_disc_0_offset and 7 columns per obstacle at every stage
    assert got["differ"] == 0 and got["selected_differ"] == 0
