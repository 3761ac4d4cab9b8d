"""GPU: reference paths fitted on device (tmpc_fit_path; csrc/tmpc_aux_kernels.hpp) -- waypoints to cubic segments, what
Contouring::onDataReceived (contouring.cpp:126-157) and PathReferenceVelocity::onDataReceived (path_reference_velocity.cpp:28-40) do when a path
arrives; DESIGN.md U15.  The kernel against the host mirror (mpc_planner_amd/modules.py fit_path, pinned on hand values and against scipy in
tests/test_path_fit.py) bit for bit, the standard tests/test_gpu_path.py holds the tracking kernel to; then the chain fit_path -> track_path ->
set_path_parameters -> solve on device against the same three mirrors on the host."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
N, M, S = 20, 8, 5
ROW_TOL = 1e-14          # road rows on device vs mirror: the line of tests/test_gpu_road.py


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda"))


def _fit_on_device(s, case, n_seg_max, given_s, extras):
    """One launch into buffers prefilled with -3.0 (status 7, count -3); returns what came back, keyed like path_fit_cases.mirror."""
    import torch
    import path_fit_cases as pf
    dev = torch.device("cuda")
    Q, P = len(case["count"]), case["n_pts_max"]
    f64 = dict(dtype=torch.float64, device=dev)
    t_xy, t_cnt, t_s, t_left, t_right, t_v = (_up(case[k]) for k in ("xy", "count", "s", "left", "right", "v"))
    t_path = torch.full((Q, n_seg_max, 9), pf.PREFILL, **f64); t_pc = torch.full((Q,), -3, dtype=torch.int32, device=dev)
    t_len = torch.full((Q,), pf.PREFILL, **f64); t_status = torch.full((Q,), 7, dtype=torch.uint8, device=dev)
    t_bounds = torch.full((Q, 2, n_seg_max, 8), pf.PREFILL, **f64); t_vel = torch.full((Q, n_seg_max, 4), pf.PREFILL, **f64)
    t_rw = torch.full((Q,), pf.PREFILL, **f64)
    kw = dict(d_left_xy=t_left.data_ptr(), d_right_xy=t_right.data_ptr(), d_v=t_v.data_ptr(), d_bounds=t_bounds.data_ptr(), d_velocity=t_vel.data_ptr(),
              d_road_width=t_rw.data_ptr()) if extras else {}
    s.fit_path(Q, P, n_seg_max, t_xy.data_ptr(), t_cnt.data_ptr(), t_path.data_ptr(), t_pc.data_ptr(), t_len.data_ptr(),
               d_s=t_s.data_ptr() if given_s else None, d_status=t_status.data_ptr(), **kw)
    s.synchronize()
    got = dict(path=t_path.cpu().numpy(), count=t_pc.cpu().numpy(), length=t_len.cpu().numpy(), status=t_status.cpu().numpy(),
               bounds=t_bounds.cpu().numpy(), velocity=t_vel.cpu().numpy(), road_width=t_rw.cpu().numpy())
    return got


def _compare(got, want, extras):
    import path_fit_cases as pf
    for key in ("count", "status", "length", "path") + (("bounds", "velocity", "road_width") if extras else ()):
        err = np.abs(got[key].astype(float) - want[key].astype(float)).max()
        print(f"[fit] {key}: max |device - mirror| = {err:.3e}, bitwise equal: {np.array_equal(got[key], want[key])}")
    for key in ("count", "status", "length", "path") + (("bounds", "velocity", "road_width") if extras else ()):
        assert np.array_equal(got[key], want[key]), key
    if not extras:                                                       # the NULL outputs are really optional: nothing of them is written
        assert (got["bounds"] == pf.PREFILL).all() and (got["velocity"] == pf.PREFILL).all() and (got["road_width"] == pf.PREFILL).all()


@pytest.mark.parametrize("given_s", [False, True])
@pytest.mark.parametrize("extras", [True, False])
def test_device_fit_equals_the_mirror_bitwise(given_s, extras):
    """Twelve scenes in one launch, n_pts_max = 1025, n_seg_max = 1024 (tests/path_fit_cases.py): counts 0, 1 (too short), 2, 3, 4, 64, 65, 66,
    130, 1025, 2000 (clipped to 1025) and ten points with a repeated waypoint (invalid).  Integers equal, floats np.array_equal for path,
    count, length, bounds, velocity, road_width and status.  Every output is prefilled with -3.0 (status 7): rows at or beyond a scene's count
    keep the prefill (the mirror's layout carries it), as does everything of the invalid and too-short scenes except count and status.
    Chord knots or given s; with or without bounds, velocity and road width."""
    import path_fit_cases as pf
    from mpc_planner_amd import solver
    case = pf.bitwise_launch()
    want = pf.mirror(case, 1024, given_s, extras)
    assert want["count"].tolist() == [0, 0, 1, 2, 3, 63, 64, 65, 129, 1024, 1024, 0]     # (what the cases are meant to reach: the mirror's own answers)
    assert want["status"].tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]
    s = solver.BatchedSolver(solver.default_dims(N=N, S=S, n_lin=M, M=M), B_max=4)          # no batch: the stream only
    got = _fit_on_device(s, case, 1024, given_s, extras)
    s.close()
    _compare(got, want, extras)
    for q in (0, 1, 11):                                                 # invalid: nothing but count and status
        assert (got["path"][q] == pf.PREFILL).all() and got["length"][q] == pf.PREFILL and got["count"][q] == 0 and got["status"][q] == 1
        assert (got["bounds"][q] == pf.PREFILL).all() and (got["velocity"][q] == pf.PREFILL).all() and got["road_width"][q] == pf.PREFILL
    assert (got["path"][5, 63:] == pf.PREFILL).all() and (got["path"][5, :63] != pf.PREFILL).any(axis=1).all()


def test_row_stride_is_independent_of_the_point_stride():
    """n_pts_max = 5 with n_seg_max = 70: counts 5, 3, 2, 7 (clipped to 5), 1 (too short), 4 with a repeated waypoint."""
    import path_fit_cases as pf
    from mpc_planner_amd import solver
    case = pf.small_launch()
    want = pf.mirror(case, 70, True, True)
    assert want["count"].tolist() == [4, 2, 1, 4, 0, 0]
    s = solver.BatchedSolver(solver.default_dims(N=N, S=S, n_lin=M, M=M), B_max=4)
    got = _fit_on_device(s, case, 70, True, True)
    _compare(got, want, True)
    want = pf.mirror(case, 4, False, False)                              # the tightest stride the contract allows
    got = _fit_on_device(s, case, 4, False, False)
    _compare(got, want, False)
    s.close()


@functools.lru_cache(maxsize=None)
def _chain():
    """fit_path -> track_path -> set_path_parameters (-> road_halfspaces) -> solve on device, nothing read back in between, and the same from
    the three mirrors on the host, solved on a second handle.  One make_scene batch of 16 trajectories; the waypoints are 25 points on the
    scene's own reference cubics, from 3 m behind the robot on (the first cubic continued backwards), the bounds 2 m to the left and 1.5 m
    to the right of them.  The path parameter at the robot is then about 3, not 0: as scenes.with_long_path does, the spline entry of xinit
    becomes the mirror's closest_s and the spline column of the warm start is advanced by it -- the same arrays for both handles."""
    import torch
    from mpc_planner_amd import scenes, solver, modules as md
    B = 16
    sc = scenes.make_scene(83, N=N, M=M, B=B)
    seg = sc["segments"]
    length0 = float(seg[-1, 8] + (seg[-1, 8] - seg[-2, 8]))
    ss = np.linspace(-3.0, length0, 25)
    pts = np.array([md._road_segment_eval(seg[:, :8], seg[:, 8], float(v)) for v in ss])          # x, y, dx, dy
    xy = pts[:, :2]
    nrm = np.stack([-pts[:, 3], pts[:, 2]], 1) / np.hypot(pts[:, 2], pts[:, 3])[:, None]
    left, right = xy + 2.0 * nrm, xy - 1.5 * nrm
    pos = sc["xinit"][0, :2]
    r = scenes.ROBOT_RADIUS
    pm = sc["pm"]
    spl = np.array([pm.index(n.format(i)) for i in range(S) for n in ("spline_x{}_a", "spline_x{}_b", "spline_x{}_c", "spline_x{}_d",
                                                                       "spline_y{}_a", "spline_y{}_b", "spline_y{}_c", "spline_y{}_d", "spline{}_start")])
    # ---- host: the three mirrors ----
    fit = md.fit_path(xy, left=left, right=right)
    tr = md.track_path(fit["path"], fit["length"], pos, S, segment=-1, left=fit["left"], right=fit["right"])
    xinit, x0 = sc["xinit"].copy(), sc["x0"].copy()
    xinit[:, 4] = tr["s"]; x0[:, :, md.IDX["spline"]] += tr["s"]
    host = sc["params"].copy()
    for b in range(B):
        md.contouring_set_parameters(pm, host[b], scenes.WEIGHTS, tr["window"])
    rows = md.road_halfspaces_from_bounds(tr["window"], tr["left"], tr["right"], x0[0, :N, 6], r)
    dims = solver.default_dims(N=N, S=S, n_lin=M, M=M)
    ref_s = solver.BatchedSolver(dims, B_max=B)
    ref_s.set_batch(xinit, x0, host); ref_s.solve(); ref = ref_s.get()
    ref_s.close()
    # ---- device ----
    dev = torch.device("cuda")
    f64 = dict(dtype=torch.float64, device=dev)
    s = solver.BatchedSolver(dims, B_max=B)
    p0 = sc["params"].copy(); p0[:, :, spl] = -3.0                       # the spline columns have to come from the device
    s.set_batch(xinit, x0, p0)
    P, R = 32, 40
    t_xy = torch.zeros((1, P, 2), **f64); t_xy[0, :25] = _up(xy)
    t_left = torch.zeros((1, P, 2), **f64); t_left[0, :25] = _up(left)
    t_right = torch.zeros((1, P, 2), **f64); t_right[0, :25] = _up(right)
    t_cnt = torch.full((1,), 25, dtype=torch.int32, device=dev)
    t_path = torch.zeros((1, R, 9), **f64); t_pc = torch.zeros(1, dtype=torch.int32, device=dev); t_len = torch.zeros(1, **f64)
    t_bounds = torch.zeros((1, 2, R, 8), **f64)
    t_pos = _up(pos.copy().reshape(1, 2)); t_seg = torch.full((1,), -1, dtype=torch.int32, device=dev); t_cs = torch.zeros(1, **f64)
    t_win = torch.zeros((1, S, 9), **f64); t_bw = torch.zeros((1, 2, S, 8), **f64)
    t_sc = torch.zeros(B, dtype=torch.int32, device=dev); t_main = torch.zeros(1, dtype=torch.int32, device=dev)
    t_stat = torch.zeros((1, N, 2, 3), **f64)
    torch.cuda.synchronize()
    s.fit_path(1, P, R, t_xy.data_ptr(), t_cnt.data_ptr(), t_path.data_ptr(), t_pc.data_ptr(), t_len.data_ptr(), d_left_xy=t_left.data_ptr(),
               d_right_xy=t_right.data_ptr(), d_bounds=t_bounds.data_ptr())
    s.track_path(1, R, t_path.data_ptr(), t_pc.data_ptr(), t_len.data_ptr(), t_pos.data_ptr(), 2, t_seg.data_ptr(), t_cs.data_ptr(), t_win.data_ptr(),
                 d_bounds=t_bounds.data_ptr(), d_bound_window=t_bw.data_ptr())
    s.set_path_parameters(t_win.data_ptr(), t_sc.data_ptr(), 1)
    s.road_halfspaces(t_main.data_ptr(), 1, r, r, t_stat.data_ptr(), 2, first_row=0, d_bound_segments=t_bw.data_ptr())
    s.solve(sync=False)
    s.synchronize()
    out = dict(fit=fit, tr=tr, host=host, rows=rows, ref=ref, spl=spl, got=s.get(), p_dev=s.debug_get_params(), seg=int(t_seg.item()), cs=float(t_cs.item()),
               win=t_win.cpu().numpy()[0], bw=t_bw.cpu().numpy()[0], rows_dev=t_stat.cpu().numpy()[0], count=int(t_pc.item()))
    s.close()
    return out


def test_chain_fit_track_write_solve_equals_the_host_mirrors():
    """Window, bound window, closest_s, segment and the written spline columns np.array_equal the mirrors'; then the solve on the device-built
    rows equals the solve on the host-built rows: every integer, and floats bitwise."""
    c = _chain()
    assert c["count"] == 24 and c["tr"]["segment"] == 2 and 2.5 < c["tr"]["s"] < 3.5 and c["seg"] == c["tr"]["segment"] and c["cs"] == c["tr"]["s"]
    assert np.array_equal(c["win"], c["tr"]["window"])
    assert np.array_equal(c["bw"][0], c["tr"]["left"]) and np.array_equal(c["bw"][1], c["tr"]["right"])
    assert np.array_equal(c["p_dev"][:, :, c["spl"]], c["host"][:, :, c["spl"]])
    assert np.array_equal(c["p_dev"], c["host"])                          # and nothing else moved
    got, ref = c["got"], c["ref"]
    print(f"[fit chain] segment {c['seg']}, closest_s {c['cs']!r}, exit codes {got['exit_code'].tolist()}")
    assert (ref["exit_code"] == 1).any()                                  # (the scene is one the solver can do something with)
    assert sorted(got) == sorted(ref)
    for key in ref:
        a, b = np.asarray(got[key]), np.asarray(ref[key])
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), key


def test_road_rows_from_the_fitted_bounds():
    """The bound window of the fitted bounds, fed to tmpc_road_halfspaces, against modules.road_halfspaces_from_bounds on the mirror's bound
    window; tolerance: tests/test_gpu_road.py's own."""
    c = _chain()
    err = np.abs(c["rows_dev"][1:] - c["rows"][1:]).max()
    print(f"[fit chain] road rows: max |device - mirror| = {err:.3e}")
    assert np.abs(c["rows"][1:]).max() > 0.1
    np.testing.assert_allclose(c["rows_dev"][1:], c["rows"][1:], rtol=ROW_TOL, atol=ROW_TOL)


def test_contract_errors_launch_nothing():
    import torch
    from mpc_planner_amd import solver
    s = solver.BatchedSolver(solver.default_dims(N=N, S=S, n_lin=M, M=M), B_max=4)
    dev = torch.device("cuda")
    f64 = dict(dtype=torch.float64, device=dev)
    P, R = 4, 5
    t_xy = torch.zeros((1, P, 2), **f64); t_xy[0, :, 0] = torch.arange(P, **f64)
    t_cnt = torch.full((1,), P, dtype=torch.int32, device=dev)
    t_path = torch.full((1, R, 9), -3.0, **f64); t_pc = torch.full((1,), -3, dtype=torch.int32, device=dev); t_len = torch.full((1,), -3.0, **f64)
    t_bounds = torch.full((1, 2, R, 8), -3.0, **f64); t_vel = torch.full((1, R, 4), -3.0, **f64); t_v = torch.ones((1, P), **f64)
    base = dict(n_scenes=1, n_pts_max=P, n_seg_max=R, d_xy=t_xy.data_ptr(), d_count=t_cnt.data_ptr(), d_path=t_path.data_ptr(),
                d_path_count=t_pc.data_ptr(), d_path_length=t_len.data_ptr())
    fit = lambda **kw: s.fit_path(**dict(base, **kw))
    both = dict(d_left_xy=t_xy.data_ptr(), d_right_xy=t_xy.data_ptr(), d_bounds=t_bounds.data_ptr())
    for kw, msg in ((dict(n_pts_max=1), "n_pts_max"), (dict(n_pts_max=1026, n_seg_max=1024), "n_pts_max"), (dict(n_seg_max=P - 2), "n_seg_max"),
                    (dict(n_seg_max=1025), "n_seg_max"), (dict(n_scenes=0), "n_scenes"),
                    (dict(both, d_right_xy=None), "go together"), (dict(both, d_left_xy=None), "go together"), (dict(both, d_bounds=None), "go together"),
                    (dict(d_bounds=t_bounds.data_ptr()), "go together"),
                    (dict(d_v=t_v.data_ptr()), "go together"), (dict(d_velocity=t_vel.data_ptr()), "go together"),
                    (dict(d_xy=None), "NULL input"), (dict(d_count=None), "NULL input"), (dict(d_path=None), "NULL output"),
                    (dict(d_path_count=None), "NULL output"), (dict(d_path_length=None), "NULL output")):
        with pytest.raises(solver.TmpcError, match=msg):
            fit(**kw)
    s.synchronize()
    assert (t_path == -3.0).all() and t_pc.item() == -3 and t_len.item() == -3.0 and (t_bounds == -3.0).all() and (t_vel == -3.0).all()      # nothing ran
    assert s.lib.tmpc_fit_path(None, 1, P, R, *([None] * 13)) == -1      # no handle
    fit(n_seg_max=P - 1)                                                  # the limit itself, no batch needed
    s.synchronize()
    assert t_pc.item() == P - 1 and t_len.item() == float(P - 1) and (t_path[0, :P - 1, 2] == 1.0).all()
    s.close()
