"""GPU: the velocity profile along the reference path on device (tmpc_path_velocity_window; csrc/tmpc_aux_kernels.hpp) --
PathReferenceVelocity::setParameters, path_reference_velocity.cpp:59-95, and the value the guidance planner is given,
guidance_constraints.cpp:91-94 -- and the parameter writer of generated solvers (tmpc_scatter_parameters), against the host mirrors
(mpc_planner_amd/modules.py path_velocity_window / path_velocity_at / scatter_parameters, pinned on hand values in tests/test_path_velocity.py)
bit for bit; then the generated `path_velocity` stack end to end: fit -> track -> velocity window -> scatter -> solve without a host round
trip, against the same ticks prepared on the host."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
N = 20
SENTINEL = -3.0
REF_V = 1.7
SPLINE_NAMES = ("spline_x{}_a", "spline_x{}_b", "spline_x{}_c", "spline_x{}_d", "spline_y{}_a", "spline_y{}_b", "spline_y{}_c", "spline_y{}_d", "spline{}_start")


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda"))


def _full(shape, value, dtype):
    import torch
    return torch.full(shape, value, dtype=dtype, device=torch.device("cuda"))


def _hand_written(B_max=4):
    from mpc_planner_amd import solver
    return solver.BatchedSolver(solver.default_dims(N=N, S=5, n_lin=8, M=8), B_max=B_max)


def _mirror_window(fits, flags, segment, closest_s, S, with_velocity=True):
    """The mirrors' answer to one launch: window [Q][S][4] and v_ref [Q].  The kernel clamps the segment into [0, count - 1] and takes
    count <= 0 or a cleared flag for "no profile": the mirror is called with the clamped segment, and with None for such a scene."""
    from mpc_planner_amd import modules as md
    Q = len(fits)
    window, v_ref = np.zeros((Q, S, 4)), np.zeros(Q)
    for q, fit in enumerate(fits):
        profile = with_velocity and flags[q] and fit["count"] > 0
        vel = fit["velocity"] if profile else None
        seg = min(max(int(segment[q]), 0), max(fit["count"] - 1, 0))
        window[q] = md.path_velocity_window(vel, fit["count"], seg, S, REF_V)
        v_ref[q] = md.path_velocity_at(vel, fit["path"], fit["count"], fit["length"], closest_s[q], REF_V)
    return window, v_ref


def test_window_and_v_ref_equal_the_mirrors_bitwise():
    """Six scenes fitted ON DEVICE (tmpc_fit_path, 9 / 6 / 5 / 4 / 1 / 3 waypoints with a velocity; n_seg_max 8), S = 3: the segment in the
    middle; count - 2 (one zero slot); count - 1 (two); -1 with count > 0 (clamped to 0); count 0 (one waypoint is no path: the default row);
    a cleared flag with count > 0 (the default row).  closest_s: inside a segment, ON a knot, at the length, below the first knot.
    Outputs prefilled with a sentinel, np.array_equal against the mirrors.  Then d_velocity = NULL and d_v_ref = NULL: default rows, the
    sentinel stays in v_ref.  Then n_seg_max = 130, S = 5, count = 129: the lookup beyond one round of 64 lanes."""
    import torch
    import path_fit_cases as pf
    from mpc_planner_amd import modules as md
    Q, P, R, S = 6, 9, 8, 3
    counts = np.array([9, 6, 5, 4, 1, 3], np.int32)
    xy, v = np.full((Q, P, 2), 77.0), np.full((Q, P), 55.0)
    fits = []
    for q, n in enumerate(counts):
        xy[q, :n] = pf.waypoints(np.random.default_rng(40 + q), n)
        v[q, :n] = np.random.default_rng(140 + q).uniform(0.5, 2.5, n)
        fits.append(md.fit_path(xy[q, :n], v=v[q, :n]))
    assert [f["count"] for f in fits] == [8, 5, 4, 3, 0, 2]
    s = _hand_written()
    t_xy, t_cnt_in, t_v = _up(xy), _up(counts), _up(v)
    t_path, t_cnt, t_len = _full((Q, R, 9), SENTINEL, torch.float64), _full((Q,), -3, torch.int32), _full((Q,), SENTINEL, torch.float64)
    t_vel = _full((Q, R, 4), SENTINEL, torch.float64)
    s.fit_path(Q, P, R, t_xy.data_ptr(), t_cnt_in.data_ptr(), t_path.data_ptr(), t_cnt.data_ptr(), t_len.data_ptr(), d_v=t_v.data_ptr(),
               d_velocity=t_vel.data_ptr())
    segment = np.array([3, 3, 3, -1, 2, 0], np.int32)
    flags = np.array([1, 1, 1, 1, 1, 0], np.uint8)
    closest = np.array([0.5 * (fits[0]["path"][3, 8] + fits[0]["path"][4, 8]), fits[1]["path"][3, 8], fits[2]["length"], -0.5, 1.0,
                        0.25 * fits[5]["length"]])
    want_w, want_v = _mirror_window(fits, flags, segment, closest, S)
    assert (want_w[1, 2] == 0.0).all() and want_w[1, 1].any() and (want_w[2, 1:] == 0.0).all() and want_w[2, 0].any()   # one and two zero slots
    assert np.array_equal(want_w[3], fits[3]["velocity"][:3]) and want_w[4].tolist() == [[0.0, 0.0, 0.0, REF_V]] * 3 and np.array_equal(want_w[5], want_w[4])
    assert want_v[1] == fits[1]["velocity"][3, 3] and want_v[4] == REF_V and want_v[5] == REF_V                          # on a knot: the right segment's d
    t_seg, t_cs, t_flag = _up(segment), _up(closest), _up(flags)
    t_win, t_vref = _full((Q + 1, S, 4), SENTINEL, torch.float64), _full((Q + 1,), SENTINEL, torch.float64)
    call = lambda **kw: s.path_velocity_window(**dict(dict(n_scenes=Q, n_seg_max=R, S=S, d_path=t_path.data_ptr(), d_path_count=t_cnt.data_ptr(),
                                                           d_path_length=t_len.data_ptr(), d_segment=t_seg.data_ptr(), d_closest_s=t_cs.data_ptr(),
                                                           d_window=t_win.data_ptr(), d_velocity=t_vel.data_ptr(), d_has_velocity=t_flag.data_ptr(),
                                                           reference_velocity=REF_V, d_v_ref=t_vref.data_ptr()), **kw))
    call()
    s.synchronize()
    got_w, got_v = t_win.cpu().numpy(), t_vref.cpu().numpy()
    print(f"[velocity] v_ref {got_v[:Q].tolist()} (mirror {want_v.tolist()}), max |window - mirror| {np.abs(got_w[:Q] - want_w).max():.3e}")
    assert np.array_equal(got_w[:Q], want_w) and np.array_equal(got_v[:Q], want_v)
    assert (got_w[Q] == SENTINEL).all() and got_v[Q] == SENTINEL                              # nothing behind the last scene
    assert np.array_equal(t_seg.cpu().numpy(), segment)                                       # inputs are inputs
    # without flags every scene with a path has a profile
    t_win.fill_(SENTINEL); t_vref.fill_(SENTINEL)
    call(d_has_velocity=None)
    s.synchronize()
    want_w2, want_v2 = _mirror_window(fits, np.ones(Q, np.uint8), segment, closest, S)
    assert np.array_equal(t_win.cpu().numpy()[:Q], want_w2) and np.array_equal(t_vref.cpu().numpy()[:Q], want_v2)
    assert np.array_equal(want_w2[5, :2], fits[5]["velocity"]) and want_w2[5, 2].tolist() == [0.0] * 4          # the scene whose flag was cleared
    # no profile at all, no v_ref: the default rows, the sentinel elsewhere
    t_win.fill_(SENTINEL); t_vref.fill_(SENTINEL)
    call(d_velocity=None, d_v_ref=None)
    s.synchronize()
    got_w = t_win.cpu().numpy()
    assert (got_w[:Q, :, :3] == 0.0).all() and (got_w[:Q, :, 3] == REF_V).all() and (got_w[Q] == SENTINEL).all()
    assert (t_vref.cpu().numpy() == SENTINEL).all()
    # ---- 129 segments, S = 5: three scenes on one path; s in segment 100, ON knot 64, just before it; windows at 98, 127 (three zero slots), 62
    big = md.fit_path(pf.waypoints(np.random.default_rng(47), 130), v=np.random.default_rng(147).uniform(0.5, 2.5, 130))
    assert big["count"] == 129
    Rb, Sb, Qb = 130, 5, 3
    path_b, vel_b = np.full((Qb, Rb, 9), 9e9), np.full((Qb, Rb, 4), 9e9)                      # the row behind the count would win any `<=` test
    path_b[:, :129], vel_b[:, :129] = big["path"], big["velocity"]
    path_b[:, 129, 8] = -1.0
    knots = big["path"][:, 8]
    closest_b = np.array([0.5 * (knots[100] + knots[101]), knots[64], np.nextafter(knots[64], 0.0)])
    segment_b = np.array([98, 127, 62], np.int32)
    want_wb, want_vb = _mirror_window([big] * Qb, np.ones(Qb, np.uint8), segment_b, closest_b, Sb)
    assert (want_wb[1, 2:] == 0.0).all() and want_vb[1] == big["velocity"][64, 3] and want_vb[2] != want_vb[1]
    t_pb, t_vb, t_cb, t_lb = _up(path_b), _up(vel_b), _up(np.full(Qb, 129, np.int32)), _up(np.full(Qb, big["length"]))
    t_sb, t_csb = _up(segment_b), _up(closest_b)
    t_wb, t_vrb = _full((Qb, Sb, 4), SENTINEL, torch.float64), _full((Qb,), SENTINEL, torch.float64)
    s.path_velocity_window(Qb, Rb, Sb, t_pb.data_ptr(), t_cb.data_ptr(), t_lb.data_ptr(), t_sb.data_ptr(), t_csb.data_ptr(), t_wb.data_ptr(),
                           d_velocity=t_vb.data_ptr(), reference_velocity=REF_V, d_v_ref=t_vrb.data_ptr())
    s.synchronize()
    assert np.array_equal(t_wb.cpu().numpy(), want_wb) and np.array_equal(t_vrb.cpu().numpy(), want_vb)
    s.close()


def test_scatter_equals_the_path_writer_and_the_mirror():
    """Hand-written library, B = 12, N = 20.  scatter_parameters with the 45 spline columns and track_path's window leaves
    tmpc_debug_get_params bit-equal to tmpc_set_path_parameters on a twin handle; per_stage = 1 with 128 columns in a shuffled order against
    the mirror; entries whose scene is -1 or beyond n_scenes, and every column not named, keep their prefill."""
    import path_cases as pc
    from mpc_planner_amd import scenes, solver, modules as md
    S, M, B = 5, 8, 12
    sc = scenes.make_scene(90, N=N, M=M, B=B)
    pm = sc["pm"]
    dims = solver.default_dims(N=N, S=S, n_lin=M, M=M)
    case = pc.bitwise_scenes()
    windows = np.stack([md.path_window(case["path"][3, :70], 140.0, 31, S), md.path_window(case["path"][1, :3], 6.0, 1, S)])
    scene_of = np.array([0, 0, 0, 0, -1, -1, 2, 7, 1, 1, 0, 1], np.int32)
    cols = [pm.index(n.format(i)) for i in range(S) for n in SPLINE_NAMES]
    prefill = np.full_like(sc["params"], SENTINEL)
    a, b = solver.BatchedSolver(dims, B_max=B), solver.BatchedSolver(dims, B_max=B)
    a.set_batch(sc["xinit"], sc["x0"], prefill); b.set_batch(sc["xinit"], sc["x0"], prefill)
    t_win, t_sc = _up(windows), _up(scene_of)
    a.scatter_parameters(cols, t_win.data_ptr(), t_sc.data_ptr(), 2)
    b.set_path_parameters(t_win.data_ptr(), t_sc.data_ptr(), 2)
    a.synchronize(); b.synchronize()
    got = a.debug_get_params()
    assert np.array_equal(got, b.debug_get_params())
    assert (got[[4, 5, 6, 7]] == SENTINEL).all() and (got != SENTINEL).sum() == 8 * N * 9 * S
    want = prefill.copy()
    md.scatter_parameters(want, cols, windows.reshape(2, -1), scene_of)
    assert np.array_equal(got, want)
    # per stage: 128 of the 135 columns, shuffled, three scenes
    rng = np.random.default_rng(8)
    cols2 = rng.permutation(dims.npar)[:128].tolist()
    values = rng.normal(size=(3, N, 128))
    a.scatter_parameters(cols2, _up(values).data_ptr(), t_sc.data_ptr(), 3, per_stage=True)
    a.synchronize()
    md.scatter_parameters(want, cols2, values, scene_of, per_stage=True)
    got = a.debug_get_params()
    assert np.array_equal(got, want)
    assert (got[[4, 5, 7]] == SENTINEL).all() and not (got[6][:, cols2] == SENTINEL).any()
    rest = np.setdiff1d(np.arange(dims.npar), cols2)
    assert np.array_equal(got[:, :, rest], b.debug_get_params()[:, :, rest])                  # the columns not named: as they were
    a.close(); b.close()


def test_bad_arguments():
    """Every refusal with its message; nothing is launched (the buffers named here are a few bytes: a launch would fault or write the sentinel)."""
    import torch
    from mpc_planner_amd import scenes, solver
    from test_gpu_parity import _generated_lib
    s = _hand_written(B_max=4)
    f64 = torch.float64
    t_path, t_cnt, t_len = _full((1, 4, 9), 0.0, f64), _full((1,), 4, torch.int32), _full((1,), 4.0, f64)
    t_seg, t_cs, t_win, t_vel = _full((1,), 0, torch.int32), _full((1,), 0.5, f64), _full((1, 3, 4), SENTINEL, f64), _full((1, 4, 4), 1.0, f64)
    base = dict(n_scenes=1, n_seg_max=4, S=3, d_path=t_path.data_ptr(), d_path_count=t_cnt.data_ptr(), d_path_length=t_len.data_ptr(),
                d_segment=t_seg.data_ptr(), d_closest_s=t_cs.data_ptr(), d_window=t_win.data_ptr(), d_velocity=t_vel.data_ptr())
    for kw, msg in ((dict(d_path=None), "NULL input"), (dict(d_path_count=None), "NULL input"), (dict(d_path_length=None), "NULL input"),
                    (dict(d_segment=None), "NULL input"), (dict(d_closest_s=None), "NULL input"), (dict(d_window=None), "NULL output"),
                    (dict(S=0), "1 <= S <= 64"), (dict(S=65), "1 <= S <= 64"), (dict(n_scenes=0), "n_scenes"), (dict(n_seg_max=0), "n_seg_max"),
                    (dict(n_seg_max=1025), "n_seg_max")):
        with pytest.raises(solver.TmpcError, match=msg):
            s.path_velocity_window(**dict(base, **kw))
    s.synchronize()
    assert (t_win.cpu().numpy() == SENTINEL).all()
    s.path_velocity_window(**base)                                           # the same call, accepted: no batch is needed
    s.synchronize()
    assert (t_win.cpu().numpy() == [1.0] * 4).all()
    assert s.lib.tmpc_path_velocity_window(None, 1, 4, 3, None, None, None, None, None, None, None, C.c_double(1.0), None, None) == -1
    # the scatter needs a batch
    t_val, t_sc = _full((1, 128), 2.0, f64), _full((4,), 0, torch.int32)
    with pytest.raises(solver.TmpcError, match="no batch"):
        s.scatter_parameters([0, 1], t_val.data_ptr(), t_sc.data_ptr(), 1)
    sc = scenes.make_scene(91, N=N, M=8, B=4)
    s.set_batch(sc["xinit"], sc["x0"], sc["params"])
    npar = s.npar
    for args, kw, msg in ((([0, 1], None, t_sc.data_ptr(), 1), {}, "bad argument"), (([0, 1], t_val.data_ptr(), None, 1), {}, "bad argument"),
                          ((None, t_val.data_ptr(), t_sc.data_ptr(), 1), {}, "bad argument"), (([0, 1], t_val.data_ptr(), t_sc.data_ptr(), 0), {}, "bad argument"),
                          (([], t_val.data_ptr(), t_sc.data_ptr(), 1), {}, "n_cols"), ((list(range(129)), t_val.data_ptr(), t_sc.data_ptr(), 1), {}, "n_cols"),
                          (([0, npar], t_val.data_ptr(), t_sc.data_ptr(), 1), {}, "outside"), (([0, -1], t_val.data_ptr(), t_sc.data_ptr(), 1), {}, "outside"),
                          (([3, 5, 3], t_val.data_ptr(), t_sc.data_ptr(), 1), {}, "duplicate")):
        with pytest.raises(solver.TmpcError, match=msg):
            s.scatter_parameters(*args, **kw)
    assert s.lib.tmpc_scatter_parameters(s._h, (C.c_int32 * 2)(0, 1), 2, C.c_void_p(t_val.data_ptr()), 2, C.c_void_p(t_sc.data_ptr()), 1) == -1   # per_stage 2
    assert b"per_stage" in s.lib.tmpc_last_error(s._h)
    assert s.lib.tmpc_scatter_parameters(None, None, 1, None, 0, None, 1) == -1
    s.synchronize()
    assert np.array_equal(s.debug_get_params(), sc["params"])                 # none of the refused calls wrote anything
    s.scatter_parameters(list(range(128)), t_val.data_ptr(), t_sc.data_ptr(), 1)      # the limit itself
    s.synchronize()
    assert (s.debug_get_params()[:, :, :128] == 2.0).all()
    # window_segments on the hand-written library: 0 or the handle's S
    t_pos, t_w9 = _full((1, 2), 0.0, f64), _full((1, 5, 9), 0.0, f64)
    t_path[0, :, 2] = 1.0; t_path[0, :, 6] = 0.0; t_path[0, :, 8] = torch.arange(4, dtype=f64, device=t_path.device)
    track = lambda **kw: s.track_path(1, 4, t_path.data_ptr(), t_cnt.data_ptr(), t_len.data_ptr(), t_pos.data_ptr(), 2, t_seg.data_ptr(), t_cs.data_ptr(),
                                      t_w9.data_ptr(), **kw)
    track(window_segments=5); track(window_segments=0)
    for ws, msg in ((3, "window_segments must be 0 or the handle's S"), (-1, "0 <= window_segments <= 64"), (65, "0 <= window_segments <= 64")):
        with pytest.raises(solver.TmpcError, match=msg):
            track(window_segments=ws)
    # the struct's first revision (8 bytes, no window_segments) is still taken
    class FirstRevision(C.Structure):
        _fields_ = [("size", C.c_uint32), ("search_range", C.c_int32)]
    vp = C.c_void_p
    raw = lambda opt: s.lib.tmpc_track_path(s._h, 1, 4, vp(t_path.data_ptr()), vp(t_cnt.data_ptr()), vp(t_len.data_ptr()), None, vp(t_pos.data_ptr()), 2,
                                            opt, vp(t_seg.data_ptr()), vp(t_cs.data_ptr()), vp(t_w9.data_ptr()), None, None)
    assert raw(C.cast(C.byref(FirstRevision(8, 2)), C.POINTER(solver.TmpcPathOptions))) == 0
    assert raw(C.cast(C.byref(FirstRevision(6, 2)), C.POINTER(solver.TmpcPathOptions))) == -1
    s.synchronize(); s.close()
    # a generated solver: track_path with window_segments, the velocity window and the scatter work; the path writer keeps refusing
    path, meta = _generated_lib("path_velocity")
    sg = solver.BatchedSolver(solver.default_dims(N=N, lib_path=path), B_max=4, lib_path=path)
    trackg = lambda **kw: sg.track_path(1, 4, t_path.data_ptr(), t_cnt.data_ptr(), t_len.data_ptr(), t_pos.data_ptr(), 2, t_seg.data_ptr(), t_cs.data_ptr(),
                                        t_w9.data_ptr(), **kw)
    with pytest.raises(solver.TmpcError, match="generated solver"):
        trackg()
    with pytest.raises(solver.TmpcError, match="0 <= window_segments <= 64"):
        trackg(window_segments=65)
    t_w9.fill_(SENTINEL)
    trackg(window_segments=3)
    sg.path_velocity_window(**base)
    sg.synchronize()
    w9 = t_w9.cpu().numpy().reshape(-1)
    assert (w9[:27] != SENTINEL).all() and (w9[27:] == SENTINEL).all() and w9[[8, 17, 26]].tolist() == [0.0, 1.0, 2.0]
    with pytest.raises(solver.TmpcError, match="no batch"):
        sg.scatter_parameters([0], t_val.data_ptr(), t_sc.data_ptr(), 1)
    with pytest.raises(solver.TmpcError, match="generated solver"):
        sg.set_path_parameters(t_w9.data_ptr(), t_sc.data_ptr(), 1)
    sg.close()


# ---- the generated stack end to end -------------------------------------------------------------------------------------------------------
S_GEN, Q_GEN, B_GEN, R_GEN, P_GEN, TICKS = 3, 6, 12, 8, 9, 5
WP_COUNTS = (9, 7, 4, 3, 9, 6)
WP_STEP = (0.5, 0.8, 1.5, 2.0, 0.6, 1.0)
START_S = (0.38, 0.65, 1.9, 0.5, 0.45, 0.8)             # scene 2 starts on its second of three segments: its window straddles the end at once
HAS_PROFILE = (1, 1, 1, 1, 0, 1)


def _arc(q):
    n, step = WP_COUNTS[q], WP_STEP[q]
    heading = 0.3 * q + (0.08 if q % 2 else -0.06) * np.arange(n)
    return np.cumsum(np.stack([np.cos(heading), np.sin(heading)], 1) * step, 0) + np.array([3.0 * q, -2.0 * q])


@functools.lru_cache(maxsize=None)
def _gen_scenes(profile=None):
    """Six paths (gentle arcs, 8 / 6 / 3 / 2 / 8 / 5 segments) with a velocity at every waypoint (profile: that constant instead), a robot
    0.05 m beside each at START_S driving along it at 1 m/s, two entries per scene: the second has an obstacle 1.2 m beside the path 2 m ahead."""
    from mpc_planner_amd import modules as md, scenes
    xy, v = np.zeros((Q_GEN, P_GEN, 2)), np.zeros((Q_GEN, P_GEN))
    fits, state = [], np.zeros((Q_GEN, 5))
    obstacle = np.zeros((Q_GEN, 2))
    for q, n in enumerate(WP_COUNTS):
        xy[q, :n] = _arc(q)
        v[q, :n] = (0.9 + 0.5 * np.sin(0.7 * np.arange(n) + q)) if profile is None else profile
        fit = md.fit_path(xy[q, :n], v=v[q, :n])
        fits.append(fit)
        i = max(j for j in range(fit["count"]) if fit["path"][j, 8] <= START_S[q])
        x, y, dx, dy = md._path_cubic(fit["path"][i, :8], START_S[q] - fit["path"][i, 8])
        nrm = np.hypot(dx, dy)
        state[q] = [x - 0.05 * dy / nrm, y + 0.05 * dx / nrm, np.arctan2(dy, dx), 1.0, START_S[q]]
        obstacle[q] = [x + 2.0 * dx / nrm + 1.2 * dy / nrm, y + 2.0 * dy / nrm - 1.2 * dx / nrm]
    return dict(xy=xy, v=v, count=np.array(WP_COUNTS, np.int32), fits=fits, state=state, obstacle=obstacle, weights=scenes.WEIGHTS,
                radius=scenes.ROBOT_RADIUS)


def _base_params(meta, sc):
    """[B][N][npar]: weights, disc, obstacles (dummies; entry 1 of each scene: one real obstacle from stage 1 on); spline and spline_v: SENTINEL."""
    pm = meta["parameter_map"]
    p = np.zeros((B_GEN, N, meta["npar"]))
    for name in ("acceleration", "angular_velocity", "contour", "lag", "velocity", "reference_velocity", "terminal_angle", "terminal_contouring"):
        p[:, :, pm[name]] = sc["weights"][name]
    p[:, :, pm["ego_disc_radius"]] = sc["radius"]
    for j in range(2):
        for name, val in dict(x=50.0, y=50.0, psi=0.0, major=0.0, minor=0.0, chi=1.0, r=0.1).items():
            p[:, :, pm[f"ellipsoid_obst_{j}_{name}"]] = val
    for q in range(Q_GEN):
        p[2 * q + 1, 1:, pm["ellipsoid_obst_0_x"]] = sc["obstacle"][q, 0]; p[2 * q + 1, 1:, pm["ellipsoid_obst_0_y"]] = sc["obstacle"][q, 1]
        p[2 * q + 1, 1:, pm["ellipsoid_obst_0_r"]] = 0.3
    spl = [pm[n.format(i)] for i in range(S_GEN) for n in SPLINE_NAMES]
    vcols = [pm[f"spline_v{i}_{k}"] for i in range(S_GEN) for k in "abcd"]
    p[:, :, spl + vcols] = SENTINEL
    return p, spl, vcols


class _Params:
    def __init__(self, pm):
        self.pm = pm

    def index(self, name):
        return self.pm[name]


def _device_paths(dev, sc):
    """The paths and velocity profiles fitted on device, once."""
    import torch
    t = dict(xy=_up(sc["xy"]), cnt_in=_up(sc["count"]), v=_up(sc["v"]), path=_full((Q_GEN, R_GEN, 9), SENTINEL, torch.float64),
             cnt=_full((Q_GEN,), -3, torch.int32), len=_full((Q_GEN,), SENTINEL, torch.float64), vel=_full((Q_GEN, R_GEN, 4), SENTINEL, torch.float64))
    dev.fit_path(Q_GEN, P_GEN, R_GEN, t["xy"].data_ptr(), t["cnt_in"].data_ptr(), t["path"].data_ptr(), t["cnt"].data_ptr(), t["len"].data_ptr(),
                 d_v=t["v"].data_ptr(), d_velocity=t["vel"].data_ptr())
    return t


def _device_tick(dev, t, t_pos, t_seg, t_cs, t_win, t_vwin, t_vref, t_flag, t_sc, spl, vcols):
    """track -> velocity window -> two scatters -> solve: enqueued on the handle's stream, nothing read back in between."""
    dev.track_path(Q_GEN, R_GEN, t["path"].data_ptr(), t["cnt"].data_ptr(), t["len"].data_ptr(), t_pos.data_ptr(), 5, t_seg.data_ptr(), t_cs.data_ptr(),
                   t_win.data_ptr(), window_segments=S_GEN)
    dev.path_velocity_window(Q_GEN, R_GEN, S_GEN, t["path"].data_ptr(), t["cnt"].data_ptr(), t["len"].data_ptr(), t_seg.data_ptr(), t_cs.data_ptr(),
                             t_vwin.data_ptr(), d_velocity=t["vel"].data_ptr(), d_has_velocity=None if t_flag is None else t_flag.data_ptr(),
                             reference_velocity=REF_V, d_v_ref=t_vref.data_ptr())
    dev.scatter_parameters(spl, t_win.data_ptr(), t_sc.data_ptr(), Q_GEN)
    dev.scatter_parameters(vcols, t_vwin.data_ptr(), t_sc.data_ptr(), Q_GEN)
    dev.solve(sync=False)


def test_generated_stack_end_to_end_five_ticks():
    """libtmpc_hip_path_velocity.so (contouring + path reference velocity with a dynamic velocity reference + ellipsoids, three segments),
    B = 12, two entries per scene, five ticks.  DEVICE: paths and profiles fitted once (tmpc_fit_path); every tick track_path
    (window_segments = 3) -> path_velocity_window -> scatter of the 27 spline columns and of the 12 spline_v columns from the stack's
    parameter map -> solve, with the spline and spline_v columns of the uploaded rows holding a sentinel.  HOST, on a second handle of the
    same library: modules.track_path, path_velocity_window, path_velocity_set_parameters, set_batch.  Each tick the robot of a scene moves to
    node 1 of its entry 0's plan of the host loop.  Parameters bit-equal every tick; exit codes, iteration counts and trajectories bitwise
    equal (same library, same inputs); v_ref equals path_velocity_at.  Conditions: the window start of a scene advances; the window of a
    scene straddles its path's end; at least half of all solves succeed."""
    import torch
    from mpc_planner_amd import solver, modules as md
    from test_gpu_parity import _generated_lib
    path, meta = _generated_lib("path_velocity")
    assert meta["npar"] == 63 and meta["nh"] == 2
    sc = _gen_scenes()
    fits = sc["fits"]
    base, spl, vcols = _base_params(meta, sc)
    assert len(spl) == 27 and len(vcols) == 12
    pm = _Params(meta["parameter_map"])
    dims = solver.default_dims(N=N, lib_path=path)
    dev, host = solver.BatchedSolver(dims, B_max=B_GEN, lib_path=path), solver.BatchedSolver(dims, B_max=B_GEN, lib_path=path)
    t = _device_paths(dev, sc)
    scene_of = np.repeat(np.arange(Q_GEN, dtype=np.int32), 2)
    t_sc, t_flag = _up(scene_of), _up(np.array(HAS_PROFILE, np.uint8))
    t_seg = _full((Q_GEN,), -1, torch.int32)                                  # new paths: the global search on the first tick
    t_cs, t_win = _full((Q_GEN,), SENTINEL, torch.float64), _full((Q_GEN, S_GEN, 9), SENTINEL, torch.float64)
    t_vwin, t_vref = _full((Q_GEN, S_GEN, 4), SENTINEL, torch.float64), _full((Q_GEN,), SENTINEL, torch.float64)
    state = sc["state"].copy()
    seg_prev = np.full(Q_GEN, -1)
    seg_hist, straddles, codes = [], False, []
    for tick in range(TICKS):
        # ---- host: the mirrors ----
        host_p = base.copy()
        tracked = []
        for q in range(Q_GEN):
            tr = md.track_path(fits[q]["path"], fits[q]["length"], state[q, :2], S_GEN, segment=int(seg_prev[q]), search_range=2)
            vwin = md.path_velocity_window(fits[q]["velocity"] if HAS_PROFILE[q] else None, fits[q]["count"], tr["segment"], S_GEN, REF_V)
            tr["v_ref"] = md.path_velocity_at(fits[q]["velocity"] if HAS_PROFILE[q] else None, fits[q]["path"], fits[q]["count"], fits[q]["length"], tr["s"], REF_V)
            straddles |= bool(HAS_PROFILE[q] and tr["segment"] + S_GEN > fits[q]["count"] and (vwin[-1] == 0.0).all())
            state[q, 4] = tr["s"]                                           # state.set("spline", closest_s)
            for b in (2 * q, 2 * q + 1):
                host_p[b][:, spl] = tr["window"].ravel()
                md.path_velocity_set_parameters(pm, host_p[b], vwin)
            tracked.append(tr)
        xinit = np.repeat(state, 2, axis=0)
        x0 = np.stack([md.initialize_with_forward_propagation(x, N, 0.2) for x in xinit])
        assert not (host_p == SENTINEL).any()
        host.set_batch(xinit, x0, host_p); host.solve(); ref = host.get()
        # ---- device ----
        dev.set_batch(xinit, x0, base)
        t_pos = _up(state)
        _device_tick(dev, t, t_pos, t_seg, t_cs, t_win, t_vwin, t_vref, t_flag, t_sc, spl, vcols)
        dev.synchronize()
        got = dev.get()
        seg_dev = t_seg.cpu().numpy()
        assert seg_dev.tolist() == [tr["segment"] for tr in tracked]
        assert np.array_equal(t_cs.cpu().numpy(), np.array([tr["s"] for tr in tracked]))
        assert np.array_equal(t_vref.cpu().numpy(), np.array([tr["v_ref"] for tr in tracked]))
        assert np.array_equal(dev.debug_get_params(), host_p)
        ok = ref["exit_code"] == 1
        print(f"[path velocity loop] tick {tick}: segments {seg_dev.tolist()}, v_ref {t_vref.cpu().numpy().round(4).tolist()}, successes {ok.sum()} / {B_GEN}, "
              f"terminal v {ref['xtraj'][:, -1, 3].round(3).tolist()}")
        for key in ("exit_code", "sqp_iter", "qp_iter_total", "xtraj", "utraj", "pobj"):
            assert np.array_equal(got[key], ref[key]), key
        codes.append(ref["exit_code"].copy())
        seg_hist.append(seg_dev.tolist())
        seg_prev = seg_dev.copy()
        state = ref["xtraj"][0::2, 1, :].copy()                              # node 1 of entry 0's plan
    seg_hist = np.array(seg_hist)
    print(f"[path velocity loop] window starts per tick: {seg_hist.tolist()}")
    assert (np.diff(seg_hist, axis=0) > 0).any()                             # a window start advances
    assert straddles
    assert (np.concatenate(codes) == 1).mean() >= 0.5
    dev.close(); host.close()


def test_the_profile_is_really_tracked():
    """The same scenes through the device pipeline, once with a constant 0.6 m/s profile at every waypoint and once with 1.8 m/s (every scene
    has a profile): the mean terminal v over the successful solves is strictly larger in the second run.  The direction only."""
    import torch
    from mpc_planner_amd import solver
    from test_gpu_parity import _generated_lib
    path, meta = _generated_lib("path_velocity")
    dims = solver.default_dims(N=N, lib_path=path)
    from mpc_planner_amd import modules as md
    mean_v = []
    for profile in (0.6, 1.8):
        sc = _gen_scenes(profile)
        base, spl, vcols = _base_params(meta, sc)
        dev = solver.BatchedSolver(dims, B_max=B_GEN, lib_path=path)
        t = _device_paths(dev, sc)
        xinit = np.repeat(sc["state"], 2, axis=0)
        x0 = np.stack([md.initialize_with_forward_propagation(x, N, 0.2) for x in xinit])
        dev.set_batch(xinit, x0, base)
        t_sc, t_pos, t_seg = _up(np.repeat(np.arange(Q_GEN, dtype=np.int32), 2)), _up(sc["state"]), _full((Q_GEN,), -1, torch.int32)
        t_cs, t_win = _full((Q_GEN,), SENTINEL, torch.float64), _full((Q_GEN, S_GEN, 9), SENTINEL, torch.float64)
        t_vwin, t_vref = _full((Q_GEN, S_GEN, 4), SENTINEL, torch.float64), _full((Q_GEN,), SENTINEL, torch.float64)
        _device_tick(dev, t, t_pos, t_seg, t_cs, t_win, t_vwin, t_vref, None, t_sc, spl, vcols)
        dev.synchronize()
        got = dev.get()
        ok = got["exit_code"] == 1
        assert ok.any() and np.allclose(t_vref.cpu().numpy(), profile, rtol=0, atol=1e-12)       # a natural spline through constant values
        mean_v.append(got["xtraj"][ok, -1, 3].mean())
        print(f"[path velocity] profile {profile}: successes {ok.sum()} / {B_GEN}, mean terminal v {mean_v[-1]:.4f}")
        dev.close()
    assert mean_v[1] > mean_v[0]
