"""GPU: the reference path tracked on device (tmpc_track_path, tmpc_set_path_parameters; csrc/tmpc_aux_kernels.hpp) -- Contouring::update
on a whole path (contouring.cpp:28-48, :94-124): closest point, segment window, spline rows.  The kernels against the host mirrors
(mpc_planner_amd/modules.py find_closest_point / path_window / track_path, pinned on hand-derived values in tests/test_path_tracking.py) bit
for bit, the standard tests/test_gpu_obstacles.py holds the obstacle kernels to, and a closed loop of ten ticks in which the window moves
along a 12-segment path without a host round trip (tolerances of tests/test_gpu_road.py's five-tick loop)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
N, M, S = 20, 8, 5
ROW_TOL = 1e-14          # rows derived from the warm start on device vs mirror: the line of tests/test_gpu_road.py


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda"))


@pytest.mark.parametrize("with_bounds", [False, True])
def test_device_tracking_equals_the_mirror_bitwise(with_bounds):
    """Seven scenes in one launch, n_seg_max = 70 (tests/path_cases.py): counts 1, 3 < S, 12, 70 (two candidates on some lanes), 0, 12, 75
    (clipped); previous segments -1, -1, 4, -1, -1, 99 (clamped), 68; positions before the start, beyond the end, on a knot, generic.
    Integers equal, floats np.array_equal; the count-0 scene keeps its prefill."""
    import torch
    import path_cases as pc
    from mpc_planner_amd import solver
    case = pc.bitwise_scenes()
    want = pc.mirror(case, with_bounds)
    n_sc = len(case["count"])
    s = solver.BatchedSolver(solver.default_dims(N=N, S=S, n_lin=M, M=M), B_max=4)          # no batch: S and the stream only
    dev = torch.device("cuda")
    t_path, t_cnt, t_len, t_pos = _up(case["path"]), _up(case["count"]), _up(case["length"]), _up(case["pos"])
    t_bounds = _up(case["bounds"])
    t_seg = _up(case["segment"].copy())
    t_s = torch.full((n_sc,), -3.0, dtype=torch.float64, device=dev); t_win = torch.full((n_sc, S, 9), -3.0, dtype=torch.float64, device=dev)
    t_bw = torch.full((n_sc, 2, S, 8), -3.0, dtype=torch.float64, device=dev); t_reached = torch.full((n_sc,), 7, dtype=torch.uint8, device=dev)
    s.track_path(n_sc, pc.N_SEG_MAX, t_path.data_ptr(), t_cnt.data_ptr(), t_len.data_ptr(), t_pos.data_ptr(), 4, t_seg.data_ptr(), t_s.data_ptr(),
                 t_win.data_ptr(), d_bounds=t_bounds.data_ptr() if with_bounds else None, d_bound_window=t_bw.data_ptr() if with_bounds else None,
                 d_reached=t_reached.data_ptr(), search_range=pc.SEARCH_RANGE)
    s.synchronize()
    got = dict(segment=t_seg.cpu().numpy(), s=t_s.cpu().numpy(), window=t_win.cpu().numpy(), bound_window=t_bw.cpu().numpy(),
               reached=t_reached.cpu().numpy())
    print(f"[path] bounds {with_bounds}: segments {got['segment'].tolist()} (mirror {want['segment'].tolist()}), s {got['s'].tolist()}, "
          f"max |s - mirror| {np.abs(got['s'] - want['s']).max():.3e}, max |window - mirror| {np.abs(got['window'] - want['window']).max():.3e}, "
          f"reached {got['reached'].tolist()}")
    assert want["segment"].tolist() == [0, 2, 4, 66, -1, 10, 69]         # (what the cases are meant to reach: the mirror's own answers)
    for key in ("segment", "s", "window", "bound_window", "reached"):
        assert np.array_equal(got[key], want[key]), key
    assert (got["window"][4] == -3.0).all() and got["s"][4] == -3.0 and got["reached"][4] == 7 and got["segment"][4] == -1
    assert (got["window"][1, 1:, 8] == 6.0).all()                        # count 3 < S found at its last segment: four padded slots
    # without d_reached the same answers; a local search that cannot see the closest segment stays inside its range
    t_seg2 = _up(np.array([-1, -1, 0, 3, -1, 0, 0], np.int32)); t_win.fill_(-3.0)
    s.track_path(n_sc, pc.N_SEG_MAX, t_path.data_ptr(), t_cnt.data_ptr(), t_len.data_ptr(), t_pos.data_ptr(), 4, t_seg2.data_ptr(), t_s.data_ptr(),
                 t_win.data_ptr(), search_range=1)
    s.synchronize()
    case2 = dict(case, segment=np.array([-1, -1, 0, 3, -1, 0, 0], np.int32))
    want2 = pc.mirror(case2, False, search_range=1)
    assert want2["segment"].tolist() == [0, 2, 1, 4, -1, 1, 1]
    assert np.array_equal(t_seg2.cpu().numpy(), want2["segment"]) and np.array_equal(t_s.cpu().numpy(), want2["s"])
    assert np.array_equal(t_win.cpu().numpy(), want2["window"])
    s.close()


@pytest.mark.parametrize("slack", [0, 1])
def test_parameter_writer_touches_the_spline_columns_only(slack):
    """Twelve entries, two scenes: the 9 S spline columns of every stage of the named entries equal modules.contouring_set_parameters of the
    mirror's window, every other column keeps its -3.0 prefill, entries with scene_of = -1 or beyond n_scenes are untouched; d_state's spline
    column is set and nothing else.  Both parameter strides (slack 0 / 1)."""
    import torch
    import path_cases as pc
    from mpc_planner_amd import scenes, solver, modules as md
    kw = dict(slack=True, n_decomp=12) if slack else {}
    sc = scenes.make_scene(90, N=N, M=M, B=12, **kw)
    pm = sc["pm"]
    B, nx = 12, 5 + slack
    dims = solver.default_dims(N=N, S=S, n_lin=M, M=M, n_slk=12 if slack else 0, slack=slack)
    assert dims.npar == pm.length()
    case = pc.bitwise_scenes()
    windows = np.stack([md.path_window(case["path"][3, :70], 140.0, 31, S), md.path_window(case["path"][1, :3], 6.0, 1, S)])
    closest = np.array([63.25, 2.5])
    scene_of = np.array([0, 0, 0, 0, -1, -1, 2, 7, 1, 1, 0, 1], np.int32)
    so = solver.BatchedSolver(dims, B_max=B)
    so.set_batch(sc["xinit"], sc["x0"], np.full_like(sc["params"], -3.0))
    t_win, t_sc, t_cs = _up(windows), _up(scene_of), _up(closest)
    t_state = _up(np.full((B, nx), 9.0))
    so.set_path_parameters(t_win.data_ptr(), t_sc.data_ptr(), 2)         # without the state
    so.synchronize()
    want = np.full_like(sc["params"], -3.0)
    weight_cols = [pm.index(n) for n in ("contour", "lag", "terminal_angle", "terminal_contouring")]
    for b in range(B):
        if 0 <= scene_of[b] < 2:
            md.contouring_set_parameters(pm, want[b], scenes.WEIGHTS, windows[scene_of[b]])
            want[b][:, weight_cols] = -3.0                                # (the writer does not touch the weights)
    got = so.debug_get_params()
    assert np.array_equal(got, want)
    assert (got[[4, 5, 6, 7]] == -3.0).all() and (got != -3.0).sum() == 8 * N * 9 * S
    assert (t_state.cpu().numpy() == 9.0).all()
    so.set_path_parameters(t_win.data_ptr(), t_sc.data_ptr(), 2, d_closest_s=t_cs.data_ptr(), d_state=t_state.data_ptr())
    so.synchronize()
    assert np.array_equal(so.debug_get_params(), want)
    st = np.full((B, nx), 9.0)
    for b in range(B):
        if 0 <= scene_of[b] < 2:
            st[b, 4] = closest[scene_of[b]]
    assert np.array_equal(t_state.cpu().numpy(), st)
    so.close()


def _bounds_of(path, dl, dr):
    left, right = path[:, :8].copy(), path[:, :8].copy()
    left[:, 7] += dl; right[:, 7] -= dr
    return left, right


def test_closed_loop_ten_ticks_the_window_moves_without_host_round_trip():
    """track_path -> set_path_parameters -> warmstart -> road_halfspaces (bounds mode, from d_bound_window) -> init_with_guidance ->
    linearize_topology_ex -> solve -> select -> gather, ten ticks, 3 sets x 16 trajectories, parameter sharing on, 12 x 2 m paths moved so
    that the robots start 0.05, 0.3 and 0.6 m before the first interior knot; nothing is read back before the solve is enqueued.  Then the
    same tick is rebuilt on the host from debug_get_x0() and the mirrors and solved on a second handle (tolerances of
    tests/test_gpu_road.py::test_closed_loop_five_ticks_without_host_round_trip).  Every set's window start must increase at least once
    and never decrease, and the spline columns before and after that tick differ."""
    import torch
    from mpc_planner_amd import scenes, solver, modules as md
    n_sets, traj, ticks, n_seg = 3, 16, 10, 12
    r = scenes.ROBOT_RADIUS
    scs, full_bounds = [], []
    for i, before_knot in enumerate((0.05, 0.3, 0.6)):
        sc = scenes.with_long_path(scenes.make_scene(80 + i, N=N, M=M, B=traj), np.random.default_rng(80 + i), n_segments=n_seg, seg_len=2.0,
                                   shift=2.0 - before_knot)
        assert sc["path_segment"] == 0
        lb, rb = _bounds_of(sc["path"], 2.0, 2.0)
        _, wl, wr = md.path_window(sc["path"], sc["path_length"], 0, S, lb, rb)
        scs.append(scenes.add_road_constraints(sc, 4.0, left=wl, right=wr)); full_bounds.append(np.stack([lb, rb]))
    xinit = np.concatenate([s_["xinit"] for s_ in scs]); x0 = np.concatenate([s_["x0"] for s_ in scs]); params = np.concatenate([s_["params"] for s_ in scs])
    scene_of = np.repeat(np.arange(n_sets, dtype=np.int32), traj); lead = np.arange(n_sets) * traj
    B = n_sets * traj
    pm = scs[0]["pm"]
    spl = np.array([pm.index(n.format(i)) for i in range(S) for n in ("spline_x{}_a", "spline_x{}_b", "spline_x{}_c", "spline_x{}_d",
                                                                       "spline_y{}_a", "spline_y{}_b", "spline_y{}_c", "spline_y{}_d", "spline{}_start")])
    obst = np.ascontiguousarray(np.stack([sc["obstacles"]["pos"] for sc in scs]))
    gpos0 = np.concatenate([sc["guidance_pos"] for sc in scs]); gvel = np.concatenate([sc["guidance_vel"] for sc in scs])
    paths = np.stack([sc["path"] for sc in scs]); lengths = np.array([sc["path_length"] for sc in scs]); full_bounds = np.stack(full_bounds)
    dims = solver.default_dims(N=N, S=S, n_lin=M + 2, M=M)
    own = solver.own_parameter_columns(dims)
    dev = torch.device("cuda")
    s = solver.BatchedSolver(dims, B_max=B)
    ref_s = solver.BatchedSolver(dims, B_max=B)
    # device state: garbage in everything the device has to produce; the shared rows in the lead entries only, their spline columns garbage too
    t_xinit = _up(xinit.copy())
    t_x0 = _up(np.repeat(x0[lead], traj, axis=0).reshape(B, -1))          # every planner starts as a copy of the main solver
    p0 = np.full_like(params, -3.0); p0[lead] = params[lead]; p0[:, :, spl] = -3.0
    t_params = _up(p0.reshape(B, -1))
    s.set_batch_device(B, t_xinit.data_ptr(), t_x0.data_ptr(), t_params.data_ptr())
    base_of = np.repeat(lead, traj).astype(np.int32)
    s.set_param_sharing(base_of)
    t_lead = _up(lead.astype(np.int32)); t_base = _up(base_of)
    t_gpos0 = _up(gpos0); t_gvel = _up(gvel); t_ob = _up(obst); t_sc = _up(scene_of)
    t_stat = torch.zeros((n_sets, N, 2, 3), dtype=torch.float64, device=dev)
    t_state = _up(xinit.copy()); t_sx = t_state[t_lead.long(), 0].contiguous()
    t_gp = t_gpos0.clone(); t_src = t_base.clone()
    t_rec = torch.zeros((B, 2), dtype=torch.int64, device=dev); t_best = torch.full((n_sets,), -2, dtype=torch.int32, device=dev)
    t_wx = torch.zeros((n_sets, (N + 1) * 5), dtype=torch.float64, device=dev); t_wu = torch.zeros((n_sets, N * 2), dtype=torch.float64, device=dev)
    # the paths, uploaded once
    t_path, t_cnt, t_len, t_fb = _up(paths), _up(np.full(n_sets, n_seg, np.int32)), _up(lengths), _up(full_bounds)
    t_seg = torch.full((n_sets,), -1, dtype=torch.int32, device=dev)      # a new path: global search on the first tick
    t_cs = torch.zeros(n_sets, dtype=torch.float64, device=dev); t_win = torch.zeros((n_sets, S, 9), dtype=torch.float64, device=dev)
    t_bw = torch.zeros((n_sets, 2, S, 8), dtype=torch.float64, device=dev)
    hs = torch.cuda.ExternalStream(s.stream_ptr(), device=dev)
    torch.cuda.synchronize()
    seg_prev = np.full(n_sets, -1)
    seg_hist, spl_before, moved = [], None, np.zeros(n_sets, bool)
    for tick in range(ticks):
        # ---- device: everything stream-ordered on the handle's stream, nothing read back before the solve is enqueued ----
        with torch.cuda.stream(hs):
            if tick > 0:
                # the robot moved one step along the set's selected plan (no winner: the lead planner's); every planner restarts from it
                win = torch.where(t_best >= 0, t_best, torch.zeros_like(t_best)).long() + t_lead.long()
                node1 = t_wx.view(n_sets, N + 1, 5)[:, 1, :]
                t_state.copy_(torch.where((t_best >= 0)[:, None], node1, t_x0.view(B, N + 1, 7)[t_lead.long(), 1, 2:7]).repeat_interleave(traj, 0))
                t_src.copy_(win.to(torch.int32).repeat_interleave(traj, 0))
                t_sx.copy_(t_state[t_lead.long(), 0])
                t_gp.copy_(t_gpos0 + (t_state[:, None, 0:2] - t_gpos0[:, 0:1, :]))            # the guidance trajectories start at the robot
            # the lead entry's state row stands for its scene: pos_stride = traj x 5 doubles
            s.track_path(n_sets, n_seg, t_path.data_ptr(), t_cnt.data_ptr(), t_len.data_ptr(), t_state.data_ptr(), traj * 5, t_seg.data_ptr(),
                         t_cs.data_ptr(), t_win.data_ptr(), d_bounds=t_fb.data_ptr(), d_bound_window=t_bw.data_ptr())
            s.set_path_parameters(t_win.data_ptr(), t_sc.data_ptr(), n_sets, d_closest_s=t_cs.data_ptr(), d_state=t_state.data_ptr())
            if tick > 0:
                s.warmstart(t_state.data_ptr(), None, t_src.data_ptr())
            s.road_halfspaces(t_lead.data_ptr(), n_sets, r, r, t_stat.data_ptr(), 2, first_row=0, d_bound_segments=t_bw.data_ptr())
            s.init_with_guidance(t_gp.data_ptr(), t_gvel.data_ptr())
            s.linearize_topology_ex(t_ob.data_ptr(), M, t_sc.data_ptr(), t_sx.data_ptr(), r, d_static_halfspaces=t_stat.data_ptr(), n_static=2)
            s.solve(sync=False)
            s.pack_records(t_rec.data_ptr()); s.select_best_records(t_rec.data_ptr(), 1, n_sets, traj, t_best.data_ptr())
            s.gather_best(t_best.data_ptr(), n_sets, traj, t_wx.data_ptr(), t_wu.data_ptr())
        # ---- host: the same tick from the device's warm start and the mirrors ----
        s.synchronize()
        got = s.get()
        x0_dev, xinit_dev = s.debug_get_x0()
        p_dev = s.debug_get_params()
        rows_dev = t_stat.cpu().numpy(); state_dev = t_state.cpu().numpy()
        seg_dev, cs_dev, win_dev, bw_dev = t_seg.cpu().numpy(), t_cs.cpu().numpy(), t_win.cpu().numpy(), t_bw.cpu().numpy()
        host = np.zeros_like(params)
        for q in range(n_sets):
            tr = md.track_path(paths[q], lengths[q], state_dev[lead[q], :2], S, segment=int(seg_prev[q]), search_range=2,
                               left=full_bounds[q, 0], right=full_bounds[q, 1])
            assert seg_dev[q] == tr["segment"] and cs_dev[q] == tr["s"]
            assert np.array_equal(win_dev[q], tr["window"]) and np.array_equal(bw_dev[q, 0], tr["left"]) and np.array_equal(bw_dev[q, 1], tr["right"])
            assert (state_dev[lead[q]:lead[q] + traj, 4] == tr["s"]).all()
            if tick > 0:                                                 # warmstart after the writer: the solve starts from the fresh closest_s
                assert (xinit_dev[lead[q]:lead[q] + traj, 4] == tr["s"]).all()
            rows = md.road_halfspaces_from_bounds(tr["window"], tr["left"], tr["right"], x0_dev[lead[q], :N, 6], r)
            np.testing.assert_allclose(rows_dev[q, 1:], rows[1:], rtol=ROW_TOL, atol=ROW_TOL)
            for b in range(lead[q], lead[q] + traj):
                host[b] = params[lead[q]]                                # shared rows: the lead entry's
                md.contouring_set_parameters(pm, host[b], scenes.WEIGHTS, tr["window"])
                lin = md.linearized_update(x0_dev[b], obst[q], r, static=rows)
                md.linearized_set_parameters(pm, host[b], xinit_dev[lead[q], 0], lin, n_rows=M + 2)
        assert np.array_equal(p_dev[:, :, spl], host[:, :, spl])          # every entry of a set carries the window: the sharing map stays valid
        np.testing.assert_allclose(p_dev[:, :, own], host[:, :, own], rtol=1e-14, atol=1e-14)
        np.testing.assert_allclose(p_dev[lead], host[lead], rtol=1e-14, atol=1e-14)
        if tick > 0:
            assert (seg_dev >= seg_prev).all()                           # never back
            stepped = seg_dev > seg_prev
            for q in np.nonzero(stepped)[0]:                             # the tick the window moved: other spline columns
                assert not np.array_equal(p_dev[lead[q]][:, spl], spl_before[lead[q]])
            moved |= stepped
        seg_hist.append(seg_dev.tolist())
        seg_prev, spl_before = seg_dev.copy(), p_dev[:, :, spl].copy()
        ref_s.set_batch(xinit_dev, x0_dev, host); ref_s.solve(); ref = ref_s.get()
        ref_best = [ref_s.select_best(first=int(l), count=traj) for l in lead]
        ok = ref["exit_code"] == 1
        differ = (got["qp_iter_total"][ok] != ref["qp_iter_total"][ok]).mean() if ok.any() else 0.0
        print(f"[path loop] tick {tick}: segments {seg_dev.tolist()}, closest_s {cs_dev.tolist()}, successes {ok.sum()} / {B}, "
              f"qp_iter_total differs on {differ:.3f}")
        assert (got["exit_code"] == ref["exit_code"]).all() and (got["sqp_iter"] == ref["sqp_iter"]).all()
        assert differ <= 0.05
        np.testing.assert_allclose(got["xtraj"][ok], ref["xtraj"][ok], rtol=0, atol=1e-7)
        best = t_best.cpu().numpy()
        for si in range(n_sets):
            a, b = int(best[si]), int(ref_best[si])
            assert (a < 0) == (b < 0)
            if a != b:
                assert abs(got["pobj"][lead[si] + a] - ref["pobj"][lead[si] + b]) <= 1e-9 * max(1.0, abs(ref["pobj"][lead[si] + b]))
    print(f"[path loop] window starts per tick: {seg_hist}")
    assert moved.all()
    s.close(); ref_s.close()


def test_bad_arguments_and_generated_solver():
    import ctypes as C
    import torch
    from mpc_planner_amd import scenes, solver
    sc = scenes.make_scene(80, N=N, M=M, B=4)
    dims = solver.default_dims(N=N, S=S, n_lin=M, M=M)
    s = solver.BatchedSolver(dims, B_max=4)
    dev = torch.device("cuda")
    f64 = dict(dtype=torch.float64, device=dev)
    t_path = torch.zeros((1, 4, 9), **f64); t_path[0, :, 2] = 1.0; t_path[0, :, 8] = torch.arange(4, **f64)
    t_cnt = torch.full((1,), 4, dtype=torch.int32, device=dev); t_len = torch.full((1,), 4.0, **f64); t_pos = torch.zeros((1, 2), **f64)
    t_seg = torch.full((1,), -1, dtype=torch.int32, device=dev); t_cs = torch.zeros(1, **f64); t_win = torch.zeros((1, S, 9), **f64)
    t_b = torch.zeros((1, 2, 4, 8), **f64); t_bw = torch.zeros((1, 2, S, 8), **f64)
    base = dict(n_scenes=1, n_seg_max=4, d_path=t_path.data_ptr(), d_path_count=t_cnt.data_ptr(), d_path_length=t_len.data_ptr(), d_pos=t_pos.data_ptr(),
                pos_stride=2, d_segment=t_seg.data_ptr(), d_closest_s=t_cs.data_ptr(), d_window=t_win.data_ptr())
    track = lambda **kw: s.track_path(**dict(base, **kw))
    track()                                                               # no batch needed
    s.synchronize()
    assert t_seg.item() == 0 and t_cs.item() == 0.0
    for kw, msg in ((dict(d_path=None), "NULL input"), (dict(d_path_count=None), "NULL input"), (dict(d_path_length=None), "NULL input"),
                    (dict(d_pos=None), "NULL input"), (dict(d_segment=None), "NULL output"), (dict(d_closest_s=None), "NULL output"),
                    (dict(d_window=None), "NULL output"), (dict(n_scenes=0), "n_scenes"), (dict(n_scenes=-3), "n_scenes"),
                    (dict(n_seg_max=0), "n_seg_max"), (dict(n_seg_max=1025), "n_seg_max"), (dict(search_range=-1), "search_range"),
                    (dict(search_range=32), "search_range"), (dict(pos_stride=1), "pos_stride"),
                    (dict(d_bounds=t_b.data_ptr()), "both or neither"), (dict(d_bound_window=t_bw.data_ptr()), "both or neither")):
        with pytest.raises(solver.TmpcError, match=msg):
            track(**kw)
    track(n_seg_max=1024, n_scenes=1, search_range=31, d_path_count=torch.zeros(1, dtype=torch.int32, device=dev).data_ptr())    # the limits themselves (count 0: nothing read)
    # the options struct: a short size, a longer one with a zero / non-zero tail; NULL = the defaults
    vp = lambda p_: C.c_void_p(p_) if p_ else None
    raw_call = lambda opt: s.lib.tmpc_track_path(s._h, 1, 4, vp(base["d_path"]), vp(base["d_path_count"]), vp(base["d_path_length"]), None,
                                                 vp(base["d_pos"]), 2, opt, vp(base["d_segment"]), vp(base["d_closest_s"]), vp(base["d_window"]), None, None)
    assert raw_call(None) == 0
    assert raw_call(C.byref(solver.TmpcPathOptions(4, 2))) == -1
    buf = (C.c_char * 16)(); C.memmove(buf, bytes(solver.TmpcPathOptions(16, 2)), 8)
    assert raw_call(C.cast(buf, C.POINTER(solver.TmpcPathOptions))) == 0
    buf[12] = b"\x01"
    assert raw_call(C.cast(buf, C.POINTER(solver.TmpcPathOptions))) == -1
    assert s.lib.tmpc_track_path(None, 1, 4, None, None, None, None, None, 2, None, None, None, None, None, None) == -1      # no handle
    # the parameter writer needs a batch
    t_sc = torch.zeros(4, dtype=torch.int32, device=dev); t_state = torch.zeros((4, 5), **f64)
    with pytest.raises(solver.TmpcError, match="no batch"):
        s.set_path_parameters(t_win.data_ptr(), t_sc.data_ptr(), 1)
    s.set_batch(sc["xinit"], sc["x0"], sc["params"])
    s.set_path_parameters(t_win.data_ptr(), t_sc.data_ptr(), 1)
    for args, kw, msg in (((None, t_sc.data_ptr(), 1), {}, "bad argument"), ((t_win.data_ptr(), None, 1), {}, "bad argument"),
                          ((t_win.data_ptr(), t_sc.data_ptr(), 0), {}, "bad argument"),
                          ((t_win.data_ptr(), t_sc.data_ptr(), 1), dict(d_closest_s=t_cs.data_ptr()), "both or neither"),
                          ((t_win.data_ptr(), t_sc.data_ptr(), 1), dict(d_state=t_state.data_ptr()), "both or neither")):
        with pytest.raises(solver.TmpcError, match=msg):
            s.set_path_parameters(*args, **kw)
    assert s.lib.tmpc_set_path_parameters(None, None, None, 1, None, None) == -1
    s.synchronize(); s.close()
    # a generated solver refuses both, like tmpc_road_halfspaces does: its parameter layout is the module stack's
    path = os.path.join(os.path.dirname(HERE), "build", "generated", "libtmpc_hip_tmpc_cfg2.so")
    if not os.path.exists(path):
        import __graft_entry__ as g
        g.build_generated_demo()
    d = solver.default_dims(N=N, lib_path=path)
    sg = solver.BatchedSolver(d, B_max=4, lib_path=path)
    sg.set_batch(sc["xinit"], sc["x0"], sc["params"])
    with pytest.raises(solver.TmpcError, match="generated solver"):
        sg.track_path(**base)
    with pytest.raises(solver.TmpcError, match="generated solver"):
        sg.set_path_parameters(t_win.data_ptr(), t_sc.data_ptr(), 1)
    sg.close()
