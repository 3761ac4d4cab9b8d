"""GPU: the static environment of a generated stack by column, include/tmpc_hip_stack_env.h (csrc/tmpc_row_entries.hpp;
mpc_planner_amd/stack_env.py) -- the path window, the road rows and the free-space (decomp) rows.

1. On the product library the column entries, given the hand-written layout's own columns, leave the parameter rows, the road buffer and the
   state bit-equal to tmpc_set_path_parameters, tmpc_road_halfspaces (three modes) and tmpc_set_halfspace_rows, and touch nothing else.
2. On the generated road_decomp library they equal the numpy mirrors (path window, road rows) and the product library's decomposition, also with
   the columns permuted within the table.
3. Three ticks of that stack with every row built on device, against the same ticks built by the mirrors on the host and solved on a second handle.
4. Every refusal, with its message and without a launch; the entries of tmpc_hip.h keep refusing in a generated solver.
Every comparison is np.array_equal: both sides run the same arithmetic in the same order."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
N = 20


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda"))


def _full(shape, value, dtype):
    import torch
    return torch.full(shape, value, dtype=dtype, device=torch.device("cuda"))


def _sentinel_rows(B, n, npar):
    """A different negative value in every entry: a column written by mistake, or from the wrong place, cannot pass for untouched."""
    return -(1.0e3 + np.arange(B * n * npar, dtype=np.float64)).reshape(B, n, npar)


def _bound_cubics(path, dl, dr):
    """Left / right bound cubics [n][8] on the path's knots: the centreline moved sideways in y."""
    left, right = path[:, :8].copy(), path[:, :8].copy()
    left[:, 7] += dl; right[:, 7] -= dr
    return left, right


def _road_modes():
    from mpc_planner_amd import modules as md, scenes
    r = scenes.ROBOT_RADIUS
    return (("centreline", md.road_offsets(4.0, r)), ("two_way", md.road_offsets(5.0, r, True)), ("bounds", (r, r)))


def _tracked(positions, S):
    """The fitted path of tests/free_space_cases.py (11 segments), tracked from a reset at each position: the mirror's windows."""
    import free_space_cases as fs
    from mpc_planner_amd import modules as md
    fit = fs.fitted_path()
    left, right = _bound_cubics(fit["path"], 2.0, 1.5)
    return fit, left, right, [md.track_path(fit["path"], fit["length"], p, S, segment=-1, left=left, right=right) for p in positions]


# ---- 1. the product library: the same inputs through the layout entries and through the column entries ---------------------------------------
def test_column_entries_equal_the_layout_entries_on_the_product_library():
    """Two handles of libtmpc_hip.so (N = 20, S = 5, 10 topology rows, 8 obstacles, 12 slack rows, slack model), 8 entries over 3 scenes, the rows
    prefilled with a sentinel pattern.  Entry 5 names a scene outside [0, 3) and scene 2's main entry lies outside the batch: both are left
    alone by both forms.  The slack rows 2 .. 8 are written (first_row = 2 on the layout side, their columns on the other)."""
    import free_space_cases as fs
    from mpc_planner_amd import solver
    from mpc_planner_amd.parameters import define_parameters
    from mpc_planner_amd.stack_env import StackEnvironment, decomp_columns, path_columns
    S, B, Q, n_rows, first_row = 5, 8, 3, 7, 2
    dims = solver.default_dims(N=N, S=S, n_lin=10, M=8, n_slk=12, slack=1)
    pm = define_parameters(S, 8, add_halfspaces=2, slack=True, n_decomp=12)._params
    assert len(pm) == dims.npar and dims.nvar == 8
    pcols, dall = path_columns(pm, S), decomp_columns(pm, 12)
    dcols = [dall[0]] + dall[1 + 3 * first_row:1 + 3 * (first_row + n_rows)]
    rng = np.random.default_rng(11)
    way = fs.waypoints()
    fit, left, right, tracked = _tracked([way[1] + [0.1, -0.2], way[3] + [-0.2, 0.3], way[6]], S)
    window = np.stack([t["window"] for t in tracked])
    bounds = np.stack([np.stack([t["left"], t["right"]]) for t in tracked])                          # [Q][2][S][8]
    closest_s = np.array([t["s"] for t in tracked])
    scene_of = np.array([0, 1, 2, 0, 1, 7, 2, 0], np.int32)
    main_of = np.array([3, 1, 99], np.int32)
    xinit, x0 = rng.normal(size=(B, 6)), rng.normal(size=(B, N + 1, 8))
    for b in range(B):                                                                               # below the first knot of the window, through it, beyond it
        x0[b, :, 6] = closest_s[scene_of[b] % Q] - 0.6 + 0.37 * np.arange(N + 1) + rng.normal(0.0, 0.05, N + 1)
    rows = rng.normal(size=(Q, N, n_rows, 3))
    start = _sentinel_rows(B, N, dims.npar)
    state0 = -(7.0 + np.arange(B * 6, dtype=np.float64)).reshape(B, 6)
    fill = rng.normal(size=(Q, N, 3, 3))
    a, b_ = solver.BatchedSolver(dims, B_max=B), solver.BatchedSolver(dims, B_max=B)
    env = StackEnvironment(b_)
    t_win, t_sc, t_main, t_cs, t_bounds, t_rows = _up(window), _up(scene_of), _up(main_of), _up(closest_s), _up(bounds), _up(rows)
    got = {}
    for name, s in (("layout", a), ("columns", b_)):
        s.set_batch(xinit, x0, start)
        t_state = _up(state0)
        t_stat = {mode: _up(fill) for mode, _ in _road_modes()}
        if name == "layout":
            s.set_path_parameters(t_win.data_ptr(), t_sc.data_ptr(), Q, d_closest_s=t_cs.data_ptr(), d_state=t_state.data_ptr())
        else:
            env.set_path_columns(pcols, t_win.data_ptr(), t_sc.data_ptr(), Q, d_closest_s=t_cs.data_ptr(), d_state=t_state.data_ptr())
        for mode, offs in _road_modes():
            kw = dict(first_row=1, d_bound_segments=t_bounds.data_ptr() if mode == "bounds" else None)
            if name == "layout":
                s.road_halfspaces(t_main.data_ptr(), Q, offs[0], offs[1], t_stat[mode].data_ptr(), 3, **kw)
            else:
                env.road_halfspaces(pcols, t_main.data_ptr(), Q, offs[0], offs[1], t_stat[mode].data_ptr(), 3, **kw)
        if name == "layout":
            s.set_halfspace_rows(t_rows.data_ptr(), n_rows, t_sc.data_ptr(), Q, first_row=first_row, disc_offset=0.07)
        else:
            env.set_halfspace_columns(dcols, t_rows.data_ptr(), t_sc.data_ptr(), Q, disc_offset=0.07)
        s.synchronize()
        got[name] = dict(params=s.debug_get_params(), state=t_state.cpu().numpy(), **{mode: t.cpu().numpy() for mode, t in t_stat.items()})
    lay, col = got["layout"], got["columns"]
    named = sorted(pcols + dcols)
    rest = np.setdiff1d(np.arange(dims.npar), named)
    valid = np.nonzero((scene_of >= 0) & (scene_of < Q))[0]
    print(f"[stack env] product library: {len(named)} named columns of {dims.npar}, rows bitwise equal {np.array_equal(lay['params'], col['params'])}, "
          + ", ".join(f"{mode} road bitwise equal {np.array_equal(lay[mode], col[mode])}" for mode, _ in _road_modes()))
    assert np.array_equal(col["params"], lay["params"])
    assert np.array_equal(col["params"][:, :, rest], start[:, :, rest]) and len(rest) > 0
    assert (col["params"][valid][:, :, named] != start[valid][:, :, named]).all()
    assert np.array_equal(col["params"][5], start[5])                                                # the entry of no scene
    assert np.array_equal(col["params"][0][:, pcols], np.tile(window[0].reshape(-1), (N, 1)))
    assert np.array_equal(col["state"], lay["state"])
    want_state = state0.copy(); want_state[valid, 4] = closest_s[scene_of[valid]]
    assert np.array_equal(col["state"], want_state)
    for mode, _ in _road_modes():
        assert np.array_equal(col[mode], lay[mode])
        assert np.array_equal(col[mode][2], fill[2]) and np.array_equal(col[mode][:, 0], fill[:, 0]) and np.array_equal(col[mode][:, :, 0], fill[:, :, 0])
        assert (col[mode][:2, 1:, 1:3] != fill[:2, 1:, 1:3]).all()
    assert not np.array_equal(col["centreline"], col["two_way"]) and not np.array_equal(col["centreline"], col["bounds"])
    a.close(); b_.close()


# ---- 2. the generated road_decomp library -------------------------------------------------------------------------------------------------------
def _generated_case():
    """B = 6 entries over 2 scenes of tests/free_space_cases.py's scattered launch (400 costmap points each, the fitted path of 11 segments: more
    than the window's 3), main entries 2 and 1."""
    import free_space_cases as fs
    from mpc_planner_amd import modules as md
    launch = fs.scattered_launch()
    Q, B, S = 2, 6, 3
    way = fs.waypoints()
    pos = np.stack([way[2] + [0.1, -0.2], way[5] + [-0.15, 0.25]])
    fit, left, right, tracked = _tracked(pos, S)
    n = fit["count"]
    assert n == 11 > S
    scene_of, main_of = np.array([0, 1, 0, 1, 0, 1], np.int32), np.array([2, 1], np.int32)
    rng = np.random.default_rng(12)
    xinit, x0 = rng.normal(size=(B, 6)), rng.normal(size=(B, N + 1, 8))
    for b in range(B):
        q = scene_of[b]
        x0[b, :, md.IDX["v"]] = launch["v"][q] + 0.01 * b
        x0[b, :, md.IDX["spline"]] = tracked[q]["s"] - 0.3 + 0.25 * np.arange(N + 1) + 0.02 * b
    bounds = np.full((Q, 2, fs.N_SEG_MAX, 8), -3.0)
    bounds[:, 0, :n], bounds[:, 1, :n] = left, right
    return dict(Q=Q, B=B, S=S, launch=launch, pos=pos, fit=fit, tracked=tracked, scene_of=scene_of, main_of=main_of, xinit=xinit, x0=x0, bounds=bounds,
                window=np.stack([t["window"] for t in tracked]), closest_s=np.array([t["s"] for t in tracked]))


def _road_want(cs, mode, offs, fill, first_row):
    from mpc_planner_amd import modules as md, scenes
    want = fill.copy()
    for q, t in enumerate(cs["tracked"]):
        s_of_k = cs["x0"][cs["main_of"][q], :N, md.IDX["spline"]]
        rows = md.road_halfspaces_from_bounds(t["window"], t["left"], t["right"], s_of_k, scenes.ROBOT_RADIUS) if mode == "bounds" \
            else md.road_halfspaces(t["window"], s_of_k, *offs)
        want[q, 1:, first_row:first_row + 2] = rows[1:]
    return want


def test_generated_road_decomp_library_equals_the_mirrors_and_the_product_decomposition():
    """libtmpc_hip_road_decomp.so (76 parameters): tmpc_track_path(window_segments = 3) -> set_path_columns equals modules.track_path's window in
    the stack's spline columns; road_halfspaces equals modules.road_halfspaces(_from_bounds) in all three modes; tmpc_stack_decomp_halfspaces
    equals the product library's tmpc_decomp_halfspaces for the same warm start and points; set_halfspace_columns puts those rows and the disc
    offset into the stack's decomp columns; every column not named keeps its sentinel.  Then again with the columns permuted within the
    table: the values follow the permutation (the table is read, not the layout) and the road rows, read back through it, stay the same."""
    import torch
    import free_space_cases as fs
    from mpc_planner_amd import solver
    from mpc_planner_amd.stack_env import StackEnvironment, decomp_columns, path_columns
    from test_gpu_parity import _generated_lib
    path, meta = _generated_lib("road_decomp")
    pmap = meta["parameter_map"]
    cs = _generated_case()
    Q, B, S, launch = cs["Q"], cs["B"], cs["S"], cs["launch"]
    n_rows, n_pts_max, first_row = 4, launch["n_pts_max"], 1
    dims = solver.default_dims(N=N, S=S, lib_path=path)
    assert meta["npar"] == dims.npar == 76 and dims.nvar == 8 and meta["spill_free"]
    pcols, dcols = path_columns(pmap, S), decomp_columns(pmap, n_rows)
    g = solver.BatchedSolver(dims, B_max=B, lib_path=path)
    env = StackEnvironment(g)
    start = _sentinel_rows(B, N, 76)
    f64, i32, u8 = torch.float64, torch.int32, torch.uint8
    t_path, t_pc, t_len = _up(launch["path"][:Q]), _up(launch["path_count"][:Q]), _up(launch["path_length"][:Q])
    t_bounds, t_pos, t_sc, t_main = _up(cs["bounds"]), _up(cs["pos"]), _up(cs["scene_of"]), _up(cs["main_of"])
    t_pts, t_cnt, t_s0, t_sx = _up(launch["points"][:Q]), _up(launch["count"][:Q]), _up(launch["s0"][:Q]), _up(launch["state_x"][:Q])
    fill = np.random.default_rng(3).normal(size=(Q, N, 3, 3))
    # the product library's decomposition of the same warm start and points
    dp = solver.default_dims(N=N, S=5, n_lin=10, M=8, n_slk=12, slack=1)
    p = solver.BatchedSolver(dp, B_max=B)
    p.set_batch(cs["xinit"], cs["x0"], np.zeros((B, N, dp.npar)))
    ref_rows, ref_count, ref_status = _full((Q, N, n_rows, 3), -3.0, f64), _full((Q, N), -3, i32), _full((Q, N), 7, u8)
    p.decomp_halfspaces(t_main.data_ptr(), Q, fs.N_SEG_MAX, t_path.data_ptr(), t_pc.data_ptr(), t_len.data_ptr(), t_s0.data_ptr(), t_sx.data_ptr(),
                        t_pts.data_ptr(), t_cnt.data_ptr(), n_pts_max, fs.RANGE, n_rows, ref_rows.data_ptr(), ref_count.data_ptr(), ref_status.data_ptr())
    p.synchronize()
    ref_rows, ref_count, ref_status = ref_rows.cpu().numpy(), ref_count.cpu().numpy(), ref_status.cpu().numpy()
    p.close()
    assert (ref_count[:, 1:] > 0).all() and (ref_status != 7).all() and not (ref_rows == -3.0).any()
    road_first = None
    for trial, perm_seed in enumerate((None, 21)):
        pc, dc = list(pcols), list(dcols)
        if perm_seed is not None:
            prng = np.random.default_rng(perm_seed)
            pc, dc = [pcols[i] for i in prng.permutation(len(pcols))], [dcols[i] for i in prng.permutation(len(dcols))]
            assert pc != pcols and dc != dcols
        g.set_batch(cs["xinit"], cs["x0"], start)
        t_seg, t_cs, t_win, t_bwin = _full((Q,), -1, i32), _full((Q,), -3.0, f64), _full((Q, S, 9), -3.0, f64), _full((Q, 2, S, 8), -3.0, f64)
        t_state = _up(cs["xinit"])
        t_stat = {mode: _up(fill) for mode, _ in _road_modes()}
        t_rows, t_count, t_status = _full((Q, N, n_rows, 3), -3.0, f64), _full((Q, N), -3, i32), _full((Q, N), 7, u8)
        torch.cuda.synchronize()
        g.track_path(Q, fs.N_SEG_MAX, t_path.data_ptr(), t_pc.data_ptr(), t_len.data_ptr(), t_pos.data_ptr(), 2, t_seg.data_ptr(), t_cs.data_ptr(),
                     t_win.data_ptr(), d_bounds=t_bounds.data_ptr(), d_bound_window=t_bwin.data_ptr(), window_segments=S)
        env.set_path_columns(pc, t_win.data_ptr(), t_sc.data_ptr(), Q, d_closest_s=t_cs.data_ptr(), d_state=t_state.data_ptr())
        for mode, offs in _road_modes():
            env.road_halfspaces(pc, t_main.data_ptr(), Q, offs[0], offs[1], t_stat[mode].data_ptr(), 3, first_row=first_row,
                                d_bound_segments=t_bwin.data_ptr() if mode == "bounds" else None)
        env.decomp_halfspaces(t_main.data_ptr(), Q, fs.N_SEG_MAX, t_path.data_ptr(), t_pc.data_ptr(), t_len.data_ptr(), t_s0.data_ptr(), t_sx.data_ptr(),
                              t_pts.data_ptr(), t_cnt.data_ptr(), n_pts_max, fs.RANGE, n_rows, t_rows.data_ptr(), t_count.data_ptr(), t_status.data_ptr())
        env.set_halfspace_columns(dc, t_rows.data_ptr(), t_sc.data_ptr(), Q, disc_offset=0.07)
        g.synchronize()
        got = g.debug_get_params()
        # the path window: the mirror's, in the order of the table
        assert np.array_equal(t_win.cpu().numpy(), cs["window"]) and np.array_equal(t_cs.cpu().numpy(), cs["closest_s"])
        for b in range(B):
            assert np.array_equal(got[b][:, pc], np.tile(cs["window"][cs["scene_of"][b]].reshape(-1), (N, 1)))
        want_state = cs["xinit"].copy(); want_state[:, 4] = cs["closest_s"][cs["scene_of"]]
        assert np.array_equal(t_state.cpu().numpy(), want_state)
        # the road rows: the mirrors', read through the table
        road = {mode: t.cpu().numpy() for mode, t in t_stat.items()}
        for mode, offs in _road_modes():
            want = _road_want(cs, mode, offs, fill, first_row)
            print(f"[stack env] road_decomp trial {trial} {mode}: road rows bitwise equal {np.array_equal(road[mode], want)}, "
                  f"max |device - mirror| {np.abs(road[mode] - want).max():.3e}")
            assert np.array_equal(road[mode], want)
        if road_first is None:
            road_first = road
        for mode in road:
            assert np.array_equal(road[mode], road_first[mode])
        # the decomposition: the product library's
        rows = t_rows.cpu().numpy()
        assert np.array_equal(rows, ref_rows) and np.array_equal(t_count.cpu().numpy(), ref_count) and np.array_equal(t_status.cpu().numpy(), ref_status)
        for b in range(B):
            assert np.array_equal(got[b][:, dc[1:]], rows[cs["scene_of"][b]].reshape(N, 3 * n_rows))
        assert (got[:, :, dc[0]] == 0.07).all()
        rest = np.setdiff1d(np.arange(76), pcols + dcols)
        assert len(rest) == 76 - 27 - 13 and np.array_equal(got[:, :, rest], start[:, :, rest])
    g.close()


# ---- 3. three ticks, every row built on device ----------------------------------------------------------------------------------------------------
def test_three_ticks_with_every_row_built_on_device():
    """road_decomp, 2 scenes x 2 planners, 3 ticks.  Handle A, per tick on one stream: tmpc_warmstart -> tmpc_track_path(window_segments = 3) ->
    set_path_columns -> tmpc_stack_prepare_obstacles -> set_obstacle_columns -> road_halfspaces -> linearize_topology_columns(n_static = 2) ->
    tmpc_costmap_points -> decomp_halfspaces -> set_halfspace_columns -> tmpc_solve; every column of its rows but the nine weights starts at a
    sentinel.  Handle H (same library): the warm start read back, the rows built by tests/stack_env_cases.host_tick (the numpy mirrors), uploaded
    with set_batch.  After each tick's writers A's parameter tensor equals the host-built one, and A's solve returns what H's returns, all bit for
    bit.  Each tick the robots move to stage 1 of H's main solutions and the obstacles one step on.  (As chosen, the first planner of each scene
    succeeds in every tick and the second ends with exit code 4: 6 of the 12 solves succeed.)"""
    import torch
    import stack_env_cases as cases
    from mpc_planner_amd import solver
    from mpc_planner_amd.stack_env import StackEnvironment, decomp_columns, path_columns
    from mpc_planner_amd.stack_writers import StackWriters, obstacle_columns, topology_columns
    from test_gpu_parity import _generated_lib
    path, meta = _generated_lib("road_decomp")
    pmap = meta["parameter_map"]
    Q, P, B, M, S = cases.Q, cases.P, cases.B, cases.M, cases.S
    pb = cases.problem()
    pcols, dcols = path_columns(pmap, S), decomp_columns(pmap, cases.N_ROWS)
    ocols, tcols = obstacle_columns(pmap, M, 0), topology_columns(pmap, cases.N_TOPO)
    written = sorted(set(pcols + dcols + ocols + tcols))
    assert len(written) == 76 - 9
    base = cases.base_rows(pmap)
    blank = base.copy(); blank[:, :, written] = -3.0
    dims = solver.default_dims(N=N, S=S, lib_path=path)
    A, H = solver.BatchedSolver(dims, B_max=B, lib_path=path), solver.BatchedSolver(dims, B_max=B, lib_path=path)
    W, E = StackWriters(A), StackEnvironment(A)
    f64, i32, u8 = torch.float64, torch.int32, torch.uint8
    t_xinit, t_x0, t_params = _up(pb["xinit"]), _up(pb["x0"]), _up(blank)
    A.set_batch_device(B, t_xinit.data_ptr(), t_x0.data_ptr(), t_params.data_ptr())
    H.set_batch(pb["xinit"], pb["x0"], blank)
    sc0 = pb["scenes"][0]
    size_y, size_x = sc0["costmap"].shape
    resolution = sc0["costmap_resolution"]
    t_cost, t_org = _up(np.stack([sc["costmap"] for sc in pb["scenes"]])), _up(np.stack([sc["costmap_origin"] for sc in pb["scenes"]]))
    t_path, t_pc, t_len = _up(pb["path"]), _up(pb["path_count"]), _up(pb["path_length"])
    t_sc, t_main, t_rcnt, t_rr, t_rv = _up(pb["scene_of"]), _up(pb["main_of"]), _up(pb["raw_count"]), _up(pb["raw_radius"]), _up(pb["raw_vel"])
    t_seg, t_cs, t_win = _full((Q,), -1, i32), _full((Q,), -3.0, f64), _full((Q, S, 9), -3.0, f64)
    o_pos, o_shape = _full((Q, M, N, 2), -7777.0, f64), _full((Q, M, N, 3), -7777.0, f64)
    o_rad, o_g, o_sel = _full((Q, M), -7777.0, f64), _full((Q, M), 0xEE, u8), _full((Q, M), -99, i32)
    t_stat = _full((Q, N, 2, 3), -5.0, f64)
    t_pts, t_np, t_ov = _full((Q, cases.P_MAX, 2), -3.0, f64), _full((Q,), -3, i32), _full((Q,), 9, u8)
    t_rows, t_count, t_status = _full((Q, N, cases.N_ROWS, 3), -3.0, f64), _full((Q, N), -3, i32), _full((Q, N), 7, u8)
    state = pb["xinit"][::P].copy()
    segment = np.full(Q, -1, np.int32)
    r = pb["robot_radius"]
    roads, segments, n_ok, n_solves = [], [], 0, 0
    for tick in range(3):
        stateB = np.repeat(state, P, axis=0)
        mode = np.full(B, 0 if tick == 0 else 1, np.int32)                    # tick 0: the warm start given with the batch; then the shifted solution
        t_state, t_stateB, t_state4, t_sx, t_mode = _up(state), _up(stateB), _up(state[:, :4]), _up(state[:, 0]), _up(mode)
        t_rp = _up(pb["raw_pos"] + pb["raw_vel"] * cases.DT * tick)
        torch.cuda.synchronize()
        # ---- A: one stream, nothing read back before the solve is enqueued
        A.warmstart(t_stateB.data_ptr(), t_mode.data_ptr())
        A.track_path(Q, cases.N_SEG_MAX, t_path.data_ptr(), t_pc.data_ptr(), t_len.data_ptr(), t_state.data_ptr(), 6, t_seg.data_ptr(), t_cs.data_ptr(),
                     t_win.data_ptr(), window_segments=S)
        E.set_path_columns(pcols, t_win.data_ptr(), t_sc.data_ptr(), Q)
        W.prepare_obstacles(Q, M, M, t_rcnt.data_ptr(), t_state4.data_ptr(), t_rp.data_ptr(), t_rr.data_ptr(), o_pos.data_ptr(), o_shape.data_ptr(),
                            o_rad.data_ptr(), o_g.data_ptr(), o_sel.data_ptr(), d_raw_vel=t_rv.data_ptr())
        W.set_obstacle_columns(ocols, 0, M, o_pos.data_ptr(), o_shape.data_ptr(), o_rad.data_ptr(), o_g.data_ptr(), t_sc.data_ptr(), t_state4.data_ptr(), r,
                               disc_offset=cases.DISC_OFFSET)
        E.road_halfspaces(pcols, t_main.data_ptr(), Q, pb["offsets"][0], pb["offsets"][1], t_stat.data_ptr(), 2, first_row=0)
        W.linearize_topology_columns(tcols, o_pos.data_ptr(), M, t_sc.data_ptr(), t_sx.data_ptr(), r, d_static_halfspaces=t_stat.data_ptr(), n_static=2)
        A.costmap_points(Q, size_x, size_y, t_cost.data_ptr(), t_org.data_ptr(), resolution, cases.P_MAX, t_pts.data_ptr(), t_np.data_ptr(), t_ov.data_ptr())
        E.decomp_halfspaces(t_main.data_ptr(), Q, cases.N_SEG_MAX, t_path.data_ptr(), t_pc.data_ptr(), t_len.data_ptr(), t_cs.data_ptr(), t_sx.data_ptr(),
                            t_pts.data_ptr(), t_np.data_ptr(), cases.P_MAX, cases.DECOMP_RANGE, cases.N_ROWS, t_rows.data_ptr(), t_count.data_ptr(),
                            t_status.data_ptr())
        E.set_halfspace_columns(dcols, t_rows.data_ptr(), t_sc.data_ptr(), Q, disc_offset=cases.DISC_OFFSET)
        A.solve(sync=False)
        A.synchronize()
        got = A.get()
        rows_a = A.debug_get_params()
        x0_a, xinit_a = A.debug_get_x0()
        # ---- H: the same tick built on the host
        H.warmstart(t_stateB.data_ptr(), t_mode.data_ptr())
        H.synchronize()
        x0_h, xinit_h = H.debug_get_x0()
        host = cases.host_tick(pmap, pcols, base, state, x0_h, segment, tick)
        H.set_batch(xinit_h, x0_h, host["rows"]); H.solve(); ref = H.get()
        # ---- the two ticks agree
        count, status = t_count.cpu().numpy(), t_status.cpu().numpy()
        ok = ref["exit_code"] == 1
        print(f"[stack env ticks] tick {tick}: segments {host['segment'].tolist()}, exit codes {got['exit_code'].tolist()} (host {ref['exit_code'].tolist()}), "
              f"rows bitwise equal {np.array_equal(rows_a, host['rows'])}, max |rows - host| {np.abs(rows_a - host['rows']).max():.3e}, "
              f"warm start equal {np.array_equal(x0_a, x0_h)}, decomp complete stages {[(int(((count[q] > 0) & (status[q] == 0)).sum())) for q in range(Q)]}")
        for cols, what in ((pcols, "path"), (ocols, "collision"), (tcols, "topology"), (dcols, "decomp")):
            print(f"[stack env ticks]   {what} columns: max |device - host| {np.abs(rows_a[:, :, cols] - host['rows'][:, :, cols]).max():.3e}")
        assert np.array_equal(x0_a, x0_h) and np.array_equal(xinit_a, xinit_h)
        assert np.array_equal(t_seg.cpu().numpy(), host["segment"]) and np.array_equal(t_cs.cpu().numpy(), host["closest_s"])
        assert np.array_equal(t_stat.cpu().numpy()[:, 1:], host["road"][:, 1:])
        for q in range(Q):
            dc = host["decomp"][q]
            assert np.array_equal(t_rows.cpu().numpy()[q], dc["rows"]) and np.array_equal(count[q], dc["count"]) and np.array_equal(status[q], dc["status"])
            assert ((count[q] > 0) & (status[q] == 0)).any()                 # a stage of every scene with real rows and status 0
        assert not (rows_a == -3.0).any()                                    # every blanked column was written on the device
        assert np.array_equal(rows_a, host["rows"])
        assert sorted(got) == sorted(ref)
        for key in ref:
            x, y = np.asarray(got[key]), np.asarray(ref[key])
            assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), (tick, key)
        n_ok += int(ok.sum()); n_solves += B
        roads.append(host["road"].copy()); segments.append(host["segment"].copy())
        segment = host["segment"]
        for q in range(Q):
            state[q] = ref["xtraj"][pb["main_of"][q], 1]
    assert any(not np.array_equal(roads[0][q], roads[2][q]) for q in range(Q))          # the road rows of a scene moved with the robot
    assert all(not np.array_equal(roads[0][q], roads[2][q]) for q in range(Q))
    assert (segments[0] != segments[2]).any()                                          # and a window moved on along its path
    assert 2 * n_ok >= n_solves, (n_ok, n_solves)
    A.close(); H.close()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_launches_nothing():
    """On the generated road_decomp handle.  Each refusal raises solver.TmpcError with a message that names the argument; after a synchronise the
    rows, the road buffer and the decomposition outputs are what they were.  Then the same calls as they should be: accepted.  The four entries
    of tmpc_hip.h keep refusing with "generated solver"; on goal_so_unicycle (no spline state) the road call and the closest_s form of the path
    call refuse.  A launch size beyond 2^31 - 1 is refused where n_scenes sets it (road, decomp: n_scenes x N); the B x N x n_segments and
    B x N x n_rows refusals of the two column writers need a batch of millions of entries and are not run."""
    import torch
    import free_space_cases as fs
    from mpc_planner_amd import solver
    from mpc_planner_amd.stack_env import StackEnvironment, decomp_columns, path_columns
    from test_gpu_parity import _generated_lib
    path, meta = _generated_lib("road_decomp")
    pmap = meta["parameter_map"]
    cs = _generated_case()
    Q, B, S, launch = cs["Q"], cs["B"], cs["S"], cs["launch"]
    n_rows, npar = 4, 76
    pcols, dcols = path_columns(pmap, S), decomp_columns(pmap, n_rows)
    dims = solver.default_dims(N=N, S=S, lib_path=path)
    s = solver.BatchedSolver(dims, B_max=B, lib_path=path)
    env = StackEnvironment(s)
    f64, i32, u8 = torch.float64, torch.int32, torch.uint8
    t_win, t_sc, t_main, t_cs, t_state = _up(cs["window"]), _up(cs["scene_of"]), _up(cs["main_of"]), _up(cs["closest_s"]), _up(cs["xinit"])
    t_stat = _full((Q, N, 3, 3), -5.0, f64)
    t_path, t_pc, t_len = _up(launch["path"][:Q]), _up(launch["path_count"][:Q]), _up(launch["path_length"][:Q])
    t_pts, t_cnt, t_s0, t_sx = _up(launch["points"][:Q]), _up(launch["count"][:Q]), _up(launch["s0"][:Q]), _up(launch["state_x"][:Q])
    t_rows, t_count, t_status = _full((Q, N, n_rows, 3), -3.0, f64), _full((Q, N), -3, i32), _full((Q, N), 7, u8)
    path_kw = dict(cols=pcols, d_window=t_win.data_ptr(), d_scene_of=t_sc.data_ptr(), n_scenes=Q)
    road_kw = dict(cols=pcols, d_main_of=t_main.data_ptr(), n_scenes=Q, offset_first=1.5, offset_second=1.5, d_static_halfspaces=t_stat.data_ptr(), n_static=3,
                   first_row=1)
    decomp_kw = dict(d_main_of=t_main.data_ptr(), n_scenes=Q, n_seg_max=fs.N_SEG_MAX, d_path=t_path.data_ptr(), d_path_count=t_pc.data_ptr(),
                     d_path_length=t_len.data_ptr(), d_s0=t_s0.data_ptr(), d_state_x=t_sx.data_ptr(), d_points=t_pts.data_ptr(), d_count=t_cnt.data_ptr(),
                     n_pts_max=launch["n_pts_max"], decomp_range=fs.RANGE, n_rows=n_rows, d_rows=t_rows.data_ptr(), d_row_count=t_count.data_ptr(),
                     d_status=t_status.data_ptr())
    half_kw = dict(cols=dcols, d_rows=t_rows.data_ptr(), d_scene_of=t_sc.data_ptr(), n_scenes=Q, disc_offset=0.07)
    calls = dict(tmpc_stack_set_path_columns=(env.set_path_columns, path_kw), tmpc_stack_road_halfspaces=(env.road_halfspaces, road_kw),
                 tmpc_stack_decomp_halfspaces=(env.decomp_halfspaces, decomp_kw), tmpc_stack_set_halfspace_columns=(env.set_halfspace_columns, half_kw))
    # no batch yet: all four refuse
    for name, (fn, kw) in calls.items():
        with pytest.raises(solver.TmpcError, match=name + ".*no batch"):
            fn(**kw)
    start = _sentinel_rows(B, N, npar)
    s.set_batch(cs["xinit"], cs["x0"], start)
    column_checks = lambda cols, n_too_many: [
        (dict(cols=None), "NULL argument"), (dict(cols=cols[:-1] + [npar]), "outside"), (dict(cols=[-1] + cols[1:]), "outside"),
        (dict(cols=cols[:-1] + [cols[0]]), "duplicate"), (dict(cols=list(range(n_too_many))), "at most 128")]
    bad = {
        "tmpc_stack_set_path_columns": column_checks(pcols, 135) + [
            (dict(cols=[]), "n_segments"), (dict(d_window=None), "NULL argument"), (dict(d_scene_of=None), "NULL argument"), (dict(n_scenes=0), "n_scenes"),
            (dict(n_scenes=-2), "n_scenes"), (dict(d_closest_s=t_cs.data_ptr()), "go together"), (dict(d_state=t_state.data_ptr()), "go together")],
        "tmpc_stack_road_halfspaces": column_checks(pcols, 135) + [
            (dict(cols=[]), "n_segments"), (dict(d_main_of=None), "NULL argument"), (dict(d_static_halfspaces=None), "NULL argument"), (dict(n_scenes=0), "n_scenes"),
            (dict(first_row=-1), "do not fit"), (dict(first_row=2), "do not fit"), (dict(n_static=1, first_row=0), "do not fit"),
            (dict(n_scenes=2 ** 31 - 1), "too large")],                           # n_scenes x N beyond 2^31 - 1: refused before anything is read
        "tmpc_stack_decomp_halfspaces": [
            (dict(n_scenes=0), "n_scenes"), (dict(n_seg_max=0), "n_seg_max"), (dict(n_seg_max=1025), "n_seg_max"), (dict(n_pts_max=0), "n_pts_max"),
            (dict(n_pts_max=16385), "n_pts_max"), (dict(n_rows=0), "n_rows"), (dict(n_rows=65), "n_rows"), (dict(decomp_range=-1.0), "range"),
            (dict(decomp_range=float("inf")), "range"), (dict(decomp_range=float("nan")), "range"), (dict(n_scenes=2 ** 31 - 1), "too large")]
        + [({k: None}, "NULL input") for k in ("d_main_of", "d_path", "d_path_count", "d_path_length", "d_s0", "d_state_x", "d_points", "d_count")]
        + [({k: None}, "NULL output") for k in ("d_rows", "d_row_count", "d_status")],
        "tmpc_stack_set_halfspace_columns": column_checks(dcols, 130) + [
            (dict(cols=[dcols[0]]), "n_rows"), (dict(d_rows=None), "NULL argument"), (dict(d_scene_of=None), "NULL argument"), (dict(n_scenes=0), "n_scenes")],
    }
    for name, (fn, kw) in calls.items():
        for change, msg in bad[name]:
            with pytest.raises(solver.TmpcError, match=name + ".*" + msg):
                fn(**dict(kw, **change))
    with pytest.raises(ValueError, match="per entry"):
        env.set_path_columns(pcols[:-1], t_win.data_ptr(), t_sc.data_ptr(), Q)
    null = C.c_void_p()
    assert s.lib.tmpc_stack_set_path_columns(null, None, 3, null, null, 2, null, null) == -1                 # no handle
    assert s.lib.tmpc_stack_road_halfspaces(null, None, 3, null, 2, null, 1.0, 1.0, null, 2, 0) == -1
    assert s.lib.tmpc_stack_decomp_halfspaces(null, null, 2, 16, *([null] * 7), 400, 2.0, 4, null, null, null) == -1
    assert s.lib.tmpc_stack_set_halfspace_columns(null, None, 4, null, null, 2, 0.0) == -1
    s.synchronize()
    assert np.array_equal(s.debug_get_params(), start)                        # none of the refused calls wrote a row
    assert (t_stat.cpu().numpy() == -5.0).all() and (t_rows.cpu().numpy() == -3.0).all() and (t_count.cpu().numpy() == -3).all() and (t_status.cpu().numpy() == 7).all()
    assert np.array_equal(t_state.cpu().numpy(), cs["xinit"])
    # ---- tmpc_hip.h's entries keep refusing in a generated solver
    with pytest.raises(solver.TmpcError, match="generated solver"):
        s.set_path_parameters(t_win.data_ptr(), t_sc.data_ptr(), Q)
    with pytest.raises(solver.TmpcError, match="generated solver"):
        s.road_halfspaces(t_main.data_ptr(), Q, 1.5, 1.5, t_stat.data_ptr(), 3, first_row=1)
    with pytest.raises(solver.TmpcError, match="generated solver"):
        s.decomp_halfspaces(**decomp_kw)
    with pytest.raises(solver.TmpcError, match="generated solver"):
        s.set_halfspace_rows(t_rows.data_ptr(), n_rows, t_sc.data_ptr(), Q)
    # ---- accepted: the same calls as they should be
    for name, (fn, kw) in calls.items():
        fn(**kw)
    s.synchronize()
    got = s.debug_get_params()
    assert (got[:, :, pcols + dcols] != start[:, :, pcols + dcols]).all()
    assert (t_stat.cpu().numpy()[:, 1:, 1:3] != -5.0).all() and (t_count.cpu().numpy()[:, 1:] > 0).all()
    s.close()
    # ---- a generated library whose model has no spline state
    path_u, meta_u = _generated_lib("goal_so_unicycle")
    du = solver.default_dims(N=N, lib_path=path_u)
    u = solver.BatchedSolver(du, B_max=2, lib_path=path_u)
    eu = StackEnvironment(u)
    start_u = _sentinel_rows(2, N, du.npar)
    u.set_batch(np.zeros((2, du.nx)), np.zeros((2, N + 1, du.nvar)), start_u)
    cols_u = list(range(9))
    t_win1, t_sc2, t_cs1, t_state_u = _up(cs["window"][:1, :1]), _up(np.zeros(2, np.int32)), _up(cs["closest_s"][:1]), _up(np.zeros((2, du.nx)))
    with pytest.raises(solver.TmpcError, match="tmpc_stack_road_halfspaces.*no spline state"):
        eu.road_halfspaces(cols_u, t_main.data_ptr(), 1, 1.5, 1.5, t_stat.data_ptr(), 3, first_row=1)
    with pytest.raises(solver.TmpcError, match="tmpc_stack_set_path_columns.*no spline state"):
        eu.set_path_columns(cols_u, t_win1.data_ptr(), t_sc2.data_ptr(), 1, d_closest_s=t_cs1.data_ptr(), d_state=t_state_u.data_ptr())
    u.synchronize()
    assert np.array_equal(u.debug_get_params(), start_u) and (t_state_u.cpu().numpy() == 0.0).all()
    u.close()
