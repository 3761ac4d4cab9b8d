"""GPU: Contouring's road constraints on device (tmpc_road_halfspaces, csrc/tmpc_aux_kernels.hpp) -- the rows against the host mirrors
(mpc_planner_amd/modules.py road_halfspaces / road_halfspaces_from_bounds, pinned on hand-derived values in tests/test_road_halfspaces.py),
the solve with the rows active against the CPU oracle, and a closed loop of five ticks in which the rows follow the shifted warm start without
a host round trip.  Tolerances are the ones the suite holds the sibling kernels to (tests/test_gpu_parity.py, tests/test_gpu_end_to_end.py)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N, M, S = 20, 8, 5
ROW_TOL = 1e-14          # device rows vs mirror: the line of tests/test_gpu_parity.py:370 (bitwise if the operation order is the mirror's)


def _concat(scs):
    xinit = np.concatenate([s["xinit"] for s in scs]); x0 = np.concatenate([s["x0"] for s in scs]); params = np.concatenate([s["params"] for s in scs])
    scene_of = np.concatenate([np.full(len(s["xinit"]), i, np.int32) for i, s in enumerate(scs)])
    first = np.cumsum([0] + [len(s["xinit"]) for s in scs])[:-1]
    return xinit, x0, params, scene_of, first


def _bounds(segs, dl, dr):
    left, right = segs[:, :8].copy(), segs[:, :8].copy()
    left[:, 7] += dl; right[:, 7] -= dr
    return left, right


@pytest.mark.parametrize("slack", [0, 1])
def test_device_rows_equal_the_mirror(slack):
    """Both modes, three scenes, a main solver that is not the scene's first entry (and is the only entry of its scene with that spline
    column), slack and non-slack strides, rows 1 and 2 of a three-row buffer whose other entries must come back untouched."""
    import torch
    from mpc_planner_amd import scenes, solver, modules as md
    kw = dict(slack=True, n_decomp=12) if slack else {}
    scs = [scenes.make_scene(90 + i, N=N, M=M, B=8, **kw) for i in range(3)]
    xinit, x0, params, scene_of, first = _concat(scs)
    B = len(xinit)
    main_of = first.copy(); main_of[1] += 3
    x0 = x0.copy()
    x0[main_of[1], :, 6] += 0.37 * np.arange(N + 1)                      # only entry main_of[1] carries scene 1's "main" spline states
    x0[main_of[2], 3, 6] = 12.0                                          # exactly on a knot: the segment that starts there
    x0[main_of[2], 19, 6] = 31.5                                         # beyond the window: the last cubic continues
    x0[main_of[2], 2, 6] = -0.25                                         # below the first knot: segment 0
    dims = solver.default_dims(N=N, S=S, n_lin=M, M=M, n_slk=12 if slack else 0, slack=slack)
    s = solver.BatchedSolver(dims, B_max=B)
    s.set_batch(xinit, x0, params)
    dev = torch.device("cuda")
    t_main = torch.from_numpy(main_of.astype(np.int32)).to(dev)
    r = scenes.ROBOT_RADIUS
    bounds = np.stack([np.stack(_bounds(sc["segments"], 2.0 + 0.3 * i, 1.5 + 0.2 * i)) for i, sc in enumerate(scs)])     # [3][2][S][8]
    t_bounds = torch.from_numpy(np.ascontiguousarray(bounds)).to(dev)
    worst = 0.0
    for mode, offs in (("centreline", md.road_offsets(4.0, r)), ("two_way", md.road_offsets(5.0, r, True)), ("bounds", (r, r))):
        fill = np.random.default_rng(3).normal(size=(3, N, 3, 3))
        t_stat = torch.from_numpy(fill.copy()).to(dev)
        s.road_halfspaces(t_main.data_ptr(), 3, offs[0], offs[1], t_stat.data_ptr(), 3, first_row=1,
                          d_bound_segments=t_bounds.data_ptr() if mode == "bounds" else None)
        s.synchronize()
        got = t_stat.cpu().numpy()
        want = fill.copy()
        for q, sc in enumerate(scs):
            s_of_k = x0[main_of[q], :N, 6]
            rows = md.road_halfspaces_from_bounds(sc["segments"], bounds[q, 0], bounds[q, 1], s_of_k, r) if mode == "bounds" \
                else md.road_halfspaces(sc["segments"], s_of_k, *offs)
            want[q, 1:, 1:3] = rows[1:]
        np.testing.assert_array_equal(got[:, :, 0], fill[:, :, 0])        # row 0 of the buffer: untouched
        np.testing.assert_array_equal(got[:, 0], fill[:, 0])              # stage 0: untouched
        err = np.abs(got - want).max()
        worst = max(worst, err)
        print(f"[road rows] slack {slack} {mode}: max |device - mirror| = {err:.3e}, bitwise equal: {np.array_equal(got, want)}")
        np.testing.assert_allclose(got, want, rtol=ROW_TOL, atol=ROW_TOL)
        if mode != "bounds":                                              # scene 1: the rows of ITS main solver, not those of the scene's first entry
            lead_rows = md.road_halfspaces(scs[1]["segments"], x0[first[1], :N, 6], *offs)
            assert np.abs(got[1, 1:, 1:3] - lead_rows[1:]).max() > 1e-3
    s.close()


def test_device_rows_feed_linearize_topology_ex():
    """The rows as tmpc_linearize_topology_ex reads them (n_obstacles = 8, n_static = 2): the batch parameters equal the host-built ones
    (scenes.add_road_constraints = mirrors of Contouring::update + LinearizedConstraints::update / setParameters), non-guided planners included."""
    import torch
    from mpc_planner_amd import scenes, solver
    scs = [scenes.add_road_constraints(scenes.make_scene(94 + i, N=N, M=M, B=8, tmpc_pp=True), 4.0) for i in range(3)]
    xinit, x0, want, scene_of, first = _concat(scs)
    B = len(xinit)
    is_orig = np.zeros(B, np.uint8); is_orig[first + 8] = 1
    pm = scs[0]["pm"]
    start = want.copy()
    for j in range(M + 2):
        for f in ("a1", "a2", "b"):
            start[:, :, pm.index(f"lin_constraint_{j}_{f}")] = -7.0
    dims = solver.default_dims(N=N, S=S, n_lin=M + 2, M=M)
    assert dims.npar == pm.length()
    s = solver.BatchedSolver(dims, B_max=B)
    s.set_batch(xinit, x0, start)
    dev = torch.device("cuda")
    t_main = torch.from_numpy(first.astype(np.int32)).to(dev)
    t_stat = torch.full((3, N, 2, 3), -5.0, dtype=torch.float64, device=dev)
    t_ob = torch.from_numpy(np.ascontiguousarray(np.stack([sc["obstacles"]["pos"] for sc in scs]))).to(dev)
    t_sc = torch.from_numpy(scene_of).to(dev); t_sx = torch.from_numpy(np.ascontiguousarray(xinit[first, 0])).to(dev)
    t_io = torch.from_numpy(is_orig).to(dev)
    s.road_halfspaces(t_main.data_ptr(), 3, *scs[0]["road_offsets"], t_stat.data_ptr(), 2, first_row=0)
    s.linearize_topology_ex(t_ob.data_ptr(), M, t_sc.data_ptr(), t_sx.data_ptr(), scenes.ROBOT_RADIUS, d_static_halfspaces=t_stat.data_ptr(), n_static=2,
                            d_is_original=t_io.data_ptr())
    got = s.debug_get_params()
    print(f"[road rows -> params] max |device - host| = {np.abs(got - want).max():.3e}")
    np.testing.assert_allclose(got, want, rtol=ROW_TOL, atol=ROW_TOL)
    j8 = [pm.index(f"lin_constraint_8_{f}") for f in ("a1", "a2", "b")]
    np.testing.assert_array_equal(got[3, 5, j8], scs[0]["road_rows"][5, 0])                 # copied as given
    assert (got[:, 0, j8[0]] == 1.0).all() and (got[first + 8, 5, j8[0]] == 1.0).all()       # stage 0 / the non-guided planner's row 8: dummies
    s.close()


def test_solve_with_road_rows_matches_oracle():
    """Scenes 80 .. 87, B = 16: 128 trajectories with the two road rows of a 4 m road behind the eight obstacle rows (n_lin = 10), HIP against the
    CPU oracle by the suite's rule (tests/test_gpu_parity.py _compare): exit code and SQP iteration count equal on all 128; QP status,
    interior-point iteration count and trajectories (1e-8 relative per stage) where the oracle's exit code is 1 -- 29 % of these solves are
    infeasible by design (guidance guesses that start outside the road), and a diverging interior-point run may stop differently on the two sides.
    The rows must matter: at least 64 successes, a successful trajectory with a road-row value above -1e-5 (active), and no successful
    trajectory beyond qp_tol = 1e-5 (the rows are linear: the last QP's primal residual bound carries over to the stepped iterate)."""
    import sys
    sys.path.insert(0, HERE)
    import oracle_lib as O
    from mpc_planner_amd import scenes, solver
    B = 16
    scs = [scenes.add_road_constraints(scenes.make_scene(seed, N=N, M=M, B=B), 4.0, radius=scenes.ROBOT_RADIUS) for seed in range(80, 88)]
    xinit, x0, params, scene_of, first = _concat(scs)
    Bt = len(xinit)
    assert Bt == 128
    s = solver.BatchedSolver(solver.default_dims(N=N, S=S, n_lin=M + 2, M=M), B_max=Bt)
    print("[road solve] " + s.kernel_info())
    s.set_batch(xinit, x0, params); s.solve(); got = s.get()
    s.close()
    pb = O.problem(N=N, S=S, n_lin=M + 2, M=M)
    xt, ut, info = O.solve_batch(pb, xinit, x0.reshape(Bt, -1), params.reshape(Bt, -1), 16)
    ok = info["exit_code"] == 1
    print(f"[road solve] oracle successes {ok.sum()} / {Bt}; exit codes differ on {(got['exit_code'] != info['exit_code']).sum()}, "
          f"sqp_iter on {(got['sqp_iter'] != info['sqp_iter']).sum()}")
    assert (got["exit_code"] == info["exit_code"]).all()
    assert (got["sqp_iter"] == info["sqp_iter"]).all()
    assert ok.sum() >= 64
    assert (got["qp_status"][ok] == info["qp_status"][ok]).all()
    assert (got["qp_iter_total"][ok] == info["qp_iter_total"][ok]).all()
    sx = np.maximum(np.abs(xt[ok]).max(axis=2, keepdims=True), 1.0); su = np.maximum(np.abs(ut[ok]).max(axis=2, keepdims=True), 1.0)
    ex = (np.abs(got["xtraj"][ok] - xt[ok]) / sx).max(); eu = (np.abs(got["utraj"][ok] - ut[ok]) / su).max()
    print(f"[road solve] max relative difference per stage: x {ex:.3e}, u {eu:.3e}")
    assert ex <= 1e-8 and eu <= 1e-8, (ex, eu)
    # the road rows at the device's solutions
    k = np.arange(1, N)
    worst = np.full(Bt, -np.inf)
    for b in range(Bt):
        rows = scs[scene_of[b]]["road_rows"]
        for j in range(2):
            worst[b] = max(worst[b], (rows[k, j, 0] * got["xtraj"][b][k, 0] + rows[k, j, 1] * got["xtraj"][b][k, 1] - rows[k, j, 2]).max())
    print(f"[road solve] largest road-row value over the successful solves {worst[ok].max():.3e}; active (> -1e-5) on {(worst[ok] > -1e-5).sum()}")
    assert (worst[ok] > -1e-5).any()
    assert (worst[ok] <= 1e-5).all()


def test_closed_loop_five_ticks_without_host_round_trip():
    """warmstart -> road_halfspaces -> init_with_guidance -> linearize_topology_ex -> solve -> select, five ticks, parameter sharing on (the
    shared rows live in each set's lead entry, which is also the set's main solver), every input of a tick produced on the device from the
    previous tick's results -- against the same ticks rebuilt on the host from debug_get_x0() and the mirrors (tolerances of
    tests/test_gpu_end_to_end.py).  The road rows move with the spline state of the shifted warm start."""
    import torch
    from mpc_planner_amd import scenes, solver, modules as md
    n_sets, traj, ticks = 3, 16, 5
    scs = [scenes.add_road_constraints(scenes.make_scene(80 + i, N=N, M=M, B=traj), 4.0) for i in range(n_sets)]
    xinit, x0, params, scene_of, lead = _concat(scs)
    B = n_sets * traj
    pm = scs[0]["pm"]
    offs = scs[0]["road_offsets"]
    r = scenes.ROBOT_RADIUS
    obst = np.ascontiguousarray(np.stack([sc["obstacles"]["pos"] for sc in scs]))
    gpos0 = np.concatenate([sc["guidance_pos"] for sc in scs]); gvel = np.concatenate([sc["guidance_vel"] for sc in scs])
    dims = solver.default_dims(N=N, S=S, n_lin=M + 2, M=M)
    own = solver.own_parameter_columns(dims)
    dev = torch.device("cuda")
    s = solver.BatchedSolver(dims, B_max=B)
    ref_s = solver.BatchedSolver(dims, B_max=B)
    # device state: garbage in everything the device has to produce; the shared rows in the lead entries only
    t_xinit = torch.from_numpy(xinit.copy()).to(dev)
    t_x0 = torch.from_numpy(np.ascontiguousarray(np.repeat(x0[lead], traj, axis=0)).reshape(B, -1)).to(dev)      # every planner starts as a copy of the main solver
    p0 = np.full_like(params, -3.0); p0[lead] = params[lead]
    t_params = torch.from_numpy(p0.reshape(B, -1)).to(dev)
    s.set_batch_device(B, t_xinit.data_ptr(), t_x0.data_ptr(), t_params.data_ptr())
    base_of = np.repeat(lead, traj).astype(np.int32)
    s.set_param_sharing(base_of)
    t_lead = torch.from_numpy(lead.astype(np.int32)).to(dev)
    t_base = torch.from_numpy(base_of).to(dev)
    t_gpos0 = torch.from_numpy(gpos0).to(dev); t_gvel = torch.from_numpy(gvel).to(dev)
    t_ob = torch.from_numpy(obst).to(dev); t_sc = torch.from_numpy(scene_of).to(dev)
    t_stat = torch.zeros((n_sets, N, 2, 3), dtype=torch.float64, device=dev)
    t_state = torch.from_numpy(xinit.copy()).to(dev); t_sx = t_state[t_lead.long(), 0].contiguous()
    t_gp = t_gpos0.clone()
    t_src = t_base.clone()
    t_rec = torch.zeros((B, 2), dtype=torch.int64, device=dev); t_best = torch.full((n_sets,), -2, dtype=torch.int32, device=dev)
    t_wx = torch.zeros((n_sets, (N + 1) * 5), dtype=torch.float64, device=dev); t_wu = torch.zeros((n_sets, N * 2), dtype=torch.float64, device=dev)
    hs = torch.cuda.ExternalStream(s.stream_ptr(), device=dev)
    torch.cuda.synchronize()
    rows_before = None
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
                s.warmstart(t_state.data_ptr(), None, t_src.data_ptr())
            s.road_halfspaces(t_lead.data_ptr(), n_sets, offs[0], offs[1], t_stat.data_ptr(), 2, first_row=0)
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
        rows_dev = t_stat.cpu().numpy()
        host = np.zeros_like(params)
        for q in range(n_sets):
            rows = md.road_halfspaces(scs[q]["segments"], x0_dev[lead[q], :N, 6], *offs)
            np.testing.assert_allclose(rows_dev[q, 1:], rows[1:], rtol=ROW_TOL, atol=ROW_TOL)
            for b in range(lead[q], lead[q] + traj):
                host[b] = params[lead[q]]                                                     # shared rows: the lead entry's
                lin = md.linearized_update(x0_dev[b], obst[q], r, static=rows)
                md.linearized_set_parameters(pm, host[b], xinit_dev[lead[q], 0], lin, n_rows=M + 2)
        np.testing.assert_allclose(p_dev[:, :, own], host[:, :, own], rtol=1e-14, atol=1e-14)
        if rows_before is not None:                                                           # the spline state advanced: other rows
            assert won.any() and (x0_dev[lead, 1, 6] > s_before + 1e-3)[won].all()             # (sets whose last tick had a winner to follow)
            assert (np.abs(rows_dev[:, 1:] - rows_before[:, 1:]).max(axis=(1, 2, 3)) > 1e-3)[won].all()
        rows_before, s_before = rows_dev.copy(), x0_dev[lead, 1, 6].copy()
        ref_s.set_batch(xinit_dev, x0_dev, host); ref_s.solve(); ref = ref_s.get()
        ref_best = [ref_s.select_best(first=int(l), count=traj) for l in lead]
        ok = ref["exit_code"] == 1
        differ = (got["qp_iter_total"][ok] != ref["qp_iter_total"][ok]).mean() if ok.any() else 0.0
        print(f"[road loop] tick {tick}: successes {ok.sum()} / {B}, qp_iter_total differs on {differ:.3f}, s_1 of the main solvers {x0_dev[lead, 1, 6]}")
        assert (got["exit_code"] == ref["exit_code"]).all() and (got["sqp_iter"] == ref["sqp_iter"]).all()
        assert differ <= 0.05
        np.testing.assert_allclose(got["xtraj"][ok], ref["xtraj"][ok], rtol=0, atol=1e-7)
        best = t_best.cpu().numpy()
        won = best >= 0
        for si in range(n_sets):
            a, b = int(best[si]), int(ref_best[si])
            assert (a < 0) == (b < 0)
            if a != b:
                assert abs(got["pobj"][lead[si] + a] - ref["pobj"][lead[si] + b]) <= 1e-9 * max(1.0, abs(ref["pobj"][lead[si] + b]))
    s.close(); ref_s.close()


def test_bad_arguments_and_generated_solver():
    import ctypes as C
    import torch
    from mpc_planner_amd import scenes, solver
    sc = scenes.make_scene(80, N=N, M=M, B=4)
    dims = solver.default_dims(N=N, S=S, n_lin=M, M=M)
    s = solver.BatchedSolver(dims, B_max=4)
    dev = torch.device("cuda")
    t_main = torch.zeros(1, dtype=torch.int32, device=dev); t_stat = torch.zeros((1, N, 3, 3), dtype=torch.float64, device=dev)
    call = lambda **kw: s.road_halfspaces(**dict(dict(d_main_of=t_main.data_ptr(), n_scenes=1, offset_first=1.0, offset_second=1.0,
                                                     d_static_halfspaces=t_stat.data_ptr(), n_static=3, first_row=1), **kw))
    with pytest.raises(solver.TmpcError, match="no batch"):
        call()
    s.set_batch(sc["xinit"], sc["x0"], sc["params"])
    call()                                                                # the same call with a batch: accepted
    for kw, msg in ((dict(first_row=2), "n_static < first_row"), (dict(n_static=1, first_row=0), "n_static < first_row"), (dict(first_row=-1), "first_row"),
                    (dict(d_main_of=None), "bad argument"), (dict(d_static_halfspaces=None), "bad argument"), (dict(n_scenes=0), "bad argument")):
        with pytest.raises(solver.TmpcError, match=msg):
            call(**kw)
    assert s.lib.tmpc_road_halfspaces(None, None, 1, None, C.c_double(1.0), C.c_double(1.0), None, 2, 0) == -1       # no handle: TMPC_ERR_INVALID
    # an entry outside the batch: its scene's rows are left alone (nothing is read out of bounds)
    t_stat.fill_(4.0); t_main.fill_(9)
    call(); s.synchronize()
    assert (t_stat.cpu().numpy() == 4.0).all()
    s.close()
    # a generated solver refuses, like tmpc_linearize_topology_ex does: its parameter layout is the module stack's
    path = os.path.join(os.path.dirname(HERE), "build", "generated", "libtmpc_hip_tmpc_cfg2.so")
    if not os.path.exists(path):
        import __graft_entry__ as g
        g.build_generated_demo()
    d = solver.default_dims(N=N, lib_path=path)
    sg = solver.BatchedSolver(d, B_max=4, lib_path=path)
    sg.set_batch(sc["xinit"], sc["x0"], sc["params"])
    with pytest.raises(solver.TmpcError, match="generated solver"):
        sg.road_halfspaces(t_main.data_ptr(), 1, 1.0, 1.0, t_stat.data_ptr(), 3, first_row=1)
    sg.close()
