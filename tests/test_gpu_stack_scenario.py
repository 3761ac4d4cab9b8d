"""GPU: the scenario rows of a generated stack by column, include/tmpc_hip_stack_scenario.h (csrc/tmpc_row_entries.hpp;
mpc_planner_amd/stack_scenario.py) -- the SH-MPC polygons and the support of the solution.

1. On the product library the column entries, given the hand-written cfg 5 layout's own columns, leave the parameter rows, the empty-stage
   counts, the solve and the support bit-equal to tmpc_scenario_halfspaces / tmpc_scenario_support on the sample sets of
   test_device_polygon_edge_cases (both passes of the kernel, the second one below and above 48 KiB of candidate list), with and without
   discarded scenarios, and touch nothing else; with the columns permuted onto other columns of a wider row the rows land where named.
2. On the generated safe_horizon library they equal the numpy mirrors.
3. Three ticks of 2 scenes x 2 solvers with every row built on device, against the same ticks built by the mirrors and solved on a second
   handle, and against the hand-written cfg 5 kernel.
4. Every refusal, with its message and without a launch; the entries of tmpc_hip.h keep refusing in a generated solver.
8 trajectories, N = 20, 24 rows.  Every comparison but the one with the hand-written kernel is np.array_equal: both sides run the same
arithmetic in the same order."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import stack_scenario_cases as cases  # noqa: E402

N, R, RADIUS = cases.N, cases.R, cases.RADIUS


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda"))


def _equal(got, ref, what):
    assert sorted(got) == sorted(ref)
    for key in ref:
        x, y = np.asarray(got[key]), np.asarray(ref[key])
        assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), (what, key)


# ---- 1. the product library: the same inputs through the layout entries and through the column entries ---------------------------------------
@pytest.fixture(scope="module")
def product():
    from mpc_planner_amd import scenes, solver
    from mpc_planner_amd.stack_scenario import StackScenario, scenario_columns
    sc = scenes.make_scene(6, B=8, **cases.CFG5_SCENE)
    dims = solver.default_dims(**cases.CFG5_DIMS)
    cols = scenario_columns(sc["pm"]._params, R)
    assert dims.npar == len(sc["pm"]._params) == 127 and cols == [54] + list(range(55, 127))
    a, b = solver.BatchedSolver(dims, B_max=8), solver.BatchedSolver(dims, B_max=8)
    out = dict(sc=sc, dims=dims, cols=cols, a=a, b=b, scn=StackScenario(b), start=cases.sentinel(sc["params"], cols))
    yield out
    a.close(); b.close()


def _both_forms(product, o, n_scenarios, n_discard=0):
    """The layout entries on handle a, the column entries on handle b: the same sentinel-filled rows, samples o [N][n][2] of one scene."""
    sc, a, b, scn, cols, start = (product[k] for k in ("sc", "a", "b", "scn", "cols", "start"))
    n = o.shape[1]
    t_s, t_sc, t_sx = _up(o[None]), _up(np.zeros(8, np.int32)), _up(sc["xinit"][:1, 0].copy())
    got = {}
    for name, s in (("layout", a), ("columns", b)):
        s.set_batch(sc["xinit"], sc["x0"], start)
        if n_discard:
            s.scenario_discard(t_s.data_ptr(), n, n_scenarios, n_discard, t_sc.data_ptr(), RADIUS)
        if name == "layout":
            s.scenario_halfspaces(t_s.data_ptr(), n, R, t_sc.data_ptr(), t_sx.data_ptr(), RADIUS, disc_offset=0.07)
        else:
            scn.halfspaces(cols, t_s.data_ptr(), n, t_sc.data_ptr(), t_sx.data_ptr(), RADIUS, disc_offset=0.07)
        params, empty = s.debug_get_params(), s.scenario_empty_stages()
        s.solve_iterations(10)
        sol = s.get()
        support = {tol: (s.scenario_support(n_scenarios, tol) if name == "layout" else scn.support(cols, n_scenarios, tol)) for tol in (1e-6, 1e-3)}
        got[name] = dict(params=params, empty=empty, sol=sol, support=support, marks=s.scenario_discarded(n_scenarios) if n_discard else None)
    return got["layout"], got["columns"]


@pytest.mark.parametrize("shape", ["tiny", "duplicates", "contradictory", "big_ring", "ring_2000", "large", "discard"])
def test_column_entries_equal_the_layout_entries_on_the_product_library(product, shape):
    """cfg 5 (127 parameters; the scenario columns are its last 72 and ego_disc_0_offset), 8 trajectories of one scene.  The 73 named columns
    start at a sentinel pattern, the others at the scene's values.  `discard`: the 300 samples of `duplicates` as 5 obstacles x 60 scenarios, 7
    of them removed by tmpc_scenario_discard on either handle."""
    sc, cols, start = product["sc"], product["cols"], product["start"]
    o = cases.edge_samples("duplicates" if shape == "discard" else shape, sc["x0"])
    n_scenarios, n_discard = (60, 7) if shape == "discard" else (50, 0)
    lay, col = _both_forms(product, o, n_scenarios, n_discard)
    rest = np.setdiff1d(np.arange(127), cols)
    print(f"[stack scenario] {shape}: {o.shape[1]} samples, rows bitwise equal {np.array_equal(lay['params'], col['params'])}, empty stages {col['empty'].tolist()}, "
          f"exit codes {col['sol']['exit_code'].tolist()}, support {col['support'][1e-3][0].tolist()} (layout {lay['support'][1e-3][0].tolist()})")
    assert np.array_equal(col["params"], lay["params"])
    assert np.array_equal(col["params"][:, :, rest], start[:, :, rest]) and len(rest) == 54
    assert (col["params"][:, :, cols] != start[:, :, cols]).all()                  # every named column of every stage was written
    assert (col["params"][:, :, cols[0]] == 0.07).all()
    assert np.array_equal(col["empty"], lay["empty"])
    _equal(col["sol"], lay["sol"], shape)
    for tol in (1e-6, 1e-3):
        assert np.array_equal(col["support"][tol][0], lay["support"][tol][0]) and np.array_equal(col["support"][tol][1], lay["support"][tol][1])
    real = col["params"][:, 1:, cols[3::3]] != sc["xinit"][0, 0] + 100.0           # b of a dummy row is x + 100
    if shape == "tiny":
        assert real.sum(axis=2).max() <= 5 and real.any()
    if shape in ("big_ring", "ring_2000"):
        assert real.all()                                                          # truncated: 24 real rows everywhere
    if shape == "contradictory":
        assert col["empty"][3] >= 3 and real[3, 4:7].all()                         # flagged, and its rows are real halfspaces, not dummies
    if shape == "discard":
        assert np.array_equal(col["marks"], lay["marks"]) and (col["marks"].sum(axis=1) == 7).all()
        _, every = _both_forms(product, o, n_scenarios)
        assert not np.array_equal(col["params"], every["params"])                  # the removed scenarios changed the polygons


def test_permuted_columns_on_a_wider_row(product):
    """A wider hand-written shape (8 topology rows, 8 ellipsoids, 24 slack rows, slack model: 208 parameters), every entry of every row at a
    sentinel; the 73 columns of the call are drawn among the 136 columns in front of the layout's own slack rows.  The rows of the cfg 5 run on
    the same warm start and samples land in the named columns, in the table's order, and nothing else changes; support reads them there."""
    from mpc_planner_amd import solver
    from mpc_planner_amd.stack_scenario import StackScenario
    sc = product["sc"]
    dims = solver.default_dims(N=N, S=5, n_lin=8, M=8, n_slk=R, slack=1)
    assert dims.npar == 208 and dims.nvar == 8
    o = cases.edge_samples("duplicates", sc["x0"])
    lay, _ = _both_forms(product, o, 50)
    pc = [int(c) for c in np.random.default_rng(23).permutation(136)[:73]]
    assert not set(pc) & set(range(136, 208))
    start = cases.sentinel(np.zeros((8, N, 208)), list(range(208)))
    w = solver.BatchedSolver(dims, B_max=8)
    scn = StackScenario(w)
    w.set_batch(sc["xinit"], sc["x0"], start)
    t_s, t_sc, t_sx = _up(o[None]), _up(np.zeros(8, np.int32)), _up(sc["xinit"][:1, 0].copy())
    scn.halfspaces(pc, t_s.data_ptr(), o.shape[1], t_sc.data_ptr(), t_sx.data_ptr(), RADIUS, disc_offset=0.07)
    got = w.debug_get_params()
    rest = np.setdiff1d(np.arange(208), pc)
    assert np.array_equal(got[:, :, pc], lay["params"][:, :, product["cols"]])
    assert np.array_equal(got[:, :, rest], start[:, :, rest]) and len(rest) == 135
    assert np.array_equal(w.scenario_empty_stages(), lay["empty"])
    with pytest.raises(solver.TmpcError, match="tmpc_scenario_support.*not built by tmpc_scenario_halfspaces"):
        w.scenario_support(50)                                                     # the layout entry would read ip_slk: other columns
    w.close()


# ---- 2. the generated safe_horizon library -----------------------------------------------------------------------------------------------------
def test_generated_safe_horizon_library_equals_the_mirrors():
    """libtmpc_hip_safe_horizon.so (127 parameters, the cfg 5 map): the scene's own 8 x 256 samples, 5 scenarios discarded on device; the rows
    and ego_disc_0_offset equal modules.scenario_halfspaces + halfspace_rows_set_parameters on the generated map, every other column keeps its
    value, the marks equal modules.scenario_discard, and after a solve the support equals modules.scenario_support."""
    from mpc_planner_amd import modules as md, scenes, solver
    from mpc_planner_amd.stack_scenario import StackScenario, scenario_columns
    from test_gpu_parity import _generated_lib
    path, meta = _generated_lib("safe_horizon")
    pmap = meta["parameter_map"]
    pm = cases.Map(pmap)
    sc = scenes.make_scene(6, B=8, **cases.CFG5_SCENE)
    assert pmap == dict(sc["pm"]._params) and meta["spill_free"]
    dims = solver.default_dims(N=N, lib_path=path)
    assert (dims.npar, dims.n_lin, dims.n_slk, dims.slack, dims.nvar) == (127, R, 0, 1, 8)        # a generated handle counts every row of its stack in n_lin
    cols = scenario_columns(pmap, R)
    s_cen, n_discard, off = sc["samples"].shape[1], 5, 0.05
    smp = np.ascontiguousarray(sc["samples"].transpose(2, 0, 1, 3)).reshape(1, N, -1, 2)               # [M][S][N][2] -> [1][N][M S][2]
    start = cases.sentinel(sc["params"], cols)
    g = solver.BatchedSolver(dims, B_max=8, lib_path=path)
    scn = StackScenario(g)
    g.set_batch(sc["xinit"], sc["x0"], start)
    t_s, t_sc, t_sx = _up(smp), _up(np.zeros(8, np.int32)), _up(sc["xinit"][:1, 0].copy())
    g.scenario_discard(t_s.data_ptr(), smp.shape[2], s_cen, n_discard, t_sc.data_ptr(), RADIUS)
    scn.halfspaces(cols, t_s.data_ptr(), smp.shape[2], t_sc.data_ptr(), t_sx.data_ptr(), RADIUS, disc_offset=off)
    got, marks, empty = g.debug_get_params(), g.scenario_discarded(s_cen), g.scenario_empty_stages()
    want, which = start.copy(), []
    for b in range(8):
        mk = md.scenario_discard(sc["x0"][b], sc["samples"], RADIUS, n_discard)
        assert np.array_equal(marks[b], mk)
        rows = md.scenario_halfspaces(sc["x0"][b], sc["samples"], RADIUS, R, return_index=True, discard=mk)
        md.halfspace_rows_set_parameters(pm, want[b], sc["xinit"][0, 0], rows[:3], cases.PREFIX, R, off)
        which.append(rows[3])
        assert empty[b] == rows[4].sum()
    print(f"[stack scenario] safe_horizon: rows bitwise equal {np.array_equal(got, want)}, max |device - mirror| {np.abs(got - want).max():.3e}")
    assert np.array_equal(got, want)
    assert not (want[:, :, cols] == start[:, :, cols]).any()
    g.solve()
    sol = g.get()
    for tol in (1e-6, 1e-3):
        sup, act = scn.support(cols, s_cen, tol)
        ref = [md.scenario_support(sol["xtraj"][b], want[b], pm, which[b], s_cen, tol) for b in range(8)]
        assert sup.tolist() == [r[0] for r in ref] and act.tolist() == [r[1] for r in ref]
    print(f"[stack scenario] safe_horizon: exit codes {sol['exit_code'].tolist()}, support {sup.tolist()}, active rows {act.tolist()}")
    assert sup.max() >= 1 and (act >= sup).all()
    g.close()


# ---- 3. three ticks, every row built on device ----------------------------------------------------------------------------------------------------
def test_three_ticks_with_the_scenario_rows_built_on_device():
    """safe_horizon, 2 scenes x 2 parallel solvers (8 obstacles x 128 scenarios each, 4 discarded), 3 ticks.  Handle A, per tick on one stream:
    tmpc_warmstart -> tmpc_sample_scenarios -> tmpc_scenario_discard -> tmpc_stack_scenario_halfspaces -> tmpc_solve ->
    tmpc_stack_scenario_support; its scenario columns start at -3.  Handle H (same library): the warm start read back, the rows built by
    tests/stack_scenario_cases.host_rows (the numpy mirrors), uploaded with set_batch.  After each tick's writers A's parameter tensor equals the
    host-built one, A's solve returns what H's returns and A's support is the mirror's on that solution, all bit for bit.  Handle K, the
    hand-written cfg 5 kernel of libtmpc_hip.so, solves H's batch: integers equal, trajectories to 1e-9, objectives to 1e-10 relative (the bounds
    of test_generated_tmpc_solver_equals_hand_written_kernels).  Each tick the robots move to stage 1 of their scene's best plan and the
    obstacles one step on."""
    import torch
    from mpc_planner_amd import solver
    from mpc_planner_amd.stack_scenario import StackScenario, scenario_columns
    from test_gpu_parity import _generated_lib
    path, meta = _generated_lib("safe_horizon")
    pmap = meta["parameter_map"]
    pm = cases.Map(pmap)
    B, M, S_CEN = cases.B, cases.M, cases.S_CEN
    pb = cases.loop_problem()
    assert pmap == dict(pb["pm"]._params)
    cols = scenario_columns(pmap, R)
    blank = pb["params"].copy(); blank[:, :, cols] = -3.0
    dims = solver.default_dims(N=N, lib_path=path)
    A, H = solver.BatchedSolver(dims, B_max=B, lib_path=path), solver.BatchedSolver(dims, B_max=B, lib_path=path)
    K = solver.BatchedSolver(solver.default_dims(**cases.CFG5_DIMS), B_max=B)
    SA = StackScenario(A)
    t_xinit, t_x0, t_params = _up(pb["xinit"]), _up(pb["x0"]), _up(blank)
    A.set_batch_device(B, t_xinit.data_ptr(), t_x0.data_ptr(), t_params.data_ptr())
    H.set_batch(pb["xinit"], pb["x0"], blank)
    t_prob, t_sc = _up(pb["prob"]), _up(pb["scene_of"])
    t_smp = torch.empty((B, N, M * S_CEN, 2), dtype=torch.float64, device="cuda")
    t_out = torch.full((2, B), -9, dtype=torch.int32, device="cuda")
    state, src = pb["xinit"].copy(), np.arange(B, dtype=np.int32)
    n_ok, n_ok_tick, support_sum = 0, [], 0
    for tick in range(cases.TICKS):
        pred = cases.prediction(pb, tick)
        mode = np.full(B, 0 if tick == 0 else 1, np.int32)                    # tick 0: the warm start given with the batch; then the shifted plan
        t_state, t_mode, t_src, t_pred, t_sx = _up(state), _up(mode), _up(src), _up(pred), _up(state[:, 0])
        torch.cuda.synchronize()
        # ---- A: one stream, nothing read back before the support is enqueued
        A.warmstart(t_state.data_ptr(), t_mode.data_ptr(), t_src.data_ptr())
        A.sample_scenarios(t_pred.data_ptr(), t_prob.data_ptr(), B, M, cases.MODES, S_CEN, cases.SEED + tick, t_smp.data_ptr())
        A.scenario_discard(t_smp.data_ptr(), M * S_CEN, S_CEN, cases.N_DISCARD, t_sc.data_ptr(), RADIUS)
        SA.halfspaces(cols, t_smp.data_ptr(), M * S_CEN, t_sc.data_ptr(), t_sx.data_ptr(), RADIUS, disc_offset=cases.DISC_OFFSET)
        A.solve(sync=False)
        SA.support_async(cols, S_CEN, cases.TOL, t_out[0].data_ptr(), t_out[1].data_ptr())
        A.synchronize()
        got, rows_a, (x0_a, xinit_a) = A.get(), A.debug_get_params(), A.debug_get_x0()
        sup_a, act_a = t_out.cpu().numpy()
        marks_a, empty_a = A.scenario_discarded(S_CEN), A.scenario_empty_stages()
        # ---- H: the same tick built on the host
        H.warmstart(t_state.data_ptr(), t_mode.data_ptr(), t_src.data_ptr())
        H.synchronize()
        x0_h, xinit_h = H.debug_get_x0()
        rows_h, which, marks_h, empty_h = cases.host_rows(pm, pb["params"], xinit_h, x0_h, pred, pb["prob"], cases.SEED + tick)
        H.set_batch(xinit_h, x0_h, rows_h); H.solve(); ref = H.get()
        sup_h, act_h = cases.host_support(pm, ref["xtraj"], rows_h, which)
        # ---- K: the hand-written kernel on the host-built batch
        K.set_batch(xinit_h, x0_h, rows_h); K.solve(); hand = K.get()
        ok = ref["exit_code"] == 1
        print(f"[stack scenario ticks] tick {tick}: exit codes {got['exit_code'].tolist()} (host {ref['exit_code'].tolist()}, hand-written {hand['exit_code'].tolist()}), "
              f"rows bitwise equal {np.array_equal(rows_a, rows_h)}, max |rows - host| {np.abs(rows_a - rows_h).max():.3e}, support {sup_a.tolist()} (mirror {sup_h.tolist()}), "
              f"active rows {act_a.tolist()}, empty stages {empty_a.tolist()}")
        if ok.any():
            print(f"[stack scenario ticks]   generated vs hand-written: max |x| difference {np.abs(got['xtraj'][ok] - hand['xtraj'][ok]).max():.3e}, "
                  f"max relative objective difference {np.abs(got['pobj'][ok] / hand['pobj'][ok] - 1.0).max():.3e}")
        assert np.array_equal(x0_a, x0_h) and np.array_equal(xinit_a, xinit_h)
        assert np.array_equal(marks_a, marks_h) and np.array_equal(empty_a, empty_h)
        assert not (rows_a[:, :, cols] == -3.0).any()                        # every blanked column was written on the device
        assert np.array_equal(rows_a, rows_h)
        _equal(got, ref, tick)
        assert np.array_equal(sup_a, sup_h) and np.array_equal(act_a, act_h)
        assert ok.any(), tick
        assert np.array_equal(got["exit_code"], hand["exit_code"]) and np.array_equal(got["sqp_iter"], hand["sqp_iter"])
        assert np.array_equal(got["qp_iter_total"][ok], hand["qp_iter_total"][ok])
        np.testing.assert_allclose(got["xtraj"][ok], hand["xtraj"][ok], rtol=0, atol=1e-9)
        np.testing.assert_allclose(got["pobj"][ok], hand["pobj"][ok], rtol=1e-10)
        n_ok += int(ok.sum()); n_ok_tick.append(int(ok.sum())); support_sum += int(sup_a[ok].sum())
        state, src = cases.next_states(ref, xinit_h)
    print(f"[stack scenario ticks] successful solves per tick {n_ok_tick} of {B}, support summed over them {support_sum}")
    assert support_sum > 0
    A.close(); H.close(); K.close()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_launches_nothing():
    """On the generated safe_horizon handle.  Each refusal raises solver.TmpcError with a message that names the argument; after a synchronise
    the rows are what they were and the handle still works: the same calls as they should be are accepted.  tmpc_scenario_halfspaces keeps
    refusing with "generated solver", and so does tmpc_scenario_support once the column entry has built the rows."""
    from mpc_planner_amd import scenes, solver
    from mpc_planner_amd.stack_scenario import StackScenario, scenario_columns
    from test_gpu_parity import _generated_lib
    path, meta = _generated_lib("safe_horizon")
    pmap = meta["parameter_map"]
    sc = scenes.make_scene(6, B=8, **cases.CFG5_SCENE)
    cols, npar = scenario_columns(pmap, R), 127
    o = cases.edge_samples("duplicates", sc["x0"])
    n = o.shape[1]
    s = solver.BatchedSolver(solver.default_dims(N=N, lib_path=path), B_max=8, lib_path=path)
    scn = StackScenario(s)
    t_s, t_sc, t_sx = _up(o[None]), _up(np.zeros(8, np.int32)), _up(sc["xinit"][:1, 0].copy())
    t_out = _up(np.full((2, 8), -9, np.int32))
    half_kw = dict(cols=cols, d_samples=t_s.data_ptr(), n_pts=n, d_scene_of=t_sc.data_ptr(), d_state_x=t_sx.data_ptr(), radius=RADIUS)
    sup_kw = dict(cols=cols, n_scenarios=50, tol=1e-3, d_support=t_out[0].data_ptr(), d_active_rows=t_out[1].data_ptr())
    half, sup = "tmpc_stack_scenario_halfspaces", "tmpc_stack_scenario_support"
    # no batch yet
    with pytest.raises(solver.TmpcError, match=half + ".*no batch"):
        scn.halfspaces(**half_kw)
    with pytest.raises(solver.TmpcError, match=sup + ".*not built by tmpc_stack_scenario_halfspaces"):
        scn.support_async(**sup_kw)
    start = cases.sentinel(sc["params"], cols)
    s.set_batch(sc["xinit"], sc["x0"], start)
    column_checks = [(dict(cols=None), "NULL argument"), (dict(cols=cols[:-1] + [npar]), "outside"), (dict(cols=[-1] + cols[1:]), "outside"),
                     (dict(cols=cols[:-1] + [cols[0]]), "duplicate"), (dict(cols=[]), "n_rows"), (dict(cols=list(range(1 + 3 * 43))), "n_rows.*at most 42")]
    bad = {
        half: column_checks + [(dict(d_samples=None), "NULL argument"), (dict(d_scene_of=None), "NULL argument"), (dict(d_state_x=None), "NULL argument"),
                               (dict(n_pts=0), "n_pts"), (dict(n_pts=-4), "n_pts"), (dict(n_pts=6000), "n_pts.*LDS")],
        sup: column_checks + [(dict(d_support=None), "NULL argument"), (dict(n_scenarios=0), "n_scenarios"), (dict(n_scenarios=8193), "n_scenarios"),
                              (dict(tol=-1.0), "tol"), (dict(), "not built by tmpc_stack_scenario_halfspaces")],      # support before halfspaces
    }
    calls = {half: (scn.halfspaces, half_kw), sup: (scn.support_async, sup_kw)}
    for name, (fn, kw) in calls.items():
        for change, msg in bad[name]:
            with pytest.raises(solver.TmpcError, match=name + ".*" + msg):
                fn(**dict(kw, **change))
    with pytest.raises(ValueError, match="per row"):
        scn.halfspaces(**dict(half_kw, cols=cols[:-1]))
    null = C.c_void_p()
    assert s.lib.tmpc_stack_scenario_halfspaces(null, None, 24, null, 300, null, null, 0.7, 0.0) == -1          # no handle
    assert s.lib.tmpc_stack_scenario_support(null, None, 24, 50, 1e-3, null, null) == -1
    # tmpc_hip.h's entries refuse in a generated solver
    with pytest.raises(solver.TmpcError, match="tmpc_scenario_halfspaces.*generated solver"):
        s.scenario_halfspaces(t_s.data_ptr(), n, R, t_sc.data_ptr(), t_sx.data_ptr(), RADIUS)
    with pytest.raises(solver.TmpcError, match="tmpc_scenario_support"):
        s.scenario_support(50)
    s.synchronize()
    assert np.array_equal(s.debug_get_params(), start) and (t_out.cpu().numpy() == -9).all()          # none of the refused calls wrote anything
    # ---- accepted: the same calls as they should be
    scn.halfspaces(**half_kw)
    s.solve()
    scn.support_async(**sup_kw)
    s.synchronize()
    got = s.debug_get_params()
    assert (got[:, :, cols] != start[:, :, cols]).all() and (t_out.cpu().numpy() >= 0).all()
    # support with another n_rows than the rows were built with; the layout-bound support after the column halfspaces ran
    with pytest.raises(solver.TmpcError, match=sup + ".*another n_rows"):
        scn.support_async(**dict(sup_kw, cols=cols[:1 + 3 * 12]))
    with pytest.raises(solver.TmpcError, match="tmpc_scenario_support.*generated solver"):
        s.scenario_support(50)
    # a new batch forgets the bookkeeping
    s.set_batch(sc["xinit"], sc["x0"], start)
    with pytest.raises(solver.TmpcError, match=sup + ".*not built by tmpc_stack_scenario_halfspaces"):
        scn.support_async(**sup_kw)
    scn.halfspaces(**half_kw)
    s.synchronize()
    assert np.array_equal(s.debug_get_params(), got)                                                  # and the handle is as usable as before
    s.close()
