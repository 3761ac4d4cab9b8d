"""Control-tick kernel (tmpc_set_latency_mode 3, four waves per trajectory) of GENERATED solver libraries: the run-time-shape instantiations compiled
around emitted stage functions, with the stage linearisation split over the four waves by content (csrc/tmpc_kernels.hpp, the
four-wave form of linearise).  Every demo stack with rows, both horizon ranges: against the CPU oracle (the interface's rule for another
factorisation of the Newton systems: _compare_relaxed_iterations), against the product library's hand-written kernels of the same mode, and -- the
new exchange region -- bitwise from launch to launch, alone as in a batch, and after the LDS was filled with NaN patterns.

Latency mode 2 is NOT offered by generated libraries, and the tests assert that.  Its two-wave instantiations around emitted stage functions passed
every check of this file when they were built, but they did not meet the project's rule for a tick mode -- every run below every run of the
default kernel at the same shape (time_solve, five alternating runs, ms per launch; profiles/generated_tick_kernels.json):
    tmpc_cfg2   N = 20, 64 trajectories: mode 2 1.084 - 1.089, default kernel 1.007 - 1.009 (mode 3: 0.900 - 0.901)
    tmpc_cfg2   N = 20,  5 trajectories: mode 2 1.176 - 1.181, default kernel 1.098 - 1.102 (mode 3: 0.975 - 0.984)
    jackal_tmpc N = 30,  5 trajectories: mode 2 1.357 - 1.372, default kernel 1.252 - 1.255 (mode 3: 1.095 - 1.105)
    jackal_tmpc N = 30, 64 trajectories: mode 2 1.303 - 1.307, default kernel 1.220 - 1.222 (mode 3: 1.045 - 1.050)
so the slot stays empty: set_latency_mode(2) answers False and the default kernel runs."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

NARROW = "lat3=fast<-1,4,12,256,ScanQuad,0>"              # N <= 20
WIDE = "lat3=fast<-1,6,8,256,ScanQuadT<2>,0>"             # 21 <= N <= 31
FIELDS = ("xtraj", "utraj", "pobj", "exit_code", "qp_status", "sqp_iter", "qp_iter_total", "res_eq")


def _gen_solver(name, N, B, **kw):
    from mpc_planner_amd import solver
    from test_gpu_parity import _generated_lib
    path, _ = _generated_lib(name)
    return solver.BatchedSolver(solver.default_dims(N=N, lib_path=path, **kw), B_max=B, lib_path=path)


def _solve(s, sc, mode=None):
    if mode is not None:
        assert s.set_latency_mode(mode), f"mode {mode} is not offered: {s.kernel_info()}"
    s.set_batch(sc["xinit"], sc["x0"], sc["params"]); s.solve()
    return s.get()


def _mode_2_is_not_offered(s, sc):
    """set_latency_mode(2) answers False, names no kernel, and the solve is the default kernel's bit for bit."""
    base = _solve(s, sc, 0)
    assert s.set_latency_mode(2) is False and s.latency_mode_capacity(2) == 0 and "lat2=" not in s.kernel_info()
    s.solve(); got = s.get()
    for k in FIELDS:
        assert np.array_equal(got[k], base[k]), k
    assert s.set_latency_mode(0) is True


@functools.lru_cache(maxsize=None)
def _cfg2_case(scene, B=64, N=20, tmpc_pp=False):
    """A cfg-2 scene and the oracle's solve of it (computed once, shared, never written to)."""
    import oracle_lib as O
    from mpc_planner_amd import scenes
    sc = scenes.make_scene(scene, N=N, M=8, B=B, **(dict(tmpc_pp=True) if tmpc_pp else {}))
    n = sc["xinit"].shape[0]
    xt, ut, info = O.solve_batch(O.problem(N=N, S=5, n_lin=8, M=8), sc["xinit"], sc["x0"].reshape(n, -1), sc["params"].reshape(n, -1))
    return sc, (xt, ut, info)


def _against_oracle(got, ref, at_least):
    from test_gpu_parity import _compare_relaxed_iterations
    xt, ut, info = ref
    assert (info["exit_code"] == 1).sum() >= at_least, (info["exit_code"] == 1).sum()
    return _compare_relaxed_iterations(got, xt, ut, info)


def _against_product(got, sc, mode, N=20, relaxed_iterations=False):
    """The hand-written kernels of the product library in `mode` on the same inputs (the generated T-MPC stack has their parameter layout)."""
    from mpc_planner_amd import solver
    n = sc["xinit"].shape[0]
    s0 = solver.BatchedSolver(solver.default_dims(N=N, S=5, n_lin=8, M=8), B_max=n)
    ref = _solve(s0, sc, mode)
    s0.close()
    assert np.array_equal(got["exit_code"], ref["exit_code"]) and np.array_equal(got["sqp_iter"], ref["sqp_iter"])
    ok = ref["exit_code"] == 1
    if relaxed_iterations:                                                   # (the interface's promise between two roundings of the same algorithm)
        dit = np.abs(got["qp_iter_total"][ok] - ref["qp_iter_total"][ok])
        assert dit.max() <= 2 and (dit > 0).mean() <= 0.10, (dit.max(), (dit > 0).mean())
    err = max(np.abs(got["xtraj"][ok] - ref["xtraj"][ok]).max(), np.abs(got["utraj"][ok] - ref["utraj"][ok]).max()) if ok.any() else 0.0
    print(f"[generated tick] generated mode 3 against hand-written mode {mode}: {err:.2e} on {int(ok.sum())} solves")
    assert err < 1e-8, err
    return int(ok.sum())


def _bitwise_trio(s, sc, got):
    """A second launch, a launch after the LDS was poisoned, and entry 9 alone: bitwise the first result."""
    s.solve(); again = s.get()
    for k in FIELDS:
        assert np.array_equal(again[k], got[k]), ("second launch", k)
    s.debug_poison_lds()
    s.solve(); after = s.get()
    for k in FIELDS:
        assert np.array_equal(after[k], got[k]), ("after debug_poison_lds", k)
    s.set_batch(sc["xinit"][9:10], sc["x0"][9:10], sc["params"][9:10]); s.solve(); one = s.get()
    for k in FIELDS:
        assert np.array_equal(one[k][0], got[k][9]), ("entry 9 alone", k)


# ---- tmpc_cfg2, N = 20 ---------------------------------------------------------------------------------------------------------------------------
def test_cfg2_offers_mode_3_and_names_it():
    from mpc_planner_amd import solver
    s = _gen_solver("tmpc_cfg2", 20, 8)
    s0 = solver.BatchedSolver(solver.default_dims(N=20, S=5, n_lin=16, M=0), B_max=8)     # a product handle with as many rows: the same run-time-shape instantiation
    assert s.set_latency_mode(3) is True
    info = s.kernel_info()
    assert NARROW in info and "lat2=" not in info and "lat1=" not in info, info
    assert NARROW in s0.kernel_info()
    assert s.latency_mode_capacity(3) == s0.latency_mode_capacity(3) > 0
    assert s.set_latency_mode(2) is False and s.latency_mode_capacity(2) == 0          # (see the module's text)
    assert s.set_latency_mode(1) is False and s.latency_mode_capacity(1) == 0
    assert s.set_latency_mode(0) is True
    s.close(); s0.close()


@pytest.mark.parametrize("scene", [0, 3, 7])
def test_cfg2_tick_of_64(scene):
    sc, ref = _cfg2_case(scene)
    s = _gen_solver("tmpc_cfg2", 20, 64)
    got = _solve(s, sc, 3)
    _against_oracle(got, ref, 32)
    _against_product(got, sc, 3)
    _bitwise_trio(s, sc, got)
    s.close()


@pytest.mark.parametrize("mode", [0, 3])
@pytest.mark.parametrize("oid", ["bounds upper", "all off + bounds upper"])
def test_cfg2_with_active_bounds_and_options_off_their_defaults(oid, mode):
    """The generated T-MPC stack under two option cases of tests/solver_option_cases.py (model bounds that bind; those plus dt, erk_steps, reg_eps, ipm_mu0,
    ipm_thr0, n_sqp off their defaults), on its default kernel and on its control-tick kernel, against the hand-written cfg-2 oracle problem under the
    same options: integers equal, 1e-8, the discrimination rule and the active sets of tests/test_gpu_solver_options.py."""
    import solver_option_cases as SC
    import test_gpu_dispatch_matrix as T
    from test_gpu_carried_state import GENERATED_DEFAULT
    from test_gpu_parity import _compare
    r = SC.oracle_runs("N=20 (8,8) S=5", oid)
    sc, opts, xt, ut, info = r["sc"], r["opts"], r["xt"], r["ut"], r["info"]
    B = sc["xinit"].shape[0]
    s = _gen_solver("tmpc_cfg2", 20, B, **opts)
    assert s.set_latency_mode(mode) or mode == 0
    slots, th = T._slots(s.kernel_info())
    slot = T._running(slots, mode, B, th)
    assert (slot, slots[slot]) == (("lat3", NARROW.split("=")[1]) if mode else ("default", GENERATED_DEFAULT)), (slot, slots)
    assert s.npar == sc["params"].shape[2]
    s.set_batch(sc["xinit"], sc["x0"], sc["params"]); s.solve(); got = s.get()
    assert (info["exit_code"] == 1).all()
    worst = max(_compare(got, xt, ut, info))
    dist = SC.distance(got["xtraj"], got["utraj"], xt, ut)
    assert (10.0 * dist[r["mask"]] <= r["moved"][r["mask"]]).all() and r["mask"].mean() >= 0.25, (dist, r["moved"])
    lo, hi = SC.gaps(got["xtraj"], got["utraj"], opts["lb"], opts["ub"])
    assert min(lo.min(), hi.min()) > -SC.VIOLATED
    for side, var in SC.OPTION[oid]["active"]:
        want = SC.active_entries(xt, ut, opts, side, var)
        assert want.sum() >= 2 and np.array_equal(SC.active_entries(got["xtraj"], got["utraj"], opts, side, var), want), (side, var)
    print(f"[generated tick] {oid}: {slot}={slots[slot]}: worst rel diff {worst:.2e}")
    s.close()


@pytest.mark.parametrize("scene", [1, 4])
def test_cfg2_mode_2_keeps_an_empty_slot(scene):
    sc, _ = _cfg2_case(scene)
    s = _gen_solver("tmpc_cfg2", 20, 64)
    _mode_2_is_not_offered(s, sc)
    s.close()


def test_cfg2_deployed_size_4_plus_1_planners():
    sc, ref = _cfg2_case(5, B=4, tmpc_pp=True)
    assert sc["xinit"].shape[0] == 5
    s = _gen_solver("tmpc_cfg2", 20, 5)
    got = _solve(s, sc, 3)
    _against_oracle(got, ref, 3)
    _against_product(got, sc, 3)
    _mode_2_is_not_offered(s, sc)
    s.close()


def test_cfg2_mode_3_equals_the_hand_written_mode_2_to_rounding():
    """Mode 3 is mode 2's algorithm on four waves; a generated library has no mode 2 of its own, so the product's stands in."""
    sc, _ = _cfg2_case(2)
    s = _gen_solver("tmpc_cfg2", 20, 64)
    got = _solve(s, sc, 3)
    s.close()
    assert _against_product(got, sc, 2, relaxed_iterations=True) >= 32


def test_cfg2_disc_offset_takes_the_coupled_mirror_against_its_own_default_kernel():
    """A non-zero ego_disc_0_offset couples psi with x, y in the rows' Hessian: W is not block diagonal and the four-wave linearisation takes MIRROR's
    7 x 7 iteration on wave 0, which no other test of a generated library reaches.  Mode 3 against the same library's default kernel, to rounding, at
    N = 5 and at N = 20.  At N = 5 no obstacle of the scene is within reach, the rows' multipliers stay near zero and the offset moves the result at
    rounding level only (W's cross entries are non-zero all the same, which is all MIRROR's `coupled` test asks); that the library reads the offset at
    all is therefore checked at N = 20, in mode 3: the zero-offset solve differs by more than the tolerance of the comparison."""
    from mpc_planner_amd import scenes
    from test_gpu_parity import _generated_lib
    col = _generated_lib("tmpc_cfg2")[1]["parameter_map"]["ego_disc_0_offset"]
    for N in (5, 20):
        sc = scenes.make_scene(3, N=N, M=8, B=16)
        params = sc["params"].copy()
        params[:, :, col] = 0.1
        zero = dict(xinit=sc["xinit"], x0=sc["x0"], params=sc["params"])
        sc = dict(xinit=sc["xinit"], x0=sc["x0"], params=params)
        s = _gen_solver("tmpc_cfg2", N, sc["xinit"].shape[0])
        base = _solve(s, sc, 0)
        ok = base["exit_code"] == 1
        assert ok.sum() >= ok.size // 2
        got = _solve(s, sc, 3)
        assert NARROW in s.kernel_info(), s.kernel_info()
        assert np.array_equal(got["exit_code"], base["exit_code"]) and np.array_equal(got["sqp_iter"], base["sqp_iter"])
        dit = np.abs(got["qp_iter_total"][ok] - base["qp_iter_total"][ok])
        assert dit.max() <= 2 and (dit > 0).mean() <= 0.10, dit
        err = max(np.abs(got["xtraj"][ok] - base["xtraj"][ok]).max(), np.abs(got["utraj"][ok] - base["utraj"][ok]).max())
        moved = np.abs(_solve(s, zero, 3)["xtraj"][ok] - got["xtraj"][ok]).max()       # mode 3 both
        print(f"[generated tick] disc offset 0.1, N = {N}: mode 3 against mode 0: {err:.2e} on {int(ok.sum())} solves; the offset moves mode 3's trajectories by {moved:.2e}")
        assert err < 1e-8, err
        if N == 20:
            assert moved > 1e-8, moved
        s.close()


# ---- horizon edges on the same library at run-time N ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 5, 19, 21, 22, 31])
def test_horizon_edges(N):
    sc, ref = _cfg2_case(40 + N, B=8, N=N)
    s = _gen_solver("tmpc_cfg2", N, 8)
    got = _solve(s, sc, 3)
    assert (WIDE if N >= 21 else NARROW) in s.kernel_info(), s.kernel_info()
    _against_oracle(got, ref, 4)
    _mode_2_is_not_offered(s, sc)
    s.close()


def test_no_tick_kernels_past_n_31():
    sc, _ = _cfg2_case(72, B=8, N=32)
    s = _gen_solver("tmpc_cfg2", 32, 8)
    base = _solve(s, sc)
    for mode in (2, 3):
        assert s.set_latency_mode(mode) is False and s.latency_mode_capacity(mode) == 0
        s.solve(); got = s.get()
        for k in FIELDS:
            assert np.array_equal(got[k], base[k]), (mode, k)
    assert "lat2=" not in s.kernel_info() and "lat3=" not in s.kernel_info()
    s.close()


# ---- jackal_tmpc: N = 30, Gaussian rows, NH = 10 ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _jackal_case(scene, B=16):
    import oracle_lib as O
    from mpc_planner_amd import scenes
    sc = scenes.make_scene(scene, N=30, M=5, S=3, B=B, chance=True)
    xt, ut, info = O.solve_batch(O.problem(N=30, S=3, n_lin=5, M=0, n_gauss=5), sc["xinit"], sc["x0"].reshape(B, -1), sc["params"].reshape(B, -1))
    return sc, (xt, ut, info)


def test_jackal_default_stack_at_its_shipped_horizon():
    s = _gen_solver("jackal_tmpc", 30, 16, S=3)
    for scene in (1, 2):
        sc, ref = _jackal_case(scene)
        got = _solve(s, sc, 3)
        assert WIDE in s.kernel_info(), s.kernel_info()
        _against_oracle(got, ref, 8)
    _bitwise_trio(s, sc, got)
    sc, _ = _jackal_case(1)
    _mode_2_is_not_offered(s, sc)
    s.close()


# ---- safe_horizon: slack model, NH = 24 -------------------------------------------------------------------------------------------------------------
def test_safe_horizon_slack_model_and_one_iteration_calls():
    import oracle_lib as O
    from mpc_planner_amd import scenes
    from test_gpu_parity import _generated_lib
    B = 32
    sc = scenes.make_scene(5, B=B, N=20, M=8, slack=True, n_scenario=24)
    assert dict(sc["pm"]._params) == _generated_lib("safe_horizon")[1]["parameter_map"]
    ref = O.solve_batch(O.problem(N=20, S=5, n_lin=0, M=0, n_slk=24, slack=1), sc["xinit"], sc["x0"].reshape(B, -1), sc["params"].reshape(B, -1))
    s = _gen_solver("safe_horizon", 20, B)
    whole = _solve(s, sc, 3)
    assert NARROW in s.kernel_info(), s.kernel_info()
    _against_oracle(whole, ref, B // 2)
    s.set_batch(sc["xinit"], sc["x0"], sc["params"])                       # ten one-iteration calls on the tick kernel: one solve(), bit for bit
    s.solve_iterations(1, complete=False)
    for i in range(9):
        s.solve_iterations(1, keep_iterate=True, keep_multipliers=True, complete=(i == 8))
    steps = s.get()                                                         # (sqp_iter / qp_iter_total count the last call only)
    for k in ("xtraj", "utraj", "pobj", "exit_code", "qp_status", "res_eq"):
        assert np.array_equal(steps[k], whole[k]), k
    _mode_2_is_not_offered(s, sc)
    s.close()


# ---- goal_so_unicycle: NH = 4 (two rows per row wave), the model with the inert fifth state -----------------------------------------------------------
def test_second_order_unicycle_stack():
    import oracle_lib as O
    from test_gpu_second_order_unicycle import _problem
    B = 16
    xinit, x0, params = _problem(B)
    sc = dict(xinit=xinit, x0=x0, params=params)
    ref = O.solve_batch(O.problem(N=20, S=5, n_lin=0, M=4, goal_stack=1), xinit, x0.reshape(B, -1), params.reshape(B, -1))
    s = _gen_solver("goal_so_unicycle", 20, B)
    got = _solve(s, sc, 3)
    assert NARROW in s.kernel_info(), s.kernel_info()
    _against_oracle(got, ref, B // 2)
    assert not got["xtraj"][:, :, 4].any()                                  # the padding slot stays 0
    _mode_2_is_not_offered(s, sc)
    s.close()


# ---- path_velocity: NH = 2 (one row per row wave), no oracle --------------------------------------------------------------------------------------------
def test_path_velocity_stack_against_its_own_default_kernel():
    from mpc_planner_amd import modules as md
    from test_gpu_parity import _generated_lib
    import test_gpu_path_velocity as PV
    _, meta = _generated_lib("path_velocity")
    gs = PV._gen_scenes()
    params, spl, _ = PV._base_params(meta, gs)
    pm = PV._Params(meta["parameter_map"])
    state = gs["state"].copy()                                             # (the scenes are cached: never written to)
    for q, fit in enumerate(gs["fits"]):                                   # the host mirrors' first tick (test_generated_stack_end_to_end_five_ticks)
        tr = md.track_path(fit["path"], fit["length"], state[q, :2], PV.S_GEN, segment=-1, search_range=2)
        state[q, 4] = tr["s"]
        vwin = md.path_velocity_window(fit["velocity"] if PV.HAS_PROFILE[q] else None, fit["count"], tr["segment"], PV.S_GEN, PV.REF_V)
        for b in (2 * q, 2 * q + 1):
            params[b][:, spl] = tr["window"].ravel()
            md.path_velocity_set_parameters(pm, params[b], vwin)
    assert not (params == PV.SENTINEL).any()
    xinit = np.repeat(state, 2, axis=0)
    x0 = np.stack([md.initialize_with_forward_propagation(x, PV.N, 0.2) for x in xinit])
    sc = dict(xinit=xinit, x0=x0, params=params)
    s = _gen_solver("path_velocity", PV.N, PV.B_GEN)
    base = _solve(s, sc, 0)
    ok = base["exit_code"] == 1
    assert ok.sum() >= PV.B_GEN // 2
    got = _solve(s, sc, 3)
    assert NARROW in s.kernel_info(), s.kernel_info()
    assert np.array_equal(got["exit_code"], base["exit_code"]) and np.array_equal(got["sqp_iter"], base["sqp_iter"])
    dit = np.abs(got["qp_iter_total"][ok] - base["qp_iter_total"][ok])
    assert dit.max() <= 2 and (dit > 0).mean() <= 0.10, dit
    err = max(np.abs(got["xtraj"][ok] - base["xtraj"][ok]).max(), np.abs(got["utraj"][ok] - base["utraj"][ok]).max())
    assert err < 1e-8, err
    _mode_2_is_not_offered(s, sc)
    s.close()
