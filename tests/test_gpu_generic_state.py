"""GPU: the generic solve kernel's own copy of the carried-state protocol (tmpc_solve_kernel in csrc/tmpc_kernels.hpp: it loads io.z / io.pi / io.lamh with
the sign flip of the upper-bounded rows and stores them back; slot map; parameter-sharing map).  tests/test_gpu_iterations.py, test_gpu_parity.py and
test_gpu_abi_contracts.py make these checks on shapes that run fast or compact kernels; here they run on two shapes only the generic kernel takes:
N = 33 with 8 + 8 rows (no fast kernel past N = 32) and N = 32 with 18 topology + 18 ellipsoid + 12 decomposition rows on the slack model (62 interior-point
rows per stage; upper-bounded rows n_up = 30 and lower-bounded ellipsoid rows M = 18 both present, so the sign flip of lamh matters).  The oracle is its wide
build (tests/test_oracle_wide.py)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 16
SHAPES = {
    "N=33 (8,8)": (dict(N=33, M=8, B=B), dict(N=33, S=5, n_lin=8, M=8)),
    "N=32 (18,18,12) slack": (dict(N=32, M=18, B=B, slack=True, n_decomp=12), dict(N=32, S=5, n_lin=18, M=18, n_slk=12, slack=1)),
}
FIELDS = ("xtraj", "utraj", "pobj", "exit_code", "qp_status", "sqp_iter", "qp_iter_total", "res_eq")
TICKS, DOOMED, DOOMED_TICK = 4, 3, 1          # (trajectory 3 fails at tick 1 and succeeds again at tick 2 on both shapes: its reset shows in its next trajectory)


def _solver(shape, B_max=B, **opts):
    from mpc_planner_amd import solver
    s = solver.BatchedSolver(solver.default_dims(**SHAPES[shape][1], **opts), B_max=B_max)
    assert "default=generic<0>" in s.kernel_info(), s.kernel_info()
    return s


def _scene(shape, scene):
    from mpc_planner_amd import scenes
    sc = scenes.make_scene(scene, **SHAPES[shape][0])
    assert sc["xinit"].shape[0] == B
    return sc


@functools.lru_cache(maxsize=None)
def _oracle_loop(shape):
    """The closed loop of test_gpu_iterations.test_multipliers_carried_across_ticks_match_oracle on the oracle alone (every tick's inputs follow from the
    oracle's previous results): per tick (xinit, x0, params, xtraj, exit codes), and how far carrying the multipliers moves a trajectory."""
    import oracle_lib as O
    from mpc_planner_amd import modules as md
    sc = _scene(shape, 12)
    pm = sc["pm"]; pkw = SHAPES[shape][1]; N = pkw["N"]
    pb = O.problem(**pkw); fresh = O.problem(**pkw)
    assert pb._wide
    xinit, x0, params = sc["xinit"].copy(), sc["x0"].copy(), sc["params"].copy()
    pi = np.zeros((B, (N + 1) * 5)); lamh = np.zeros((B, N * pb.capacity[1]))
    ticks = []; differs_from_fresh = 0.0
    for tick in range(TICKS):
        p_t = params.copy()
        if tick == DOOMED_TICK:                                    # contradictory topology rows on one trajectory for this tick only
            for j, sg in ((0, 1.0), (1, -1.0)):
                p_t[DOOMED, 1:, pm.index(f"lin_constraint_{j}_a1")] = sg
                p_t[DOOMED, 1:, pm.index(f"lin_constraint_{j}_a2")] = 0.0
                p_t[DOOMED, 1:, pm.index(f"lin_constraint_{j}_b")] = sg * x0[DOOMED, 1:-1, 2] - 5.0
        xt = np.zeros((B, N + 1, pb.nxe)); ut = np.zeros((B, N, 2)); ec = np.zeros(B, np.int32)
        for b in range(B):
            had = pi[b].any() or lamh[b].any()
            xt[b], ut[b], info = O.solve_carry(pb, xinit[b], x0[b], p_t[b], 10, pi[b], lamh[b])
            ec[b] = info.exit_code
            if had and info.exit_code == 1:
                xf, _, _ = O.solve(fresh, xinit[b], x0[b], p_t[b])
                differs_from_fresh = max(differs_from_fresh, np.abs(xf - xt[b]).max())
        if tick == DOOMED_TICK:                                    # Solver_acados_reset: the failed Solver starts its next tick like a new capsule
            assert ec[DOOMED] != 1 and not pi[DOOMED].any() and not lamh[DOOMED].any()
        ticks.append((xinit.copy(), x0.copy(), p_t, xt, ec))
        ok = ec == 1
        for b in range(B):                                         # the robot moves to the first predicted state of its own plan; shifted warm start
            src_x, src_u = (xt[b], ut[b]) if ok[b] else (x0[b][:, 2:], x0[b][:-1, :2])
            state = src_x[1].copy()
            xinit[b] = state
            x0[b] = md.initialize_warmstart(x0[b].copy(), state, src_x, src_u, shift_previous_solution_forward=True)
    return ticks, differs_from_fresh


@pytest.mark.parametrize("shape", list(SHAPES))
def test_generic_kernel_carries_multipliers_across_ticks_like_the_oracle(shape):
    ticks, differs_from_fresh = _oracle_loop(shape)
    assert differs_from_fresh > 1e-7          # carrying the multipliers matters on this scene (exact Hessian of the first RTI iteration)
    s = _solver(shape)
    worst = 0.0
    for tick, (xinit, x0, p_t, xt, ec) in enumerate(ticks):
        s.set_batch(xinit, x0, p_t)
        s.solve_iterations(10, keep_iterate=False, keep_multipliers=True)
        g = s.get()
        if tick == DOOMED_TICK + 1:
            after_failure = g
        assert (g["exit_code"] == ec).all(), (tick, g["exit_code"], ec)
        ok = ec == 1
        assert ok.sum() >= B // 2, (tick, ec)
        sx = np.maximum(np.abs(xt[ok]).max(axis=2, keepdims=True), 1.0)
        err = (np.abs(g["xtraj"][ok] - xt[ok]) / sx).max()
        worst = max(worst, err)
        assert err < 1e-6, (tick, err)
    # the doomed Solver's tick after its failure: had its multipliers survived the failure its trajectory would be off by what carrying them does
    assert ticks[DOOMED_TICK][4][DOOMED] != 1 and ticks[DOOMED_TICK + 1][4][DOOMED] == 1
    s.close()
    # ... and directly: that tick on a handle with nothing stored gives the doomed Solver's bits, and not the bits of the Solvers that carried theirs
    f = _solver(shape)
    xinit, x0, p_t, _, ec = ticks[DOOMED_TICK + 1]
    f.set_batch(xinit, x0, p_t); f.solve_iterations(10, keep_iterate=False, keep_multipliers=True); fresh = f.get()
    f.close()
    for k in FIELDS:
        np.testing.assert_array_equal(after_failure[k][DOOMED], fresh[k][DOOMED], err_msg=k)
    carried = [b for b in range(B) if b != DOOMED and ec[b] == 1 and ticks[DOOMED_TICK][4][b] == 1]
    assert any(not np.array_equal(after_failure["xtraj"][b], fresh["xtraj"][b]) for b in carried)
    print(f"[state] {shape}: {TICKS} ticks, worst rel diff {worst:.2e}, carried multipliers move the oracle by {differs_from_fresh:.2e}")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_generic_kernel_one_iteration_calls_equal_one_solve(shape):
    """test_gpu_iterations.test_one_iteration_calls_equal_one_solve on the generic kernel: bitwise, including loops that end early and doomed entries."""
    import test_gpu_parity as T
    sc = T._make_infeasible(_scene(shape, 7), [4, 9])
    s = _solver(shape, qp_iter_max=6)                                  # a low QP iteration limit: some loops end early
    s.set_batch(sc["xinit"], sc["x0"], sc["params"]); s.solve(); ref = s.get()
    assert (ref["sqp_iter"] < 10).any() and (ref["sqp_iter"] == 10).any() and (ref["exit_code"] != 1).any()
    s.set_batch(sc["xinit"], sc["x0"], sc["params"]); s.solve_iterations(10); one = s.get()
    for k in FIELDS:
        np.testing.assert_array_equal(one[k], ref[k], err_msg=k)
    s.set_batch(sc["xinit"], sc["x0"], sc["params"])
    s.solve_iterations(1, complete=False)                          # initializeOneIteration + solveOneIteration
    for i in range(8):
        s.solve_iterations(1, keep_iterate=True, keep_multipliers=True, complete=False)
    s.solve_iterations(1, keep_iterate=True, keep_multipliers=True, complete=True)
    g = s.get()                                                        # (sqp_iter / qp_iter_total count the last call only)
    for k in ("xtraj", "utraj", "pobj", "exit_code", "qp_status", "res_eq"):
        np.testing.assert_array_equal(g[k], ref[k], err_msg=k)
    s.close()
    print(f"[state] {shape}: one-by-one == solve; sqp_iter {np.bincount(ref['sqp_iter'], minlength=11).tolist()}, failed {int((ref['exit_code'] != 1).sum())}")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_generic_kernel_keys_the_state_by_slot(shape):
    """test_gpu_iterations.test_slot_map_keys_the_state_by_slot_not_by_batch_position on the generic kernel."""
    sc = _scene(shape, 5)
    r = _solver(shape)
    r.set_batch(sc["xinit"], sc["x0"], sc["params"]); r.solve_iterations(10, keep_multipliers=True, new_solve=True); t1 = r.get()
    r.solve_iterations(10, keep_multipliers=True, new_solve=True); t2 = r.get()
    assert np.abs(t2["xtraj"] - t1["xtraj"]).max() > 1e-9                     # carried multipliers matter on this scene
    s = _solver(shape)
    perm = np.random.default_rng(3).permutation(B)
    s.set_batch(sc["xinit"][perm], sc["x0"][perm], sc["params"][perm]); s.set_slots(perm)     # batch entry b is Solver perm[b]
    s.solve_iterations(10, keep_multipliers=True, new_solve=True); a = s.get()
    for k in FIELDS:
        np.testing.assert_array_equal(a[k], t1[k][perm], err_msg=k)
    sub = np.array([11, 2, 7, 14, 0])
    s.set_batch(sc["xinit"][sub], sc["x0"][sub], sc["params"][sub]); s.set_slots(sub)
    s.solve_iterations(10, keep_multipliers=True, new_solve=True); b = s.get()
    for k in FIELDS:
        np.testing.assert_array_equal(b[k], t2[k][sub], err_msg=k)             # each got its OWN first-tick multipliers
    # a slot nothing was stored in starts fresh whatever the keep-flags say
    f = _solver(shape)
    f.set_batch(sc["xinit"][:4], sc["x0"][:4], sc["params"][:4]); f.set_slots([12, 13, 14, 15])
    f.solve_iterations(10, keep_iterate=True, keep_multipliers=True); c = f.get()
    np.testing.assert_array_equal(c["xtraj"], t1["xtraj"][:4])
    for x in (r, s, f):
        x.close()
    print(f"[state] {shape}: slot map; second tick moves the trajectories by {np.abs(t2['xtraj'] - t1['xtraj']).max():.2e}")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_generic_kernel_param_sharing_is_bitwise_neutral_and_strict_mode_refuses(shape):
    """test_gpu_parity.test_param_sharing_hint_is_bitwise_neutral and test_gpu_abi_contracts.test_strict_param_sharing_fails_instead_of_falling_back on
    the generic kernel: base_of in groups of 4."""
    from mpc_planner_amd import solver as S
    sc = _scene(shape, 3)
    s = _solver(shape)
    base = S.param_sharing_map(sc["params"], s.dims, 4)
    assert (base == np.arange(B) // 4 * 4).all(), base                         # one scene: every entry shares all but its own rows
    s.set_batch(sc["xinit"], sc["x0"], sc["params"]); s.set_param_sharing(None); s.solve(); ref = s.get()
    assert (ref["exit_code"] == 1).sum() >= B // 2
    s.set_param_sharing(base); s.solve(); got = s.get()
    for k in FIELDS:
        assert np.array_equal(ref[k], got[k]), k
    # copies not maintained: the shared columns of every non-base entry poisoned -- the same bits (they are never read) ...
    own = S.own_parameter_columns(s.dims)
    p = sc["params"].copy().reshape(B, s.N, -1)
    shared = np.setdiff1d(np.arange(p.shape[2]), own)
    for b in range(B):
        if base[b] != b:
            p[b][:, shared] = np.nan
    s.set_batch(sc["xinit"], sc["x0"], p); s.set_param_sharing(base, copies_not_maintained=True); s.solve(); strict = s.get()
    for k in FIELDS:
        assert np.array_equal(ref[k], strict[k]), k
    s.solve_iterations(10); it = s.get()
    assert np.array_equal(it["xtraj"], ref["xtraj"])
    # ... and whatever would read them is refused: the generic kernel's profiled run, a solve after new inputs dropped the map
    with pytest.raises(S.TmpcError):
        s.debug_profile()
    s.set_batch(sc["xinit"], sc["x0"], p)
    with pytest.raises(S.TmpcError, match="not in force"):
        s.solve()
    with pytest.raises(S.TmpcError, match="not in force"):
        s.solve_iterations(1)
    s.set_param_sharing(None)                                   # cleared: a plain handle again
    s.set_batch(sc["xinit"], sc["x0"], sc["params"]); s.solve()
    assert np.array_equal(s.get()["xtraj"], ref["xtraj"])
    s.close()
    print(f"[state] {shape}: sharing in groups of 4 bitwise neutral, strict mode refuses")
