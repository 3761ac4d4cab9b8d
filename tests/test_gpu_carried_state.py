"""GPU: the carried solver state (StateIO: z, pi, lamh, stopped, valid) of every solve-kernel family, against an oracle that carries its multipliers itself.

The code that loads and stores a slot's state exists three times (tmpc_solve_fast_kernel and tmpc_solve_compact_kernel in csrc/tmpc_fast.hpp, the generic
kernel in csrc/tmpc_kernels.hpp), and in the first two the row multipliers return to lamh through a per-lane map that depends on lanes per stage, waves per
trajectory and the run-time row split.  A device-against-device check cannot see a wrong sign, stride or lane in that store -- the same kernel reads it back
the same wrong way -- so every family runs the closed loop of tests/test_gpu_generic_state.py here: 16 trajectories of scene 12, 4 control ticks, every tick
a shifted primal warm start and the slot's kept multipliers, one trajectory made infeasible at tick 1 (its state is reset, Solver_acados_reset).  The cases
are rows of tests/test_gpu_dispatch_matrix.DISPATCH_CASES, by id; tests/test_carried_state_cpu.py (no GPU) checks the loop's inputs on the oracle alone
and requires a case here for every (kind, lanes per stage, threads, team) the pick functions name.  The second half is the state protocol device
against device, bitwise: slot map, the persistent compact kernel, a mode switch between ticks, tmpc_clear_slot, tmpc_copy_state."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, TICKS, SCENE, DOOMED, DOOMED_TICK = 16, 4, 12, 3, 1
FIELDS = ("xtraj", "utraj", "pobj", "exit_code", "qp_status", "sqp_iter", "qp_iter_total", "res_eq")
HARD = 1e-6                                   # what the project asserts on this loop (test_gpu_iterations, test_gpu_generic_state)

# ids of DISPATCH_CASES.  The last three are not in the list the loop was first drawn up for: they are the remaining (lanes, threads, team) tuples of the pick
# functions (the family guard of tests/test_carried_state_cpu.py), two of them lab twins
LOOP_CASES = [
    "m0 (8,8) N=20", "m0 (8,8) N=20 compact", "m0 (8,8) N=30", "m0 (8,8) N=30 compact", "m0 (8,8) N=32", "m0 (12,12) N=20 compact",
    "m0 (20,8) N=30", "m0 (20,8) N=30 cp2",                                  # the slack model: upper and lower rows both present
    "m0 <-1,13,3> nr=39", "m0 <-1,10,3> nr=30 compact", "m0 <-1,9,6> nr=54", "m0 <-1,12,4> nr=48", "m0 <-1,6,4> nr=24 cp2",
    "m1 (8,8) N=20", "m2 (8,8) N=20", "m2 (8,8) N=31", "m3 (8,8) N=20", "m3 (8,8) N=21", "m3 <-1,4,12> nr=39 N=20",
    "ca (20,8) N=30", "g (5,5) N=30", "cm3 N=30 m3", "sqrt <-1,13,3> N=20",
    "m3 (8,8) N=2",                            # exit codes, integers and trajectories only: at N = 2 carrying changes nothing; the lane map at the smallest horizon
    "sqrt <-1,12,4> N=30", "m2 (8,8) N=20 one wave", "m3 (8,8) N=20 one-wave factorisation",
]
# (kind, lanes per stage, threads, team) tuples of the pick functions without a loop above, and why
EXCLUDED = {
    ("generic", 0, 64, ""): "the generic kernel is no pick_*_kernel instantiation; its closed loop is tests/test_gpu_generic_state.py (two shapes only it takes)",
}
SCENE_OF = {}                                 # case id -> another scene of scenes.make_scene, where scene 12 does not support the loop (none so far)
GENERATED_DEFAULT = "fast<tmpc_gen::NH,0,3,64,Solo,0>"

# Measured on an MI355X: the worst relative difference per stage between device and oracle over the 4 ticks is 5.0e-13 .. 3.7e-10 over the cases,
# 2.5e-16 at N = 2 -- at most 1e-9 everywhere, so every case is also held to the suite's regression line
TIGHT = 1e-8


# The loop with model bounds that bind (tests/solver_option_cases.py "bounds upper": a, v and s from above) in force over the 4 ticks: case id -> (scene, the
# upper bounds).  Derived on the CPU from the oracle's own loop on that scene; no doomed entry -- every Solver carries its multipliers through all 4 ticks.  (What a slot
# keeps is pi and the general rows' lamh: a box row is linear and adds nothing to the Hessian.  The loop is here for the multipliers that were formed next to
# binding box rows, and for the warm start that sits on a bound.)  Preconditions: tests/test_carried_state_cpu.py
BOUNDED_LOOPS = {
    "m0 (8,8) N=20": (19, dict(v=1.8, s=6.5, a=0.5)),             # active entries per tick: v 13 13 12 5, s 0 0 7 7, a 15 7 8 10
    "m0 (20,8) N=30 cp2": (0, dict(v=1.93, s=10.58, a=0.46)),      # v 11 11 11 0, s 0 0 0 11, a 4 4 4 4
}


def bounded_options(cid):
    import solver_option_cases as SC
    return SC._box({}, BOUNDED_LOOPS[cid][1])


def _case(cid, scene=None):
    import test_gpu_dispatch_matrix as T
    (c,) = [c for c in T.DISPATCH_CASES if c["id"] == cid]
    assert isinstance(c["B"], int) and not c["refused"] and not c["doomed"] and not c["disc_offset"], cid
    return dict(c, ids=(SCENE_OF.get(cid, SCENE) if scene is None else scene,), B=B)


def family(name):
    """(kind, lanes per stage, threads, team) of an instantiation name of tmpc_kernel_info."""
    kind, args = name.rstrip(">").split("<", 1)
    a = args.split(",")
    if kind == "generic":
        return ("generic", 0, 64, "")
    return (kind, int(a[2]), int(a[3]), a[4] if kind == "fast" else "")


def _shape_key(c, rf):
    return (c["N"], c["S"], c["n_lin"], c["M"], c["n_slk"], c["cm"], c["gauss"], rf, c["ids"], None if c["scene"] is None else tuple(sorted(c["scene"].items())))


_loops = {}


def oracle_loop(cid, rf=None, fresh=True, opts=None, scene=None):
    """The closed loop on the oracle alone (every tick's inputs follow from the oracle's previous results; a failed entry keeps its old warm start):
    per tick a dict of the inputs (xinit, x0, params) and the oracle's results, and how far carrying the multipliers moves a trajectory against a
    fresh oracle solve of the same inputs.  rf: the Riccati form of the oracle (default: the case's).  opts: orc_problem fields off their defaults, in force
    over the whole loop -- and then no entry is doomed; scene: another scene than the case's.  Cached per shape, shared, never written to."""
    import oracle_lib as O
    import test_gpu_dispatch_matrix as T
    from mpc_planner_amd import modules as md
    c = _case(cid, scene)
    rf = c["rf"] if rf is None else rf
    key = _shape_key(c, rf) + (None if opts is None else tuple(sorted(opts.items())),)
    if key in _loops and (_loops[key][1] is not None or not fresh):
        return _loops[key]
    sc = T._scenes(c, B)
    pm = sc["pm"]; N = c["N"]
    pb = T._problem(dict(c, rf=rf)); fr = T._problem(dict(c, rf=rf))
    for k, v in (opts or {}).items():
        setattr(pb, k, v); setattr(fr, k, v)
    xinit, x0, params = sc["xinit"].copy(), sc["x0"].copy(), sc["params"].copy()
    assert xinit.shape[0] == B and params.shape[2] == pb.npar
    pi = np.zeros((B, (N + 1) * O.NX)); lamh = np.zeros((B, N * pb.capacity[1]))
    ticks = []; differs = 0.0 if fresh else None
    for tick in range(TICKS):
        p_t = params.copy()
        if tick == DOOMED_TICK and opts is None:                   # contradictory topology rows on one trajectory for this tick only
            for j, sg in ((0, 1.0), (1, -1.0)):
                p_t[DOOMED, 1:, pm.index(f"lin_constraint_{j}_a1")] = sg
                p_t[DOOMED, 1:, pm.index(f"lin_constraint_{j}_a2")] = 0.0
                p_t[DOOMED, 1:, pm.index(f"lin_constraint_{j}_b")] = sg * x0[DOOMED, 1:-1, 2] - 5.0
        r = dict(xinit=xinit.copy(), x0=x0.copy(), params=p_t, xtraj=np.zeros((B, N + 1, pb.nxe)), utraj=np.zeros((B, N, 2)),
                 **{k: np.zeros(B, np.int32) for k in ("exit_code", "qp_status", "sqp_iter", "qp_iter_total")})
        for b in range(B):
            had = pi[b].any() or lamh[b].any()
            r["xtraj"][b], r["utraj"][b], info = O.solve_carry(pb, xinit[b], x0[b], p_t[b], 10, pi[b], lamh[b])
            for k in ("exit_code", "qp_status", "sqp_iter", "qp_iter_total"):
                r[k][b] = getattr(info, k)
            if fresh and had and info.exit_code == 1:
                xf, _, _ = O.solve(fr, xinit[b], x0[b], p_t[b])
                differs = max(differs, np.abs(xf - r["xtraj"][b]).max())
            if info.exit_code != 1:                                    # Solver_acados_reset: the failed Solver starts its next tick like a new capsule
                assert not pi[b].any() and not lamh[b].any()
        for v in r.values():
            v.setflags(write=False)
        ticks.append(r)
        ok = r["exit_code"] == 1
        for b in range(B):                                         # the robot moves to the first predicted state of its own plan; shifted warm start
            src_x, src_u = (r["xtraj"][b], r["utraj"][b]) if ok[b] else (x0[b][:, 2:], x0[b][:-1, :2])
            state = src_x[1].copy()
            xinit[b] = state
            x0[b] = md.initialize_warmstart(x0[b].copy(), state, src_x, src_u, shift_previous_solution_forward=True)
    _loops[key] = (ticks, differs)
    return _loops[key]


def check_loop_inputs(cid, ticks, differs):
    """What the scene has to give for the loop to test anything (asserted on the CPU for every case, and again where the GPU test uses the loop)."""
    N = _case(cid)["N"]
    assert ticks[DOOMED_TICK]["exit_code"][DOOMED] == 4, (cid, ticks[DOOMED_TICK]["exit_code"])
    for t, r in enumerate(ticks):
        assert (r["exit_code"] == 1).sum() >= (B - 1 if t else B // 2), (cid, t, r["exit_code"])
    assert (ticks[DOOMED_TICK]["exit_code"] == 1).sum() == B - 1
    if N >= 20 and differs is not None:
        assert differs > 1e-7, (cid, differs)                      # carrying the multipliers matters on this scene (exact Hessian of the first RTI iteration)


def check_bounded_loop_inputs(cid, ticks, differs):
    """The same for the loop of BOUNDED_LOOPS: every entry succeeds at every tick; at every tick at least two of the three bounds are active
    (tests/solver_option_cases.ACTIVE) in at least 2 entries each, and each bound is at some tick (the robot moves: v binds while it accelerates, s once the
    horizon reaches it); no entry sits within THRESHOLD_GUARD of that threshold; no bound is violated; and carrying the multipliers matters."""
    import solver_option_cases as SC
    opts = bounded_options(cid)
    ever = {var: 0 for var in BOUNDED_LOOPS[cid][1]}
    for t, r in enumerate(ticks):
        assert (r["exit_code"] == 1).all(), (cid, t, r["exit_code"])
        lo, hi = SC.gaps(r["xtraj"], r["utraj"], opts["lb"], opts["ub"])
        assert min(lo.min(), hi.min()) > -SC.VIOLATED, (cid, t)
        now = 0
        for var in ever:
            gap = hi[:, SC.VARS.index(var)]
            assert (np.abs(np.abs(gap) - SC.ACTIVE) > SC.THRESHOLD_GUARD).all(), (cid, t, var, gap)
            n = int((np.abs(gap) < SC.ACTIVE).sum())
            ever[var] = max(ever[var], n); now += n >= 2
        assert now >= 2, (cid, t)
    assert min(ever.values()) >= 2, (cid, ever)
    if differs is not None:
        assert differs > 1e-7, (cid, differs)


# ---- handles ---------------------------------------------------------------------------------------------------------------------------------------
def _lab(c, request, monkeypatch):
    if c["lab"]:
        for k, v in c["lab"].items():
            monkeypatch.setenv(k, v)
        request.getfixturevalue("lab_library")


def _handle(c, B_max=B, launch=B, opts=None):
    """A handle of the case's shape in the case's mode; the slot a launch of `launch` entries runs holds the expected instantiation.  opts: tmpc_dims fields
    off their defaults."""
    import test_gpu_dispatch_matrix as T
    from mpc_planner_amd import solver
    dims = T._dims(c)
    for k, v in (opts or {}).items():
        setattr(dims, k, v)
    s = solver.BatchedSolver(dims, B_max=B_max)
    assert s.set_latency_mode(c["mode"]) or c["mode"] == 0
    slots, th = T._slots(s.kernel_info())
    slot = T._running(slots, c["mode"], launch, th)
    assert slots.get(slot) == c["expect"], (slot, slots)
    return s, slot


def _tick(s, r, lo=0, hi=None, **kw):
    s.set_batch(r["xinit"][lo:hi], r["x0"][lo:hi], r["params"][lo:hi])
    s.solve_iterations(10, keep_iterate=False, keep_multipliers=True, **kw)
    return s.get()


def _same_bits(a, b, what, index=slice(None), index_b=None):
    for k in FIELDS:
        np.testing.assert_array_equal(a[k][index], b[k][index if index_b is None else index_b], err_msg=f"{what}: {k}")


def _against_oracle(g, r, relaxed, what):
    """Exit code and SQP count of every entry; QP status and interior-point count of the successful ones (latency mode 2: the rule of
    test_gpu_parity._compare_relaxed_iterations); the worst relative difference per stage of xtraj and utraj on the successful ones."""
    assert (g["exit_code"] == r["exit_code"]).all(), (what, g["exit_code"], r["exit_code"])
    assert (g["sqp_iter"] == r["sqp_iter"]).all(), (what, g["sqp_iter"], r["sqp_iter"])
    ok = r["exit_code"] == 1
    assert ok.sum() >= B // 2, (what, r["exit_code"])
    assert (g["qp_status"][ok] == r["qp_status"][ok]).all(), (what, g["qp_status"], r["qp_status"])
    dit = np.abs(g["qp_iter_total"][ok] - r["qp_iter_total"][ok])
    if relaxed:
        assert dit.max() <= 2 and (dit > 0).mean() <= 0.10, (what, dit)
    else:
        assert dit.max() == 0, (what, g["qp_iter_total"], r["qp_iter_total"])
    sx = np.maximum(np.abs(r["xtraj"][ok]).max(axis=2, keepdims=True), 1.0); su = np.maximum(np.abs(r["utraj"][ok]).max(axis=2, keepdims=True), 1.0)
    return max((np.abs(g["xtraj"][ok] - r["xtraj"][ok]) / sx).max(), (np.abs(g["utraj"][ok] - r["utraj"][ok]) / su).max())


def _closed_loop(cid, make, relaxed, opts=None, scene=None):
    """The loop on handles `make()` builds: per tick against the oracle; then the doomed entry's tick after its failure against a handle with nothing
    stored.  opts, scene: of oracle_loop (the handles `make()` builds have the same options) -- no entry is doomed then."""
    ticks, differs = oracle_loop(cid, opts=opts, scene=scene)
    if opts is None:
        check_loop_inputs(cid, ticks, differs)
    else:
        check_bounded_loop_inputs(cid, ticks, differs)
    N = ticks[0]["utraj"].shape[1]
    s = make()
    worst = 0.0; got = []
    for t, r in enumerate(ticks):
        g = _tick(s, r); got.append(g)
        err = _against_oracle(g, r, relaxed, (cid, t))
        worst = max(worst, err)
        print(f"[carried] {cid}: tick {t}: successes {int((r['exit_code'] == 1).sum())}/{B}, rel diff {err:.2e}")
    s.close()
    print(f"[carried] {cid}: worst rel diff over {TICKS} ticks {worst:.3e}; carried multipliers move the oracle by {differs:.2e}")
    assert worst < HARD, worst
    assert worst < TIGHT, worst
    if opts is not None:
        import solver_option_cases as SC
        # the bounds bind on the device where they bind on the oracle, tick by tick; none is violated; and the multipliers the Solvers carried matter
        for t, (g, r) in enumerate(zip(got, ticks)):
            lo, hi = SC.gaps(g["xtraj"], g["utraj"], opts["lb"], opts["ub"])
            assert min(lo.min(), hi.min()) > -SC.VIOLATED, (cid, t)
            for var in BOUNDED_LOOPS[cid][1]:
                want = SC.active_entries(r["xtraj"], r["utraj"], opts, "ub", var)
                np.testing.assert_array_equal(SC.active_entries(g["xtraj"], g["utraj"], opts, "ub", var), want, err_msg=f"{cid}: tick {t}: ub {var}")
        f = make(); fresh = _tick(f, ticks[2]); f.close()
        assert any(not np.array_equal(got[2]["xtraj"][b], fresh["xtraj"][b]) for b in range(B)), cid
        return worst
    if N == 2:
        return worst
    # the doomed Solver's first solve after its failure: bit for bit what a handle with nothing stored returns for it (where its stale warm start dooms it
    # again, the failed slot's zeroed state shows the same way), and not so for the Solvers that carried their multipliers
    t = DOOMED_TICK + 1
    f = make(); fresh = _tick(f, ticks[t]); f.close()
    _same_bits(got[t], fresh, "after the failure", DOOMED)
    carried = [b for b in range(B) if b != DOOMED and ticks[t]["exit_code"][b] == 1 and ticks[t - 1]["exit_code"][b] == 1]
    assert any(not np.array_equal(got[t]["xtraj"][b], fresh["xtraj"][b]) for b in carried), cid
    return worst


@pytest.mark.parametrize("cid", LOOP_CASES)
def test_closed_loop_carries_multipliers_like_the_oracle(cid, request, monkeypatch):
    c = _case(cid)
    _lab(c, request, monkeypatch)
    slot_of = {}

    def make():
        s, slot_of["slot"] = _handle(c)
        return s
    probe = make(); probe.close()
    _closed_loop(cid, make, relaxed=slot_of["slot"] == "lat2")


@pytest.mark.parametrize("cid", sorted(BOUNDED_LOOPS))
def test_closed_loop_carries_the_multipliers_of_active_bounds(cid, request, monkeypatch):
    """The loop with three model bounds binding at every tick."""
    c = _case(cid, BOUNDED_LOOPS[cid][0])
    _lab(c, request, monkeypatch)
    opts = bounded_options(cid)
    slot_of = {}

    def make():
        s, slot_of["slot"] = _handle(c, opts=opts)
        return s
    probe = make(); probe.close()
    _closed_loop(cid, make, relaxed=slot_of["slot"] == "lat2", opts=opts, scene=BOUNDED_LOOPS[cid][0])


@pytest.mark.parametrize("mode", [0, 3])
def test_closed_loop_on_the_generated_cfg2_library(mode):
    """The generated T-MPC stack (the hand-written kernels' parameter layout, test_gpu_parity.test_generated_tmpc_solver_equals_hand_written_kernels) on its
    default kernel and on its control-tick kernel; the reference is the hand-written cfg-2 oracle problem's loop."""
    import test_gpu_dispatch_matrix as T
    from test_gpu_generated_tick import NARROW, _gen_solver

    def make():
        s = _gen_solver("tmpc_cfg2", 20, B)
        assert s.set_latency_mode(mode) or mode == 0
        slots, th = T._slots(s.kernel_info())
        slot = T._running(slots, mode, B, th)
        assert (slot, slots[slot]) == (("lat3", NARROW.split("=")[1]) if mode else ("default", GENERATED_DEFAULT)), (slot, slots)
        return s
    ticks, _ = oracle_loop("m0 (8,8) N=20")
    probe = make()
    assert probe.npar == ticks[0]["params"].shape[2]
    probe.close()
    _closed_loop("m0 (8,8) N=20", make, relaxed=False)


# ---- the state protocol, device against device, bitwise -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["m0 (8,8) N=20 compact", "m0 (20,8) N=30 cp2", "m3 (8,8) N=20", "m2 (8,8) N=31"])
def test_slot_map_keys_the_state_by_slot(cid, request, monkeypatch):
    """test_gpu_iterations.test_slot_map_keys_the_state_by_slot_not_by_batch_position on the compact one-wave and two-wave kernels and the tick kernels."""
    c = _case(cid)
    _lab(c, request, monkeypatch)
    ticks, _ = oracle_loop(cid, fresh=False)
    r0 = ticks[0]
    kw = dict(new_solve=True)
    r, _ = _handle(c)
    t1 = _tick(r, r0, **kw)
    r.solve_iterations(10, keep_multipliers=True, new_solve=True); t2 = r.get()
    assert np.abs(t2["xtraj"] - t1["xtraj"]).max() > 1e-9                     # carried multipliers matter on this scene
    s, _ = _handle(c)
    perm = np.random.default_rng(3).permutation(B)
    s.set_batch(r0["xinit"][perm], r0["x0"][perm], r0["params"][perm]); s.set_slots(perm)     # batch entry b is Solver perm[b]
    s.solve_iterations(10, keep_multipliers=True, new_solve=True); a = s.get()
    _same_bits(a, t1, "permuted", slice(None), perm)
    sub = np.array([11, 2, 7, 14, 0])
    s.set_batch(r0["xinit"][sub], r0["x0"][sub], r0["params"][sub]); s.set_slots(sub)
    s.solve_iterations(10, keep_multipliers=True, new_solve=True); b = s.get()
    _same_bits(b, t2, "subset", slice(None), sub)                              # each got its OWN first-tick multipliers
    # a slot nothing was stored in starts fresh whatever the keep-flags say
    f, _ = _handle(c)
    f.set_batch(r0["xinit"][:4], r0["x0"][:4], r0["params"][:4]); f.set_slots([12, 13, 14, 15])
    f.solve_iterations(10, keep_iterate=True, keep_multipliers=True); d = f.get()
    _same_bits(d, t1, "unused slots", slice(None), slice(0, 4))
    for x in (r, s, f):
        x.close()


def test_persistent_compact_kernel_carries_the_state_of_the_fast_twin():
    """The product library, no lab switch: cp_min_B + 1 entries run the compact kernel's persistent ticket loop, 16 run its fast twin, and the two are bitwise
    equal by design -- over two ticks with kept multipliers every copy of the tiled scene returns the bits of the 16-entry handle."""
    import test_gpu_dispatch_matrix as T
    cid = "m0 (8,8) N=20"
    c = _case(cid)
    r0 = oracle_loop(cid, fresh=False)[0][0]
    small, slot = _handle(c)
    slots, th = T._slots(small.kernel_info())
    assert slot == "small" and slots["default"] == "compact<8,8,3,64,0>", slots
    n = th["cp_min_B"] + 1
    assert 16 < n <= 4096, th
    big, slot = _handle(dict(c, expect="compact<8,8,3,64,0>"), B_max=n, launch=n)
    assert slot == "default"
    idx = np.arange(n) % B
    tiled = {k: r0[k][idx] for k in ("xinit", "x0", "params")}
    a1 = _tick(small, r0, new_solve=True); b1 = _tick(big, tiled, new_solve=True)
    _same_bits(b1, a1, "tick 1", slice(None), idx)
    small.solve_iterations(10, keep_multipliers=True, new_solve=True); a2 = small.get()
    big.solve_iterations(10, keep_multipliers=True, new_solve=True); b2 = big.get()
    assert np.abs(a2["xtraj"] - a1["xtraj"]).max() > 1e-9                     # carried multipliers matter
    _same_bits(b2, a2, "tick 2", slice(None), idx)
    small.close(); big.close()


def test_mode_switch_between_ticks_keeps_the_multipliers():
    """One (8,8) N = 20 handle: tick 0 on the throughput kernel, tick 1 on the four-wave tick kernel with the multipliers the other kernel stored."""
    cid = "m0 (8,8) N=20"
    c = _case(cid)
    ticks, _ = oracle_loop(cid)
    s, _ = _handle(c)
    _tick(s, ticks[0])
    assert s.set_latency_mode(3)
    g = _tick(s, ticks[1])
    err = _against_oracle(g, ticks[1], False, "mode 0 -> mode 3")
    print(f"[carried] mode 0 then mode 3: rel diff at the second tick {err:.2e}")
    assert err < HARD and err < TIGHT, err
    s.close()
    f, slot = _handle(_case("m3 (8,8) N=20"))
    assert slot == "lat3"
    fresh = _tick(f, ticks[1]); f.close()
    ok = ticks[1]["exit_code"] == 1
    carried = ok & (ticks[0]["exit_code"] == 1)
    print(f"[carried] mode 0 then mode 3: the kept multipliers move the second tick by {np.abs(fresh['xtraj'][carried] - g['xtraj'][carried]).max():.2e}")
    assert any(not np.array_equal(fresh["xtraj"][b], g["xtraj"][b]) for b in np.flatnonzero(carried))


@pytest.mark.parametrize("cid", ["m0 (8,8) N=20", "m0 (20,8) N=30"])
def test_clear_slot_forgets_one_slot_only(cid):
    from mpc_planner_amd import solver
    c = _case(cid)
    ticks, _ = oracle_loop(cid, fresh=False)
    k = 6
    assert all(r["exit_code"][k] == 1 for r in ticks[:3])
    s, _ = _handle(c); w, _ = _handle(c); f, _ = _handle(c)
    for r in ticks[:2]:
        _same_bits(_tick(s, r), _tick(w, r), "twin handles")
    s.clear_slot(k)
    a = _tick(s, ticks[2]); without = _tick(w, ticks[2]); fresh = _tick(f, ticks[2])
    _same_bits(a, fresh, "the cleared slot", k)
    others = np.arange(B) != k
    _same_bits(a, without, "the other slots", others)
    assert not np.array_equal(a["xtraj"][k], without["xtraj"][k])             # the call did something
    for bad in (-1, B):
        with pytest.raises(solver.TmpcError):
            s.clear_slot(bad)
    _same_bits(_tick(s, ticks[3]), _tick(w, ticks[3]), "after the refused calls", others)
    for x in (s, w, f):
        x.close()


def test_copy_state_to_a_larger_handle_keeps_every_slot():
    cid = "m0 (20,8) N=30"
    c = _case(cid)
    ticks, _ = oracle_loop(cid, fresh=False)
    r, _ = _handle(c)
    _tick(r, ticks[0]); _tick(r, ticks[1])
    g, _ = _handle(c, B_max=2 * B)
    g.copy_state_from(r)
    e = _tick(g, ticks[2]); t3 = _tick(r, ticks[2])
    _same_bits(e, t3, "copied state")
    f, _ = _handle(c)
    fresh = _tick(f, ticks[2])
    assert not np.array_equal(fresh["xtraj"], t3["xtraj"])                     # (the state mattered)
    for x in (r, g, f):
        x.close()
