"""CPU: the numpy mirrors of the guidance hand-off (mpc_planner_amd/modules.py sample_guidance / guidance_plan / guidance_decide)
pinned on hand values.  The device kernels and the C++ header are compared with these mirrors bit for bit in tests/test_gpu_guidance_handoff.py
and tests/test_cpp_guidance_handoff.py."""
import numpy as np

from mpc_planner_amd import modules as md

N, DT = 20, 0.2


def test_two_nodes_are_linear_interpolation():
    """(t, x, y) = (0, 1, -2) -> (4, 3, 6): x = 1 + 0.5 t, y = -2 + 2 t exactly (every value is a dyadic rational), velocity (0.5, 2)."""
    pos, vel, status = md.sample_guidance([[0.0, 1.0, -2.0], [4.0, 3.0, 6.0]], 8, 0.5)
    assert status == 0
    t = np.arange(9) * 0.5
    assert np.array_equal(pos[:, 0], 1.0 + 0.5 * t) and np.array_equal(pos[:, 1], -2.0 + 2.0 * t)
    assert np.array_equal(vel, np.tile([0.5, 2.0], (9, 1)))


def test_three_nodes_equal_the_closed_form_natural_spline():
    """Knots 0, 1, 2 with values (0, 1, 0): the natural spline has M_1 = 6 (y_0 - 2 y_1 + y_2) / 4 = -3, so on [0, 1]
    y = 1.5 t - 0.5 t^3 and on [1, 2], with u = t - 1, y = 1 - 1.5 u^2 + 0.5 u^3; y' = 1.5 - 1.5 t^2 and -3 u + 1.5 u^2.  x = t."""
    pos, vel, status = md.sample_guidance([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 0.0]], 8, 0.25)
    assert status == 0
    t = np.arange(9) * 0.25
    u = t - 1.0
    y = np.where(t < 1.0, 1.5 * t - 0.5 * t ** 3, 1.0 - 1.5 * u ** 2 + 0.5 * u ** 3)
    dy = np.where(t < 1.0, 1.5 - 1.5 * t ** 2, -3.0 * u + 1.5 * u ** 2)
    np.testing.assert_allclose(pos[:, 1], y, rtol=0, atol=2e-15)
    np.testing.assert_allclose(vel[:, 1], dy, rtol=0, atol=2e-15)
    np.testing.assert_allclose(pos[:, 0], t, rtol=0, atol=2e-15)
    np.testing.assert_allclose(vel[:, 0], 1.0, rtol=0, atol=2e-15)
    assert pos[4, 1] == 1.0 and pos[4, 0] == 1.0                      # ON the knot: the right segment's d


def test_the_end_cubics_continue_outside_the_node_span():
    """t_0 = 0.5 and a span of 1 s, N dt = 2 s: k = 0, 1, 2 lie before t_0 (no knot at or below them: segment 0, tau < 0), k >= 8 past the
    last node (segment n - 2).  Two nodes: the line, so the continuation is the line."""
    pos, vel, status = md.sample_guidance([[0.5, 1.0, 0.0], [1.5, 3.0, 0.0]], 10, 0.25)
    assert status == 0
    t = np.arange(11) * 0.25
    assert np.array_equal(pos[:, 0], 1.0 + 2.0 * (t - 0.5)) and pos[0, 0] == 0.0 and pos[10, 0] == 5.0
    assert (vel[:, 0] == 2.0).all()
    # three nodes: past the end the LAST cubic continues (it is not the tangent line)
    nodes = [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 0.0]]
    pos, vel, _ = md.sample_guidance(nodes, 3, 1.0)
    u = 2.0
    assert abs(pos[3, 1] - (1.0 - 1.5 * u ** 2 + 0.5 * u ** 3)) < 4e-15 and abs(vel[3, 1] - (-3.0 * u + 1.5 * u ** 2)) < 4e-15


def test_invalid_node_lists():
    ok = [[0.0, 0.0, 0.0], [1.0, 1.0, 0.0], [2.0, 2.0, 0.0]]
    for nodes in (np.zeros((0, 3)), [[0.0, 1.0, 1.0]], [[0.0, 0.0, 0.0], [1.0, 1.0, 0.0], [1.0, 2.0, 0.0]], [[0.0, 0.0, 0.0], [float("nan"), 1.0, 0.0], [2.0, 2.0, 0.0]],
                  [[0.0, 0.0, 0.0], [2.0, 1.0, 0.0], [1.0, 2.0, 0.0]], [[0.0, 0.0, 0.0], [float("inf"), 1.0, 0.0]]):
        pos, vel, status = md.sample_guidance(nodes, N, DT)
        assert status == 1 and pos.shape == (N + 1, 2) and not pos.any() and not vel.any()
    assert md.sample_guidance(ok, N, DT)[2] == 0 and md.sample_guidance(ok, N, DT, n_nodes_max=2)[2] == 1       # more nodes than the buffer holds


def _state(Q, P):
    return np.full((Q, P), -1, np.int32), np.tile(np.array([-1, 0, -1], np.int32), (Q, 1))


def test_plan_existing_guidance_equals_the_mapping_mirror():
    rng = np.random.default_rng(5)
    for case in range(300):
        n_paths = int(rng.integers(1, 7)); tmpcpp = bool(rng.integers(0, 2)); P = n_paths + tmpcpp
        ids = rng.integers(-1, 5, (1, P)).astype(np.int32)
        count = int(rng.integers(0, n_paths + 1))
        cls = rng.integers(0, 5, (1, n_paths)).astype(np.int32)
        plan = md.guidance_plan([count], cls, ids, [[-1, 0, -1]], n_paths, use_tmpcpp=tmpcpp)
        _, _, existing = md.map_guidance_trajectories_to_planners(ids[0].tolist(), cls[0, :count].tolist())
        assert plan["existing_guidance"].tolist() == [int(e) for e in existing], case


def test_plan_keeps_the_missing_break():
    """Planners hold (7, -1, -1); trajectories of classes (3, 4, 7).  Class 3 finds nobody; class 4 neither; class 7 takes planner 0.  The
    second loop has no `break`: trajectory 0 claims planners 1 AND 2, trajectory 1 gets none -- existing_guidance is (1, 0, 0).  With
    warmstart_with_mpc_solution planner 0 restarts from its own solution, planners 1 and 2 are initialised with the guidance."""
    ids = np.array([[7, -1, -1, 6]], np.int32)
    mapping, taken, existing = md.map_guidance_trajectories_to_planners(ids[0].tolist(), [3, 4, 7])
    assert mapping == {2: 0, 0: 3} and taken == [True] * 4 and existing == [True, False, False, False]
    plan = md.guidance_plan([3], [[3, 4, 7]], ids, [[7, 0, 0]], 3, warmstart_with_mpc_solution=True, shift_previous_solution_forward=False)
    assert plan["existing_guidance"].tolist() == [1, 0, 0, 0]
    assert plan["mode"].tolist() == [2, 2, 2, 2] and plan["src"].tolist() == [0, 0, 0, 0]            # own solution / the main start: both entry 0 here
    assert plan["init_enabled"].tolist() == [0, 1, 1, 0]
    # planner p follows trajectory p, not the map: planner 0 solves class 3 although it is "reserved" for class 7
    assert plan["guidance_id"].tolist() == [3, 4, 7, 6]


def test_plan_branches():
    """Two scenes, n_paths = 3 + the non-guided planner.  Scene 0: two trajectories, no previous solution (braking start).  Scene 1: three,
    last best = planner 2, planner 1 held class 5 last tick."""
    ids = np.array([[-1, -1, -1, -1], [4, 5, 9, 6]], np.int32)
    sel = np.array([[-1, 0, -1], [9, 0, 2]], np.int32)
    cls = np.array([[1, 2, 0], [8, 5, 9]], np.int32)
    plan = md.guidance_plan([2, 3], cls, ids, sel, 3, warmstart_with_mpc_solution=True, selection_weight_consistency=0.8)
    assert plan["disabled"].tolist() == [0, 0, 1, 0, 0, 0, 0, 0]
    assert plan["guidance_id"].tolist() == [1, 2, -1, 6, 8, 5, 9, 6]                                   # disabled: -1; non-guided: 2 n_paths
    assert plan["rows_dummy"].tolist() == [0, 0, 1, 1, 0, 0, 0, 1]
    assert plan["mode"].tolist() == [3, 3, 3, 3, 1, 1, 1, 1]
    assert plan["src"].tolist() == [0, 1, 2, 3, 6, 5, 6, 6]                                            # planners 5 and 6: their own solutions
    assert plan["init_enabled"].tolist() == [1, 1, 0, 0, 1, 0, 0, 0]
    assert plan["weight"].tolist() == [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.8, 1.0]                         # class 9 was selected
    # the selected planner was the non-guided one: no class is preferred, whatever its number
    sel2 = sel.copy(); sel2[1] = (6, 1, 3)
    plan2 = md.guidance_plan([2, 3], cls, ids, sel2, 3, selection_weight_consistency=0.8)
    assert (plan2["weight"] == 1.0).all() and plan2["src"].tolist()[4:] == [7, 7, 7, 7] and plan2["init_enabled"].tolist() == [1, 1, 0, 0, 1, 1, 1, 0]
    # an explicit previously_selected overrides the state: per trajectory, guided and enabled planners only
    plan3 = md.guidance_plan([2, 3], cls, ids, sel, 3, selection_weight_consistency=0.8, previously_selected=[[1, 0, 1], [0, 1, 0]])
    assert plan3["weight"].tolist() == [0.8, 1.0, 1.0, 1.0, 1.0, 0.8, 1.0, 1.0]
    # without the non-guided planner P = n_paths and nobody is "original"; counts are clipped to [0, n_paths]
    plan4 = md.guidance_plan([-2, 9], cls, ids[:, :3], sel, 3, use_tmpcpp=False)
    assert plan4["disabled"].tolist() == [1, 1, 1, 0, 0, 0] and plan4["guidance_id"].tolist() == [-1, -1, -1, 8, 5, 9]
    assert plan4["rows_dummy"].tolist() == [1, 1, 1, 0, 0, 0]


def _solution(B, seed=3):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(B, N + 1, 5)), rng.normal(size=(B, N, 2))


def test_decide():
    P, n_paths = 4, 3
    xtraj, utraj = _solution(4 * P)
    ids, sel = _state(4, P); sel[3] = (5, 0, 1)
    #                 scene 0: a tie        scene 1: the best is disabled   scene 2: all failed     scene 3: planner 0 disabled, none
    pobj = np.array([3.0, 2.0, 2.0, 9.0,    1.0, 5.0, 4.0, 6.0,             1.0, 1.0, 1.0, 1.0,     1.0, 1.0, 1.0, 1.0])
    code = np.array([1, 1, 1, 1,            1, 1, 1, 0,                     0, -1, 2, 0,            1, 0, 1, 3], np.int32)
    dis = np.array([0, 0, 0, 0,             1, 0, 0, 0,                     0, 0, 0, 0,             1, 0, 1, 0], np.uint8)
    gid = np.array([4, 5, 6, 6,             -1, 2, 3, 6,                    1, 2, 3, 6,             -1, 7, -1, 6], np.int32)
    w = np.array([1.0, 1.0, 1.0, 1.0,       1.0, 1.0, 1.0, 1.0,             1.0, 1.0, 1.0, 1.0,     1.0, 1.0, 1.0, 1.0])
    state = np.zeros((4, 5)); state[:, 3] = (1.0, 1.0, 0.1, 2.0)
    out = md.guidance_decide(pobj, code, dis, gid, w, state, xtraj, utraj, ids, sel, n_paths, deceleration=3.0, control_dt=0.05)
    assert out["best"].tolist() == [1, 2, -1, -1]                      # the lowest index of the tie; the disabled 1.0 is skipped
    assert out["exit"].tolist() == [1, 1, 0, -1]                       # no winner: planner 0's code, or -1 if it is disabled
    assert out["cmd"][0].tolist() == [xtraj[1, 1, 3], utraj[1, 0, 1]] and out["cmd"][1].tolist() == [xtraj[4 + 2, 1, 3], utraj[4 + 2, 0, 1]]
    assert out["cmd"][2].tolist() == [0.0, 0.0] and out["cmd"][3].tolist() == [2.0 - 3.0 * 0.05, 0.0]      # braking: clipped at 0 / v - a dt
    assert np.array_equal(out["planner_ids"], gid.reshape(4, P))       # whatever the verdict
    assert out["selection"].tolist() == [[5, 0, 1], [3, 0, 2], [-1, 0, -1], [5, 0, -1]]                    # untouched without a winner
    assert (ids == -1).all() and sel[0].tolist() == [-1, 0, -1]        # the inputs are inputs
    # the weight decides, and the non-guided planner as the winner is recorded as such
    w2 = w.copy(); w2[0] = 0.5; pobj2 = pobj.copy(); pobj2[7] = 0.1; code2 = code.copy(); code2[7] = 1
    out2 = md.guidance_decide(pobj2, code2, dis, gid, w2, state, xtraj, utraj, ids, sel, n_paths, enable_output=False)
    assert out2["best"].tolist() == [0, 3, -1, -1] and out2["selection"][1].tolist() == [6, 1, 3] and out2["selection"][0].tolist() == [4, 0, 0]
    assert out2["cmd"][0].tolist() == [1.0 - 3.0 * 0.05, 0.0]          # a winner, but no output: the braking command
    # an objective at or above 1e10 never wins
    out3 = md.guidance_decide(np.full(16, 1e10), np.ones(16, np.int32), dis, gid, w, state, xtraj, utraj, ids, sel, n_paths)
    assert out3["best"].tolist() == [-1] * 4 and out3["exit"].tolist() == [1, -1, 1, -1]
