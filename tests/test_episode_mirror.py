"""The numpy mirror of the episode step (mpc_planner_amd/modules.py episode_step) without a GPU: the plant against the closed-form
circular arc, the properties the header states on hand-computed cases, and the script of the GPU equality test (tests/episode_cases.py), which
has to make every event occur."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import episode_cases as ec  # noqa: E402


def _world(n_slots=2, max_episodes=2, nx=5, P=2, start=(0.0, 0.0, 0.0, 1.0)):
    """One scene's arrays: the robot at `start`, n_slots obstacles far away at rest."""
    plant0 = np.array(list(start) + [np.cos(start[2]), np.sin(start[2])])
    w = dict(plant0=plant0, plant=plant0.copy(), raw_pos0=np.full((n_slots, 2), 50.0), raw_vel0=np.zeros((n_slots, 2)), raw_radius=np.full(n_slots, 0.5),
             episode=np.zeros(4, np.int32), episode_f=np.zeros(2), log=np.full((max_episodes, 4), ec.SENTINEL), state_nx=np.full(nx, ec.SENTINEL),
             state_batch=np.full((P, nx), ec.SENTINEL), planner_ids=np.full(P, 5, np.int32), selection=np.array([4, 1, 2], np.int32),
             segment=np.array([7], np.int32))
    w["raw_pos"], w["raw_vel"] = w["raw_pos0"].copy(), w["raw_vel0"].copy()
    return w


def _step(w, cmd, count=None, box=None, goal=None, **kw):
    from mpc_planner_amd import modules as md
    opt = dict(substeps=1, timeout_ticks=0, control_dt=0.05, max_acceleration=0.0, max_angular_velocity=2.0, robot_radius=0.5)
    opt.update(kw)
    return md.episode_step(cmd, w["plant"], w["plant0"], len(w["raw_radius"]) if count is None else count, w["raw_pos"], w["raw_vel"], w["raw_radius"],
                           w["raw_pos0"], w["raw_vel0"], w["episode"], w["episode_f"], w["log"], box=box, goal=goal, state_nx=w["state_nx"],
                           state_batch=w["state_batch"], planner_ids=w["planner_ids"], selection=w["selection"], segment=w["segment"], **opt)


def test_constant_command_follows_the_circular_arc():
    """Constant (v, w), v at its commanded value from the start, 400 ticks of 0.05 s, substeps 1 .. 4; 200 seeded draws, v in [0.1, 3], |w| <= 2,
    any start heading.  The reference is the closed form: after time t the chord v t sinc(w t / 2) along the heading psi0 + w t / 2.
    Measured here, the maximum over every draw, tick and substep count: position error 6.2e-15 (1 + path length), |(c, s) - (cos psi, sin psi)|
    1.4e-12 (the plant's own psi, which carries 400 .. 1600 rounded additions of w h).  Asserted: 1e-12 and 1e-10."""
    from mpc_planner_amd import modules as md
    rng = np.random.default_rng(2024)
    dt, ticks = 0.05, 400
    worst_pos, worst_head = 0.0, 0.0
    t = dt * np.arange(1, ticks + 1)
    for draw in range(200):
        v, w, psi0 = rng.uniform(0.1, 3.0), rng.uniform(-2.0, 2.0), rng.uniform(-np.pi, np.pi)
        x0, y0 = rng.uniform(-5.0, 5.0, 2)
        half = w * t / 2.0
        chord = v * t * np.sinc(half / np.pi)
        want = np.stack([x0 + chord * np.cos(psi0 + half), y0 + chord * np.sin(psi0 + half)], 1)
        for substeps in (1, 2, 3, 4):
            world = _world(n_slots=0, start=(x0, y0, psi0, v))
            got = np.zeros((ticks, 6))
            for k in range(ticks):
                _step(world, (v, w), substeps=substeps, control_dt=dt)
                got[k] = world["plant"]
            err = np.sqrt(((got[:, 0:2] - want) ** 2).sum(1)) / (1.0 + v * t)
            head = np.sqrt((got[:, 4] - np.cos(got[:, 2])) ** 2 + (got[:, 5] - np.sin(got[:, 2])) ** 2)
            worst_pos, worst_head = max(worst_pos, err.max()), max(worst_head, head.max())
            assert np.array_equal(got[:, 3], np.full(ticks, v))
    print(f"[arc] position error / (1 + path length) {worst_pos:.3e}, heading vector error {worst_head:.3e}")
    assert worst_pos < 1e-12 and worst_head < 1e-10


def test_acceleration_limit_per_substep_and_clipped_w():
    """max_acceleration 2, control_dt 0.05, 4 substeps: v rises by exactly 2 x 0.0125 per substep towards the command and stops at it; the
    distance covered is that of the mean velocities.  w = 5 is clipped to 2 (psi += 2 x 0.05), w = -5 to -2; without a limit v jumps."""
    w = _world(n_slots=0, start=(0.0, 0.0, 0.0, 1.0))
    _step(w, (2.0, 0.0), substeps=4, max_acceleration=2.0)
    h = 0.05 / 4.0
    v, x = 1.0, 0.0
    for _ in range(4):
        v1 = v + 2.0 * h
        x = x + ((v + v1) / 2.0 * h) * 1.0
        v = v1
    assert w["plant"][3] == v and abs(v - 1.1) < 1e-15 and w["plant"][0] == x and w["plant"][1] == 0.0
    w = _world(n_slots=0, start=(0.0, 0.0, 0.0, 1.0))
    _step(w, (1.03, 0.0), substeps=4, max_acceleration=2.0)                      # reached within the second substep: no overshoot
    assert w["plant"][3] == 1.03
    w = _world(n_slots=0, start=(0.0, 0.0, 0.0, 1.0))
    _step(w, (0.0, 0.0), substeps=2, max_acceleration=2.0)                       # and downwards
    assert w["plant"][3] == 1.0 - 2.0 * 0.025 - 2.0 * 0.025
    w = _world(n_slots=0, start=(0.0, 0.0, 0.0, 1.0))
    _step(w, (2.5, 0.0))
    assert w["plant"][3] == 2.5                                                  # no limit: at once
    for cmd_w, want in ((5.0, 2.0), (-5.0, -2.0), (1.5, 1.5)):
        w = _world(n_slots=0, start=(0.0, 0.0, 0.25, 1.0))
        _step(w, (1.0, cmd_w))
        assert w["plant"][2] == 0.25 + want * 0.05
    w = _world(n_slots=0)
    _step(w, (np.nan, np.nan))                                                   # a NaN passes through both clips
    assert np.isnan(w["plant"]).all()


def test_reflection_flips_the_component_and_keeps_the_position():
    w = _world(n_slots=3)
    w["raw_pos"][:] = ((0.98, 0.0), (0.0, -0.99), (0.5, 0.5)); w["raw_vel"][:] = ((1.0, 0.25), (0.5, -1.0), (1.0, 1.0))
    _step(w, (1.0, 0.0), box=(-1.0, 1.0, -1.0, 1.0), robot_radius=0.0)
    assert w["raw_pos"].tolist() == [[0.98 + 1.0 * 0.05, 0.0 + 0.25 * 0.05], [0.0 + 0.5 * 0.05, -0.99 + -1.0 * 0.05], [0.55, 0.55]]
    assert w["raw_pos"][0, 0] > 1.0 and w["raw_pos"][1, 1] < -1.0                # outside, and not mirrored back
    assert w["raw_vel"].tolist() == [[-1.0, 0.25], [0.5, 1.0], [1.0, 1.0]]
    _step(w, (1.0, 0.0), box=(-1.0, 1.0, -1.0, 1.0), robot_radius=0.0)           # the next tick brings them back inside: no second flip
    assert w["raw_vel"].tolist() == [[-1.0, 0.25], [0.5, 1.0], [1.0, 1.0]] and w["raw_pos"][0, 0] == 0.98 + 0.05 - 0.05
    w = _world(n_slots=1)
    w["raw_pos"][:] = ((0.98, 0.0),); w["raw_vel"][:] = ((1.0, 0.0),)
    _step(w, (1.0, 0.0))                                                         # no box: no reflection
    assert w["raw_vel"].tolist() == [[1.0, 0.0]]


def test_intrusion_on_hand_computed_cases():
    """The robot (radius 0.5) stands still at the origin; obstacles at rest.  3-4-5 triangles make the distances exact."""
    w = _world(n_slots=3, start=(0.0, 0.0, 0.0, 0.0))
    w["raw_pos"][:] = ((3.0, 4.0), (0.0, 1.0), (-6.0, 8.0)); w["raw_radius"][:] = (0.5, 0.5, 0.25)
    _step(w, (0.0, 0.0))                                                         # obstacle 1 touches exactly: (0.5 + 0.5) - 1 = 0, not a collision
    assert w["episode_f"].tolist() == [0.0, 0.0] and w["episode"].tolist() == [1, 0, 0, 0]
    w["raw_pos"][1] = (0.0, 0.75)
    _step(w, (0.0, 0.0))
    assert w["episode_f"].tolist() == [0.25, 0.25] and w["episode"].tolist() == [2, 1, 0, 0]
    w["raw_pos"][0] = (-0.5, 0.0); w["raw_pos"][1] = (0.0, 0.875)                # 1 - 0.5 = 0.5 beats 1 - 0.875
    _step(w, (0.0, 0.0))
    assert w["episode_f"].tolist() == [0.5, 0.5] and w["episode"].tolist() == [3, 2, 0, 0]
    w["raw_pos"][0] = (3.0, 4.0); w["raw_pos"][1] = (0.0, 5.0)
    _step(w, (0.0, 0.0))                                                         # apart again: the maximum of the episode stays
    assert w["episode_f"].tolist() == [0.5, 0.0] and w["episode"].tolist() == [4, 2, 0, 0]
    w["raw_pos"][2] = (np.nan, 0.0)
    _step(w, (0.0, 0.0))                                                         # a NaN candidate never enters
    assert w["episode_f"].tolist() == [0.5, 0.0]
    w["raw_pos"][1] = (0.0, 0.75)
    _step(w, (0.0, 0.0), count=1)                                                # slots at or beyond the count are not looked at
    assert w["episode_f"].tolist() == [0.5, 0.0]


def test_log_rows_reset_and_the_cap():
    """timeout_ticks 3, max_episodes 2; an obstacle overlaps during the first episode only.  Rows: (3 x 0.05, 0, collision ticks, max
    intrusion); the third and fourth episode are counted and not written; a reset restores plant and obstacles bit for bit, zeroes the
    counters and the planner's cross-tick state, and zeroes the state entries behind v."""
    w = _world(n_slots=3, max_episodes=2, start=(0.1, 0.2, 0.3, 1.0))
    w["raw_pos0"][:] = ((0.1, 0.95), (9.0, 9.0), (33.0, 44.0)); w["raw_vel0"][:] = ((0.0, 0.0), (1.0, -1.0), (0.5, 0.5))
    w["raw_pos"][:] = w["raw_pos0"]; w["raw_vel"][:] = w["raw_vel0"]
    guard = w["log"].copy()
    resets = []
    for tick in range(12):
        if tick == 3:
            w["raw_pos"][0] = (50.0, 50.0)                                       # moved away by hand: the second episode is collision-free ...
            w["raw_pos0"][0] = (50.0, 50.0)                                      # ... and so are the later ones
        reset, state4 = _step(w, (1.0, 0.5), count=2, timeout_ticks=3)
        resets.append(bool(reset))
        assert np.array_equal(state4, w["plant"][0:4]) and np.array_equal(w["state_nx"][0:4], state4) and np.array_equal(w["state_batch"][:, 0:4], np.tile(state4, (2, 1)))
        assert w["raw_pos"][2].tolist() == [33.0, 44.0] and w["raw_vel"][2].tolist() == [0.5, 0.5]      # behind the count: untouched
        if tick < 2:
            assert (w["state_nx"][4:] == ec.SENTINEL).all() and w["planner_ids"].tolist() == [5, 5] and w["segment"].tolist() == [7]
        if reset:
            assert np.array_equal(w["plant"], w["plant0"]) and np.array_equal(w["raw_pos"][:2], w["raw_pos0"][:2]) and np.array_equal(w["raw_vel"][:2], w["raw_vel0"][:2])
            assert w["episode"][:2].tolist() == [0, 0] and w["episode_f"][0] == 0.0 and w["episode"][2] == (tick + 1) // 3
            assert (w["state_nx"][4:] == 0.0).all() and (w["state_batch"][:, 4:] == 0.0).all()
            assert w["planner_ids"].tolist() == [-1, -1] and w["selection"].tolist() == [-1, 0, -1] and w["segment"].tolist() == [-1]
            w["planner_ids"][:] = 5; w["selection"][:] = (4, 1, 2); w["segment"][:] = 7
        if tick == 5:
            guard = w["log"].copy()
    assert resets == [False, False, True] * 4
    assert w["log"][0, 0] == 3.0 * 0.05 and w["log"][0, 1] == 0.0 and w["log"][0, 2] == 3.0 and 0.0 < w["log"][0, 3] < 1.0
    assert w["log"][1].tolist() == [3.0 * 0.05, 0.0, 0.0, 0.0]
    assert np.array_equal(w["log"], guard) and w["episode"].tolist() == [0, 0, 4, 0]                   # beyond the cap: counted, not written


def test_completion_by_goal_x_and_by_the_goal_disc():
    w = _world(n_slots=0, start=(0.0, 0.0, 0.0, 1.0))
    r1, _ = _step(w, (1.0, 0.0), goal_x=0.05)                                    # x = 0.05 exactly: `>` is strict
    r2, _ = _step(w, (1.0, 0.0), goal_x=0.05)
    assert (r1, r2) == (False, True) and w["log"][0].tolist() == [2.0 * 0.05, 1.0, 0.0, 0.0]
    w = _world(n_slots=0, start=(0.0, 0.0, 0.0, 1.0))
    r1, _ = _step(w, (1.0, 0.0), goal=(1.05, 0.0, 1.0))                          # |p - g| = 1.0 exactly: `<` is strict
    r2, _ = _step(w, (1.0, 0.0), goal=(1.05, 0.0, 1.0))
    assert (r1, r2) == (False, True) and w["log"][0, 1] == 1.0
    w = _world(n_slots=0, start=(0.0, 0.0, 0.0, 1.0))
    r, _ = _step(w, (1.0, 0.0), goal=(0.0, 0.0, 1.0), goal_x=-1.0, timeout_ticks=1)      # completed wins over the timeout
    assert r and w["log"][0, 1] == 1.0


@pytest.mark.parametrize("config", ec.CONFIGS)
def test_the_gpu_script_makes_every_event_occur(config):
    """tests/episode_cases.py on the mirror alone: a goal-disc completion, a goal_x completion, a timeout, the NaN scene timing out and coming
    back bitwise at its start, a collision tick, a log overflow, a clipped w and, with a box, a reflection on each of the four sides."""
    substeps, boxed, acc = config
    case = ec.make_case(7, boxed)
    history, seen = ec.run_mirror(case, ec.options(substeps, acc))
    assert len(history) == ec.TICKS
    assert all(seen[k] for k in ec.expected_events(boxed)), seen
    last = history[-1]
    assert (last["episode"][:, 2] > ec.MAX_EPISODES).all() and not (last["log"] == ec.SENTINEL).any()
    for q in range(ec.Q):                                                        # slots at or beyond the count never move
        n = ec.COUNTS[q]
        assert all(np.array_equal(h["raw_pos"][q, n:], case["raw_pos0"][q, n:]) and np.array_equal(h["raw_vel"][q, n:], case["raw_vel0"][q, n:]) for h in history)
    assert np.abs(np.nan_to_num(case["commands"][:, :, 1])).max() > ec.MAX_W
    assert np.isnan(history[ec.NAN_FROM + 1]["plant"][ec.NAN_SCENE]).all()
