"""The scripted worlds of the episode-step tests (tests/test_episode_mirror.py, test_cpp_episode.py, test_gpu_episode.py): six scenes whose
starts, obstacles and commands make every event of tmpc_episode_step occur, the mirror's run over them, and the events it saw.  No test here."""
import numpy as np

SENTINEL = -3.0
Q, N_SLOTS, P, MAX_EPISODES, TICKS = 6, 70, 3, 2, 40
COUNTS = (0, 1, 3, 64, 70, 70)
CONTROL_DT, MAX_W, ROBOT_RADIUS, GOAL_X, TIMEOUT = 0.05, 2.0, 0.325, 0.5, 9
BOX = (-8.0, -2.0, -3.0, 3.0)
NAN_SCENE, NAN_FROM = 2, 3
# (substeps, box given, acceleration limit)
CONFIGS = [(1, True, 3.0), (4, False, 0.0), (4, True, 0.0), (1, False, 3.0)]
IN_OUT = ("plant", "raw_pos", "raw_vel", "episode", "episode_f")
OUTPUTS = ("log", "was_reset", "state4", "state_nx", "state_batch", "planner_ids", "selection", "segment")


def options(substeps, max_acceleration, timeout_ticks=TIMEOUT, max_episodes=MAX_EPISODES, goal_x=GOAL_X):
    return dict(substeps=substeps, timeout_ticks=timeout_ticks, max_episodes=max_episodes, control_dt=CONTROL_DT, max_acceleration=max_acceleration,
                max_angular_velocity=MAX_W, robot_radius=ROBOT_RADIUS, goal_x=goal_x)


def make_case(seed, boxed, nx=5, ticks=TICKS):
    """The inputs: plant0 [Q][6], count, raw_pos0 / raw_vel0 / raw_radius over all N_SLOTS slots (those behind the count hold values too: they
    must stay), box or None, goal [Q][3], commands [ticks][Q][2].
      scene 0 (no obstacle)   starts 0.3 m before goal_x, heading along x: completes by goal_x
      scene 1 (1 obstacle)    its goal disc (radius 0.15) lies 0.3 m ahead: completes by the disc
      scene 2 (3 obstacles)   NaN commands from tick 3 on: times out, completed = 0
      scene 3 (64 obstacles)  obstacle 0 sits on the robot's start: collision ticks
      scene 4 (70 obstacles)  obstacles 0 .. 3 sit 0.04 m inside the four walls and move outwards: a reflection on every side
      scene 5 (70 obstacles)  random"""
    rng = np.random.default_rng(seed)
    xlo, xhi, ylo, yhi = BOX
    psi = rng.uniform(-np.pi, np.pi, Q)
    start = np.stack([rng.uniform(-6.0, -4.0, Q), rng.uniform(-1.0, 1.0, Q), psi, rng.uniform(0.8, 1.5, Q)], 1)
    start[0, 0:3] = (GOAL_X - 0.3, 0.1, 0.0)
    plant0 = np.concatenate([start, np.cos(start[:, 2:3]), np.sin(start[:, 2:3])], 1)
    raw_pos0 = np.stack([rng.uniform(xlo + 0.5, xhi - 0.5, (Q, N_SLOTS)), rng.uniform(ylo + 0.5, yhi - 0.5, (Q, N_SLOTS))], 2)
    raw_vel0 = rng.uniform(-2.0, 2.0, (Q, N_SLOTS, 2))
    raw_radius = rng.uniform(0.1, 0.4, (Q, N_SLOTS))
    raw_pos0[3, 0] = plant0[3, 0:2]; raw_vel0[3, 0] = (0.1, -0.1)
    raw_pos0[4, 0:4] = ((xlo + 0.04, 0.0), (xhi - 0.04, 1.0), (-5.0, ylo + 0.04), (-4.0, yhi - 0.04))
    raw_vel0[4, 0:4] = ((-1.5, 0.2), (1.5, 0.2), (0.2, -1.5), (0.2, 1.5))
    goal = np.tile(np.array([1e3, 1e3, 1.0]), (Q, 1))
    goal[1] = (plant0[1, 0] + 0.3 * plant0[1, 4], plant0[1, 1] + 0.3 * plant0[1, 5], 0.15)
    commands = np.stack([rng.uniform(0.8, 2.0, (ticks, Q)), rng.uniform(-3.0, 3.0, (ticks, Q))], 2)
    commands[:, 0, 1] = rng.uniform(-0.3, 0.3, ticks); commands[:, 1, 1] = rng.uniform(-0.3, 0.3, ticks)
    commands[NAN_FROM:, NAN_SCENE] = np.nan
    return dict(plant0=plant0, count=np.array(COUNTS, np.int32), raw_pos0=raw_pos0, raw_vel0=raw_vel0, raw_radius=raw_radius,
                box=np.tile(np.array(BOX), (Q, 1)) if boxed else None, goal=goal, commands=commands, nx=nx)


def initial_arrays(case, max_episodes=MAX_EPISODES):
    """The in/out arrays at their start and the outputs sentinel-filled, as the device test allocates them."""
    nx = case["nx"]
    return dict(plant=case["plant0"].copy(), raw_pos=case["raw_pos0"].copy(), raw_vel=case["raw_vel0"].copy(), episode=np.zeros((Q, 4), np.int32),
                episode_f=np.zeros((Q, 2)), log=np.full((Q, max_episodes, 4), SENTINEL), was_reset=np.full(Q, 9, np.uint8),
                state4=np.full((Q, 4), SENTINEL), state_nx=np.full((Q, nx), SENTINEL), state_batch=np.full((Q * P, nx), SENTINEL),
                planner_ids=np.full((Q, P), -7, np.int32), selection=np.full((Q, 3), -7, np.int32), segment=np.full(Q, -7, np.int32))


def mirror_tick(case, arr, cmd, opt):
    """One tick of every scene by modules.episode_step, in place on `arr`."""
    from mpc_planner_amd import modules as md
    kw = {k: v for k, v in opt.items() if k != "max_episodes"}
    for q in range(len(case["plant0"])):
        reset, state4 = md.episode_step(cmd[q], arr["plant"][q], case["plant0"][q], case["count"][q], arr["raw_pos"][q], arr["raw_vel"][q],
                                        case["raw_radius"][q], case["raw_pos0"][q], case["raw_vel0"][q], arr["episode"][q], arr["episode_f"][q],
                                        arr["log"][q], box=None if case["box"] is None else case["box"][q],
                                        goal=None if case["goal"] is None else case["goal"][q], state_nx=arr["state_nx"][q],
                                        state_batch=arr["state_batch"][q * P:(q + 1) * P], planner_ids=arr["planner_ids"][q],
                                        selection=arr["selection"][q], segment=arr["segment"][q:q + 1], **kw)
        arr["was_reset"][q] = 1 if reset else 0
        arr["state4"][q] = state4


def run_mirror(case, opt, ticks=None):
    """Every tick's arrays (copies) and the events the run made occur."""
    arr = initial_arrays(case, opt["max_episodes"])
    history = []
    seen = dict(goal_disc=False, goal_x=False, timeout=False, collision=False, overflow=False, clipped_w=False, nan_timeout=False,
                reflect_xlo=False, reflect_xhi=False, reflect_ylo=False, reflect_yhi=False)
    for tick in range(len(case["commands"]) if ticks is None else ticks):
        cmd = case["commands"][tick]
        before = {k: arr[k].copy() for k in ("raw_vel", "episode", "log")}
        mirror_tick(case, arr, cmd, opt)
        history.append({k: v.copy() for k, v in arr.items()})
        seen["clipped_w"] |= bool((np.abs(cmd[:, 1]) > opt["max_angular_velocity"]).any())
        seen["collision"] |= bool((arr["episode_f"][:, 1] > 0.0).any() and (arr["episode"][:, 1] > 0).any())
        for q in range(len(cmd)):
            n_before = int(before["episode"][q, 2])
            if arr["was_reset"][q]:
                if n_before >= opt["max_episodes"]:
                    seen["overflow"] |= bool(np.array_equal(arr["log"][q], before["log"][q]) and arr["episode"][q, 2] == n_before + 1)
                    continue
                row = arr["log"][q, n_before]
                done = row[1] == 1.0
                seen["goal_x"] |= bool(done and q == 0)
                seen["goal_disc"] |= bool(done and q == 1)
                late = (not done) and row[0] == float(opt["timeout_ticks"]) * opt["control_dt"]
                seen["timeout"] |= bool(late)
                seen["nan_timeout"] |= bool(late and q == NAN_SCENE and tick >= NAN_FROM and np.array_equal(arr["plant"][q], case["plant0"][q]))
            elif case["box"] is not None:
                n = min(max(int(case["count"][q]), 0), N_SLOTS)
                flipped = arr["raw_vel"][q, :n] != before["raw_vel"][q, :n]
                pos = arr["raw_pos"][q, :n]
                seen["reflect_xlo"] |= bool((flipped[:, 0] & (pos[:, 0] < BOX[0])).any()); seen["reflect_xhi"] |= bool((flipped[:, 0] & (pos[:, 0] > BOX[1])).any())
                seen["reflect_ylo"] |= bool((flipped[:, 1] & (pos[:, 1] < BOX[2])).any()); seen["reflect_yhi"] |= bool((flipped[:, 1] & (pos[:, 1] > BOX[3])).any())
    return history, seen


def expected_events(boxed):
    return ["goal_disc", "goal_x", "timeout", "collision", "overflow", "clipped_w", "nan_timeout"] + \
           (["reflect_xlo", "reflect_xhi", "reflect_ylo", "reflect_yhi"] if boxed else [])
