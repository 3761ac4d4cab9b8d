"""Scenes of the guidance search (tmpc_guidance_search) shared by the mirror, host-twin and GPU tests, and the mirror run over
them in the device's layouts.  A case is dict(N, dt, opt, ticks): opt the fields of tmpc_guidance_search_options, ticks a list of
dict(state4 [Q][4], goals [Q][G][3], obstacle_pos [Q][M][N][2], obstacle_radius [Q][M], selected [Q][M] i32, was_reset [Q] u8)."""
import numpy as np

from mpc_planner_amd import modules

OUTPUTS = ("nodes", "node_count", "traj_count", "topology_class", "status")
CARRIED = ("prev_traj", "prev_class", "prev_count", "next_class")
NODE_SENTINEL, INT_SENTINEL = -3.0, -7


def options(**kw):
    opt = dict(n_paths=4, n_samples=30, seed=0, n_nodes_max=64, max_expansions=4096, robot_radius=0.325, max_velocity=3.0, margin=0.5,
               weight_length=1.0)
    opt.update(kw)
    return opt


def fresh_arrays(Q, N, opt):
    """The outputs sentinel-filled and the carried arrays zeroed, as a caller allocates them."""
    P, R = opt["n_paths"], opt["n_nodes_max"]
    return dict(nodes=np.full((Q * P, R, 3), NODE_SENTINEL), node_count=np.full(Q * P, INT_SENTINEL, np.int32),
                traj_count=np.full(Q, INT_SENTINEL, np.int32), topology_class=np.full((Q, P), INT_SENTINEL, np.int32),
                status=np.full(Q, INT_SENTINEL, np.int32), prev_traj=np.zeros((Q, P, N + 1, 2)), prev_class=np.zeros((Q, P), np.int32),
                prev_count=np.zeros(Q, np.int32), next_class=np.zeros(Q, np.int32))


def mirror_tick(arrays, tick, N, dt, opt):
    """One tick of every scene through modules.guidance_search, in place on `arrays`."""
    Q, P = len(tick["state4"]), opt["n_paths"]
    for q in range(Q):
        reset = tick.get("was_reset") is not None and bool(tick["was_reset"][q])
        count, status = modules.guidance_search(
            tick["state4"][q], tick["goals"][q], tick["obstacle_pos"][q], tick["obstacle_radius"][q], tick["selected"][q], N, dt, q,
            opt["n_paths"], opt["n_samples"], opt["seed"], opt["n_nodes_max"], opt["max_expansions"], opt["robot_radius"], opt["max_velocity"],
            opt["margin"], opt["weight_length"], arrays["prev_traj"][q], arrays["prev_class"][q], arrays["prev_count"][q:q + 1],
            arrays["next_class"][q:q + 1], arrays["nodes"][q * P:(q + 1) * P], arrays["node_count"][q * P:(q + 1) * P],
            arrays["topology_class"][q], was_reset=reset)
        arrays["traj_count"][q] = count
        arrays["status"][q] = status


def run_mirror(case):
    """Every array after every tick: a list of dicts of copies."""
    arrays = fresh_arrays(len(case["ticks"][0]["state4"]), case["N"], case["opt"])
    history = []
    for tick in case["ticks"]:
        mirror_tick(arrays, tick, case["N"], case["dt"], case["opt"])
        history.append({k: v.copy() for k, v in arrays.items()})
    return history


def same(a, b):
    """Bit for bit, a NaN equal to a NaN in the same place."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def tick_of(starts, goals, obstacles, N, dt, M=None, was_reset=None):
    """A tick from scene descriptions: starts [Q][2], goals [Q][G][3], obstacles per scene a list of (x, y, vx, vy, radius) in prepared
    order -- constant velocity, prediction step s at p + v dt (s + 1) --, the other slots dummies as prepare_obstacles leaves them."""
    Q = len(starts)
    M = max(1, max(len(o) for o in obstacles)) if M is None else M
    state4 = np.zeros((Q, 4)); state4[:, 0:2] = np.asarray(starts, float)
    pos = np.zeros((Q, M, N, 2)); rad = np.zeros((Q, M)); sel = np.full((Q, M), -1, np.int32)
    steps = np.arange(1, N + 1)[:, None] * dt
    for q in range(Q):
        pos[q] = (state4[q, 0:2] + 100.0)[None, None, :]
        for j, (x, y, vx, vy, r) in enumerate(obstacles[q]):
            pos[q, j] = np.array([x, y])[None, :] + np.array([vx, vy])[None, :] * steps
            rad[q, j] = r; sel[q, j] = j
    return dict(state4=state4, goals=np.asarray(goals, float).reshape(Q, -1, 3), obstacle_pos=pos, obstacle_radius=rad, selected=sel,
                was_reset=np.zeros(Q, np.uint8) if was_reset is None else np.asarray(was_reset, np.uint8))


# ---- the one-obstacle scene of the issue: radius 0.5 midway between a start and a single goal 6 m apart, N = 20, dt = 0.2; 128 samples and margin 6 (the issue's 64 do not
# give both sides for every seed: tests/test_guidance_search_mirror.py) ----
ONE_N, ONE_DT = 20, 0.2
ONE_OPT = dict(n_samples=128, margin=6.0)


def one_obstacle(seed, n_paths=4, **kw):
    opt = options(seed=seed, n_paths=n_paths, **dict(ONE_OPT, **kw))
    return dict(N=ONE_N, dt=ONE_DT, opt=opt, ticks=[tick_of([(0.0, 0.0)], [[(6.0, 0.0, 0.0)]], [[(3.0, 0.0, 0.0, 0.0, 0.5)]], ONE_N, ONE_DT)])


def no_obstacle(seed=3):
    """Every slot a dummy; three goals, the middle one the cheapest, the first out of reach."""
    opt = options(seed=seed, n_samples=40, margin=1.0)
    goals = [[(40.0, 0.0, -5.0), (5.0, 1.0, 0.5), (5.0, -1.0, 0.25)]]
    return dict(N=ONE_N, dt=ONE_DT, opt=opt, ticks=[tick_of([(0.0, 0.0)], goals, [[]], ONE_N, ONE_DT, M=3)])


def identity_run(seed=58, ticks=6, reset_at=None, velocity=(-0.1, 0.05)):
    """The one-obstacle scene over `ticks` ticks: each tick the start moves to stage 1 of the cheapest trajectory the mirror found and the
    obstacle moves at a constant velocity.  Then one tick with the obstacle passed (3 m behind the start): the two classes merge."""
    opt = options(seed=seed, n_paths=4, **ONE_OPT)
    arrays = fresh_arrays(1, ONE_N, opt)
    start, ob, out = np.zeros(2), np.array([3.0, 0.0]), []
    for t in range(ticks + 1):
        where = ob if t < ticks else start - np.array([3.0, 0.0])
        tick = tick_of([start], [[(6.0, 0.0, 0.0)]], [[(where[0], where[1], velocity[0], velocity[1], 0.5)]], ONE_N, ONE_DT,
                       was_reset=[1 if reset_at == t else 0])
        out.append(tick)
        mirror_tick(arrays, tick, ONE_N, ONE_DT, opt)
        if arrays["traj_count"][0] > 0:
            start = arrays["prev_traj"][0, 0, 1].copy()
        ob = ob + np.array(velocity) * ONE_DT
    return dict(N=ONE_N, dt=ONE_DT, opt=opt, ticks=out)


# ---- the working shape: N = 20, 8 prepared obstacles out of raw lists of 5 .. 12, 9 goals on a 3 x 3 grid, n_paths = 4 ----
WORK_N, WORK_DT, WORK_M, WORK_SLOTS = 20, 0.2, 8, 12


def working_raw(Q, seed=11):
    """Raw obstacle lists per scene (count, pos, vel, radius over WORK_SLOTS slots) and the robots' states."""
    rng = np.random.default_rng(seed)
    count = rng.integers(5, WORK_SLOTS + 1, Q).astype(np.int32)
    state4 = np.zeros((Q, 4)); state4[:, 0] = rng.uniform(-1.0, 1.0, Q); state4[:, 1] = rng.uniform(-0.5, 0.5, Q); state4[:, 3] = 1.5
    pos = np.stack([rng.uniform(1.5, 7.0, (Q, WORK_SLOTS)), rng.uniform(-2.5, 2.5, (Q, WORK_SLOTS))], 2) + state4[:, None, 0:2]
    vel = rng.uniform(-0.6, 0.6, (Q, WORK_SLOTS, 2))
    radius = rng.uniform(0.2, 0.45, (Q, WORK_SLOTS))
    return dict(count=count, state4=state4, raw_pos=pos, raw_vel=vel, raw_radius=radius)


def goal_grid(state4, nx=3, ny=3, ahead=6.0, dx=1.0, dy=1.5):
    """n = nx ny goals ahead of each robot: (x + ahead + dx i, y + dy (j - (ny - 1) / 2)), the cost the lateral offset plus what is cut short."""
    Q = len(state4)
    goals = np.zeros((Q, nx * ny, 3))
    for i in range(nx):
        for j in range(ny):
            off = dy * (j - (ny - 1) / 2)
            goals[:, i * ny + j] = np.stack([state4[:, 0] + ahead + dx * i, state4[:, 1] + off, np.full(Q, abs(off) + 0.5 * dx * (nx - 1 - i))], 1)
    return goals


def prepared_tick(raw, goals, N, dt, M, was_reset=None):
    """A tick whose obstacle arrays are modules.prepare_obstacles' of the raw lists (the device test prepares them with
    tmpc_prepare_obstacles)."""
    Q = len(raw["state4"])
    pos = np.zeros((Q, M, N, 2)); rad = np.zeros((Q, M)); sel = np.zeros((Q, M), np.int32)
    for q in range(Q):
        c = int(raw["count"][q])
        prep = modules.prepare_obstacles(raw["state4"][q], raw["raw_pos"][q][:c], raw["raw_radius"][q][:c], M, N, dt, raw_vel=raw["raw_vel"][q][:c])
        pos[q], rad[q], sel[q] = prep["pos"], prep["radius"], prep["selected"]
    return dict(state4=raw["state4"].copy(), goals=goals, obstacle_pos=pos, obstacle_radius=rad, selected=sel,
                was_reset=np.zeros(Q, np.uint8) if was_reset is None else np.asarray(was_reset, np.uint8))


def working_case(seed, n_samples, Q=16):
    raw = working_raw(Q)
    opt = options(seed=seed, n_paths=4, n_samples=n_samples, margin=1.0, max_velocity=3.0)
    return dict(N=WORK_N, dt=WORK_DT, opt=opt, raw=raw, ticks=[prepared_tick(raw, goal_grid(raw["state4"]), WORK_N, WORK_DT, WORK_M)])


def limits_case(Q=4):
    """32 obstacles, 16 goals, 256 samples, n_paths = 16, R = 64."""
    rng = np.random.default_rng(5)
    N, dt = 20, 0.2
    starts = np.stack([rng.uniform(-1, 1, Q), rng.uniform(-1, 1, Q)], 1)
    goals = [[(starts[q, 0] + 7.0 + 0.5 * (i % 2), starts[q, 1] - 3.75 + 0.5 * i, 0.05 * i) for i in range(16)] for q in range(Q)]
    obstacles = [[(starts[q, 0] + rng.uniform(1.0, 6.5), starts[q, 1] + rng.uniform(-4, 4), rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5),
                   rng.uniform(0.1, 0.3)) for _ in range(32)] for q in range(Q)]
    opt = options(seed=9, n_paths=16, n_samples=256, n_nodes_max=64, margin=1.0, max_velocity=4.0, robot_radius=0.2)
    return dict(N=N, dt=dt, opt=opt, ticks=[tick_of(starts, goals, obstacles, N, dt)])


def smallest_cases():
    """The smallest shapes, each built to yield a trajectory, with the counts the mirror has to give (test_guidance_search_mirror.py asserts
    them, so the device comparison has content).  Each scene has its own dt: a handle for it is created with that dt."""
    # N = 2, one obstacle, one goal, one sample: the obstacle sits on the direct connection at stage 1, the one sample (its only possible
    # stage is 1) passes beside it: one trajectory of 3 nodes through stage 1
    two = dict(N=2, dt=0.5, opt=options(seed=3, n_samples=1, margin=1.0, max_velocity=6.0), want=dict(count=1, nodes=[3]),
               ticks=[tick_of([(0.0, 0.0)], [[(2.0, 0.0, 0.0)]], [[(1.0, 0.0, 0.0, 0.0, 0.2)]], 2, 0.5)])
    # N = 3, n_paths = 1: the obstacle blocks the direct connection, both sides are found, one is returned
    three = dict(N=3, dt=0.5, opt=options(seed=3, n_paths=1, n_samples=40, margin=1.5, max_velocity=6.0), want=dict(count=1, nodes=[3]),
                 ticks=[tick_of([(0.0, 0.0)], [[(3.0, 0.0, 0.0)]], [[(1.5, 0.0, 0.0, 0.0, 0.3)]], 3, 0.5)])
    # n_samples = 0 beside a real obstacle: the direct connection alone
    none = dict(N=ONE_N, dt=ONE_DT, opt=options(seed=0, n_samples=0), want=dict(count=1, nodes=[2]),
                ticks=[tick_of([(0.0, 0.0)], [[(6.0, 0.0, 0.0)]], [[(3.0, 2.0, 0.0, 0.0, 0.5)]], ONE_N, ONE_DT)])
    # the start inside an obstacle at stage 0 (0.3 m from the centre of a disc of 0.2 + 0.325 that moves away behind the robot at 2 m/s; stage
    # 0 and stage 1 both see prepared step 0): stage 0 is never tested, so trajectories exist -- they have to be clear of it at stage 1, which
    # the direct connection is not --, and some go through two connectors (5 nodes)
    inside = dict(N=10, dt=0.2, opt=options(seed=2, n_samples=60, margin=1.5, max_velocity=6.0), want=dict(count=3, nodes=[3, 5, 5]),
                  ticks=[tick_of([(0.0, 0.0)], [[(4.0, 0.0, 0.0)]], [[(0.7, 0.0, -2.0, 0.0, 0.2), (2.5, 0.0, 0.0, 0.0, 0.4)]], 10, 0.2)])
    return [two, three, none, dict(no_obstacle(), want=dict(count=1, nodes=[2])), inside]


def chain_case():
    """Three goals behind three obstacles at a max_velocity that leaves many samples out of reach of the start or the goals: they become
    intermediate guards, and one of the three classes is reached only through two connectors (5 nodes): the descent below depth 0."""
    goals = [[(6.0, -1.5 + 1.5 * i, 0.1 * i) for i in range(3)]]
    obstacles = [[(2.0, 0.0, 0.0, 0.0, 0.4), (4.0, 1.0, 0.0, -0.3, 0.4), (4.0, -1.2, 0.0, 0.3, 0.4)]]
    return dict(N=20, dt=0.2, opt=options(seed=3, n_paths=8, n_samples=96, margin=1.0, max_velocity=2.5, robot_radius=0.2),
                want=dict(count=3, nodes=[3, 3, 5]), ticks=[tick_of([(0.0, 0.0)], goals, obstacles, 20, 0.2)])


# ---- the capacity flags, one scene each ----
def flag_guards_full():
    """No connection is reachable at this max_velocity: every sample becomes a guard until the table of 32 is full."""
    opt = options(seed=5, n_samples=64, max_velocity=1e-3, margin=1.0)
    return dict(N=10, dt=0.2, opt=opt, ticks=[tick_of([(0.0, 0.0)], [[(4.0, 0.0, 0.0)]], [[(2.0, 0.0, 0.0, 0.0, 0.3)]], 10, 0.2)])


def flag_connectors_full():
    """16 goals and four columns of 8 tiny obstacles that cross the field in alternating directions, every sample reachable: more than 128
    (guard pair, class) combinations among 256 samples."""
    opt = options(seed=2, n_samples=256, n_paths=16, margin=0.5, robot_radius=0.01, max_velocity=100.0)
    goals = [[(8.0, (-7.5 + 1.0 * i) * 0.5, 0.1 * (i % 3)) for i in range(16)]]
    obstacles = [[(1.0 + 2.0 * (j // 8), (-7.0 + 2.0 * (j % 8) + 1.0 * ((j // 8) % 2)) * 0.5, 0.0, 3.0 * (1 if j % 2 else -1), 0.02) for j in range(32)]]
    return dict(N=8, dt=0.25, opt=opt, ticks=[tick_of([(0.0, 0.0)], goals, obstacles, 8, 0.25)])


def flag_expansions():
    case = one_obstacle(0, max_expansions=1)
    return case


def flag_nodes():
    return one_obstacle(0, n_nodes_max=2)


FLAG_CASES = ((1, flag_guards_full), (2, flag_connectors_full), (4, flag_expansions), (8, flag_nodes))


def well_formed(case, out):
    """What every result has to satisfy, whatever the flags: counts in range, nodes of increasing stage from the start to a present goal."""
    N, dt, opt = case["N"], case["dt"], case["opt"]
    P, R = opt["n_paths"], opt["n_nodes_max"]
    tick = case["ticks"][-1]
    for q in range(len(tick["state4"])):
        count = int(out["traj_count"][q])
        assert 0 <= count <= P and 0 <= int(out["status"][q]) < 16
        assert count == int(out["prev_count"][q])
        for i in range(P):
            n = int(out["node_count"][q * P + i])
            if i >= count:
                assert n == 0 and out["topology_class"][q][i] == -1
                continue
            nd = out["nodes"][q * P + i]
            assert 2 <= n <= R and np.all(nd[n:] == NODE_SENTINEL)
            ks = np.rint(nd[:n, 0] / dt).astype(int)
            assert np.array_equal(ks.astype(float) * dt, nd[:n, 0]) and np.all(np.diff(ks) > 0) and ks[0] == 0 and ks[-1] == N
            assert np.array_equal(nd[0, 1:], tick["state4"][q][0:2])
            assert any(np.array_equal(nd[n - 1, 1:], g[0:2]) for g in tick["goals"][q])
        cls = out["topology_class"][q][:count]
        assert len(set(cls.tolist())) == count and np.all(cls >= 0)
