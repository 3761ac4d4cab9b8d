"""The closed loop of the stack-environment tests (helper, no tests): two scenes of the generated `road_decomp` stack (rosnavigation T-MPC: N = 20,
3 path segments, 2 obstacles + 2 road rows in 4 topology rows, 2 ellipsoids, 4 decomp rows, slack model), each on a long reference path with a
costmap, and the host's answer to one tick -- every row of the stack by the numpy mirrors of mpc_planner_amd.modules, placed by the stack's own
parameter map.  Shared by tests/test_gpu_stack_env.py (device against this) and tests/test_stack_env_header.py (the conditions the scenes were
chosen for hold on the mirrors, without a GPU)."""
import functools

import numpy as np

from mpc_planner_amd import modules as md, scenes

N, M, S, N_TOPO, N_ROWS = 20, 2, 3, 4, 4
Q, P = 2, 2                                                  # scenes, planners (batch entries) per scene
B = Q * P
DT = scenes.DT
# 1 m either side of the polyline: the walls of scenes.with_costmap stand 0.9 - 1.6 m off the path, so some stages see them (more rows than the
# stack's four: truncated, status 1) and others see nothing and get the four rows of the box (status 0)
DECOMP_RANGE = 1.0
ROAD_WIDTH = 4.0
DISC_OFFSET = 0.02
P_MAX = 4096
N_SEG_MAX = 16
SCENES = (3, 1)                                              # chosen on the mirrors: in both, pillars truncate some stages and leave others complete
SHIFT = (2.8, 5.7)                                           # path parameter at the robot: a knot (every 3 m) is crossed within two ticks
RAW_COUNT = (2, 1)                                           # scene 1: one raw obstacle, the second prepared one is a dummy


class Map:
    """A stack's parameter map (name -> column) behind the .index() the numpy mirrors call."""

    def __init__(self, parameter_map):
        self.parameter_map = parameter_map

    def index(self, name):
        return self.parameter_map[name]


@functools.lru_cache(maxsize=None)
def problem():
    """The two scenes: make_scene's slack model, on scenes.with_long_path's path of 12 segments of 3 m (the window holds 3),
    with scenes.with_costmap's walls and pillars; the costmap's points by the mirror, once."""
    scs = []
    for i, idx in enumerate(SCENES):
        sc = scenes.make_scene(idx, N=N, M=M, B=P, S=S, slack=True, n_decomp=12)     # (its own synthetic corridor needs 8 rows; only its state, warm starts, obstacles and weights are used)
        sc = scenes.with_long_path(sc, np.random.default_rng(100 + idx), n_segments=12, seg_len=3.0, shift=SHIFT[i])
        sc = scenes.with_costmap(sc, 5000 + idx)
        pts, n_pts, overflow = md.costmap_points(sc["costmap"], sc["costmap_origin"], sc["costmap_resolution"], P_MAX)
        assert not overflow and n_pts > 100
        sc["points"] = pts
        scs.append(sc)
    raw_pos = np.stack([sc["obstacles"]["pos"][:, 0] for sc in scs])
    raw_vel = np.stack([(sc["obstacles"]["pos"][:, 1] - sc["obstacles"]["pos"][:, 0]) / DT for sc in scs])
    path = np.full((Q, N_SEG_MAX, 9), -3.0)
    for q, sc in enumerate(scs):
        path[q, :len(sc["path"])] = sc["path"]
    return dict(scenes=scs, xinit=np.concatenate([sc["xinit"] for sc in scs]), x0=np.concatenate([sc["x0"] for sc in scs]),
                scene_of=np.repeat(np.arange(Q, dtype=np.int32), P), main_of=(np.arange(Q, dtype=np.int32) * P),
                raw_pos=raw_pos, raw_vel=raw_vel, raw_radius=np.full((Q, M), scenes.OBSTACLE_RADIUS), raw_count=np.array(RAW_COUNT, np.int32),
                path=path, path_count=np.array([len(sc["path"]) for sc in scs], np.int32), path_length=np.array([sc["path_length"] for sc in scs]),
                offsets=md.road_offsets(ROAD_WIDTH, scenes.ROBOT_RADIUS), robot_radius=scenes.ROBOT_RADIUS)


def base_rows(parameter_map):
    """[B][N][npar] of the stack: the weights of the scenes' own rows placed by name, everything else zero (every other column of the stack is
    written each tick)."""
    pb = problem()
    rows = np.zeros((B, N, len(parameter_map)))
    for q, sc in enumerate(pb["scenes"]):
        for name in ("acceleration", "angular_velocity", "slack", "velocity", "reference_velocity", "contour", "lag", "terminal_angle", "terminal_contouring"):
            rows[q * P:(q + 1) * P, :, parameter_map[name]] = sc["params"][:, :, sc["pm"].index(name)]
    return rows


def host_tick(parameter_map, pcols, base, state, x0, prev_segment, tick):
    """One tick's rows on the host.  state [Q][6] = (x, y, psi, v, spline, slack), x0 [B][N + 1][8] the warm start, prev_segment [Q] the closest
    segments of the previous tick (-1: reset).  Returns dict(rows [B][N][npar], segment [Q], closest_s [Q], window [Q][S][9], road [Q][N][2][3],
    decomp = the mirror's dict per scene, obstacles = prepare_obstacles per scene)."""
    pb = problem()
    pm = Map(parameter_map)
    r = pb["robot_radius"]
    rows = base.copy()
    out = dict(rows=rows, segment=np.zeros(Q, np.int32), closest_s=np.zeros(Q), window=np.zeros((Q, S, 9)), road=np.zeros((Q, N, 2, 3)), decomp=[],
               obstacles=[])
    for q, sc in enumerate(pb["scenes"]):
        main = int(pb["main_of"][q])
        tr = md.track_path(sc["path"], sc["path_length"], state[q, :2], S, segment=int(prev_segment[q]))
        n_raw = int(pb["raw_count"][q])
        raw_pos = pb["raw_pos"][q] + pb["raw_vel"][q] * DT * tick
        obs = md.prepare_obstacles(state[q, :4], raw_pos[:n_raw], pb["raw_radius"][q, :n_raw], M, N, DT, raw_vel=pb["raw_vel"][q, :n_raw])
        road = md.road_halfspaces(tr["window"], x0[main, :N, md.IDX["spline"]], *pb["offsets"])
        dc = md.decomp_halfspaces(sc["path"], sc["path_length"], tr["s"], x0[main, :N, md.IDX["v"]], DT, sc["points"], DECOMP_RANGE, N_ROWS, state[q, 0])
        for b in range(q * P, (q + 1) * P):
            rows[b][:, pcols] = tr["window"].reshape(-1)[None, :]
            md.ellipsoid_set_parameters(pm, rows[b], state[q, :2], obs, r, disc_offset=DISC_OFFSET)
            lin = md.linearized_update(x0[b], obs["pos"], r, None, static=road)
            md.linearized_set_parameters(pm, rows[b], state[q, 0], lin, n_rows=N_TOPO)
            md.halfspace_rows_set_parameters(pm, rows[b], state[q, 0], (dc["a1"], dc["a2"], dc["b"]), "disc_0_decomp", N_ROWS, disc_offset=DISC_OFFSET)
        out["segment"][q], out["closest_s"][q], out["window"][q], out["road"][q] = tr["segment"], tr["s"], tr["window"], road
        out["decomp"].append(dc); out["obstacles"].append(obs)
    return out
