"""What the tests of include/tmpc_hip_stack_scenario.h share (tests/test_gpu_stack_scenario.py, tests/test_gpu_cpp_stack_scenario.py): the sample
sets of test_gpu_parity.test_device_polygon_edge_cases plus a ring of 2000, and a Safe-Horizon closed loop of 2 scenes x 2 parallel solvers whose
every tick is also built on the host by the numpy mirrors (modules.sample_scenarios -> scenario_discard -> scenario_halfspaces ->
halfspace_rows_set_parameters)."""
import numpy as np

N, R, M, MODES = 20, 24, 8, 3
CFG5_SCENE = dict(N=N, M=M, slack=True, n_scenario=R)                       # scenes.make_scene
CFG5_DIMS = dict(N=N, S=5, n_lin=0, M=0, n_slk=R, slack=1)                  # solver.default_dims
RADIUS = 0.4 + 0.325                                                        # scenes.OBSTACLE_RADIUS + scenes.ROBOT_RADIUS
PREFIX = "disc_0_scenario_constraint"
EDGE_COUNTS = dict(tiny=5, duplicates=300, contradictory=400, big_ring=1500, ring_2000=2000, large=3000)

# the closed loop
SCENES, P, S_CEN, N_DISCARD, TICKS, SEED, TOL, DISC_OFFSET = (41, 44), 2, 128, 4, 3, 1000, 1e-3, 0.0
Q = len(SCENES)
B = Q * P


class Map:
    """parameters.ParameterMap.index() on a generated library's parameter_map (name -> column), for the mirrors that take a map."""

    def __init__(self, parameter_map):
        self._params = dict(parameter_map)

    def index(self, name):
        return self._params[name]


def edge_samples(shape, x0):
    """o [N][n][2] as test_device_polygon_edge_cases draws it (same generator, same seed) for the guesses x0 [B][N + 1][nv]: fewer samples than
    rows, exact duplicates, an EMPTY polygon at stages 5 .. 7 of trajectory 3, rings that overflow the first pass's candidate list (1500: the
    second pass's list below 48 KiB, 2000: above), 3000 samples."""
    n = EDGE_COUNTS[shape]
    rng = np.random.default_rng(17)
    p_mid = x0[:, :, 2:4].mean(axis=(0, 1))
    if shape in ("big_ring", "ring_2000"):
        th = rng.uniform(0, 2 * np.pi, (N, n))
        o = np.stack([np.cos(th), np.sin(th)], axis=-1) * 9.0 + p_mid                  # far: nearly every sample is an edge
    else:
        o = p_mid + rng.normal(0, 8.0, (N, n, 2))
        if shape == "duplicates":
            o[:, 150:] = o[:, :150]
    for k in range(1, N):                                                              # keep the samples off the guess positions
        d = np.linalg.norm(o[k - 1][None] - x0[:, k, None, 2:4], axis=2).min(axis=0)
        o[k - 1][d < 0.8] += 40.0
    if shape == "contradictory":
        for k in (5, 6, 7):
            o[k - 1, :6] = x0[3, k, 2:4] + np.array([[0.3, 0.0], [-0.3, 0.0], [0.31, 0.02], [-0.31, 0.02], [0.0, 0.35], [0.0, -0.35]])
    return o


def sentinel(start, cols):
    """start with a different negative value in every entry of the columns `cols`: a column written by mistake, or from the wrong place, cannot
    pass for untouched."""
    out = start.copy()
    out[:, :, cols] = -(1.0e3 + np.arange(out[:, :, cols].size, dtype=np.float64)).reshape(out[:, :, cols].shape)
    return out


def loop_problem():
    """Q scenes (scenes.make_scene, cfg 5) x P parallel solvers: batch entry b = q P + p is solver b of the sampler (every solver draws its own
    scenarios from its scene's mixture prediction, scenario_constraints.cpp:121-131) and starts from its scene's main warm start (:73)."""
    from mpc_planner_amd import scenes
    scs = [scenes.make_scene(i, B=P, **CFG5_SCENE) for i in SCENES]
    rep = lambda key: np.concatenate([np.repeat(sc[key][:1], P, 0) for sc in scs])
    long_pred = np.stack([scenes.mixture_prediction(sc["obstacles"]["pos"], TICKS) for sc in scs])        # [Q][M][3][N + TICKS][6]
    return dict(pm=scs[0]["pm"], xinit=rep("xinit"), x0=rep("x0"), params=rep("params"), long_pred=long_pred,
                prob=np.tile(scenes.MIXTURE_WEIGHTS, (B, M, 1)), scene_of=np.arange(B, dtype=np.int32))


def prediction(pb, tick):
    """[B][M][3][N][6]: the obstacles moved on one step per tick; the P solvers of a scene see the same prediction."""
    return np.ascontiguousarray(np.repeat(pb["long_pred"][:, :, :, tick:tick + N, :], P, 0))


def host_rows(pm, base, xinit, x0, pred, prob, seed, n_discard=N_DISCARD, s_cen=S_CEN, disc_offset=DISC_OFFSET):
    """One tick's scenario rows by the mirrors: base [B][N][npar] with the scenario columns and ego_disc_0_offset of every entry rewritten.
    Returns rows, which [B][N][R] (the flat sample index behind each row, -1: dummy), marks [B][s_cen], empty [B] (stages with an empty polygon)."""
    from mpc_planner_amd import modules as md
    smp_all = md.sample_scenarios(pred, prob, s_cen, seed)
    rows, which, marks, empty = base.copy(), [], [], []
    for b in range(len(base)):
        smp = smp_all[b].reshape(N, M, s_cen, 2).transpose(1, 2, 0, 3)                                    # [M][s_cen][N][2]
        mk = md.scenario_discard(x0[b], smp, RADIUS, n_discard) if n_discard else None
        a1, a2, bb, idx, emp = md.scenario_halfspaces(x0[b], smp, RADIUS, R, return_index=True, discard=mk)
        md.halfspace_rows_set_parameters(pm, rows[b], xinit[b, 0], (a1, a2, bb), PREFIX, R, disc_offset)
        which.append(idx); marks.append(mk if mk is not None else np.zeros(s_cen, bool)); empty.append(int(emp.sum()))
    return rows, np.stack(which), np.stack(marks), np.array(empty, np.int32)


def host_support(pm, xtraj, rows, which, s_cen=S_CEN, tol=TOL):
    from mpc_planner_amd import modules as md
    out = np.array([md.scenario_support(xtraj[b], rows[b], pm, which[b], s_cen, tol) for b in range(len(rows))], np.int32)
    return out[:, 0], out[:, 1]


def next_states(got, xinit):
    """Per scene: the robot moves to stage 1 of its best successful solver's plan (lowest objective, scenario_constraints.cpp:93-107) and every
    solver of the scene restarts from that plan, shifted (:73, :82); a scene without a successful solver keeps its first solver's plan.
    Returns state [B][nx], src [B]."""
    state, src = np.empty_like(xinit), np.zeros(B, np.int32)
    for q in range(Q):
        mine = np.arange(q * P, (q + 1) * P)
        ok = mine[got["exit_code"][mine] == 1]
        best = int(ok[np.argmin(got["pobj"][ok])]) if len(ok) else int(mine[0])
        state[mine] = got["xtraj"][best, 1]
        src[mine] = best
    return state, src
