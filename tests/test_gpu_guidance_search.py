"""GPU: the guidance search on device (tmpc_guidance_search; include/tmpc_hip_guidance_search.h; csrc/tmpc_guidance_search.hpp)
against the host mirror (mpc_planner_amd/modules.py guidance_search, pinned on its properties in tests/test_guidance_search_mirror.py).
Equality is bitwise on every output and every carried array: the results are decisions, copies and fixed-order + - x / sqrt expressions.
Then the closed loop of tests/test_gpu_episode.py with the canned guidance replaced by the search, enqueued back to back on one stream,
against the same ticks driven from the host."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import guidance_search_cases as gc  # noqa: E402
from test_gpu_episode import SENTINEL, _full, _generated_solver, _loop_scene_velocities, _same, _up  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = {np.dtype(np.float64): gc.NODE_SENTINEL, np.dtype(np.int32): gc.INT_SENTINEL}
PER_SCENE = {"nodes": "P", "node_count": "P"}                                                        # arrays whose leading axis is n_scenes n_paths


def _solver(N, B_max=12, dt=0.2):
    """A handle with horizon N and time step dt: the search reads both from it."""
    from mpc_planner_amd import solver
    s = solver.BatchedSolver(solver.default_dims(N=N, S=5, n_lin=8, M=8, dt=float(dt)), B_max=B_max)
    assert float(s.dims.dt) == float(dt) and int(s.dims.N) == N
    return s


class _DeviceSearch:
    """The outputs sentinel-filled and the carried arrays zeroed on the device, every array one scene longer than the launch covers: the
    guard scene has to keep its fill."""

    def __init__(self, s, Q, N, opt):
        from mpc_planner_amd import guidance_search as gs
        self.s, self.Q, self.P, self.entry, self.opt = s, Q, opt["n_paths"], gs.GuidanceSearch(s), gs.guidance_search_options(**opt)
        start = gc.fresh_arrays(Q + 1, N, opt)
        for k in gc.CARRIED:
            start[k][Q:] = FILL[start[k].dtype]
        self.t = {k: _up(v) for k, v in start.items()}

    def pointers(self):
        return {"d_" + k: v.data_ptr() for k, v in self.t.items()}

    def search(self, n_goals, M, d_state4, d_goals, d_pos, d_rad, d_sel, d_was_reset=None):
        self.entry.search(self.Q, n_goals, M, self.opt, d_state4, d_goals, d_pos, d_rad, d_sel, d_was_reset=d_was_reset, **self.pointers())

    def check(self, want, tick=0):
        for k, t in self.t.items():
            got = t.cpu().numpy()
            n = self.Q * (self.P if k in PER_SCENE else 1)
            assert _same(got[:n], want[k]), (tick, k)
            assert (got[n:] == FILL[got.dtype]).all(), (tick, k, "the guard scene was written")


def _run_case(s, case):
    """Every tick of a case: upload its inputs, search, compare every output and carried array with the mirror's."""
    history = gc.run_mirror(case)
    t0 = case["ticks"][0]
    Q, G, M = len(t0["state4"]), t0["goals"].shape[1], t0["selected"].shape[1]
    dev = _DeviceSearch(s, Q, case["N"], case["opt"])
    for tick, (inp, want) in enumerate(zip(case["ticks"], history)):
        u = {k: _up(inp[k]) for k in ("state4", "goals", "obstacle_pos", "obstacle_radius", "selected", "was_reset")}
        dev.search(G, M, u["state4"].data_ptr(), u["goals"].data_ptr(), u["obstacle_pos"].data_ptr(), u["obstacle_radius"].data_ptr(),
                   u["selected"].data_ptr(), d_was_reset=u["was_reset"].data_ptr())
        s.synchronize()
        dev.check(want, tick)
        for k, v in u.items():
            assert _same(v.cpu().numpy(), inp[k]), k                                                 # inputs are inputs
    return history


def test_smallest_shapes():
    """N = 2 with one sample, one obstacle, one goal (a 3-node trajectory through stage 1); N = 3 with n_paths = 1; n_samples = 0; every slot
    a dummy; the start inside an obstacle at stage 0 (three trajectories that leave it).  Each scene on a handle of its own N and dt; the
    counts are those tests/test_guidance_search_mirror.py pins on the mirror, so nodes, classes and carried trajectories are compared."""
    for case in gc.smallest_cases():
        s = _solver(case["N"], dt=case["dt"])
        out = _run_case(s, case)[-1]
        want = case["want"]
        assert out["traj_count"][0] == want["count"] and out["node_count"][:want["count"]].tolist() == want["nodes"]
        print(f"[smallest N={case['N']}] count {out['traj_count'].tolist()} nodes {out['node_count'].tolist()} status {out['status'].tolist()}")
        s.close()


@pytest.mark.parametrize("n_samples", (30, 64))
def test_working_shape_on_device_prepared_obstacles(n_samples):
    """N = 20, 8 obstacles prepared by tmpc_prepare_obstacles on device from raw lists of 5 .. 12, 9 goals on a 3 x 3 grid, n_paths = 4,
    16 scenes, three seeds, 30 samples (the reference's configuration) and 64."""
    import torch
    s = _solver(gc.WORK_N)
    assert float(s.dims.dt) == gc.WORK_DT
    Q, M, N = 16, gc.WORK_M, gc.WORK_N
    found = []
    for seed in (1, 2, 3):
        case = gc.working_case(seed, n_samples, Q)
        raw, tick = case["raw"], case["ticks"][0]
        want = gc.run_mirror(case)[-1]
        u = {k: _up(raw[k]) for k in ("count", "state4", "raw_pos", "raw_vel", "raw_radius")}
        o_pos, o_shape = _full((Q, M, N, 2), SENTINEL, torch.float64), _full((Q, M, N, 3), SENTINEL, torch.float64)
        o_rad, o_gauss, o_sel = _full((Q, M), SENTINEL, torch.float64), _full((Q, M), 9, torch.uint8), _full((Q, M), -7, torch.int32)
        s.prepare_obstacles(Q, gc.WORK_SLOTS, M, u["count"].data_ptr(), u["state4"].data_ptr(), u["raw_pos"].data_ptr(), u["raw_radius"].data_ptr(),
                            o_pos.data_ptr(), o_shape.data_ptr(), o_rad.data_ptr(), o_gauss.data_ptr(), o_sel.data_ptr(), d_raw_vel=u["raw_vel"].data_ptr())
        dev, t_goals = _DeviceSearch(s, Q, N, case["opt"]), _up(tick["goals"])
        dev.search(9, M, u["state4"].data_ptr(), t_goals.data_ptr(), o_pos.data_ptr(), o_rad.data_ptr(), o_sel.data_ptr())
        s.synchronize()
        assert _same(o_pos.cpu().numpy(), tick["obstacle_pos"]) and np.array_equal(o_sel.cpu().numpy(), tick["selected"])
        dev.check(want)
        found.append(want["traj_count"].tolist())
    print(f"[working n_samples={n_samples}] trajectories per scene {found}")
    assert max(max(f) for f in found) >= 2
    s.close()


def test_limits_chains_and_capacity_flags():
    """32 obstacles, 16 goals, 256 samples, n_paths = 16, R = 64, four scenes; the chain scene, whose third class goes through two connectors
    (5 nodes: the descent below depth 0); then each capacity-flag scene of the CPU tests."""
    for name, case in [("limits", gc.limits_case()), ("chain", gc.chain_case())] + [("flag %d" % f, make()) for f, make in gc.FLAG_CASES]:
        s = _solver(case["N"], dt=case["dt"])
        out = _run_case(s, case)[-1]
        print(f"[{name}] count {out['traj_count'].tolist()} nodes {out['node_count'].tolist()} status {out['status'].tolist()}")
        if name == "chain":
            assert out["node_count"].max() >= 5
        elif name != "limits":
            assert out["status"][0] & int(name.split()[1])
        s.close()


def test_eight_ticks_of_carried_state_with_the_episode_step():
    """Four scenes, eight ticks: tmpc_episode_step moves the robots and the obstacles and writes d_was_reset, tmpc_prepare_obstacles the
    predictions, the search reads both.  Scene 1 reaches its goal disc mid-run and restarts: its class ids start at 0 again."""
    import torch
    from mpc_planner_amd import episode, modules as md
    s = _solver(gc.WORK_N)
    Q, M, N, P, ticks, dt = 4, gc.WORK_M, gc.WORK_N, 3, 8, float(s.dims.dt)
    raw = gc.working_raw(Q, seed=21)
    count = np.full(Q, M, np.int32)
    start = raw["state4"].copy(); start[:, 2] = 0.0; start[:, 3] = 1.5
    plant0 = np.concatenate([start, np.cos(start[:, 2:3]), np.sin(start[:, 2:3])], 1)
    raw_pos0, raw_vel0, raw_radius = raw["raw_pos"][:, :M].copy(), raw["raw_vel"][:, :M].copy(), raw["raw_radius"][:, :M].copy()
    goal = np.stack([start[:, 0] + 50.0, start[:, 1], np.full(Q, 0.1)], 1); goal[1, 0] = start[1, 0] + 0.3
    eopt = dict(substeps=2, timeout_ticks=0, max_episodes=2, control_dt=0.05, max_acceleration=0.0, max_angular_velocity=2.0, robot_radius=0.325)
    sopt = gc.options(seed=6, n_paths=4, n_samples=48, margin=1.0, max_velocity=3.0)
    world = episode.EpisodeWorld(s, P, plant0, raw_pos0, raw_vel0, raw_radius, episode.episode_options(**eopt), count=count, goal=goal)
    cmd = np.tile(np.array([1.5, 0.1]), (Q, 1)); t_cmd = _up(cmd)
    base_goals = gc.goal_grid(np.zeros((Q, 4)))
    o_pos, o_shape = _full((Q, M, N, 2), SENTINEL, torch.float64), _full((Q, M, N, 3), SENTINEL, torch.float64)
    o_rad, o_gauss, o_sel = _full((Q, M), SENTINEL, torch.float64), _full((Q, M), 9, torch.uint8), _full((Q, M), -7, torch.int32)
    dev = _DeviceSearch(s, Q, N, sopt)
    h = dict(plant=plant0.copy(), raw_pos=raw_pos0.copy(), raw_vel=raw_vel0.copy(), episode=np.zeros((Q, 4), np.int32), episode_f=np.zeros((Q, 2)),
             log=np.zeros((Q, 2, 4)))
    arrays = gc.fresh_arrays(Q, N, sopt)
    resets = []
    for tick in range(ticks):
        world.step(t_cmd.data_ptr())
        s.prepare_obstacles(Q, M, M, world.count.data_ptr(), world.state4.data_ptr(), world.raw_pos.data_ptr(), world.raw_radius.data_ptr(), o_pos.data_ptr(),
                            o_shape.data_ptr(), o_rad.data_ptr(), o_gauss.data_ptr(), o_sel.data_ptr(), d_raw_vel=world.raw_vel.data_ptr())
        s.synchronize()
        state4 = world.state4.cpu().numpy()
        goals = base_goals.copy(); goals[:, :, 0:2] += state4[:, None, 0:2]
        t_goals = _up(goals)
        dev.search(9, M, world.state4.data_ptr(), t_goals.data_ptr(), o_pos.data_ptr(), o_rad.data_ptr(), o_sel.data_ptr(), d_was_reset=world.was_reset.data_ptr())
        s.synchronize()
        host4, reset = np.zeros((Q, 4)), np.zeros(Q, np.uint8)
        for q in range(Q):
            reset[q], host4[q] = md.episode_step(cmd[q], h["plant"][q], plant0[q], count[q], h["raw_pos"][q], h["raw_vel"][q], raw_radius[q], raw_pos0[q],
                                                 raw_vel0[q], h["episode"][q], h["episode_f"][q], h["log"][q], goal=goal[q], **{k: v for k, v in eopt.items() if k != "max_episodes"})
        assert _same(state4, host4) and np.array_equal(world.was_reset.cpu().numpy(), reset), tick
        rawt = dict(count=count, state4=host4, raw_pos=h["raw_pos"], raw_vel=h["raw_vel"], raw_radius=raw_radius)
        gc.mirror_tick(arrays, gc.prepared_tick(rawt, goals, N, dt, M, was_reset=reset), N, dt, sopt)
        dev.check(arrays, tick)
        resets.append(reset.tolist())
        print(f"[carried] tick {tick}: reset {reset.tolist()} count {arrays['traj_count'].tolist()} classes {arrays['topology_class'].tolist()} next {arrays['next_class'].tolist()}")
    assert any(r[1] for r in resets[2:]) and not any(r[0] for r in resets)
    s.close()


def test_every_refusal():
    """Each condition of the header's list returns TMPC_ERR_INVALID with a message naming tmpc_guidance_search and launches nothing: the
    sentinel-filled outputs and the carried arrays stay as they were.  A NULL handle returns -1."""
    from mpc_planner_amd import guidance_search as gs, solver
    s = _solver(gc.ONE_N)
    case = gc.one_obstacle(0)
    tick, base = case["ticks"][0], case["opt"]
    dev = _DeviceSearch(s, 1, case["N"], base)
    u = {k: _up(tick[k]) for k in ("state4", "goals", "obstacle_pos", "obstacle_radius", "selected", "was_reset")}
    args = dict(n_scenes=1, n_goals=1, max_obstacles=1, options=dev.opt, d_state4=u["state4"].data_ptr(), d_goals=u["goals"].data_ptr(),
                d_obstacle_pos=u["obstacle_pos"].data_ptr(), d_obstacle_radius=u["obstacle_radius"].data_ptr(), d_selected=u["selected"].data_ptr(),
                d_was_reset=u["was_reset"].data_ptr(), **dev.pointers())
    before = {k: v.cpu().numpy().copy() for k, v in dev.t.items()}
    opt = lambda **kw: gs.guidance_search_options(**dict(base, **kw))
    good = opt()
    short = opt(); short.size = C.sizeof(short) - 8
    long_dirty = (C.c_char * (C.sizeof(good) + 8)).from_buffer_copy(bytes(good) + b"\0\0\0\1\0\0\0\0")
    dirty = C.cast(long_dirty, C.POINTER(gs.TmpcGuidanceSearchOptions)).contents; dirty.size = C.sizeof(good) + 8
    opt_reserved = opt(); opt_reserved.reserved = 1
    required = [a for a in gs.ARRAYS if a not in gs.OPTIONAL]
    assert len(required) == 14
    inf, nan = float("inf"), float("nan")
    refusals = [(dict(options=None), "NULL options"), (dict(n_scenes=0), "n_scenes"), (dict(n_scenes=-1), "n_scenes"), (dict(n_goals=0), "n_goals"),
                (dict(n_goals=17), "n_goals"), (dict(max_obstacles=0), "max_obstacles"), (dict(max_obstacles=33), "max_obstacles"),
                (dict(options=opt(n_paths=0)), "n_paths"), (dict(options=opt(n_paths=17)), "n_paths"), (dict(options=opt(n_samples=-1)), "n_samples"),
                (dict(options=opt(n_samples=257)), "n_samples"), (dict(options=opt(n_nodes_max=1)), "n_nodes_max"),
                (dict(options=opt(n_nodes_max=65)), "n_nodes_max"), (dict(options=opt(max_expansions=0)), "max_expansions"),
                (dict(options=opt(max_expansions=65537)), "max_expansions"), (dict(options=opt(robot_radius=-0.1)), "robot_radius"),
                (dict(options=opt(robot_radius=nan)), "robot_radius"), (dict(options=opt(max_velocity=0.0)), "max_velocity"),
                (dict(options=opt(max_velocity=inf)), "max_velocity"), (dict(options=opt(max_velocity=nan)), "max_velocity"),
                (dict(options=opt(weight_length=0.0)), "weight_length"), (dict(options=opt(weight_length=inf)), "weight_length"),
                (dict(options=opt(margin=-0.5)), "margin"), (dict(options=opt(margin=inf)), "margin"), (dict(options=opt(margin=nan)), "margin"),
                (dict(options=opt_reserved), "reserved"), (dict(options=short), "smaller"), (dict(options=dirty), "non-zero field")] + [(dict([(k, None)]), "NULL") for k in required]
    for kw, msg in refusals:
        with pytest.raises(solver.TmpcError, match=msg) as e:
            dev.entry.search(**dict(args, **kw))
        assert "tmpc_guidance_search" in str(e.value) and "(-1)" in str(e.value), (kw, str(e.value))
    s.synchronize()
    for k, v in dev.t.items():
        assert _same(v.cpu().numpy(), before[k]), k                                                  # nothing was launched
    assert s.lib.tmpc_guidance_search(None, 1, 1, 1, C.byref(good), *([None] * 15)) == -1            # no handle: TMPC_ERR_INVALID
    # accepted: the same call, without a batch; d_was_reset NULL; a newer, longer options struct with a zero tail
    want = gc.run_mirror(case)[-1]
    dev.entry.search(**args)
    s.synchronize(); dev.check(want)
    long_clean = (C.c_char * (C.sizeof(good) + 8)).from_buffer_copy(bytes(good) + b"\0" * 8)
    clean = C.cast(long_clean, C.POINTER(gs.TmpcGuidanceSearchOptions)).contents; clean.size = C.sizeof(good) + 8
    dev2 = _DeviceSearch(s, 1, case["N"], base)
    dev2.entry.search(**dict(args, options=clean, d_was_reset=None, **dev2.pointers()))
    s.synchronize(); dev2.check(want)
    s.close()


def test_a_generated_library_equals_the_mirror():
    """The same call on the generated tmpc_cfg2 library (its parameter layout is the module stack's: the search reads no column): the working
    shape on four scenes and the class-identity run of seven ticks."""
    s = _generated_solver()
    assert hasattr(s.lib, "tmpc_guidance_search")
    assert float(s.dims.dt) == gc.WORK_DT == gc.ONE_DT
    _run_case(s, gc.working_case(1, 30, Q=4))
    _run_case(s, gc.identity_run())
    s.close()


def test_the_loop_closes_on_the_device_with_the_search():
    """The device loop of tests/test_gpu_episode.py with the canned nodes, counts and classes replaced by tmpc_guidance_search on the obstacles
    tmpc_prepare_obstacles just wrote and a goal grid ahead of the robot: 2 scenes x (2 + 1) planners, N = 20, M = 8, 12 ticks of 0.05 s.
    Handle A enqueues all twelve ticks back to back on its stream -- episode_step -> prepare_obstacles -> guidance_search -> guidance_plan ->
    warmstart -> sample_guidance -> init_with_guidance -> set_obstacle_parameters -> linearize_topology_ex -> solve -> guidance_decide --,
    every tick's results copied into per-tick tensors on the stream, one synchronisation at the end.  Handle B runs the same ticks driven
    from the host with the mirrors.  xtraj, utraj, pobj, the exit codes, best, the command and the world state are equal bit for bit at
    every tick, and so is everything the search wrote."""
    import torch
    from mpc_planner_amd import distributed, episode, guidance_search as gs, modules as md, scenes, solver
    from test_gpu_episode import M, N, S, _solver as _loop_solver
    from test_gpu_guidance_handoff import E2E_SEEDS
    seeds = E2E_SEEDS
    Q, n_paths, P, ticks, R, G = 2, 2, 3, 12, 6, 9
    B = Q * P
    scs = [scenes.make_scene(seed, N=N, M=M, B=n_paths, tmpc_pp=True) for seed in seeds]
    xinit = np.concatenate([sc["xinit"] for sc in scs]); params = np.concatenate([sc["params"] for sc in scs])
    nx = xinit.shape[1]
    x0 = np.full((B, N + 1, 7), SENTINEL)
    scene_of = np.repeat(np.arange(Q, dtype=np.int32), P)
    r, decel, cdt, w_cons = scenes.ROBOT_RADIUS, 3.0, 0.05, 0.8
    kw = dict(use_tmpcpp=True, warmstart_with_mpc_solution=True, shift_previous_solution_forward=True, selection_weight_consistency=w_cons)
    gopt = solver.guidance_options(n_paths, **kw)
    eopt = dict(substeps=2, timeout_ticks=5, max_episodes=2, control_dt=cdt, max_acceleration=3.0, max_angular_velocity=2.0, robot_radius=r, goal_x=0.3)
    sopt = gc.options(seed=4, n_paths=n_paths, n_samples=30, n_nodes_max=R, margin=1.0, max_velocity=3.0, robot_radius=r)
    d_eopt = episode.episode_options(**eopt)
    start = np.array([[0.0, 0.0, 0.0, 2.0], [-1.0, 0.0, 0.0, 1.0]])
    plant0 = np.concatenate([start, np.cos(start[:, 2:3]), np.sin(start[:, 2:3])], 1)
    raw_pos0 = np.ascontiguousarray(np.stack([sc["obstacles"]["pos"][:, 0] for sc in scs]))
    raw_vel0 = np.stack([_loop_scene_velocities(seed) for seed in seeds])
    raw_radius = np.stack([sc["obstacles"]["radius"] for sc in scs])
    count = np.full(Q, M, np.int32)
    cmd0 = np.stack([start[:, 3], np.zeros(Q)], 1)
    base_goals = gc.goal_grid(np.zeros((Q, 4)), ahead=5.0)
    A, Bh = _loop_solver(B), _loop_solver(B)
    dt = float(A.dims.dt)
    i32, u8, f64 = torch.int32, torch.uint8, torch.float64
    # ---- handle A: everything on the device, nothing read back before the end
    t_xinit, t_x0, t_params = _up(xinit), _up(x0), _up(params)
    A.set_batch_device(B, t_xinit.data_ptr(), t_x0.data_ptr(), t_params.data_ptr())
    world = episode.EpisodeWorld(A, P, plant0, raw_pos0, raw_vel0, raw_radius, d_eopt, count=count)
    search = gs.GuidanceSearchState(A, Q, gs.guidance_search_options(**sopt))
    t_cmd = _up(cmd0)
    t_base_goals, t_goals = _up(base_goals), _up(base_goals)
    t_nodes, t_ncnt, t_sc, t_sx = _full((B, R, 3), -9e9, f64), _full((B,), 0, i32), _up(scene_of), _full((Q,), SENTINEL, f64)
    o_pos, o_shape = _full((Q, M, N, 2), SENTINEL, f64), _full((Q, M, N, 3), SENTINEL, f64)
    o_rad, o_gauss, o_sel = _full((Q, M), SENTINEL, f64), _full((Q, M), 9, u8), _full((Q, M), -7, i32)
    t_mode, t_src, t_gid = _full((B,), -7, i32), _full((B,), -7, i32), _full((B,), -7, i32)
    t_init, t_dummy, t_dis, t_w = _full((B,), 9, u8), _full((B,), 9, u8), _full((B,), 9, u8), _full((B,), SENTINEL, f64)
    t_gpos, t_gvel, t_status = _full((B, N + 1, 2), SENTINEL, f64), _full((B, N + 1, 2), SENTINEL, f64), _full((B,), -7, i32)
    t_best, t_exit, t_each = _full((Q,), -7, i32), _full((Q,), -7, i32), _full((B,), 0, i32)
    rec = dict(xtraj=_full((ticks, B, (N + 1) * nx), SENTINEL, f64), utraj=_full((ticks, B, N * 2), SENTINEL, f64), records=_full((ticks, B, 2), 0, torch.int64),
               best=_full((ticks, Q), -7, i32), cmd=_full((ticks, Q, 2), SENTINEL, f64), plant=_full((ticks, Q, 6), SENTINEL, f64),
               raw_pos=_full((ticks, Q, M, 2), SENTINEL, f64), raw_vel=_full((ticks, Q, M, 2), SENTINEL, f64), episode=_full((ticks, Q, 4), -7, i32),
               episode_f=_full((ticks, Q, 2), SENTINEL, f64), log=_full((ticks, Q, 2, 4), SENTINEL, f64), was_reset=_full((ticks, Q), 9, u8),
               mode=_full((ticks, B), -7, i32), o_pos=_full((ticks, Q, M, N, 2), SENTINEL, f64), traj_count=_full((ticks, Q), -7, i32),
               topology_class=_full((ticks, Q, n_paths), -7, i32), node_count=_full((ticks, Q * n_paths), -7, i32),
               nodes=_full((ticks, Q * n_paths, R, 3), SENTINEL, f64), prev_traj=_full((ticks, Q, n_paths, N + 1, 2), SENTINEL, f64),
               status=_full((ticks, Q), -7, i32))
    d_pobj, d_code = A.result_device_ptrs()
    hs = torch.cuda.ExternalStream(A.stream_ptr(), device=torch.device("cuda"))
    torch.cuda.synchronize()
    for tick in range(ticks):
        world.step(t_cmd.data_ptr())
        with torch.cuda.stream(hs):
            for k, t in (("plant", world.plant), ("raw_pos", world.raw_pos), ("raw_vel", world.raw_vel), ("episode", world.episode), ("episode_f", world.episode_f),
                         ("log", world.log_rows), ("was_reset", world.was_reset)):
                rec[k][tick].copy_(t)
            t_sx.copy_(world.state4[:, 0])
            t_goals.copy_(t_base_goals); t_goals[:, :, 0:2] += world.state4[:, None, 0:2]
        A.prepare_obstacles(Q, M, M, world.count.data_ptr(), world.state4.data_ptr(), world.raw_pos.data_ptr(), world.raw_radius.data_ptr(), o_pos.data_ptr(),
                            o_shape.data_ptr(), o_rad.data_ptr(), o_gauss.data_ptr(), o_sel.data_ptr(), d_raw_vel=world.raw_vel.data_ptr())
        search.search(G, M, world.state4.data_ptr(), t_goals.data_ptr(), o_pos.data_ptr(), o_rad.data_ptr(), o_sel.data_ptr(), d_was_reset=world.was_reset.data_ptr())
        with torch.cuda.stream(hs):                                                                  # the search's [Q n_paths] rows into the batch's [Q P] rows
            t_nodes.view(Q, P, R, 3)[:, :n_paths].copy_(search.nodes.view(Q, n_paths, R, 3))
            t_ncnt.view(Q, P)[:, :n_paths].copy_(search.node_count.view(Q, n_paths))
            for k in ("traj_count", "topology_class", "node_count", "nodes", "prev_traj", "status"):
                rec[k][tick].copy_(getattr(search, k))
        A.guidance_plan(Q, gopt, search.traj_count.data_ptr(), search.topology_class.data_ptr(), world.planner_ids.data_ptr(), world.selection.data_ptr(),
                        t_mode.data_ptr(), t_src.data_ptr(), t_init.data_ptr(), t_dummy.data_ptr(), t_dis.data_ptr(), t_gid.data_ptr(), t_w.data_ptr())
        A.warmstart(world.state_batch.data_ptr(), t_mode.data_ptr(), t_src.data_ptr(), deceleration=decel)
        A.sample_guidance(B, R, t_nodes.data_ptr(), t_ncnt.data_ptr(), t_gpos.data_ptr(), t_gvel.data_ptr(), t_status.data_ptr())
        A.init_with_guidance(t_gpos.data_ptr(), t_gvel.data_ptr(), t_init.data_ptr())
        A.set_obstacle_parameters(o_pos.data_ptr(), o_shape.data_ptr(), o_rad.data_ptr(), o_gauss.data_ptr(), t_sc.data_ptr(), world.state4.data_ptr(), r)
        A.linearize_topology_ex(o_pos.data_ptr(), M, t_sc.data_ptr(), t_sx.data_ptr(), r, d_is_original=t_dummy.data_ptr())
        A.solve(sync=False)
        A.guidance_decide(Q, gopt, d_pobj, d_code, t_dis.data_ptr(), t_gid.data_ptr(), t_w.data_ptr(), world.state_nx.data_ptr(), t_best.data_ptr(),
                          t_exit.data_ptr(), t_cmd.data_ptr(), world.planner_ids.data_ptr(), world.selection.data_ptr(), deceleration=decel, control_dt=cdt)
        A.gather_best(t_each.data_ptr(), B, 1, rec["xtraj"][tick].data_ptr(), rec["utraj"][tick].data_ptr())
        A.pack_records(rec["records"][tick].data_ptr())
        with torch.cuda.stream(hs):
            for k, t in (("best", t_best), ("cmd", t_cmd), ("mode", t_mode), ("o_pos", o_pos)):
                rec[k][tick].copy_(t)
    A.synchronize()                                                                                  # the one synchronisation
    got = {k: v.cpu().numpy() for k, v in rec.items()}
    records = got["records"].view(distributed.RECORD_DTYPE).reshape(ticks, B)
    # ---- handle B: the same ticks, driven from the host
    Bh.set_batch(xinit, x0, params)
    h = dict(plant=plant0.copy(), raw_pos=raw_pos0.copy(), raw_vel=raw_vel0.copy(), episode=np.zeros((Q, 4), np.int32), episode_f=np.zeros((Q, 2)),
             log=np.zeros((Q, 2, 4)), state_nx=np.zeros((Q, nx)), state_batch=np.zeros((B, nx)), ids=np.full((Q, P), -1, np.int32),
             sel=np.tile(np.array([-1, 0, -1], np.int32), (Q, 1)), segment=np.full(Q, -1, np.int32))
    h["state_nx"][:, 0:4] = start; h["state_batch"][:, 0:4] = np.repeat(start, P, 0)
    arrays = gc.fresh_arrays(Q, N, sopt)
    arrays["nodes"][:] = 0.0                                                                         # GuidanceSearchState starts from zeros
    cmd = cmd0.copy()
    step_kw = {k: v for k, v in eopt.items() if k != "max_episodes"}
    counts_seen, through_connector = [], False
    for tick in range(ticks):
        state4, reset = np.zeros((Q, 4)), np.zeros(Q, np.uint8)
        for q in range(Q):
            reset[q], state4[q] = md.episode_step(cmd[q], h["plant"][q], plant0[q], count[q], h["raw_pos"][q], h["raw_vel"][q], raw_radius[q], raw_pos0[q],
                                                  raw_vel0[q], h["episode"][q], h["episode_f"][q], h["log"][q], state_nx=h["state_nx"][q],
                                                  state_batch=h["state_batch"][q * P:(q + 1) * P], planner_ids=h["ids"][q], selection=h["sel"][q],
                                                  segment=h["segment"][q:q + 1], **step_kw)
        for k in ("plant", "raw_pos", "raw_vel", "episode", "episode_f", "log"):
            assert _same(got[k][tick], h[k]), (tick, k)
        assert np.array_equal(got["was_reset"][tick], reset), tick
        obs = [md.prepare_obstacles(state4[q], h["raw_pos"][q], raw_radius[q], M, N, dt, raw_vel=h["raw_vel"][q]) for q in range(Q)]
        opos = np.stack([o["pos"] for o in obs])
        assert _same(got["o_pos"][tick], opos), tick
        goals = base_goals.copy(); goals[:, :, 0:2] += state4[:, None, 0:2]
        gc.mirror_tick(arrays, dict(state4=state4, goals=goals, obstacle_pos=opos, obstacle_radius=np.stack([o["radius"] for o in obs]),
                                    selected=np.stack([o["selected"] for o in obs]), was_reset=reset), N, dt, sopt)
        for k in ("traj_count", "topology_class", "node_count", "nodes", "prev_traj", "status"):
            assert _same(got[k][tick], arrays[k]), (tick, k)
        counts_seen.append(arrays["traj_count"].tolist())
        through_connector = through_connector or bool((arrays["node_count"] >= 3).any())
        plan = md.guidance_plan(arrays["traj_count"], arrays["topology_class"], h["ids"], h["sel"], n_paths, **kw)
        assert np.array_equal(got["mode"][tick], plan["mode"])
        nodes, node_count = np.full((B, R, 3), -9e9), np.zeros(B, np.int32)
        nodes.reshape(Q, P, R, 3)[:, :n_paths] = arrays["nodes"].reshape(Q, n_paths, R, 3)
        node_count.reshape(Q, P)[:, :n_paths] = arrays["node_count"].reshape(Q, n_paths)
        samples = [md.sample_guidance(nodes[b, :node_count[b]], N, dt, n_nodes_max=R) for b in range(B)]
        gpos, gvel = np.stack([sm[0] for sm in samples]), np.stack([sm[1] for sm in samples])
        u = dict(state=_up(h["state_batch"]), mode=_up(plan["mode"]), src=_up(plan["src"]), init=_up(plan["init_enabled"]), dummy=_up(plan["rows_dummy"]),
                 gpos=_up(gpos), gvel=_up(gvel), sx=_up(state4[:, 0].copy()), state4=_up(state4), opos=_up(opos), oshape=_up(np.stack([o["shape"] for o in obs])),
                 orad=_up(np.stack([o["radius"] for o in obs])), ogauss=_up(np.stack([o["gaussian"] for o in obs]).astype(np.uint8)))
        torch.cuda.synchronize()
        Bh.warmstart(u["state"].data_ptr(), u["mode"].data_ptr(), u["src"].data_ptr(), deceleration=decel)
        Bh.init_with_guidance(u["gpos"].data_ptr(), u["gvel"].data_ptr(), u["init"].data_ptr())
        Bh.set_obstacle_parameters(u["opos"].data_ptr(), u["oshape"].data_ptr(), u["orad"].data_ptr(), u["ogauss"].data_ptr(), t_sc.data_ptr(), u["state4"].data_ptr(), r)
        Bh.linearize_topology_ex(u["opos"].data_ptr(), M, t_sc.data_ptr(), u["sx"].data_ptr(), r, d_is_original=u["dummy"].data_ptr())
        Bh.solve()
        ref = Bh.get()
        dec = md.guidance_decide(ref["pobj"], ref["exit_code"], plan["disabled"], plan["guidance_id"], plan["weight"], h["state_nx"], ref["xtraj"], ref["utraj"],
                                 h["ids"], h["sel"], n_paths, True, deceleration=decel, control_dt=cdt)
        h["ids"], h["sel"], cmd = dec["planner_ids"], dec["selection"], dec["cmd"]
        print(f"[closed loop + search] tick {tick}: reset {reset.tolist()}, found {arrays['traj_count'].tolist()}, classes {arrays['topology_class'].tolist()}, "
              f"exit codes {ref['exit_code'].tolist()}, best {dec['best'].tolist()}, cmd {cmd.tolist()}")
        assert _same(got["xtraj"][tick].reshape(B, N + 1, nx), ref["xtraj"]) and _same(got["utraj"][tick].reshape(B, N, 2), ref["utraj"]), tick
        assert _same(records["objective"][tick], ref["pobj"]) and np.array_equal(records["exit_code"][tick], ref["exit_code"]), tick
        assert np.array_equal(got["best"][tick], dec["best"]) and _same(got["cmd"][tick], dec["cmd"]), tick
    # the loop did plan through the search's topologies: a scene with two classes on every tick, each of them through a connector
    assert all(max(c) >= 2 for c in counts_seen) and through_connector
    A.close(); Bh.close()
