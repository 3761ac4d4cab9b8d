"""GPU: the episode step on device (tmpc_episode_step; include/tmpc_hip_episode.h; csrc/tmpc_aux_kernels.hpp) against the host
mirror (mpc_planner_amd/modules.py episode_step, pinned on hand values and on the closed-form arc in tests/test_episode_mirror.py).  Equality
is bitwise, floats included: kernel and mirror share the operation order and use neither fused multiply-adds nor transcendental functions.
Then the whole closed loop -- step, obstacle preparation, guidance hand-off, warm start, rows, solve, decision -- enqueued back to back on
one stream, against the same ticks driven from the host."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import episode_cases as ec  # noqa: E402

pytestmark = pytest.mark.gpu

N, S, M = 20, 5, 8
SENTINEL = ec.SENTINEL


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda"))


def _full(shape, value, dtype):
    import torch
    return torch.full(shape, value, dtype=dtype, device=torch.device("cuda"))


def _bits(a):
    """The bit patterns of an array; every NaN becomes one pattern: IEEE 754 leaves a NaN's sign and payload to the implementation (x86
    keeps the operand's, gfx950's subtraction -- an addition with a negated source -- flips its sign), so "the same NaN" means NaN in the
    same place.  Every other value, signed zeros and infinities included, keeps its bits."""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float64:
        return a
    bits = a.view(np.uint64).copy()
    bits[np.isnan(a)] = np.uint64(0x7ff8000000000000)
    return bits


def _same(a, b):
    """Bitwise equality; a NaN equals a NaN in the same place (_bits)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _solver(B_max=12):
    from mpc_planner_amd import solver
    return solver.BatchedSolver(solver.default_dims(N=N, S=S, n_lin=M, M=M), B_max=B_max)


def _generated_solver(name="tmpc_cfg2", B_max=12):
    from mpc_planner_amd import solver
    path = os.path.join(ROOT, "build", "generated", f"libtmpc_hip_{name}.so")
    if not os.path.exists(path):
        import __graft_entry__ as g
        g.build_generated_demo()
    return solver.BatchedSolver(solver.default_dims(N=N, lib_path=path), B_max, lib_path=path)


class _DeviceWorld:
    """The case's arrays on the device, every per-scene array one scene longer than the launch covers: the guard scene has to keep its fill."""

    def __init__(self, case, max_episodes):
        guard = lambda a, fill: np.concatenate([a, np.full((a.shape[0] // ec.Q,) + a.shape[1:], fill, a.dtype)])
        start = ec.initial_arrays(case, max_episodes)
        self.fill = {k: (9 if v.dtype == np.uint8 else -7 if v.dtype == np.int32 else SENTINEL) for k, v in start.items()}
        self.t = {k: _up(guard(v, self.fill[k])) for k, v in start.items()}
        self.const = {k: _up(case[k]) for k in ("plant0", "count", "raw_pos0", "raw_vel0", "raw_radius", "goal")}
        self.box = None if case["box"] is None else _up(case["box"])

    def step(self, entry, opt, t_cmd, n_slots=ec.N_SLOTS):
        t, c = self.t, self.const
        entry.step(ec.Q, n_slots, ec.P, opt, t_cmd.data_ptr(), t["plant"].data_ptr(), c["plant0"].data_ptr(), c["count"].data_ptr(), t["raw_pos"].data_ptr(),
                   t["raw_vel"].data_ptr(), c["raw_radius"].data_ptr(), c["raw_pos0"].data_ptr(), c["raw_vel0"].data_ptr(), t["episode"].data_ptr(),
                   t["episode_f"].data_ptr(), t["log"].data_ptr(), t["was_reset"].data_ptr(), t["state4"].data_ptr(),
                   d_box=None if self.box is None else self.box.data_ptr(), d_goal=c["goal"].data_ptr(), d_state_nx=t["state_nx"].data_ptr(),
                   d_state_batch=t["state_batch"].data_ptr(), d_planner_ids=t["planner_ids"].data_ptr(), d_selection=t["selection"].data_ptr(),
                   d_segment=t["segment"].data_ptr())

    def check(self, want, tick):
        for k, t in self.t.items():
            got = t.cpu().numpy()
            n = len(want[k])
            assert _same(got[:n], want[k]), (tick, k)
            assert (got[n:] == self.fill[k]).all(), (tick, k, "the guard scene was written")


def _run_against_the_mirror(s, config, ticks):
    from mpc_planner_amd import episode
    substeps, boxed, acc = config
    case = ec.make_case(7, boxed, nx=int(s.dims.nx), ticks=ticks)
    opt = ec.options(substeps, acc)
    history, seen = ec.run_mirror(case, opt)
    world, entry = _DeviceWorld(case, opt["max_episodes"]), episode.Episode(s)
    d_opt = episode.episode_options(**opt)
    t_cmds = _up(case["commands"])
    constants = {k: v.cpu().numpy().copy() for k, v in world.const.items()}
    for tick in range(ticks):
        world.step(entry, d_opt, t_cmds[tick])
        s.synchronize()
        world.check(history[tick], tick)
    for k, v in world.const.items():
        assert _same(v.cpu().numpy(), constants[k])                                                  # inputs are inputs
    assert _same(t_cmds.cpu().numpy(), case["commands"])
    return history, seen, case


@pytest.mark.parametrize("config", ec.CONFIGS)
def test_equals_the_mirror_bitwise_over_40_ticks(config):
    """6 scenes, 70 slots (past one wave: the stride loop runs), counts (0, 1, 3, 64, 70, 70), P = 3, max_episodes = 2, timeout 9 ticks;
    substeps 1 and 4, box given and NULL, acceleration limit on and off.  Seeded scripted commands with |w| above the limit; scene 2 receives
    NaN commands from tick 3 on, ends by timeout with completed = 0 and comes back bitwise at its start state.  Every in/out and output
    array is compared after every tick by bit pattern, NaNs by position; the outputs start sentinel-filled and carry a guard scene."""
    s = _solver()
    history, seen, case = _run_against_the_mirror(s, config, ec.TICKS)
    assert all(seen[k] for k in ec.expected_events(config[1])), seen
    q = ec.NAN_SCENE
    rows = history[-1]["log"][q]
    assert (rows[:, 1] == 0.0).all() and (rows[:, 0] == float(ec.TIMEOUT) * ec.CONTROL_DT).all()
    back = [h for h in history[ec.NAN_FROM:] if h["was_reset"][q]]
    assert len(back) >= 3 and all(np.array_equal(h["plant"][q], case["plant0"][q]) for h in back)
    print(f"[episode {config}] episodes finished {history[-1]['episode'][:, 2].tolist()}, events {sorted(k for k, v in seen.items() if v)}")
    s.close()


def test_every_refusal():
    """Each condition of the header's list returns TMPC_ERR_INVALID with a message naming tmpc_episode_step and launches nothing: the
    sentinel-filled outputs and the carried arrays stay as they were.  A NULL handle returns -1."""
    from mpc_planner_amd import episode, solver
    s = _solver()
    case = ec.make_case(7, True, nx=int(s.dims.nx), ticks=1)
    world, entry = _DeviceWorld(case, ec.MAX_EPISODES), episode.Episode(s)
    t_cmd = _up(case["commands"][0])
    t, c = world.t, world.const
    base = ec.options(4, 3.0)
    args = dict(n_scenes=ec.Q, n_slots=ec.N_SLOTS, P=ec.P, options=episode.episode_options(**base), d_cmd=t_cmd.data_ptr(), d_plant=t["plant"].data_ptr(),
                d_plant0=c["plant0"].data_ptr(), d_count=c["count"].data_ptr(), d_raw_pos=t["raw_pos"].data_ptr(), d_raw_vel=t["raw_vel"].data_ptr(),
                d_raw_radius=c["raw_radius"].data_ptr(), d_raw_pos0=c["raw_pos0"].data_ptr(), d_raw_vel0=c["raw_vel0"].data_ptr(),
                d_episode=t["episode"].data_ptr(), d_episode_f=t["episode_f"].data_ptr(), d_log=t["log"].data_ptr(), d_was_reset=t["was_reset"].data_ptr(),
                d_state4=t["state4"].data_ptr(), d_box=world.box.data_ptr(), d_goal=c["goal"].data_ptr(), d_state_nx=t["state_nx"].data_ptr(),
                d_state_batch=t["state_batch"].data_ptr(), d_planner_ids=t["planner_ids"].data_ptr(), d_selection=t["selection"].data_ptr(),
                d_segment=t["segment"].data_ptr())
    before = {k: v.cpu().numpy().copy() for k, v in t.items()}
    opt = lambda **kw: episode.episode_options(**dict(base, **kw))
    good = episode.episode_options(**base)
    short = episode.episode_options(**base); short.size = C.sizeof(short) - 8
    long_dirty = (C.c_char * (C.sizeof(good) + 8)).from_buffer_copy(bytes(good) + b"\0\0\0\1\0\0\0\0")
    dirty = C.cast(long_dirty, C.POINTER(episode.TmpcEpisodeOptions)).contents; dirty.size = C.sizeof(good) + 8
    required = [a for a in episode.ARRAYS if a not in episode.OPTIONAL]
    assert len(required) == 14
    refusals = [(dict(options=None), "NULL options"), (dict(n_scenes=0), "n_scenes"), (dict(n_scenes=-1), "n_scenes"), (dict(n_slots=-1), "n_slots"),
                (dict(n_slots=1025), "n_slots"), (dict(P=0), "P must"), (dict(options=opt(substeps=0)), "substeps"), (dict(options=opt(substeps=17)), "substeps"),
                (dict(options=opt(control_dt=0.0)), "control_dt"), (dict(options=opt(control_dt=-0.05)), "control_dt"),
                (dict(options=opt(control_dt=float("inf"))), "control_dt"), (dict(options=opt(control_dt=float("nan"))), "control_dt"),
                (dict(options=opt(max_angular_velocity=0.0)), "max_angular_velocity"), (dict(options=opt(max_angular_velocity=-1.0)), "max_angular_velocity"),
                (dict(options=opt(max_angular_velocity=10.1)), "at most 0.125"), (dict(options=opt(substeps=1, max_angular_velocity=2.6)), "at most 0.125"),
                (dict(options=opt(max_episodes=0)), "max_episodes"), (dict(options=opt(max_episodes=4097)), "max_episodes"),
                (dict(options=opt(timeout_ticks=-1)), "timeout_ticks"), (dict(options=opt(robot_radius=-0.1)), "robot_radius"),
                (dict(options=short), "smaller"), (dict(options=dirty), "non-zero field")] + [(dict([(k, None)]), "NULL") for k in required]
    for kw, msg in refusals:
        with pytest.raises(solver.TmpcError, match=msg) as e:
            entry.step(**dict(args, **kw))
        assert "tmpc_episode_step" in str(e.value) and "(-1)" in str(e.value), (kw, str(e.value))
    s.synchronize()
    for k, v in t.items():
        assert _same(v.cpu().numpy(), before[k]), k                                                  # nothing was launched
    assert s.lib.tmpc_episode_step(None, ec.Q, ec.N_SLOTS, ec.P, C.byref(good), *([None] * 21)) == -1     # no handle: TMPC_ERR_INVALID
    # accepted: the same call, without a batch; every optional pointer NULL; a newer, longer options struct with a zero tail; the limits themselves
    entry.step(**args)
    entry.step(**dict(args, **{k: None for k in episode.OPTIONAL}))
    long_clean = (C.c_char * (C.sizeof(good) + 8)).from_buffer_copy(bytes(good) + b"\0" * 8)
    clean = C.cast(long_clean, C.POINTER(episode.TmpcEpisodeOptions)).contents; clean.size = C.sizeof(good) + 8
    entry.step(**dict(args, options=clean))
    entry.step(**dict(args, options=opt(substeps=16, max_angular_velocity=40.0, max_episodes=2, timeout_ticks=0)))      # 40 x 0.05 / 16 = 0.125
    s.synchronize()
    assert (t["was_reset"].cpu().numpy()[:ec.Q] != 9).all() and (t["was_reset"].cpu().numpy()[ec.Q:] == 9).all()
    s.close()


def test_a_generated_library_equals_the_mirror():
    """The same call on the generated tmpc_cfg2 library (its parameter layout is the module stack's: the step reads no column), 10 ticks of
    the configuration (4 substeps, box, no acceleration limit)."""
    s = _generated_solver()
    _run_against_the_mirror(s, (4, True, 0.0), 10)
    s.close()


def _loop_scene_velocities(seed):
    """The obstacle velocities scenes.make_scene draws (its first random numbers; it does not return them)."""
    from mpc_planner_amd import scenes
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    rng.uniform(0.5, 2.0)
    scenes.reference_path_segments(rng, S)
    speed = rng.uniform(0.6, 1.6, M)
    heading = np.where(rng.uniform(size=M) < 0.5, 1.0, -1.0) * np.pi / 2 + rng.uniform(-0.5, 0.5, M)
    return np.stack([speed * np.cos(heading), speed * np.sin(heading)], 1)


def test_the_loop_closes_on_the_device(seeds=None):
    """2 scenes x (2 + 1) planners, N = 20, M = 8, 12 ticks of 0.05 s.  Handle A enqueues all twelve ticks back to back on its stream --
    episode_step -> prepare_obstacles -> guidance_plan -> warmstart -> sample_guidance -> init_with_guidance -> set_obstacle_parameters ->
    linearize_topology_ex (on the prepared positions) -> solve -> guidance_decide --, every tick's results copied into per-tick tensors on the
    stream, one synchronisation at the end.  Handle B runs the same ticks driven from the host: the mirror step, modules.prepare_obstacles
    and the guidance mirrors, uploaded around the same calls.  Both see bit-identical inputs, so xtraj, utraj, pobj, the exit codes, best,
    cmd, the plant, the obstacle arrays, the counters and the log are equal bit for bit at every tick.  Scene 0 has goal_x 0.3 m ahead of its
    start, scene 1 starts 1 m further back and runs into the timeout of 5 ticks: both kinds of reset occur, the tick of a reset plans with
    mode 3 (braking) from planner_ids = -1, the obstacles' predictions differ from tick to tick and every tick has a successful solve."""
    import torch
    from mpc_planner_amd import distributed, episode, modules as md, scenes, solver
    from test_gpu_guidance_handoff import E2E_CLASSES, E2E_COUNTS, E2E_NODE_STAGES, E2E_SEEDS
    seeds = E2E_SEEDS if seeds is None else seeds
    Q, n_paths, P, ticks, R = 2, 2, 3, 12, 6
    B = Q * P
    scs = [scenes.make_scene(seed, N=N, M=M, B=n_paths, tmpc_pp=True) for seed in seeds]
    xinit = np.concatenate([sc["xinit"] for sc in scs]); params = np.concatenate([sc["params"] for sc in scs])
    nx = xinit.shape[1]
    x0 = np.full((B, N + 1, 7), SENTINEL)                                                            # every warm start is the device's
    scene_of = np.repeat(np.arange(Q, dtype=np.int32), P)
    r, decel, cdt, w_cons = scenes.ROBOT_RADIUS, 3.0, 0.05, 0.8
    kw = dict(use_tmpcpp=True, warmstart_with_mpc_solution=True, shift_previous_solution_forward=True, selection_weight_consistency=w_cons)
    gopt = solver.guidance_options(n_paths, **kw)
    eopt = dict(substeps=2, timeout_ticks=5, max_episodes=2, control_dt=cdt, max_acceleration=3.0, max_angular_velocity=2.0, robot_radius=r, goal_x=0.3)
    d_eopt = episode.episode_options(**eopt)
    # the world: the scenes' own obstacles as raw states, the robots at the scenes' start (scene 1 one metre back)
    start = np.array([[0.0, 0.0, 0.0, 2.0], [-1.0, 0.0, 0.0, 1.0]])
    plant0 = np.concatenate([start, np.cos(start[:, 2:3]), np.sin(start[:, 2:3])], 1)
    raw_pos0 = np.ascontiguousarray(np.stack([sc["obstacles"]["pos"][:, 0] for sc in scs]))
    raw_vel0 = np.stack([_loop_scene_velocities(seed) for seed in seeds])
    raw_radius = np.stack([sc["obstacles"]["radius"] for sc in scs])
    count = np.full(Q, M, np.int32)
    cmd0 = np.stack([start[:, 3], np.zeros(Q)], 1)
    base_nodes, node_count = np.full((B, R, 3), -9e9), np.zeros(B, np.int32)
    for q, sc in enumerate(scs):
        for p in range(n_paths):
            st = np.array(E2E_NODE_STAGES[p])
            base_nodes[q * P + p, :len(st)] = np.concatenate([st[:, None] * 0.2, sc["guidance_pos"][p][st] - xinit[q * P, None, 0:2]], 1)
            node_count[q * P + p] = len(st)
    counts_all = np.array([E2E_COUNTS[t % 6] for t in range(ticks)], np.int32); classes_all = np.array([E2E_CLASSES[t % 6] for t in range(ticks)], np.int32)
    dev = torch.device("cuda")
    A, Bh = _solver(B), _solver(B)
    i32, u8, f64 = torch.int32, torch.uint8, torch.float64
    # ---- handle A: everything on the device, nothing read back before the end
    t_xinit, t_x0, t_params = _up(xinit), _up(x0), _up(params)
    A.set_batch_device(B, t_xinit.data_ptr(), t_x0.data_ptr(), t_params.data_ptr())
    world = episode.EpisodeWorld(A, P, plant0, raw_pos0, raw_vel0, raw_radius, d_eopt, count=count)
    assert world.nx == nx and _same(world.state_batch.cpu().numpy()[:, 0:4], np.repeat(start, P, 0))
    t_cmd = _up(cmd0)
    t_base, t_nodes, t_ncnt, t_sc, t_sx = _up(base_nodes), _up(base_nodes), _up(node_count), _up(scene_of), _full((Q,), SENTINEL, f64)
    t_cnts, t_clss = _up(counts_all), _up(classes_all)
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
               ids_before=_full((ticks, Q, P), -7, i32), mode=_full((ticks, B), -7, i32), o_pos=_full((ticks, Q, M, N, 2), SENTINEL, f64))
    d_pobj, d_code = A.result_device_ptrs()
    hs = torch.cuda.ExternalStream(A.stream_ptr(), device=dev)
    torch.cuda.synchronize()
    for tick in range(ticks):
        world.step(t_cmd.data_ptr())
        with torch.cuda.stream(hs):
            for k, t in (("plant", world.plant), ("raw_pos", world.raw_pos), ("raw_vel", world.raw_vel), ("episode", world.episode), ("episode_f", world.episode_f),
                         ("log", world.log_rows), ("was_reset", world.was_reset), ("ids_before", world.planner_ids)):
                rec[k][tick].copy_(t)
            t_sx.copy_(world.state4[:, 0])
            t_nodes.copy_(t_base); t_nodes[:, :, 1:3] += world.state_batch[:, None, 0:2]
        A.prepare_obstacles(Q, M, M, world.count.data_ptr(), world.state4.data_ptr(), world.raw_pos.data_ptr(), world.raw_radius.data_ptr(), o_pos.data_ptr(),
                            o_shape.data_ptr(), o_rad.data_ptr(), o_gauss.data_ptr(), o_sel.data_ptr(), d_raw_vel=world.raw_vel.data_ptr())
        A.guidance_plan(Q, gopt, t_cnts[tick].data_ptr(), t_clss[tick].data_ptr(), world.planner_ids.data_ptr(), world.selection.data_ptr(), t_mode.data_ptr(),
                        t_src.data_ptr(), t_init.data_ptr(), t_dummy.data_ptr(), t_dis.data_ptr(), t_gid.data_ptr(), t_w.data_ptr())
        A.warmstart(world.state_batch.data_ptr(), t_mode.data_ptr(), t_src.data_ptr(), deceleration=decel)
        A.sample_guidance(B, R, t_nodes.data_ptr(), t_ncnt.data_ptr(), t_gpos.data_ptr(), t_gvel.data_ptr(), t_status.data_ptr())
        A.init_with_guidance(t_gpos.data_ptr(), t_gvel.data_ptr(), t_init.data_ptr())
        A.set_obstacle_parameters(o_pos.data_ptr(), o_shape.data_ptr(), o_rad.data_ptr(), o_gauss.data_ptr(), t_sc.data_ptr(), world.state4.data_ptr(), r)
        A.linearize_topology_ex(o_pos.data_ptr(), M, t_sc.data_ptr(), t_sx.data_ptr(), r, d_is_original=t_dummy.data_ptr())
        A.solve(sync=False)
        A.guidance_decide(Q, gopt, d_pobj, d_code, t_dis.data_ptr(), t_gid.data_ptr(), t_w.data_ptr(), world.state_nx.data_ptr(), t_best.data_ptr(),
                          t_exit.data_ptr(), t_cmd.data_ptr(), world.planner_ids.data_ptr(), world.selection.data_ptr(), deceleration=decel, control_dt=cdt)
        A.gather_best(t_each.data_ptr(), B, 1, rec["xtraj"][tick].data_ptr(), rec["utraj"][tick].data_ptr())       # every trajectory: B sets of one
        A.pack_records(rec["records"][tick].data_ptr())
        with torch.cuda.stream(hs):
            for k, t in (("best", t_best), ("cmd", t_cmd), ("mode", t_mode), ("o_pos", o_pos)):
                rec[k][tick].copy_(t)
    A.synchronize()                                                                                  # the one synchronisation
    got = {k: v.cpu().numpy() for k, v in rec.items()}
    records = got["records"].view(distributed.RECORD_DTYPE).reshape(ticks, B)
    final = world.log()
    # ---- handle B: the same ticks, driven from the host
    Bh.set_batch(xinit, x0, params)
    h = dict(plant=plant0.copy(), raw_pos=raw_pos0.copy(), raw_vel=raw_vel0.copy(), episode=np.zeros((Q, 4), np.int32), episode_f=np.zeros((Q, 2)),
             log=np.zeros((Q, 2, 4)), state_nx=np.zeros((Q, nx)), state_batch=np.zeros((B, nx)), ids=np.full((Q, P), -1, np.int32),
             sel=np.tile(np.array([-1, 0, -1], np.int32), (Q, 1)), segment=np.full(Q, -1, np.int32))
    h["state_nx"][:, 0:4] = start; h["state_batch"][:, 0:4] = np.repeat(start, P, 0)
    cmd = cmd0.copy()
    step_kw = {k: v for k, v in eopt.items() if k != "max_episodes"}
    resets = np.zeros((ticks, Q), bool)
    for tick in range(ticks):
        state4 = np.zeros((Q, 4))
        for q in range(Q):
            resets[tick, q], state4[q] = md.episode_step(cmd[q], h["plant"][q], plant0[q], count[q], h["raw_pos"][q], h["raw_vel"][q], raw_radius[q], raw_pos0[q],
                                                         raw_vel0[q], h["episode"][q], h["episode_f"][q], h["log"][q], state_nx=h["state_nx"][q],
                                                         state_batch=h["state_batch"][q * P:(q + 1) * P], planner_ids=h["ids"][q], selection=h["sel"][q],
                                                         segment=h["segment"][q:q + 1], **step_kw)
        for k in ("plant", "raw_pos", "raw_vel", "episode", "episode_f", "log"):
            assert _same(got[k][tick], h[k]), (tick, k)
        assert np.array_equal(got["was_reset"][tick], resets[tick].astype(np.uint8)) and np.array_equal(got["ids_before"][tick], h["ids"])
        obs = [md.prepare_obstacles(state4[q], h["raw_pos"][q], raw_radius[q], M, N, Bh.dims.dt, raw_vel=h["raw_vel"][q]) for q in range(Q)]
        opos = np.stack([o["pos"] for o in obs])
        assert _same(got["o_pos"][tick], opos), tick
        plan = md.guidance_plan(counts_all[tick], classes_all[tick], h["ids"], h["sel"], n_paths, **kw)
        assert np.array_equal(got["mode"][tick], plan["mode"])
        for q in range(Q):
            if resets[tick, q]:
                assert (plan["mode"][q * P:(q + 1) * P] == 3).all() and (h["ids"][q] == -1).all()     # the freshly constructed planner: braking
        nodes = base_nodes.copy(); nodes[:, :, 1:3] += h["state_batch"][:, None, 0:2]
        samples = [md.sample_guidance(nodes[b, :node_count[b]], N, Bh.dims.dt, n_nodes_max=R) for b in range(B)]
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
        print(f"[closed loop] tick {tick}: reset {resets[tick].tolist()}, x {state4[:, 0].tolist()}, exit codes {ref['exit_code'].tolist()}, best {dec['best'].tolist()}, "
              f"cmd {cmd.tolist()}")
        assert _same(got["xtraj"][tick].reshape(B, N + 1, nx), ref["xtraj"]) and _same(got["utraj"][tick].reshape(B, N, 2), ref["utraj"]), tick
        assert _same(records["objective"][tick], ref["pobj"]) and np.array_equal(records["exit_code"][tick], ref["exit_code"]), tick
        assert np.array_equal(got["best"][tick], dec["best"]) and _same(got["cmd"][tick], dec["cmd"]), tick
        assert (ref["exit_code"] == 1).any(), tick                                                   # at least one solve per tick succeeds
        if tick > 0:
            assert not np.array_equal(got["o_pos"][tick], got["o_pos"][tick - 1])                    # the obstacles moved: other predictions
    # both kinds of reset, and the log EpisodeWorld returns
    assert resets[:, 0].any() and resets[:, 1].any()
    assert h["log"][0, 0, 1] == 1.0 and h["log"][0, 0, 0] < 5 * cdt                                  # scene 0: completed, before the timeout
    assert h["log"][1, 0].tolist()[:2] == [5 * cdt, 0.0]                                             # scene 1: the timeout, not completed
    for q in range(Q):
        assert final[q]["finished"] == h["episode"][q, 2] and _same(final[q]["rows"], h["log"][q][:min(int(h["episode"][q, 2]), 2)])
        assert final[q]["ticks"] == h["episode"][q, 0] and final[q]["max_intrusion"] == h["episode_f"][q, 0]
    A.close(); Bh.close()
