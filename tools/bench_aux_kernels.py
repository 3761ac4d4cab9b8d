"""Launch the auxiliary device kernels (f-1 topology linearisation, f-2 warm start / guidance init, f-3 scenario reduction,
records + selection, Contouring's road halfspaces, obstacle preparation) at the bench batch size; run under `rocprofv3 --kernel-trace --stats`
to get their durations.  The road kernel works per (scene, stage): it is launched for 512 scenes (bench.py's default), the 64 generated ones repeated.
Obstacle preparation (tmpc_prepare_obstacles, tmpc_set_obstacle_parameters) runs at bench.py's default launch, 512 scenes x 64 trajectories, with
`--slots R` raw-obstacle slots per scene, all of them filled (default 64; `--slots 1024`, the cap, runs the obstacle kernels alone so that a
profile of that run holds the R = 1024 durations only).  Besides the profile, one JSON line per obstacle kernel: the mean of 50 back-to-back
launches between two HIP events on the handle's stream (launch gaps included: an upper bound of the kernel time).
`--path local|global [--segments n]`: the reference-path kernels alone (tmpc_track_path, tmpc_set_path_parameters) at the same launch, 512 paths of
n segments (default 64; 1024 is the cap) of 2 m, searched 2 segments either side of the previous one (local) or over every segment (global: the
previous segment is put back to -1 before every launch, a 512-int copy that the event times include and the profile lists separately).
`--fit [--points n]`: the path-fit kernel alone (tmpc_fit_path), 512 scenes of n waypoints (default 65; 1025 is the cap) with bounds and a velocity
profile -- seven curves per scene --, chord knots; needs no batch.  One JSON line: the mean of 50 launches between two HIP events.
`--decomp [--cells n]`: the free-space kernels alone (tmpc_costmap_points, tmpc_decomp_halfspaces, tmpc_set_halfspace_rows) at cfg 3's shape (N = 30,
slack model, 12 decomp rows): 512 scenes x 64 trajectories, n x n maps (default 100) from scenes.with_costmap, 16 generated ones repeated, the
polyline along each scene's own warm start.  One JSON line per kernel with the event time, the points per scene and the rows per stage.
`--velocity [--segments n]`: the velocity-profile kernel and the column scatter alone (tmpc_path_velocity_window, tmpc_scatter_parameters) at
512 scenes x 64 trajectories, S = 5, N = 20: 512 paths of n segments (default 64) fitted on device with a velocity at every waypoint, closest_s
anywhere on the path, v_ref requested; the scatter writes the window's S x 4 = 20 values into 20 columns of every stage of every entry.  One
JSON line per kernel: the mean of 50 launches between two HIP events.
`--guidance`: the three guidance hand-off kernels alone (tmpc_sample_guidance, tmpc_guidance_plan, tmpc_guidance_decide) at 512 scenes x (4 + 1)
planners = 2560 entries, 8 nodes per trajectory, N = 30 (cfg 2's rows): 16 generated scenes repeated, two to four trajectories found per scene,
the state carried from launch to launch.  tmpc_guidance_decide needs a solved batch, so the run holds ONE tmpc_solve before the timed launches
(its kernel is listed separately in a profile).  One JSON line per kernel: the mean of 50 launches between two HIP events."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
torch.cuda.init()
from mpc_planner_amd import scenes, solver
dev = torch.device("cuda")
slots = int(sys.argv[sys.argv.index("--slots") + 1]) if "--slots" in sys.argv else 64


def obstacle_kernels(R, n_scenes=512, traj=64, M=8, N=20):
    rng = np.random.default_rng(7)
    B = n_scenes * traj
    so = solver.BatchedSolver(solver.default_dims(), B_max=B)
    f64 = dict(dtype=torch.float64, device=dev)
    xinit = torch.zeros((B, 5), **f64); x0 = torch.zeros((B, N + 1, 7), **f64); params = torch.zeros((B, N, so.dims.npar), **f64)
    so.set_batch_device(B, xinit.data_ptr(), x0.data_ptr(), params.data_ptr())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cnt = up(np.full(n_scenes, R, np.int32)); state = up(np.tile([0.0, 0.0, 0.1, 1.2], (n_scenes, 1)))
    pos = up(np.stack([rng.uniform(1.0, 15.0, (n_scenes, R)), rng.uniform(-5.0, 5.0, (n_scenes, R))], 2)); rad = up(np.full((n_scenes, R), 0.4))
    vel = up(rng.uniform(-1.0, 1.0, (n_scenes, R, 2)))
    o_pos = torch.zeros((n_scenes, M, N, 2), **f64); o_shape = torch.zeros((n_scenes, M, N, 3), **f64); o_rad = torch.zeros((n_scenes, M), **f64)
    o_g = torch.zeros((n_scenes, M), dtype=torch.uint8, device=dev); o_sel = torch.zeros((n_scenes, M), dtype=torch.int32, device=dev)
    scene_of = up(np.repeat(np.arange(n_scenes, dtype=np.int32), traj))
    prepare = lambda: so.prepare_obstacles(n_scenes, R, M, cnt.data_ptr(), state.data_ptr(), pos.data_ptr(), rad.data_ptr(), o_pos.data_ptr(), o_shape.data_ptr(),
                                           o_rad.data_ptr(), o_g.data_ptr(), o_sel.data_ptr(), d_raw_vel=vel.data_ptr(), probabilistic=True, propagate_passes=2)
    write = lambda: so.set_obstacle_parameters(o_pos.data_ptr(), o_shape.data_ptr(), o_rad.data_ptr(), o_g.data_ptr(), scene_of.data_ptr(), state.data_ptr(), 0.325)
    hs = torch.cuda.ExternalStream(so.stream_ptr(), device=dev)
    for name, call in (("tmpc_prepare_obstacles_kernel", prepare), ("tmpc_set_obstacle_parameters_kernel", write)):
        for _ in range(10):
            call()
        so.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(hs):
            e0.record()
            for _ in range(50):
                call()
            e1.record()
        so.synchronize()
        print(json.dumps(dict(kernel=name, n_scenes=n_scenes, trajectories=B, slots=R, M=M, N=N, us_per_launch_events=e0.elapsed_time(e1) * 1e3 / 50)), flush=True)
    so.close()


def path_kernels(mode, n_seg, n_scenes=512, traj=64, N=20, S=5):
    rng = np.random.default_rng(11)
    B = n_scenes * traj
    so = solver.BatchedSolver(solver.default_dims(), B_max=B)
    f64 = dict(dtype=torch.float64, device=dev)
    xinit = torch.zeros((B, 5), **f64); x0 = torch.zeros((B, N + 1, 7), **f64); params = torch.zeros((B, N, so.dims.npar), **f64)
    so.set_batch_device(B, xinit.data_ptr(), x0.data_ptr(), params.data_ptr())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    base = np.stack([scenes.reference_path_segments(np.random.default_rng(s_), S=n_seg, seg_len=2.0) for s_ in range(16)])
    paths = up(np.tile(base, (n_scenes // 16, 1, 1))); cnt = up(np.full(n_scenes, n_seg, np.int32)); length = up(np.full(n_scenes, 2.0 * n_seg))
    bounds = up(np.tile(np.stack([base[:, :, :8], base[:, :, :8]], 1), (n_scenes // 16, 1, 1, 1)))
    x = rng.uniform(0.0, 2.0 * n_seg, n_scenes)
    state = up(np.stack([x, rng.uniform(-1.0, 1.0, n_scenes), np.zeros(n_scenes), np.full(n_scenes, 1.2)], 1))
    seg0 = up(np.full(n_scenes, -1, np.int32) if mode == "global" else np.clip((x // 2.0).astype(np.int32) - 1, 0, n_seg - 1))
    seg = seg0.clone(); cs = torch.zeros(n_scenes, **f64); win = torch.zeros((n_scenes, S, 9), **f64); bw = torch.zeros((n_scenes, 2, S, 8), **f64)
    reached = torch.zeros(n_scenes, dtype=torch.uint8, device=dev)
    scene_of = up(np.repeat(np.arange(n_scenes, dtype=np.int32), traj)); st = torch.zeros((B, 5), **f64)
    hs = torch.cuda.ExternalStream(so.stream_ptr(), device=dev)

    def track():
        with torch.cuda.stream(hs):
            seg.copy_(seg0)                                            # (tmpc_track_path leaves the segment it found: the next launch would be a local search)
        so.track_path(n_scenes, n_seg, paths.data_ptr(), cnt.data_ptr(), length.data_ptr(), state.data_ptr(), 4, seg.data_ptr(), cs.data_ptr(), win.data_ptr(),
                      d_bounds=bounds.data_ptr(), d_bound_window=bw.data_ptr(), d_reached=reached.data_ptr(), search_range=2)
    write = lambda: so.set_path_parameters(win.data_ptr(), scene_of.data_ptr(), n_scenes, d_closest_s=cs.data_ptr(), d_state=st.data_ptr())
    for name, call in (("tmpc_track_path_kernel", track), ("tmpc_set_path_parameters_kernel", write)):
        for _ in range(10):
            call()
        so.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(hs):
            e0.record()
        for _ in range(50):
            call()
        with torch.cuda.stream(hs):
            e1.record()
        so.synchronize()
        print(json.dumps(dict(kernel=name, n_scenes=n_scenes, trajectories=B, segments=n_seg, search=mode, S=S, N=N,
                              us_per_launch_events=e0.elapsed_time(e1) * 1e3 / 50)), flush=True)
    so.close()


def fit_kernel(n_pts, n_scenes=512):
    so = solver.BatchedSolver(solver.default_dims(), B_max=4)
    f64 = dict(dtype=torch.float64, device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    base = []
    for s_ in range(16):
        rng = np.random.default_rng(s_)
        heading = np.cumsum(rng.normal(size=n_pts) * 0.15); step = rng.uniform(0.2, 3.0, n_pts)
        base.append(np.cumsum(np.stack([np.cos(heading) * step, np.sin(heading) * step], 1), 0))
    xy = np.tile(np.stack(base), (n_scenes // 16, 1, 1))
    t_xy, t_left, t_right = up(xy), up(xy + [0.0, 2.0]), up(xy - [0.0, 2.0])
    t_v = up(np.random.default_rng(99).uniform(0.5, 3.0, (n_scenes, n_pts))); t_cnt = up(np.full(n_scenes, n_pts, np.int32))
    R = n_pts - 1
    path = torch.zeros((n_scenes, R, 9), **f64); pc = torch.zeros(n_scenes, dtype=torch.int32, device=dev); length = torch.zeros(n_scenes, **f64)
    bounds = torch.zeros((n_scenes, 2, R, 8), **f64); vel = torch.zeros((n_scenes, R, 4), **f64); rw = torch.zeros(n_scenes, **f64)
    status = torch.zeros(n_scenes, dtype=torch.uint8, device=dev)
    call = lambda: so.fit_path(n_scenes, n_pts, R, t_xy.data_ptr(), t_cnt.data_ptr(), path.data_ptr(), pc.data_ptr(), length.data_ptr(), d_left_xy=t_left.data_ptr(),
                               d_right_xy=t_right.data_ptr(), d_v=t_v.data_ptr(), d_bounds=bounds.data_ptr(), d_velocity=vel.data_ptr(), d_road_width=rw.data_ptr(),
                               d_status=status.data_ptr())
    hs = torch.cuda.ExternalStream(so.stream_ptr(), device=dev)
    for _ in range(10):
        call()
    so.synchronize()
    assert int(status.sum().item()) == 0 and int(pc.min().item()) == R
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(hs):
        e0.record()
    for _ in range(50):
        call()
    with torch.cuda.stream(hs):
        e1.record()
    so.synchronize()
    print(json.dumps(dict(kernel="tmpc_fit_path_kernel", n_scenes=n_scenes, points=n_pts, curves=7, knots="chord",
                          us_per_launch_events=e0.elapsed_time(e1) * 1e3 / 50)), flush=True)
    so.close()


def decomp_kernels(cells, n_scenes=512, traj=64, N=30, S=5, n_rows=12, n_pts_max=16384):
    dims = solver.default_dims(N=N, S=S, n_lin=8, M=8, n_slk=n_rows, slack=1)
    B = n_scenes * traj
    so = solver.BatchedSolver(dims, B_max=B)
    f64 = dict(dtype=torch.float64, device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    gen = [scenes.with_costmap(scenes.make_scene(i, N=N, M=8, B=1, slack=True, n_decomp=n_rows), 5000 + i, size=cells, resolution=10.0 / cells) for i in range(16)]
    rep = n_scenes // 16
    x0 = torch.zeros((B, N + 1, 8), **f64)
    x0[::traj] = up(np.tile(np.stack([g["x0"][0] for g in gen]), (rep, 1, 1)))            # each scene's first entry carries its warm start
    xinit = torch.zeros((B, 6), **f64); params = torch.zeros((B, N, dims.npar), **f64)
    so.set_batch_device(B, xinit.data_ptr(), x0.data_ptr(), params.data_ptr())
    cost = up(np.tile(np.stack([g["costmap"] for g in gen]), (rep, 1, 1))); origin = up(np.tile(np.stack([g["costmap_origin"] for g in gen]), (rep, 1)))
    path = up(np.tile(np.stack([g["segments"] for g in gen]), (rep, 1, 1))); pc = up(np.full(n_scenes, S, np.int32)); length = up(np.full(n_scenes, 6.0 * S))
    s0 = torch.zeros(n_scenes, **f64); sx = torch.zeros(n_scenes, **f64)
    main = up(np.arange(0, B, traj, dtype=np.int32)); scene_of = up(np.repeat(np.arange(n_scenes, dtype=np.int32), traj))
    pts = torch.zeros((n_scenes, n_pts_max, 2), **f64); cnt = torch.zeros(n_scenes, dtype=torch.int32, device=dev); ov = torch.zeros(n_scenes, dtype=torch.uint8, device=dev)
    rows = torch.zeros((n_scenes, N, n_rows, 3), **f64); rc = torch.zeros((n_scenes, N), dtype=torch.int32, device=dev); st = torch.zeros((n_scenes, N), dtype=torch.uint8, device=dev)
    points = lambda: so.costmap_points(n_scenes, cells, cells, cost.data_ptr(), origin.data_ptr(), 10.0 / cells, n_pts_max, pts.data_ptr(), cnt.data_ptr(), ov.data_ptr())
    decomp = lambda: so.decomp_halfspaces(main.data_ptr(), n_scenes, S, path.data_ptr(), pc.data_ptr(), length.data_ptr(), s0.data_ptr(), sx.data_ptr(), pts.data_ptr(),
                                          cnt.data_ptr(), n_pts_max, 2.0, n_rows, rows.data_ptr(), rc.data_ptr(), st.data_ptr())
    write = lambda: so.set_halfspace_rows(rows.data_ptr(), n_rows, scene_of.data_ptr(), n_scenes)
    hs = torch.cuda.ExternalStream(so.stream_ptr(), device=dev)
    for name, call in (("tmpc_costmap_points_kernel", points), ("tmpc_decomp_halfspaces_kernel", decomp), ("tmpc_set_halfspace_rows_kernel", write)):
        for _ in range(5):
            call()
        so.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(hs):
            e0.record()
        for _ in range(20):
            call()
        with torch.cuda.stream(hs):
            e1.record()
        so.synchronize()
        print(json.dumps(dict(kernel=name, n_scenes=n_scenes, trajectories=B, cells=cells, N=N, n_rows=n_rows, points_mean=float(cnt.double().mean().item()),
                              points_max=int(cnt.max().item()), overflow=int(ov.sum().item()), rows_mean=float(rc[:, 1:].double().mean().item()),
                              status_counts=[int((st[:, 1:] == v).sum().item()) for v in (0, 1, 2)], us_per_launch_events=e0.elapsed_time(e1) * 1e3 / 20)), flush=True)
    so.close()


def velocity_kernels(n_seg, n_scenes=512, traj=64, N=20, S=5):
    rng = np.random.default_rng(13)
    B = n_scenes * traj
    so = solver.BatchedSolver(solver.default_dims(), B_max=B)
    f64 = dict(dtype=torch.float64, device=dev)
    xinit = torch.zeros((B, 5), **f64); x0 = torch.zeros((B, N + 1, 7), **f64); params = torch.zeros((B, N, so.dims.npar), **f64)
    so.set_batch_device(B, xinit.data_ptr(), x0.data_ptr(), params.data_ptr())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n_pts = n_seg + 1
    heading = np.cumsum(rng.normal(size=(n_scenes, n_pts)) * 0.15, 1); step = rng.uniform(0.5, 3.0, (n_scenes, n_pts))
    t_xy = up(np.cumsum(np.stack([np.cos(heading) * step, np.sin(heading) * step], 2), 1)); t_v = up(rng.uniform(0.5, 3.0, (n_scenes, n_pts)))
    t_cnt = up(np.full(n_scenes, n_pts, np.int32))
    path = torch.zeros((n_scenes, n_seg, 9), **f64); pc = torch.zeros(n_scenes, dtype=torch.int32, device=dev); length = torch.zeros(n_scenes, **f64)
    vel = torch.zeros((n_scenes, n_seg, 4), **f64)
    so.fit_path(n_scenes, n_pts, n_seg, t_xy.data_ptr(), t_cnt.data_ptr(), path.data_ptr(), pc.data_ptr(), length.data_ptr(), d_v=t_v.data_ptr(),
                d_velocity=vel.data_ptr())
    so.synchronize()
    assert int(pc.min().item()) == n_seg
    seg_np = rng.integers(0, n_seg, n_scenes)
    seg = up(seg_np.astype(np.int32))
    starts = path[:, :, 8].cpu().numpy()
    cs = up(starts[np.arange(n_scenes), seg_np] + 0.1)
    win = torch.zeros((n_scenes, S, 4), **f64); v_ref = torch.zeros(n_scenes, **f64)
    scene_of = up(np.repeat(np.arange(n_scenes, dtype=np.int32), traj))
    cols = list(range(8, 8 + 4 * S))
    window = lambda: so.path_velocity_window(n_scenes, n_seg, S, path.data_ptr(), pc.data_ptr(), length.data_ptr(), seg.data_ptr(), cs.data_ptr(), win.data_ptr(),
                                             d_velocity=vel.data_ptr(), reference_velocity=2.0, d_v_ref=v_ref.data_ptr())
    scatter = lambda: so.scatter_parameters(cols, win.data_ptr(), scene_of.data_ptr(), n_scenes)
    hs = torch.cuda.ExternalStream(so.stream_ptr(), device=dev)
    for name, call in (("tmpc_path_velocity_window_kernel", window), ("tmpc_scatter_parameters_kernel", scatter)):
        for _ in range(10):
            call()
        so.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(hs):
            e0.record()
        for _ in range(50):
            call()
        with torch.cuda.stream(hs):
            e1.record()
        so.synchronize()
        print(json.dumps(dict(kernel=name, n_scenes=n_scenes, trajectories=B, segments=n_seg, S=S, N=N, columns=len(cols),
                              us_per_launch_events=e0.elapsed_time(e1) * 1e3 / 50)), flush=True)
    so.close()


def guidance_kernels(n_scenes=512, n_paths=4, n_nodes=8, N=30, M=8, S=5):
    rng = np.random.default_rng(18)
    P = n_paths + 1
    B = n_scenes * P
    so = solver.BatchedSolver(solver.default_dims(N=N, S=S, n_lin=M, M=M), B_max=B)
    scs = [scenes.make_scene(500 + i, N=N, M=M, B=n_paths, tmpc_pp=True) for i in range(16)]
    rep = n_scenes // len(scs)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tile = lambda k: np.concatenate([np.concatenate([sc[k] for sc in scs])] * rep)
    xinit = tile("xinit")
    t_xinit, t_x0, t_params = up(xinit), up(tile("x0")), up(tile("params"))
    so.set_batch_device(B, t_xinit.data_ptr(), t_x0.data_ptr(), t_params.data_ptr())
    so.solve()
    d_pobj, d_code = so.result_device_ptrs()
    # nodes: every guided entry's guidance trajectory at n_nodes stages of the horizon; none for the non-guided planner
    stages = np.linspace(0, N, n_nodes).round().astype(int)
    nodes, node_count = np.zeros((B, n_nodes, 3)), np.zeros(B, np.int32)
    for q in range(n_scenes):
        sc = scs[q % len(scs)]
        for p in range(n_paths):
            nodes[q * P + p] = np.concatenate([stages[:, None] * so.dims.dt, sc["guidance_pos"][p][stages]], 1)
            node_count[q * P + p] = n_nodes
    t_nodes, t_ncnt = up(nodes), up(node_count)
    t_cnt, t_cls = up(rng.integers(2, n_paths + 1, n_scenes).astype(np.int32)), up(rng.integers(0, 6, (n_scenes, n_paths)).astype(np.int32))
    t_ids = torch.full((n_scenes, P), -1, dtype=torch.int32, device=dev); t_sel = up(np.tile(np.array([-1, 0, -1], np.int32), (n_scenes, 1)))
    i32, u8, f64 = torch.int32, torch.uint8, torch.float64
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    t_mode, t_src, t_gid, t_init, t_dummy, t_dis, t_w = z(B, i32), z(B, i32), z(B, i32), z(B, u8), z(B, u8), z(B, u8), z(B, f64)
    t_gpos, t_gvel, t_status = z((B, N + 1, 2), f64), z((B, N + 1, 2), f64), z(B, i32)
    t_best, t_exit, t_cmd, t_state = z(n_scenes, i32), z(n_scenes, i32), z((n_scenes, 2), f64), up(xinit[::P].copy())
    opt = solver.guidance_options(n_paths, True, True, True, 0.8)
    sample = lambda: so.sample_guidance(B, n_nodes, t_nodes.data_ptr(), t_ncnt.data_ptr(), t_gpos.data_ptr(), t_gvel.data_ptr(), t_status.data_ptr())
    plan = lambda: so.guidance_plan(n_scenes, opt, t_cnt.data_ptr(), t_cls.data_ptr(), t_ids.data_ptr(), t_sel.data_ptr(), t_mode.data_ptr(), t_src.data_ptr(),
                                    t_init.data_ptr(), t_dummy.data_ptr(), t_dis.data_ptr(), t_gid.data_ptr(), t_w.data_ptr())
    decide = lambda: so.guidance_decide(n_scenes, opt, d_pobj, d_code, t_dis.data_ptr(), t_gid.data_ptr(), t_w.data_ptr(), t_state.data_ptr(), t_best.data_ptr(),
                                        t_exit.data_ptr(), t_cmd.data_ptr(), t_ids.data_ptr(), t_sel.data_ptr())
    hs = torch.cuda.ExternalStream(so.stream_ptr(), device=dev)
    torch.cuda.synchronize()
    for name, call in (("tmpc_guidance_plan_kernel", plan), ("tmpc_sample_guidance_kernel", sample), ("tmpc_guidance_decide_kernel", decide)):
        for _ in range(10):
            call()
        so.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(hs):
            e0.record()
        for _ in range(50):
            call()
        with torch.cuda.stream(hs):
            e1.record()
        so.synchronize()
        print(json.dumps(dict(kernel=name, n_scenes=n_scenes, planners=P, entries=B, nodes=n_nodes, N=N,
                              us_per_launch_events=e0.elapsed_time(e1) * 1e3 / 50)), flush=True)
    assert int(t_status.sum().item()) == n_scenes and int((t_best >= 0).sum().item()) > 0          # the non-guided entries have no nodes; some scene has a winner
    so.close()


if "--guidance" in sys.argv:
    guidance_kernels()
    print("done")
    sys.exit(0)
if "--velocity" in sys.argv:
    velocity_kernels(int(sys.argv[sys.argv.index("--segments") + 1]) if "--segments" in sys.argv else 64)
    print("done")
    sys.exit(0)
if "--decomp" in sys.argv:
    decomp_kernels(int(sys.argv[sys.argv.index("--cells") + 1]) if "--cells" in sys.argv else 100)
    print("done")
    sys.exit(0)
if "--fit" in sys.argv:
    fit_kernel(int(sys.argv[sys.argv.index("--points") + 1]) if "--points" in sys.argv else 65)
    print("done")
    sys.exit(0)
if "--path" in sys.argv:
    path_kernels(sys.argv[sys.argv.index("--path") + 1], int(sys.argv[sys.argv.index("--segments") + 1]) if "--segments" in sys.argv else 64)
    print("done")
    sys.exit(0)
if "--slots" in sys.argv:
    obstacle_kernels(slots)
    print("done")
    sys.exit(0)
batch = scenes.make_batch(range(64), N=20, M=8, B=64)
B = batch["xinit"].shape[0]
s = solver.BatchedSolver(solver.default_dims(), B_max=B)
s.set_batch(batch["xinit"], batch["x0"], batch["params"]); s.solve()
obst = np.stack([scenes.make_scene(i, N=20, M=8, B=1)["obstacles"]["pos"] for i in range(64)])
t = dict(ob=torch.from_numpy(obst).to(dev), sc=torch.from_numpy(batch["scene_of"]).to(dev), sx=torch.zeros(64, dtype=torch.float64, device=dev),
         st=torch.from_numpy(batch["xinit"]).to(dev), gp=torch.zeros((B, 21, 2), dtype=torch.float64, device=dev),
         gv=torch.ones((B, 21, 2), dtype=torch.float64, device=dev), rec=torch.zeros((B, 2), dtype=torch.int64, device=dev),
         best=torch.zeros(64, dtype=torch.int32, device=dev),
         main=torch.from_numpy(np.tile(np.arange(0, B, 64, dtype=np.int32), 8)).to(dev),                 # [512]: each scene's first entry, 8 times over
         stat=torch.zeros((512, 20, 2, 3), dtype=torch.float64, device=dev))
for _ in range(10):
    s.warmstart(t["st"].data_ptr())
    s.init_with_guidance(t["gp"].data_ptr(), t["gv"].data_ptr())
    s.road_halfspaces(t["main"].data_ptr(), 512, 2.675, 2.675, t["stat"].data_ptr(), 2, first_row=0)
    s.linearize_topology(t["ob"].data_ptr(), t["sc"].data_ptr(), t["sx"].data_ptr(), 0.325)
    s.pack_records(t["rec"].data_ptr(), None)
    s.select_best_records(t["rec"].data_ptr(), 1, 64, 64, t["best"].data_ptr())
s.synchronize(); s.close()
obstacle_kernels(slots)
print("done")
