"""GPU: obstacle preparation on device (tmpc_prepare_obstacles, tmpc_set_obstacle_parameters; csrc/tmpc_aux_kernels.hpp) against the host
mirrors (mpc_planner_amd/modules.py prepare_obstacles, ellipsoid_set_parameters, gaussian_set_parameters -- pinned on hand-derived values in
tests/test_obstacle_preparation.py).  Every comparison is exact (assert_array_equal): the kernels keep the mirrors' operation order without
FMA contraction, and the one place where device and libm may differ -- cos / sin of the heading, which enter the ranking key only -- is kept
away from every decision by a precondition asserted ON THE MIRROR: consecutive keys among the M + 1 closest are at least 1e-9 apart."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N, M, S = 20, 8, 5
DT = 0.2
MIN_GAP = 1e-9


def _raw_scene(q, count):
    """Scene q of the issue's recipe: PCG64(4200 + q), positions uniform in [1, 15] x [-5, 5], speeds in [0.3, 1.6], headings in [-pi, pi],
    state (0.3 q, -0.2 q, 0.35 q - 0.8, v).  Also radii and a given prediction per obstacle: the constant-velocity path with a lateral
    wobble, the heading as angle, growing radii -- every third obstacle with zero uncertainty at its last step (a DETERMINISTIC prediction)."""
    rng = np.random.Generator(np.random.PCG64(4200 + q))
    pos = np.stack([rng.uniform(1.0, 15.0, count), rng.uniform(-5.0, 5.0, count)], 1)
    speed = rng.uniform(0.3, 1.6, count); heading = rng.uniform(-np.pi, np.pi, count)
    vel = np.stack([speed * np.cos(heading), speed * np.sin(heading)], 1)
    state = np.array([0.3 * q, -0.2 * q, 0.35 * q - 0.8, rng.uniform(0.5, 2.0)])
    radius = rng.uniform(0.3, 0.6, count)
    k = np.arange(N, dtype=float)
    pred = np.zeros((count, N, 5))
    pred[:, :, 0:2] = pos[:, None, :] + (vel[:, None, :] * DT) * k[None, :, None]
    pred[:, :, 1] += 0.05 * np.sin(0.7 * k)[None, :] * rng.uniform(0.0, 1.0, count)[:, None]
    pred[:, :, 2] = heading[:, None]
    pred[:, :, 3] = rng.uniform(0.05, 0.3, count)[:, None] * (1.0 + 0.1 * k[None, :])
    pred[:, :, 4] = 0.5 * pred[:, :, 3]
    pred[2::3, N - 1, 3] = 0.0
    return dict(state=state, pos=pos, vel=vel, radius=radius, pred=pred, count=count)


def _launch(s, raws, R, given, sentinel=True, **opt):
    """One tmpc_prepare_obstacles launch over the scenes `raws` with R slots each; the slots beyond a scene's count hold NaN (never read).
    Returns the five output buffers as numpy arrays (prefilled with sentinels: every entry must have been written)."""
    import torch
    dev = torch.device("cuda")
    Q = len(raws)
    cnt = np.array([r["count"] for r in raws], np.int32)
    state = np.stack([r["state"] for r in raws])
    rp = np.full((Q, R, 2), np.nan); rr = np.full((Q, R), np.nan); rv = np.full((Q, R, 2), np.nan); pr = np.full((Q, R, N, 5), np.nan)
    for q, r in enumerate(raws):
        c = r["count"]
        rp[q, :c] = r["pos"]; rr[q, :c] = r["radius"]; rv[q, :c] = r["vel"]; pr[q, :c] = r["pred"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t_cnt, t_state, t_rp, t_rr = t(cnt), t(state), t(rp), t(rr)
    t_in = t(pr) if given else t(rv)
    o_pos = torch.full((Q, M, N, 2), -7777.0, dtype=torch.float64, device=dev); o_shape = torch.full((Q, M, N, 3), -7777.0, dtype=torch.float64, device=dev)
    o_rad = torch.full((Q, M), -7777.0, dtype=torch.float64, device=dev); o_g = torch.full((Q, M), 0xEE, dtype=torch.uint8, device=dev)
    o_sel = torch.full((Q, M), -99, dtype=torch.int32, device=dev)
    s.prepare_obstacles(Q, R, M, t_cnt.data_ptr(), t_state.data_ptr(), t_rp.data_ptr(), t_rr.data_ptr(), o_pos.data_ptr(), o_shape.data_ptr(),
                        o_rad.data_ptr(), o_g.data_ptr(), o_sel.data_ptr(), d_raw_pred=t_in.data_ptr() if given else None,
                        d_raw_vel=None if given else t_in.data_ptr(), **opt)
    s.synchronize()
    return dict(pos=o_pos.cpu().numpy(), shape=o_shape.cpu().numpy(), radius=o_rad.cpu().numpy(), gaussian=o_g.cpu().numpy(), selected=o_sel.cpu().numpy())


def _mirror(raws, given, **opt):
    from mpc_planner_amd import modules as md
    outs = []
    for r in raws:
        kw = dict(raw_pred=r["pred"]) if given else dict(raw_vel=r["vel"])
        outs.append(md.prepare_obstacles(r["state"], r["pos"], r["radius"], M, N, DT, **kw, **opt))
        _assert_keys_apart(r, given, opt.get("max_obstacle_distance", 0.0))
    return dict(pos=np.stack([o["pos"] for o in outs]), shape=np.stack([o["shape"] for o in outs]), radius=np.stack([o["radius"] for o in outs]),
                gaussian=np.stack([o["gaussian"] for o in outs]).astype(np.uint8), selected=np.stack([o["selected"] for o in outs]))


def _assert_keys_apart(r, given, max_dist):
    """The precondition: where a selection takes place, consecutive ranking keys among the M + 1 closest differ by at least MIN_GAP, so a
    few-ulp difference between the device's and libm's cos / sin cannot decide an order.  A scene that fails it fails the test."""
    from mpc_planner_amd import modules as md
    pred_pos = r["pred"][:, :, 0:2] if given else r["pos"][:, None, :] + (r["vel"][:, None, :] * DT) * np.arange(N, dtype=float)[None, :, None]
    if max_dist > 0.0:
        dx = r["pos"][:, 0] - r["state"][0]; dy = r["pos"][:, 1] - r["state"][1]
        pred_pos = pred_pos[np.sqrt(dx * dx + dy * dy) < max_dist]
    if len(pred_pos) <= M:
        return np.inf
    key = np.sort(md.obstacle_selection_distance(pred_pos, r["state"]))[:M + 1]
    gap = np.diff(key).min()
    assert gap >= MIN_GAP, f"ranking keys {gap:.3e} apart: the scene cannot be checked exactly"
    return gap


def _assert_equal(got, want, what):
    for key in ("selected", "gaussian", "radius", "pos", "shape"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{what}: {key}")


def _solver(B_max=4, **kw):
    from mpc_planner_amd import solver
    return solver.BatchedSolver(solver.default_dims(N=N, S=S, n_lin=M, M=M, **kw), B_max=B_max)


SMALL = [(0, 12), (1, 8), (2, 5), (3, 0)]                     # more than M, exactly M, fewer, none: 12 slots each
WIDE = [(4, 300), (5, 70)]                                    # R = 300 slots: more slots than the workgroup has lanes
CAP = [(6, 1024)]                                             # the cap


@pytest.mark.parametrize("given", [0, 1])
@pytest.mark.parametrize("probabilistic", [0, 1])
def test_prepared_obstacles_equal_the_mirror(given, probabilistic):
    """Both input modes x probabilistic 0 / 1, each with propagate_passes 0, 1, 2 x max_obstacle_distance off / 6.0 on the four small scenes
    and the R = 300 launch, and two of those option sets at the cap R = 1024 = count."""
    s = _solver()
    small = [_raw_scene(q, c) for q, c in SMALL]; wide = [_raw_scene(q, c) for q, c in WIDE]; cap = [_raw_scene(q, c) for q, c in CAP]
    for passes in (0, 1, 2):
        for max_dist in (0.0, 6.0):
            opt = dict(probabilistic=bool(probabilistic), propagate_passes=passes, max_obstacle_distance=max_dist)
            what = f"given {given} probabilistic {probabilistic} passes {passes} max_dist {max_dist}"
            for raws, R in ((small, 12), (wide, 300)) + (((cap, 1024),) if (passes, max_dist) in ((2, 0.0), (1, 6.0)) else ()):
                got = _launch(s, raws, R, given, **opt); want = _mirror(raws, given, **opt)
                dummies = (want["selected"] < 0).sum(axis=1).tolist()
                print(f"[obstacles] {what} R {R}: dummies per scene {dummies}, gaussian {int(want['gaussian'].sum())}, "
                      f"bitwise equal {all(np.array_equal(got[k], want[k]) for k in want)}")
                _assert_equal(got, want, f"{what} R {R}")
    # the recipe's scenes do select, do pad and -- in given mode -- do mix the prediction types
    want = _mirror(small, given, probabilistic=bool(probabilistic))
    assert (want["selected"][0] >= 0).all() and sorted(want["selected"][0].tolist()) != list(range(M))
    assert want["selected"][2].tolist() == [0, 1, 2, 3, 4, -1, -1, -1] and (want["selected"][3] == -1).all()
    if given and probabilistic:
        assert 0 < want["gaussian"][1].sum() < M
    s.close()


def test_ties_on_device_keep_the_lower_raw_index():
    """psi = 0: cos and sin are exact, the mirrored pairs (x, +1) / (x, -1) have identical keys on host and device."""
    s = _solver()
    pos = np.array([[6.0, 1.0], [6.0, -1.0], [4.0, 1.0], [4.0, -1.0], [5.0, 1.0], [5.0, -1.0]])
    raw = dict(state=np.array([0.0, 0.0, 0.0, 1.0]), pos=pos, vel=np.tile([-0.5, 0.0], (6, 1)), radius=np.full(6, 0.4), pred=np.zeros((6, N, 5)), count=6)
    import torch
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    o_pos = torch.zeros((1, 3, N, 2), dtype=torch.float64, device=dev); o_shape = torch.zeros((1, 3, N, 3), dtype=torch.float64, device=dev)
    o_rad = torch.zeros((1, 3), dtype=torch.float64, device=dev); o_g = torch.zeros((1, 3), dtype=torch.uint8, device=dev)
    o_sel = torch.full((1, 3), -99, dtype=torch.int32, device=dev)
    ins = [t(np.array([6], np.int32)), t(raw["state"][None]), t(pos[None]), t(raw["radius"][None]), t(raw["vel"][None])]
    s.prepare_obstacles(1, 6, 3, *[a.data_ptr() for a in ins[:4]], o_pos.data_ptr(), o_shape.data_ptr(), o_rad.data_ptr(), o_g.data_ptr(),
                        o_sel.data_ptr(), d_raw_vel=ins[4].data_ptr())
    s.synchronize()
    assert o_sel.cpu().numpy()[0].tolist() == [2, 3, 4]
    np.testing.assert_array_equal(o_pos.cpu().numpy()[0, :, 0], pos[[2, 3, 4]])
    s.close()


def _concat(scs):
    xinit = np.concatenate([s["xinit"] for s in scs]); x0 = np.concatenate([s["x0"] for s in scs]); params = np.concatenate([s["params"] for s in scs])
    scene_of = np.concatenate([np.full(len(s["xinit"]), i, np.int32) for i, s in enumerate(scs)])
    first = np.cumsum([0] + [len(s["xinit"]) for s in scs])[:-1]
    return xinit, x0, params, scene_of, first


def _collision_columns(pm, gauss_rows):
    fields = ("x", "y", "major", "minor", "risk", "r") if gauss_rows else ("x", "y", "psi", "major", "minor", "chi", "r")
    name = "gaussian_obst" if gauss_rows else "ellipsoid_obst"
    return [pm.index(f"{name}_{j}_{f}") for j in range(M) for f in fields] + [pm.index("ego_disc_radius"), pm.index("ego_disc_0_offset")]


@pytest.mark.parametrize("case", ["ellipsoid", "ellipsoid_gaussian", "chance", "slack"])
def test_parameter_writer_equals_the_host_built_rows(case):
    """Three scenes x 8 guided entries plus the T-MPC++ entry each; the collision and disc columns start at -7 and must come back as the
    host built them (scenes.make_scene: modules.ellipsoid_set_parameters / gaussian_set_parameters), every other column untouched.
    The buffers hold what must NOT be used as well: radii for a DETERMINISTIC obstacle (row model 0 writes zeros and chi = 1), the prepared
    obstacle's own radius in row model 1 (the r column takes the configured one)."""
    import torch
    from mpc_planner_amd import scenes
    kw = dict(ellipsoid={}, ellipsoid_gaussian=dict(gaussian=True), chance=dict(chance=True), slack=dict(slack=True, n_decomp=12))[case]
    scs = [scenes.make_scene(70 + i, N=N, M=M, B=8, tmpc_pp=True, **kw) for i in range(3)]
    xinit, x0, want, scene_of, first = _concat(scs)
    B = len(xinit)
    assert B == 27
    pm = scs[0]["pm"]
    gauss_rows = case == "chance"
    cols = _collision_columns(pm, gauss_rows)
    start = want.copy(); start[:, :, cols] = -7.0
    dims_kw = dict(row_model=1) if gauss_rows else (dict(n_slk=12, slack=1) if case == "slack" else {})
    s = _solver(B_max=B, **dims_kw)
    assert s.dims.npar == pm.length()
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    is_gauss = case in ("ellipsoid_gaussian", "chance")
    obs = [sc["obstacles"] for sc in scs]
    shape = np.stack([np.stack([o["angle"], o["major"], o["minor"]], 2) for o in obs])
    radius = np.stack([o["radius"] for o in obs])
    if not is_gauss:
        shape[:, :, :, 1:] = 0.77                                     # a deterministic obstacle's radii are not used
    if gauss_rows:
        radius = radius + 0.123                                       # nor is the prepared obstacle's own radius in row model 1
    bufs = [t(np.stack([o["pos"] for o in obs])), t(shape), t(radius), t(np.full((3, M), int(is_gauss), np.uint8)), t(scene_of),
            t(xinit[first, :4])]
    call = lambda: s.set_obstacle_parameters(*[b.data_ptr() for b in bufs], scenes.ROBOT_RADIUS, disc_offset=0.0, risk=0.05,
                                             obstacle_radius=scenes.OBSTACLE_RADIUS)
    with pytest.raises(Exception, match="no batch"):
        call()
    s.set_batch(xinit, x0, start)
    call()
    got = s.debug_get_params()
    other = np.setdiff1d(np.arange(pm.length()), cols)
    np.testing.assert_array_equal(got[:, :, other], start[:, :, other])
    np.testing.assert_array_equal(got, want)
    s.close()


def _scene_velocities(scene_idx):
    """The obstacle velocities make_scene draws (its first random numbers; it does not return them)."""
    from mpc_planner_amd import scenes
    rng = np.random.Generator(np.random.PCG64(1000 + scene_idx))
    rng.uniform(0.5, 2.0)
    scenes.reference_path_segments(rng, S)
    speed = rng.uniform(0.6, 1.6, M)
    heading = np.where(rng.uniform(size=M) < 0.5, 1.0, -1.0) * np.pi / 2 + rng.uniform(-0.5, 0.5, M)
    return np.stack([speed * np.cos(heading), speed * np.sin(heading)], 1)


def test_closed_loop_prepared_on_device_solves_like_host_built():
    """prepare_obstacles -> set_obstacle_parameters -> linearize_topology_ex (fed by the prepared d_obstacle_pos) -> solve on a batch whose
    collision and topology columns were blanked, against the same batch as the host built it: exit codes, iteration counts, objectives and
    trajectories identical; the host-built handle also holds the suite's oracle line (1e-8, tests/test_gpu_parity.py _compare)."""
    import sys
    import torch
    sys.path.insert(0, HERE)
    import oracle_lib as O
    from mpc_planner_amd import scenes
    idx = [70, 71, 72]
    scs = [scenes.make_scene(i, N=N, M=M, B=8) for i in idx]
    xinit, x0, params, scene_of, first = _concat(scs)
    B = len(xinit)
    assert B == 24
    pm = scs[0]["pm"]
    a = _solver(B_max=B)
    a.set_batch(xinit, x0, params); a.solve(); ra = a.get()
    a.close()
    cols = _collision_columns(pm, False) + [pm.index(f"lin_constraint_{j}_{f}") for j in range(M) for f in ("a1", "a2", "b")]
    start = params.copy(); start[:, :, cols] = 0.0
    b = _solver(B_max=B)
    b.set_batch(xinit, x0, start)
    dev = torch.device("cuda")
    t = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
    state = xinit[first, :4]
    t_cnt = t(np.full(3, M, np.int32)); t_state = t(state); t_sx = t(state[:, 0]); t_sc = t(scene_of)
    t_rp = t(np.stack([sc["obstacles"]["pos"][:, 0] for sc in scs])); t_rr = t(np.stack([sc["obstacles"]["radius"] for sc in scs]))
    t_rv = t(np.stack([_scene_velocities(i) for i in idx]))
    o_pos = torch.zeros((3, M, N, 2), dtype=torch.float64, device=dev); o_shape = torch.zeros((3, M, N, 3), dtype=torch.float64, device=dev)
    o_rad = torch.zeros((3, M), dtype=torch.float64, device=dev); o_g = torch.zeros((3, M), dtype=torch.uint8, device=dev)
    o_sel = torch.zeros((3, M), dtype=torch.int32, device=dev)
    b.prepare_obstacles(3, M, M, t_cnt.data_ptr(), t_state.data_ptr(), t_rp.data_ptr(), t_rr.data_ptr(), o_pos.data_ptr(), o_shape.data_ptr(),
                        o_rad.data_ptr(), o_g.data_ptr(), o_sel.data_ptr(), d_raw_vel=t_rv.data_ptr())
    b.set_obstacle_parameters(o_pos.data_ptr(), o_shape.data_ptr(), o_rad.data_ptr(), o_g.data_ptr(), t_sc.data_ptr(), t_state.data_ptr(),
                              scenes.ROBOT_RADIUS)
    b.linearize_topology_ex(o_pos.data_ptr(), M, t_sc.data_ptr(), t_sx.data_ptr(), scenes.ROBOT_RADIUS)
    b.solve(); rb = b.get()
    p_dev = b.debug_get_params()
    b.close()
    np.testing.assert_array_equal(o_pos.cpu().numpy(), np.stack([sc["obstacles"]["pos"] for sc in scs]))
    print(f"[obstacle loop] parameter rows: max |device-built - host-built| = {np.abs(p_dev - params).max():.3e}, "
          f"bitwise equal {np.array_equal(p_dev, params)}; successes {(ra['exit_code'] == 1).sum()} / {B}")
    for key in ("exit_code", "sqp_iter", "qp_iter_total", "qp_status", "pobj", "xtraj", "utraj"):
        np.testing.assert_array_equal(rb[key], ra[key], err_msg=key)
    pb = O.problem(N=N, S=S, n_lin=M, M=M)
    xt, ut, info = O.solve_batch(pb, xinit, x0.reshape(B, -1), params.reshape(B, -1))
    assert (ra["exit_code"] == info["exit_code"]).all() and (ra["sqp_iter"] == info["sqp_iter"]).all()
    ok = info["exit_code"] == 1
    assert ok.sum() >= 12
    assert (ra["qp_status"][ok] == info["qp_status"][ok]).all() and (ra["qp_iter_total"][ok] == info["qp_iter_total"][ok]).all()
    sx = np.maximum(np.abs(xt[ok]).max(axis=2, keepdims=True), 1.0); su = np.maximum(np.abs(ut[ok]).max(axis=2, keepdims=True), 1.0)
    ex = (np.abs(ra["xtraj"][ok] - xt[ok]) / sx).max(); eu = (np.abs(ra["utraj"][ok] - ut[ok]) / su).max()
    ep = (np.abs(ra["pobj"][ok] - info["pobj"][ok]) / np.maximum(np.abs(info["pobj"][ok]), 1.0)).max()
    print(f"[obstacle loop] against the oracle: x {ex:.3e}, u {eu:.3e}, objective {ep:.3e}")
    assert ex < 1e-8 and eu < 1e-8 and ep < 1e-8, (ex, eu, ep)


def test_bad_arguments_launch_nothing():
    import torch
    from mpc_planner_amd import solver
    s = _solver()
    dev = torch.device("cuda")
    raw = _raw_scene(0, 12)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ins = dict(d_count=t(np.array([12], np.int32)), d_state=t(raw["state"][None]), d_raw_pos=t(raw["pos"][None]), d_raw_radius=t(raw["radius"][None]))
    vel, pred = t(raw["vel"][None]), t(raw["pred"][None])
    outs = dict(d_obstacle_pos=torch.full((1, M, N, 2), 4.0, dtype=torch.float64, device=dev),
                d_obstacle_shape=torch.full((1, M, N, 3), 4.0, dtype=torch.float64, device=dev),
                d_obstacle_radius=torch.full((1, M), 4.0, dtype=torch.float64, device=dev),
                d_obstacle_gaussian=torch.full((1, M), 4, dtype=torch.uint8, device=dev), d_selected=torch.full((1, M), 4, dtype=torch.int32, device=dev))

    def call(**kw):
        a = dict(n_scenes=1, n_slots=12, max_obstacles=M, d_raw_vel=vel.data_ptr())
        a.update({k: v.data_ptr() for k, v in ins.items()}); a.update({k: v.data_ptr() for k, v in outs.items()})
        a.update(kw)
        s.prepare_obstacles(**a)

    bad = [(dict(d_raw_vel=None), "exactly one"), (dict(d_raw_pred=pred.data_ptr()), "exactly one"), (dict(n_slots=1025), "n_slots"),
           (dict(propagate_passes=3), "propagate_passes"), (dict(propagate_passes=-1), "propagate_passes"), (dict(n_scenes=0), "n_scenes"),
           (dict(n_scenes=-2), "n_scenes"), (dict(max_obstacles=0), "max_obstacles")]
    bad += [({k: None}, "NULL input") for k in ins] + [({k: None}, "NULL output") for k in outs]
    for kw, msg in bad:
        with pytest.raises(solver.TmpcError, match=msg):
            call(**kw)
    s.synchronize()
    for v in outs.values():                                            # nothing was launched
        assert (v.cpu().numpy() == 4).all()
    # the options struct: a size this library cannot honour
    opt = solver.TmpcObstacleOptions(8, 0, 0, 0, 0.3, 0.0)
    args = [s._h, 1, 12, M] + [C.c_void_p(v.data_ptr()) for v in ins.values()] + [C.c_void_p(vel.data_ptr()), None, C.byref(opt)] \
        + [C.c_void_p(v.data_ptr()) for v in outs.values()]
    assert s.lib.tmpc_prepare_obstacles(*args) == -1 and b"size" in s.lib.tmpc_last_error(s._h)
    assert s.lib.tmpc_prepare_obstacles(None, *args[1:]) == -1                                    # no handle
    # the parameter writer without a batch
    with pytest.raises(solver.TmpcError, match="no batch"):
        s.set_obstacle_parameters(outs["d_obstacle_pos"].data_ptr(), outs["d_obstacle_shape"].data_ptr(), outs["d_obstacle_radius"].data_ptr(),
                                  outs["d_obstacle_gaussian"].data_ptr(), ins["d_count"].data_ptr(), ins["d_state"].data_ptr(), 0.325)
    call()                                                             # and the same call as it should be: accepted
    s.synchronize()
    assert (outs["d_selected"].cpu().numpy() != 4).any()
    s.close()
    # a problem without obstacle rows has nothing to write
    s0 = solver.BatchedSolver(solver.default_dims(N=N, S=S, n_lin=M, M=0), B_max=2)
    z = np.zeros
    s0.set_batch(z((2, 5)), z((2, N + 1, 7)), z((2, N, s0.dims.npar)))
    with pytest.raises(solver.TmpcError, match="M = 0"):
        s0.set_obstacle_parameters(outs["d_obstacle_pos"].data_ptr(), outs["d_obstacle_shape"].data_ptr(), outs["d_obstacle_radius"].data_ptr(),
                                   outs["d_obstacle_gaussian"].data_ptr(), ins["d_count"].data_ptr(), ins["d_state"].data_ptr(), 0.325)
    s0.close()


def test_outputs_do_not_depend_on_what_the_lds_held():
    """After tmpc_debug_poison_lds (every CU's LDS full of NaN patterns) the first launch of the mirror test gives bitwise the same outputs:
    no LDS slot is read before it is written, for any count, 0 included."""
    s = _solver()
    small = [_raw_scene(q, c) for q, c in SMALL]
    opt = dict(probabilistic=False, propagate_passes=0, max_obstacle_distance=0.0)
    before = _launch(s, small, 12, 0, **opt)
    s.debug_poison_lds()
    after = _launch(s, small, 12, 0, **opt)
    _assert_equal(after, before, "after the LDS poison")
    _assert_equal(after, _mirror(small, 0, **opt), "after the LDS poison, against the mirror")
    s.close()
