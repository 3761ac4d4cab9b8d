"""GPU: the module-stack writers of include/tmpc_hip_stack.h (csrc/tmpc_row_entries.hpp; mpc_planner_amd/stack_writers.py) -- the obstacle
and topology rows of a generated solver, written on device into the columns of the stack's parameter map.

1. On the product library the column entries, given the hand-written layout's own columns, leave the rows bit-equal to
   tmpc_set_obstacle_parameters + tmpc_linearize_topology_ex (one source, two destinations) and touch nothing else.
2. On the generated tmpc_cfg2 library (its map IS the hand-written one) they equal the layout writers of the product library.
3. On the generated jackal_tmpc library (Gaussian rows, N = 30, 5 obstacles: mpc_planner_jackal's default) they equal the numpy mirrors: the
   collision columns exactly, the topology columns to the 1e-14 tests/test_gpu_projection.py holds kernel and mirror to.
4. Three ticks of that stack with every row built on device, against the same ticks driven from the host.
5. Every refusal, with its message and without a launch; the entries of tmpc_hip.h keep refusing in a generated solver."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
DT = 0.2
RISK = 0.05
PASSES = 1


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda"))


def _full(shape, value, dtype):
    import torch
    return torch.full(shape, value, dtype=dtype, device=torch.device("cuda"))


def _ptr(t):
    return None if t is None else t.data_ptr()


def _sentinel_rows(B, N, npar):
    """A different negative value in every entry: a column written by mistake, or from the wrong place, cannot pass for untouched."""
    return -(1.0e3 + np.arange(B * N * npar, dtype=np.float64)).reshape(B, N, npar)


def _raw_scene(rng, count, N, state):
    """`count` raw obstacles ahead of the robot with given predictions (x, y, angle, major, minor): constant velocity with a wobble, growing
    radii; every third one ends with major = 0, a DETERMINISTIC prediction in probabilistic mode, the others are GAUSSIAN."""
    pos = np.stack([state[0] + rng.uniform(1.0, 9.0, count), state[1] + rng.uniform(-3.0, 3.0, count)], 1)
    speed, heading = rng.uniform(0.3, 1.4, count), rng.uniform(-np.pi, np.pi, count)
    vel = np.stack([speed * np.cos(heading), speed * np.sin(heading)], 1)
    k = np.arange(N, dtype=float)
    pred = np.zeros((count, N, 5))
    pred[:, :, 0:2] = pos[:, None, :] + (vel[:, None, :] * DT) * k[None, :, None]
    pred[:, :, 1] += 0.05 * np.sin(0.7 * k)[None, :] * rng.uniform(0.0, 1.0, count)[:, None]
    pred[:, :, 2] = heading[:, None]
    pred[:, :, 3] = rng.uniform(0.05, 0.3, count)[:, None] * (1.0 + 0.1 * k[None, :])
    pred[:, :, 4] = 0.5 * pred[:, :, 3]
    pred[2::3, N - 1, 3] = 0.0
    return dict(pos=pos, radius=rng.uniform(0.3, 0.6, count), pred=pred, count=count)


def _problem(N, M, counts, B, nvar, n_obs, n_static, seed):
    """One batch with everything the writers branch on.  len(counts) scenes with that many raw obstacles each (fewer than M: dummies; given
    predictions in probabilistic mode: GAUSSIAN and DETERMINISTIC obstacles side by side), B entries spread over the scenes, the LAST entry a
    non-guided planner (is_original), random warm starts of which entry 0's stage 1 (and a later stage, where there is one) lies INSIDE the disc
    of its scene's obstacle 0, so that the projection to safety moves it; n_static static halfspaces per scene and stage."""
    from mpc_planner_amd import modules as md, scenes
    rng = np.random.default_rng(seed)
    Q = len(counts)
    state = np.stack([np.array([0.4 * q, -0.3 * q, 0.2 * q - 0.1, rng.uniform(0.5, 2.0)]) for q in range(Q)])
    raws = [_raw_scene(rng, c, N, state[q]) for q, c in enumerate(counts)]
    R = max(max(counts), 1)
    rp, rr, pr = np.full((Q, R, 2), np.nan), np.full((Q, R), np.nan), np.full((Q, R, N, 5), np.nan)      # slots beyond the count: never read
    for q, r in enumerate(raws):
        rp[q, :r["count"]], rr[q, :r["count"]], pr[q, :r["count"]] = r["pos"], r["radius"], r["pred"]
    mirror = [md.prepare_obstacles(state[q], r["pos"], r["radius"], M, N, DT, raw_pred=r["pred"], probabilistic=True, propagate_passes=PASSES, risk=RISK)
              for q, r in enumerate(raws)]
    scene_of = (np.arange(B) % Q).astype(np.int32)
    is_original = np.zeros(B, np.uint8); is_original[B - 1] = 1
    xinit = rng.normal(size=(B, nvar - 2))
    x0 = rng.normal(size=(B, N + 1, nvar))
    for b in range(B):
        x0[b, :, 2] = state[scene_of[b], 0] + np.linspace(0.0, 6.0, N + 1) + rng.normal(0.0, 0.3, N + 1)
        x0[b, :, 3] = state[scene_of[b], 1] + rng.normal(0.0, 1.5, N + 1)
    inside = []
    for k in sorted({1, max(1, N // 2)}):                                     # stage k reads prediction step k - 1
        x0[0, k, 2:4] = mirror[scene_of[0]]["pos"][0, k - 1] + np.array([0.11, -0.07])
        inside.append(k)
    static = rng.normal(size=(Q, N, max(n_static, 1), 3))
    return dict(N=N, M=M, Q=Q, B=B, R=R, state=state, count=np.array(counts, np.int32), raw_pos=rp, raw_radius=rr, raw_pred=pr, mirror=mirror,
                scene_of=scene_of, is_original=is_original, xinit=xinit, x0=x0, inside=inside, static=static, n_obs=n_obs, n_static=n_static,
                robot_radius=scenes.ROBOT_RADIUS, obstacle_radius=scenes.OBSTACLE_RADIUS)


class _Device:
    """The problem's inputs on the device, and one set of prepare_obstacles outputs (prefilled: every entry must be written)."""

    def __init__(self, pb):
        import torch
        Q, M, N = pb["Q"], pb["M"], pb["N"]
        self.count, self.state, self.raw_pos, self.raw_radius, self.raw_pred = (_up(pb[k]) for k in ("count", "state", "raw_pos", "raw_radius", "raw_pred"))
        self.state_x = _up(pb["state"][:, 0].copy())
        self.scene_of, self.is_original, self.static = _up(pb["scene_of"]), _up(pb["is_original"]), _up(pb["static"])
        f64 = torch.float64
        self.o_pos, self.o_shape = _full((Q, M, N, 2), -7777.0, f64), _full((Q, M, N, 3), -7777.0, f64)
        self.o_radius, self.o_gauss, self.o_sel = _full((Q, M), -7777.0, f64), _full((Q, M), 0xEE, torch.uint8), _full((Q, M), -99, torch.int32)

    def outputs(self):
        return [t.cpu().numpy() for t in (self.o_pos, self.o_shape, self.o_radius, self.o_gauss, self.o_sel)]


def _prepare(writer, pb, dv):
    """writer: a BatchedSolver (tmpc_prepare_obstacles) or a StackWriters (tmpc_stack_prepare_obstacles): the same signature."""
    writer.prepare_obstacles(pb["Q"], pb["R"], pb["M"], dv.count.data_ptr(), dv.state.data_ptr(), dv.raw_pos.data_ptr(), dv.raw_radius.data_ptr(),
                             dv.o_pos.data_ptr(), dv.o_shape.data_ptr(), dv.o_radius.data_ptr(), dv.o_gauss.data_ptr(), dv.o_sel.data_ptr(),
                             d_raw_pred=dv.raw_pred.data_ptr(), probabilistic=True, propagate_passes=PASSES)


def _topology_args(pb, dv, radii):
    return dict(d_obstacle_pos=dv.o_pos.data_ptr() if pb["n_obs"] else None, n_obstacles=pb["n_obs"], d_scene_of=dv.scene_of.data_ptr(),
                d_state_x=dv.state_x.data_ptr(), robot_radius=pb["robot_radius"], d_obstacle_radius=dv.o_radius.data_ptr() if radii else None,
                d_static_halfspaces=dv.static.data_ptr() if pb["n_static"] else None, n_static=pb["n_static"], d_is_original=dv.is_original.data_ptr())


def _layout_writers(s, pb, dv, radii=False):
    """tmpc_hip.h: prepare -> collision columns -> topology rows of the handle's batch, by the hand-written layout."""
    _prepare(s, pb, dv)
    s.set_obstacle_parameters(dv.o_pos.data_ptr(), dv.o_shape.data_ptr(), dv.o_radius.data_ptr(), dv.o_gauss.data_ptr(), dv.scene_of.data_ptr(),
                              dv.state.data_ptr(), pb["robot_radius"], disc_offset=0.03, risk=RISK, obstacle_radius=pb["obstacle_radius"])
    s.linearize_topology_ex(**_topology_args(pb, dv, radii))
    s.synchronize()


def _column_writers(s, pb, dv, ocols, tcols, row_model, radii=False):
    """tmpc_hip_stack.h: the same three steps, by column."""
    from mpc_planner_amd.stack_writers import StackWriters
    w = StackWriters(s)
    _prepare(w, pb, dv)
    w.set_obstacle_columns(ocols, row_model, pb["M"], dv.o_pos.data_ptr(), dv.o_shape.data_ptr(), dv.o_radius.data_ptr(), dv.o_gauss.data_ptr(),
                           dv.scene_of.data_ptr(), dv.state.data_ptr(), pb["robot_radius"], disc_offset=0.03, risk=RISK, obstacle_radius=pb["obstacle_radius"])
    w.linearize_topology_columns(tcols, **_topology_args(pb, dv, radii))
    s.synchronize()


def _assert_conditions(pb, n_lin):
    """What every batch of these tests must contain (asserted on the mirror, so that a change of the recipe cannot hollow the test out)."""
    from mpc_planner_amd import modules as md
    gauss = np.stack([m["gaussian"] for m in pb["mirror"]]); sel = np.stack([m["selected"] for m in pb["mirror"]])
    assert gauss.any() and (sel < 0).any() and pb["is_original"].any() and not pb["is_original"].all()
    if pb["n_obs"]:
        sc = pb["scene_of"][0]
        for k in pb["inside"]:
            p = pb["x0"][0, k, 2:4]
            moved = md.project_to_safety(p, pb["mirror"][sc]["pos"][:, k - 1], 1e-3 + pb["robot_radius"])
            assert not np.array_equal(moved, p)                               # the projection is not the identity there


CASES = {
    # name: N, M, n_lin, raw counts per scene, B, n_obs, n_static, dims, per-obstacle radii
    "tiny": (2, 1, 1, (1, 0), 3, 1, 0, {}, False),
    "static_rows_and_radii": (20, 8, 10, (11, 5, 8), 14, 8, 2, {}, True),
    "static_rows_only": (5, 4, 4, (6, 2), 5, 0, 2, {}, False),
    "slack_stride": (20, 8, 8, (8, 3), 6, 8, 0, dict(n_slk=12, slack=1), False),
    "gaussian_rows": (20, 8, 8, (10, 4), 6, 8, 0, dict(row_model=1), False),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_column_writers_equal_the_layout_writers_on_the_product_library(case):
    """Two handles of libtmpc_hip.so with the same batch, the rows prefilled with a sentinel pattern: tmpc_prepare_obstacles +
    tmpc_set_obstacle_parameters + tmpc_linearize_topology_ex on one, the tmpc_stack_* entries with the columns the helpers read from the
    hand-written map on the other.  The prepared obstacles and the rows are equal bit for bit, every named column was written, every other
    column still holds its sentinel."""
    from mpc_planner_amd import solver
    from mpc_planner_amd.parameters import define_parameters
    from mpc_planner_amd.stack_writers import obstacle_columns, topology_columns
    N, M, n_lin, counts, B, n_obs, n_static, dims_kw, radii = CASES[case]
    S = 2
    dims = solver.default_dims(N=N, S=S, n_lin=n_lin, M=M, **dims_kw)
    row_model, slack = dims.row_model, dims.slack
    pm = define_parameters(S, M, add_halfspaces=n_lin - M, slack=bool(slack), ellipsoids=row_model == 0, gaussian=row_model == 1, n_decomp=dims.n_slk)._params
    assert len(pm) == dims.npar
    ocols, tcols = obstacle_columns(pm, M, row_model), topology_columns(pm, n_lin)
    pb = _problem(N, M, counts, B, dims.nvar, n_obs, n_static, seed=sorted(CASES).index(case))
    _assert_conditions(pb, n_lin)
    start = _sentinel_rows(B, N, dims.npar)
    a, b = solver.BatchedSolver(dims, B_max=B), solver.BatchedSolver(dims, B_max=B)
    a.set_batch(pb["xinit"], pb["x0"], start); b.set_batch(pb["xinit"], pb["x0"], start)
    da, db = _Device(pb), _Device(pb)
    _layout_writers(a, pb, da, radii)
    _column_writers(b, pb, db, ocols, tcols, row_model, radii)
    for x, y in zip(da.outputs(), db.outputs()):
        assert np.array_equal(x, y)
    assert (da.outputs()[4] < 0).any() and not (da.outputs()[0] == -7777.0).any()
    got_a, got_b = a.debug_get_params(), b.debug_get_params()
    named = sorted(ocols + tcols)
    rest = np.setdiff1d(np.arange(dims.npar), named)
    print(f"[stack writers] {case}: {len(named)} named columns of {dims.npar}, bitwise equal {np.array_equal(got_a, got_b)}, "
          f"max |column - layout| {np.abs(got_a - got_b).max():.3e}")
    assert np.array_equal(got_b, got_a)
    assert np.array_equal(got_b[:, :, rest], start[:, :, rest]) and len(rest) > 0
    assert (got_b[:, :, named] != start[:, :, named]).all()
    a.close(); b.close()


def test_generated_cfg2_library_equals_the_product_library():
    """libtmpc_hip_tmpc_cfg2.so (its parameter map is the hand-written cfg 2 map): the column writers on its handle, the columns read from
    its meta file, against the layout writers on a product handle with the same batch -- tmpc_debug_get_params equal bit for bit."""
    from mpc_planner_amd import solver
    from mpc_planner_amd.stack_writers import obstacle_columns, topology_columns
    from test_gpu_parity import _generated_lib
    path, meta = _generated_lib("tmpc_cfg2")
    N, M, B = 20, 8, 14
    pm = meta["parameter_map"]
    dg, dp = solver.default_dims(N=N, lib_path=path), solver.default_dims(N=N, S=5, n_lin=M, M=M)
    assert dg.npar == dp.npar == meta["npar"] == 135 and dg.nvar == dp.nvar == 7
    pb = _problem(N, M, (11, 5, 8), B, 7, M, 0, seed=20)
    _assert_conditions(pb, M)
    start = _sentinel_rows(B, N, 135)
    g, p = solver.BatchedSolver(dg, B_max=B, lib_path=path), solver.BatchedSolver(dp, B_max=B)
    g.set_batch(pb["xinit"], pb["x0"], start); p.set_batch(pb["xinit"], pb["x0"], start)
    dvg, dvp = _Device(pb), _Device(pb)
    _column_writers(g, pb, dvg, obstacle_columns(pm, M, 0), topology_columns(pm, M), 0)
    _layout_writers(p, pb, dvp)
    for x, y in zip(dvg.outputs(), dvp.outputs()):
        assert np.array_equal(x, y)
    got_g, got_p = g.debug_get_params(), p.debug_get_params()
    assert np.array_equal(got_g, got_p)
    assert (got_g != start).sum() == B * N * (2 + 7 * M + 3 * M)
    g.close(); p.close()


class _Map:
    """A stack's parameter map (name -> column) behind the .index() the numpy mirrors call."""

    def __init__(self, parameter_map):
        self.parameter_map = parameter_map

    def index(self, name):
        return self.parameter_map[name]


def _mirror_rows(pm, rows, pb, obs, x0, radii=False, disc_offset=0.03):
    """The host's answer, in place: GaussianConstraints and LinearizedConstraints of every entry by the numpy mirrors with the stack's map.
    obs: modules.prepare_obstacles per scene.  The Gaussian mirror takes its r column from the obstacles it is given: the CONFIGURED radius."""
    from mpc_planner_amd import modules as md
    for b in range(rows.shape[0]):
        q = pb["scene_of"][b]
        o = dict(obs[q], radius=np.full(pb["M"], pb["obstacle_radius"]))
        md.gaussian_set_parameters(pm, rows[b], pb["state"][q, :2], o, pb["robot_radius"], RISK, disc_offset=disc_offset)
        lin = None if pb["is_original"][b] else md.linearized_update(x0[b], obs[q]["pos"], pb["robot_radius"], obs[q]["radius"] if radii else None)
        md.linearized_set_parameters(pm, rows[b], pb["state"][q, 0], lin, n_rows=pb["M"])


def test_generated_jackal_library_equals_the_mirrors():
    """libtmpc_hip_jackal_tmpc.so (T-MPC with Gaussian chance constraints, N = 30, 5 obstacles, 82 parameters): the column writers against
    modules.prepare_obstacles, gaussian_set_parameters and linearized_update / linearized_set_parameters called with the stack's map.  Raw
    counts of at most M: no ranking takes place, so the prepared obstacles are the mirror's bit for bit (tests/test_gpu_obstacles.py)."""
    from mpc_planner_amd import solver
    from mpc_planner_amd.stack_writers import obstacle_columns, topology_columns
    from test_gpu_parity import _generated_lib
    path, meta = _generated_lib("jackal_tmpc")
    N, M, B = 30, 5, 7
    pm = meta["parameter_map"]
    dims = solver.default_dims(N=N, S=3, lib_path=path)
    assert meta["npar"] == dims.npar == 82 and dims.nvar == 7
    ocols, tcols = obstacle_columns(pm, M, 1), topology_columns(pm, M)
    pb = _problem(N, M, (5, 3), B, 7, M, 0, seed=30)
    _assert_conditions(pb, M)
    start = _sentinel_rows(B, N, 82)
    s = solver.BatchedSolver(dims, B_max=B, lib_path=path)
    s.set_batch(pb["xinit"], pb["x0"], start)
    dv = _Device(pb)
    _column_writers(s, pb, dv, ocols, tcols, 1)
    got = s.debug_get_params()
    o_pos, o_shape, o_radius, o_gauss, o_sel = dv.outputs()
    for q, m in enumerate(pb["mirror"]):
        assert np.array_equal(o_pos[q], m["pos"]) and np.array_equal(o_shape[q], m["shape"]) and np.array_equal(o_radius[q], m["radius"])
        assert np.array_equal(o_gauss[q], m["gaussian"].astype(np.uint8)) and np.array_equal(o_sel[q], m["selected"])
    want = start.copy()
    _mirror_rows(_Map(pm), want, pb, pb["mirror"], pb["x0"])
    rest = np.setdiff1d(np.arange(82), ocols + tcols)
    err = np.abs(got[:, :, tcols] - want[:, :, tcols]).max()
    print(f"[stack writers] jackal_tmpc: collision columns bitwise equal {np.array_equal(got[:, :, ocols], want[:, :, ocols])}, "
          f"max |topology - mirror| {err:.3e}")
    assert np.array_equal(got[:, :, ocols], want[:, :, ocols])
    np.testing.assert_allclose(got[:, :, tcols], want[:, :, tcols], rtol=1e-14, atol=1e-14)
    assert np.array_equal(got[:, :, rest], start[:, :, rest])
    assert np.array_equal(got[B - 1][:, tcols], np.tile([1.0, 0.0, pb["state"][pb["scene_of"][B - 1], 0] + 100.0], (N, M)))      # the non-guided planner: dummies
    s.close()


# ---- three ticks of the generated jackal stack, every row built on device -------------------------------------------------------------------
TICK_SEEDS = (1, 3)
TICK_COUNTS = [(2, 2), (2, 1), (2, 2)]
TICK_CLASSES = [((0, 1), (3, 2)), ((0, 1), (3, 2)), ((1, 0), (2, 3))]
TICK_NODE_STAGES = ((0, 8, 15, 23, 30), (0, 10, 20, 30))


def test_three_device_resident_ticks_equal_the_host_driven_ticks():
    """jackal_tmpc, 2 scenes x (2 guided + 1 non-guided) planners, 3 ticks.  Handle A: guidance_plan -> warmstart -> sample_guidance ->
    init_with_guidance -> stack.prepare_obstacles -> stack.set_obstacle_columns -> stack.linearize_topology_columns -> solve -> guidance_decide
    on one stream; the collision and topology columns of the rows it was given hold a sentinel.  Handle B (same library): the plan and the
    decision by the mirrors, the warm start read back, the rows built by modules.prepare_obstacles / gaussian_set_parameters /
    linearized_update, uploaded with set_batch.  Each tick the robots move to node 1 of B's selected plans and the obstacles one step on.
    Assertions and tolerances of test_closed_loop_replay_device_state_equals_host_driven_loop (tests/test_gpu_parity.py): equal exit codes,
    trajectories of the successful planners within 1e-9, the selected objectives within 1e-8 relative; a planner of every scene succeeds."""
    import torch
    from mpc_planner_amd import modules as md, scenes, solver
    from mpc_planner_amd.stack_writers import StackWriters, obstacle_columns, topology_columns
    from test_gpu_parity import _generated_lib
    path, meta = _generated_lib("jackal_tmpc")
    N, M, S, Q, n_paths, P, R = 30, 5, 3, 2, 2, 3, 6
    B = Q * P
    pmap = meta["parameter_map"]
    pm = _Map(pmap)
    ocols, tcols = obstacle_columns(pmap, M, 1), topology_columns(pmap, M)
    scs = [scenes.make_scene(seed, N=N, M=M, S=S, B=n_paths, tmpc_pp=True, chance=True) for seed in TICK_SEEDS]
    assert dict(scs[0]["pm"]._params) == pmap
    xinit = np.concatenate([sc["xinit"] for sc in scs])
    base = np.concatenate([sc["params"] for sc in scs])                        # weights and the path window; the rest is rewritten every tick
    blank = base.copy(); blank[:, :, ocols + tcols] = -3.0
    pos0 = np.stack([sc["obstacles"]["pos"][:, 0] for sc in scs])
    vel = np.stack([(sc["obstacles"]["pos"][:, 1] - sc["obstacles"]["pos"][:, 0]) / DT for sc in scs])
    counts_raw = np.array([M, M - 1], np.int32)                               # scene 1: one dummy
    raw_radius = np.full((Q, M), scenes.OBSTACLE_RADIUS)
    scene_of = np.repeat(np.arange(Q, dtype=np.int32), P)
    r, decel, cdt, w_cons = scenes.ROBOT_RADIUS, 3.0, 0.05, 0.8
    kw = dict(use_tmpcpp=True, warmstart_with_mpc_solution=True, shift_previous_solution_forward=True, selection_weight_consistency=w_cons)
    opt = solver.guidance_options(n_paths, **kw)
    base_nodes, node_count = np.full((B, R, 3), -9e9), np.zeros(B, np.int32)
    for q, sc in enumerate(scs):
        for p in range(n_paths):
            st = np.array(TICK_NODE_STAGES[p])
            base_nodes[q * P + p, :len(st)] = np.concatenate([st[:, None] * DT, sc["guidance_pos"][p][st] - xinit[q * P, None, 0:2]], 1)
            node_count[q * P + p] = len(st)
    dims = solver.default_dims(N=N, S=S, lib_path=path)
    A, H = solver.BatchedSolver(dims, B_max=B, lib_path=path), solver.BatchedSolver(dims, B_max=B, lib_path=path)
    W = StackWriters(A)
    i32, u8, f64 = torch.int32, torch.uint8, torch.float64
    x0 = np.full((B, N + 1, 7), -3.0)                                          # every warm start is the device's
    t_xinit, t_x0, t_params = _up(xinit), _up(x0), _up(blank)
    A.set_batch_device(B, t_xinit.data_ptr(), t_x0.data_ptr(), t_params.data_ptr())
    H.set_batch(xinit, x0, blank)
    t_sc, t_cnt_raw, t_rr = _up(scene_of), _up(counts_raw), _up(raw_radius)
    t_ids, t_sel = _full((Q, P), -1, i32), _up(np.tile(np.array([-1, 0, -1], np.int32), (Q, 1)))
    t_mode, t_src, t_gid = _full((B,), -7, i32), _full((B,), -7, i32), _full((B,), -7, i32)
    t_init, t_dummy, t_dis, t_w = _full((B,), 9, u8), _full((B,), 9, u8), _full((B,), 9, u8), _full((B,), -3.0, f64)
    t_gpos, t_gvel, t_status = _full((B, N + 1, 2), -3.0, f64), _full((B, N + 1, 2), -3.0, f64), _full((B,), -7, i32)
    t_best, t_exit, t_cmd = _full((Q,), -7, i32), _full((Q,), -7, i32), _full((Q, 2), -3.0, f64)
    o_pos, o_shape = _full((Q, M, N, 2), -7777.0, f64), _full((Q, M, N, 3), -7777.0, f64)
    o_rad, o_g, o_sel = _full((Q, M), -7777.0, f64), _full((Q, M), 0xEE, u8), _full((Q, M), -99, i32)
    d_pobj, d_code = A.result_device_ptrs()
    hs = torch.cuda.ExternalStream(A.stream_ptr(), device=torch.device("cuda"))
    state = xinit[::P].copy()
    ids, sel = np.full((Q, P), -1, np.int32), np.tile(np.array([-1, 0, -1], np.int32), (Q, 1))
    for tick in range(len(TICK_COUNTS)):
        counts = np.array(TICK_COUNTS[tick], np.int32); classes = np.array(TICK_CLASSES[tick], np.int32)
        stateB = np.repeat(state, P, axis=0)
        raw_pos = pos0 + vel * DT * tick
        nodes = base_nodes.copy(); nodes[:, :, 1:3] += stateB[:, None, 0:2]
        t_cnt, t_cls, t_state, t_stateB, t_state4, t_sx = _up(counts), _up(classes), _up(state), _up(stateB), _up(state[:, :4]), _up(state[:, 0])
        t_rp, t_rv, t_nodes, t_ncnt = _up(raw_pos), _up(vel), _up(nodes), _up(node_count)
        torch.cuda.synchronize()
        # ---- A: one stream, nothing read back before the decision is enqueued
        with torch.cuda.stream(hs):
            A.guidance_plan(Q, opt, t_cnt.data_ptr(), t_cls.data_ptr(), t_ids.data_ptr(), t_sel.data_ptr(), t_mode.data_ptr(), t_src.data_ptr(),
                            t_init.data_ptr(), t_dummy.data_ptr(), t_dis.data_ptr(), t_gid.data_ptr(), t_w.data_ptr())
            A.warmstart(t_stateB.data_ptr(), t_mode.data_ptr(), t_src.data_ptr(), deceleration=decel)
            A.sample_guidance(B, R, t_nodes.data_ptr(), t_ncnt.data_ptr(), t_gpos.data_ptr(), t_gvel.data_ptr(), t_status.data_ptr())
            A.init_with_guidance(t_gpos.data_ptr(), t_gvel.data_ptr(), t_init.data_ptr())
            W.prepare_obstacles(Q, M, M, t_cnt_raw.data_ptr(), t_state4.data_ptr(), t_rp.data_ptr(), t_rr.data_ptr(), o_pos.data_ptr(), o_shape.data_ptr(),
                                o_rad.data_ptr(), o_g.data_ptr(), o_sel.data_ptr(), d_raw_vel=t_rv.data_ptr(), probabilistic=True, propagate_passes=PASSES)
            W.set_obstacle_columns(ocols, 1, M, o_pos.data_ptr(), o_shape.data_ptr(), o_rad.data_ptr(), o_g.data_ptr(), t_sc.data_ptr(), t_state4.data_ptr(),
                                   r, risk=RISK, obstacle_radius=scenes.OBSTACLE_RADIUS)
            W.linearize_topology_columns(tcols, o_pos.data_ptr(), M, t_sc.data_ptr(), t_sx.data_ptr(), r, d_is_original=t_dummy.data_ptr())
            A.solve(sync=False)
            A.guidance_decide(Q, opt, d_pobj, d_code, t_dis.data_ptr(), t_gid.data_ptr(), t_w.data_ptr(), t_state.data_ptr(), t_best.data_ptr(),
                              t_exit.data_ptr(), t_cmd.data_ptr(), t_ids.data_ptr(), t_sel.data_ptr(), deceleration=decel, control_dt=cdt)
        A.synchronize()
        got = A.get()
        best_a = t_best.cpu().numpy()
        # ---- H: the same tick driven from the host
        plan = md.guidance_plan(counts, classes, ids, sel, n_paths, **kw)
        samples = [md.sample_guidance(nodes[b, :node_count[b]], N, dims.dt, n_nodes_max=R) for b in range(B)]
        gpos, gvel = np.stack([sm[0] for sm in samples]), np.stack([sm[1] for sm in samples])
        h_mode, h_src, h_init, h_gpos, h_gvel = _up(plan["mode"]), _up(plan["src"]), _up(plan["init_enabled"]), _up(gpos), _up(gvel)
        torch.cuda.synchronize()
        H.warmstart(t_stateB.data_ptr(), h_mode.data_ptr(), h_src.data_ptr(), deceleration=decel)
        H.init_with_guidance(h_gpos.data_ptr(), h_gvel.data_ptr(), h_init.data_ptr())
        H.synchronize()
        x0_h, xinit_h = H.debug_get_x0()
        obs = [md.prepare_obstacles(state[q, :4], raw_pos[q, :counts_raw[q]], raw_radius[q, :counts_raw[q]], M, N, DT, raw_vel=vel[q, :counts_raw[q]],
                                    probabilistic=True, propagate_passes=PASSES, risk=RISK) for q in range(Q)]
        pb = dict(scene_of=scene_of, M=M, obstacle_radius=scenes.OBSTACLE_RADIUS, robot_radius=r, state=state, is_original=plan["rows_dummy"])

        def rows_from(warm_start):
            out = base.copy()
            _mirror_rows(pm, out, pb, obs, warm_start, disc_offset=0.0)
            return out
        rows = rows_from(x0_h)
        H.set_batch(xinit_h, x0_h, rows); H.solve(); ref = H.get()
        dec = md.guidance_decide(ref["pobj"], ref["exit_code"], plan["disabled"], plan["guidance_id"], plan["weight"], state, ref["xtraj"], ref["utraj"],
                                 ids, sel, n_paths, True, deceleration=decel, control_dt=cdt)
        ids, sel = dec["planner_ids"], dec["selection"]
        # ---- the two ticks agree
        rows_a = A.debug_get_params()
        x0_a, xinit_a = A.debug_get_x0()
        # A's topology rows are linearised around A's OWN warm start: the shift of its previous solution, which equals the host loop's only to
        # the solve's tolerance from the second tick on.  Its rows are held to the mirror fed with that warm start; tick 0 starts from equal inputs
        want_a = rows if tick == 0 else rows_from(x0_a)
        ok = ref["exit_code"] == 1
        print(f"[stack ticks] tick {tick}: exit codes {got['exit_code'].tolist()} (host {ref['exit_code'].tolist()}), best {best_a.tolist()} (host "
              f"{dec['best'].tolist()}), collision columns bitwise equal {np.array_equal(rows_a[:, :, ocols], want_a[:, :, ocols])}, max |topology - mirror| "
              f"{np.abs(rows_a[:, :, tcols] - want_a[:, :, tcols]).max():.3e}, max |warm start - host| {np.abs(x0_a - x0_h).max():.3e}, "
              f"max |x - host| {np.abs(got['xtraj'][ok] - ref['xtraj'][ok]).max() if ok.any() else 0.0:.3e}")
        for k, t in (("mode", t_mode), ("src", t_src), ("init_enabled", t_init), ("rows_dummy", t_dummy), ("disabled", t_dis), ("guidance_id", t_gid)):
            assert np.array_equal(t.cpu().numpy(), plan[k]), (tick, k)
        assert np.array_equal(xinit_a, xinit_h) and (tick > 0 or np.array_equal(x0_a, x0_h))
        assert not (rows_a == -3.0).any()                                     # every blanked column was written on the device
        assert np.array_equal(rows_a[:, :, ocols], want_a[:, :, ocols])
        np.testing.assert_allclose(rows_a[:, :, tcols], want_a[:, :, tcols], rtol=1e-14, atol=1e-14)
        rest = np.setdiff1d(np.arange(dims.npar), ocols + tcols)
        assert np.array_equal(rows_a[:, :, rest], base[:, :, rest])
        assert np.array_equal(got["exit_code"], ref["exit_code"])
        assert ok.reshape(Q, P).any(axis=1).all()                              # at least one planner per scene succeeds
        np.testing.assert_allclose(got["xtraj"][ok], ref["xtraj"][ok], rtol=0, atol=1e-9)
        for q in range(Q):                                                     # planners that tie to rounding: the selected objective, not its carrier
            ba, bh = int(best_a[q]), int(dec["best"][q])
            assert ba >= 0 and bh >= 0
            pa, ph = got["pobj"][q * P + ba] * plan["weight"][q * P + ba], ref["pobj"][q * P + bh] * plan["weight"][q * P + bh]
            assert abs(pa - ph) <= 1e-8 * max(1.0, abs(ph))
            state[q] = ref["xtraj"][q * P + bh, 1]
        t_ids.copy_(_up(ids)); t_sel.copy_(_up(sel))                           # both loops go on from the host's decision
        torch.cuda.synchronize()
    A.close(); H.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_launches_nothing():
    """On the generated jackal_tmpc handle.  Each refusal raises solver.TmpcError with a message that names the argument; after a synchronise the
    rows, the prepared-obstacle outputs and the warm start are what they were.  Then the same calls as they should be: accepted.  The entries of
    tmpc_hip.h keep refusing with "generated solver".  (B x N x max_obstacles beyond 2^31 - 1 needs a batch of 3.9 million entries at N = 30 and
    the 18 obstacles 128 columns allow: not run.)"""
    import torch
    from mpc_planner_amd import solver
    from mpc_planner_amd.stack_writers import StackWriters, obstacle_columns, topology_columns
    from test_gpu_parity import _generated_lib
    path, meta = _generated_lib("jackal_tmpc")
    N, M, B = 30, 5, 4
    pmap = meta["parameter_map"]
    ocols, tcols = obstacle_columns(pmap, M, 1), topology_columns(pmap, M)
    pb = _problem(N, M, (5, 3), B, 7, M, 2, seed=50)
    dims = solver.default_dims(N=N, S=3, lib_path=path)
    s = solver.BatchedSolver(dims, B_max=B, lib_path=path)
    w = StackWriters(s)
    dv = _Device(pb)
    obstacle_args = lambda: [dv.o_pos.data_ptr(), dv.o_shape.data_ptr(), dv.o_radius.data_ptr(), dv.o_gauss.data_ptr(), dv.scene_of.data_ptr(), dv.state.data_ptr()]
    set_cols = lambda cols=ocols, row_model=1, max_obstacles=M, args=None: w.set_obstacle_columns(
        cols, row_model, max_obstacles, *(obstacle_args() if args is None else args), pb["robot_radius"], risk=RISK, obstacle_radius=pb["obstacle_radius"])
    topo = lambda cols=tcols, **kw: w.linearize_topology_columns(cols, **dict(_topology_args(pb, dv, False), **kw))
    # no batch yet: the two column writers refuse, the preparation does not need one
    for call in (set_cols, topo):
        with pytest.raises(solver.TmpcError, match="no batch"):
            call()
    start = _sentinel_rows(B, N, 82)
    s.set_batch(pb["xinit"], pb["x0"], start)
    # ---- tmpc_stack_prepare_obstacles: the checks of tmpc_prepare_obstacles
    prep = dict(n_scenes=pb["Q"], n_slots=pb["R"], max_obstacles=M, d_count=dv.count.data_ptr(), d_state=dv.state.data_ptr(), d_raw_pos=dv.raw_pos.data_ptr(),
                d_raw_radius=dv.raw_radius.data_ptr(), d_obstacle_pos=dv.o_pos.data_ptr(), d_obstacle_shape=dv.o_shape.data_ptr(),
                d_obstacle_radius=dv.o_radius.data_ptr(), d_obstacle_gaussian=dv.o_gauss.data_ptr(), d_selected=dv.o_sel.data_ptr(),
                d_raw_pred=dv.raw_pred.data_ptr(), probabilistic=True)
    bad = [(dict(d_raw_pred=None), "exactly one"), (dict(d_raw_vel=dv.raw_pos.data_ptr()), "exactly one"), (dict(n_slots=1025), "n_slots"), (dict(n_slots=-1), "n_slots"),
           (dict(propagate_passes=3), "propagate_passes"), (dict(n_scenes=0), "n_scenes"), (dict(max_obstacles=0), "max_obstacles"), (dict(max_obstacles=4097), "max_obstacles"),
           (dict(noise=-1.0), "noise")]
    bad += [({k: None}, "NULL input") for k in ("d_count", "d_state", "d_raw_pos", "d_raw_radius")]
    bad += [({k: None}, "NULL output") for k in ("d_obstacle_pos", "d_obstacle_shape", "d_obstacle_radius", "d_obstacle_gaussian", "d_selected")]
    for kw, msg in bad:
        with pytest.raises(solver.TmpcError, match="tmpc_stack_prepare_obstacles.*" + msg):
            w.prepare_obstacles(**dict(prep, **kw))
    opt = solver.TmpcObstacleOptions(8, 0, 0, 0, 0.3, 0.0)                     # an options struct this library cannot honour
    vp = C.c_void_p
    raw_args = [s._h, pb["Q"], pb["R"], M, vp(dv.count.data_ptr()), vp(dv.state.data_ptr()), vp(dv.raw_pos.data_ptr()), vp(dv.raw_radius.data_ptr()), None,
                vp(dv.raw_pred.data_ptr()), C.byref(opt), vp(dv.o_pos.data_ptr()), vp(dv.o_shape.data_ptr()), vp(dv.o_radius.data_ptr()), vp(dv.o_gauss.data_ptr()),
                vp(dv.o_sel.data_ptr())]
    assert s.lib.tmpc_stack_prepare_obstacles(*raw_args) == -1 and b"size" in s.lib.tmpc_last_error(s._h)
    assert s.lib.tmpc_stack_prepare_obstacles(None, *raw_args[1:]) == -1       # no handle
    s.synchronize()
    assert (dv.outputs()[0] == -7777.0).all() and (dv.outputs()[4] == -99).all() and (dv.outputs()[3] == 0xEE).all()
    w.prepare_obstacles(**prep)                                                # the same call as it should be
    s.synchronize()
    assert not (dv.outputs()[0] == -7777.0).any()
    # ---- tmpc_stack_set_obstacle_columns
    npar = dims.npar
    bad = [(lambda: set_cols(None), "NULL argument"), (lambda: set_cols(row_model=2), "row_model"), (lambda: set_cols(row_model=-1), "row_model"),
           (lambda: set_cols(max_obstacles=0), "max_obstacles"), (lambda: set_cols(max_obstacles=-3), "max_obstacles"),
           (lambda: set_cols(ocols[:-1]), "n_cols"), (lambda: set_cols(ocols + [0]), "n_cols"), (lambda: set_cols(row_model=0), "n_cols"),
           (lambda: set_cols(max_obstacles=M + 1), "n_cols"), (lambda: set_cols(list(range(2 + 6 * 22)), max_obstacles=22), "n_cols"),       # 134 columns: beyond the 128 of the table
           (lambda: set_cols(ocols[:-1] + [npar]), "outside"), (lambda: set_cols([-1] + ocols[1:]), "outside"),
           (lambda: set_cols(ocols[:-1] + [ocols[3]]), "duplicate")]
    for i in range(6):
        args = obstacle_args(); args[i] = None
        bad.append((lambda args=args: set_cols(args=args), "NULL argument"))
    for call, msg in bad:
        with pytest.raises(solver.TmpcError, match="tmpc_stack_set_obstacle_columns.*" + msg):
            call()
    # ---- tmpc_stack_linearize_topology_columns
    bad = [(lambda: topo(None), "n_rows"), (lambda: topo([]), "n_rows"), (lambda: topo(list(range(129))), "n_rows"),
           (lambda: topo(d_scene_of=None), "NULL argument"), (lambda: topo(d_state_x=None), "NULL argument"),
           (lambda: topo(n_obstacles=M + 1, n_static=0), "more obstacle"), (lambda: topo(n_obstacles=M - 1, n_static=2), "more obstacle"),
           (lambda: topo(n_obstacles=-1, n_static=0), "more obstacle"), (lambda: topo(n_obstacles=M, n_static=-1), "more obstacle"),
           (lambda: topo(n_obstacles=3, n_static=0, d_obstacle_pos=None), "NULL d_obstacle_pos"),
           (lambda: topo(n_obstacles=3, n_static=2, d_static_halfspaces=None), "NULL d_static_halfspaces"),
           (lambda: topo(tcols[:-1] + [npar], n_static=0), "outside"), (lambda: topo([-2] + tcols[1:], n_static=0), "outside"),
           (lambda: topo(tcols[:-1] + [tcols[0]], n_static=0), "duplicate")]
    for call, msg in bad:
        with pytest.raises(solver.TmpcError, match="tmpc_stack_linearize_topology_columns.*" + msg):
            call()
    with pytest.raises(ValueError, match="multiple of 3"):
        topo(tcols[:-1])
    null = C.c_void_p()
    assert s.lib.tmpc_stack_set_obstacle_columns(null, None, 32, 1, 5, *([null] * 6), 0.3, 0.0, 0.05, 6.0, 0.4) == -1
    assert s.lib.tmpc_stack_linearize_topology_columns(null, None, 5, null, 5, null, null, 0, null, null, 0.3, null) == -1
    s.synchronize()
    assert np.array_equal(s.debug_get_params(), start)                        # none of the refused calls wrote a row
    x0_now, _ = s.debug_get_x0()
    assert np.array_equal(x0_now, pb["x0"])
    # ---- accepted: 3 obstacle rows + 2 static rows in the stack's 5 topology rows; 128 columns are the limit, not beyond it
    set_cols(); topo(n_obstacles=3, n_static=2)
    s.synchronize()
    got = s.debug_get_params()
    assert (got[:, :, ocols + tcols] != start[:, :, ocols + tcols]).all()
    want_static = pb["static"][pb["scene_of"][0], 1:, :, :]                   # entry 0, stages 1 .. N - 1, rows 3 and 4
    assert np.array_equal(got[0, 1:][:, tcols[9:15]].reshape(N - 1, 2, 3), want_static)
    # ---- tmpc_hip.h's entries keep refusing in a generated solver
    with pytest.raises(solver.TmpcError, match="generated solver"):
        s.prepare_obstacles(**prep)
    with pytest.raises(solver.TmpcError, match="generated solver"):
        s.set_obstacle_parameters(*obstacle_args(), pb["robot_radius"])
    with pytest.raises(solver.TmpcError, match="generated solver"):
        s.linearize_topology_ex(**_topology_args(pb, dv, False))
    with pytest.raises(solver.TmpcError, match="generated solver"):
        s.linearize_topology(dv.o_pos.data_ptr(), dv.scene_of.data_ptr(), dv.state_x.data_ptr(), pb["robot_radius"])
    s.synchronize()
    assert np.array_equal(s.debug_get_params(), got)
    s.close()
