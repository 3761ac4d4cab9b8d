"""GPU: the free-space decomposition on device (tmpc_costmap_points, tmpc_decomp_halfspaces, tmpc_set_halfspace_rows; csrc/tmpc_aux_kernels.hpp)
-- what DecompConstraints::update and setParameters (decomp_constraints.cpp:52-189) do; DESIGN.md U16.  The kernels against the host mirror
(mpc_planner_amd/modules.py, pinned on hand values and geometric properties in tests/test_free_space.py) bit for bit; then the chain fit_path ->
track_path -> set_path_parameters -> costmap_points -> decomp_halfspaces -> set_halfspace_rows -> solve on device against the mirrors on the
host.  Every output buffer is prefilled (-3.0, count -3, status 7), so what a kernel leaves alone shows."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
S, M = 5, 8
DIMS = {"nx5": dict(N=20, S=S, n_lin=M, M=M), "slack": dict(N=20, S=S, n_lin=M, M=M, n_slk=12, slack=1)}
# the mirror's statuses of the bitwise launch (tests/free_space_cases.py), stage 0 .. 19 per scene: what the cases are meant to reach
S0, S1, S2, S7 = [0] * 20, [0] + [1] * 19, [0] + [2] * 19, [7] * 20


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda"))


def _decomp_on_device(s, case):
    """One launch of tmpc_decomp_halfspaces on the current batch into prefilled buffers; keyed like free_space_cases.mirror."""
    import torch
    import free_space_cases as fs
    dev = torch.device("cuda")
    Q, N, R = len(case["count"]), case["N"], case["n_rows"]
    t = {k: _up(case[k]) for k in ("main_of", "path", "path_count", "path_length", "s0", "state_x", "points", "count")}
    t_rows = torch.full((Q, N, R, 3), fs.PREFILL, dtype=torch.float64, device=dev)
    t_cnt = torch.full((Q, N), -3, dtype=torch.int32, device=dev); t_st = torch.full((Q, N), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    s.decomp_halfspaces(t["main_of"].data_ptr(), Q, case["n_seg_max"], t["path"].data_ptr(), t["path_count"].data_ptr(), t["path_length"].data_ptr(),
                        t["s0"].data_ptr(), t["state_x"].data_ptr(), t["points"].data_ptr(), t["count"].data_ptr(), case["n_pts_max"], case["range"], R,
                        t_rows.data_ptr(), t_cnt.data_ptr(), t_st.data_ptr())
    s.synchronize()
    return dict(rows=t_rows.cpu().numpy(), count=t_cnt.cpu().numpy(), status=t_st.cpu().numpy())


def _batch_for(s, case):
    import free_space_cases as fs
    Q = len(case["count"])
    s.set_batch(np.zeros((Q, s.dims.nx)), fs.x0_of(case, s.dims.nvar), np.zeros((Q, case["N"], s.dims.npar)))


def _compare(tag, got, want):
    for key in ("count", "status", "rows"):
        err = np.abs(got[key].astype(float) - want[key].astype(float)).max()
        print(f"[free space] {tag} {key}: max |device - mirror| = {err:.3e}, bitwise equal: {np.array_equal(got[key], want[key])}")
    for key in ("count", "status", "rows"):
        assert np.array_equal(got[key], want[key]), (tag, key)


@pytest.mark.parametrize("model", ["nx5", "slack"])
def test_device_decomposition_equals_the_mirror_bitwise(model):
    """The bitwise launch (fourteen scenes, n_pts_max = 1100: counts 0, 1, 63, 64, 65, 257, 1100, 2000 clipped, points outside every box, a ring
    that truncates, v = 0, a polyline past the path's end, main_of = -1, path count 0) and a scattered launch (400 points around fast
    segments: the shrink loop runs): rows, counts and statuses np.array_equal the mirror's; both warm-start strides."""
    import free_space_cases as fs
    from mpc_planner_amd import solver
    case, want = fs.bitwise_launch(), fs.bitwise_mirror()
    assert want["status"].tolist() == [S0, S0, S0, S0, S0, S0, S0, S0, S0, S1, S2, S0, S7, S7]
    s = solver.BatchedSolver(solver.default_dims(**DIMS[model]), B_max=16)
    _batch_for(s, case)
    got = _decomp_on_device(s, case)
    _compare("bitwise launch", got, want)
    for q in (fs.NO_MAIN, fs.NO_PATH):                                   # untouched scenes keep the prefill
        assert (got["rows"][q] == fs.PREFILL).all() and (got["count"][q] == -3).all() and (got["status"][q] == 7).all()
    assert (got["rows"][:fs.NO_MAIN] != fs.PREFILL).all()                # every entry of a processed scene is written, dummies included
    case, want = fs.scattered_launch(8), fs.scattered_mirror(8)
    assert want["count"].max() >= 8 and (want["status"][:, 1:] == 0).mean() > 0.9
    _batch_for(s, case)
    _compare("scattered launch", _decomp_on_device(s, case), want)
    s.close()


def _points_on_device(s, cost, origin, resolution, n_pts_max):
    import torch
    import free_space_cases as fs
    dev = torch.device("cuda")
    Q, size_y, size_x = cost.shape
    t_cost, t_org = _up(cost), _up(np.asarray(origin, float))
    t_pts = torch.full((Q, n_pts_max, 2), fs.PREFILL, dtype=torch.float64, device=dev)
    t_cnt = torch.full((Q,), -3, dtype=torch.int32, device=dev); t_ov = torch.full((Q,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    s.costmap_points(Q, size_x, size_y, t_cost.data_ptr(), t_org.data_ptr(), resolution, n_pts_max, t_pts.data_ptr(), t_cnt.data_ptr(), t_ov.data_ptr())
    s.synchronize()
    return t_pts.cpu().numpy(), t_cnt.cpu().numpy(), t_ov.cpu().numpy()


def _check_points(cost, origin, resolution, n_pts_max, got):
    import free_space_cases as fs
    from mpc_planner_amd import modules as md
    pts, cnt, ov = got
    for q in range(len(cost)):
        want, c, o = md.costmap_points(cost[q], origin[q], resolution, n_pts_max)
        assert cnt[q] == c and ov[q] == int(o), (q, cnt[q], c, ov[q], o)
        assert np.array_equal(pts[q, :c], want), q
        assert (pts[q, c:] == fs.PREFILL).all(), q                       # entries at or beyond count are not touched


def test_costmap_points_equal_the_mirror_bitwise():
    """A 100 x 100 corridor map (scenes.with_costmap) next to an empty one; 128 x 128 all occupied: exactly 16384 points, no overflow;
    130 x 130 all occupied: 16384 points and overflow; a 53 x 37 map with costs of every value, clipped at 100 points and not."""
    import free_space_cases as fs
    from mpc_planner_amd import solver
    s = solver.BatchedSolver(solver.default_dims(**DIMS["nx5"]), B_max=4)          # no batch: the stream only
    sc = fs.corridor_scene(5)
    cost = np.stack([sc["costmap"], np.zeros_like(sc["costmap"]), fs.corridor_scene(6)["costmap"]])
    origin = np.array([sc["costmap_origin"], [1.0, 2.0], fs.corridor_scene(6)["costmap_origin"]])
    got = _points_on_device(s, cost, origin, 0.1, 4096)
    _check_points(cost, origin, 0.1, 4096, got)
    assert got[1][0] > 300 and got[1][1] == 0 and got[2][1] == 0 and (got[0][1] == fs.PREFILL).all()
    for size, overflow in ((128, 0), (130, 1)):
        full = np.full((1, size, size), 254, np.uint8)
        pts, cnt, ov = _points_on_device(s, full, np.zeros((1, 2)), 0.05, 16384)
        assert cnt[0] == 16384 and ov[0] == overflow
        _check_points(full, np.zeros((1, 2)), 0.05, 16384, (pts, cnt, ov))
    rng = np.random.default_rng(3)
    odd = np.where(rng.uniform(size=(2, 37, 53)) < 0.2, rng.integers(1, 256, (2, 37, 53)), 0).astype(np.uint8)
    org = np.array([[-3.25, 7.5], [0.5, -0.25]])
    for cap in (100, 2000):
        _check_points(odd, org, 0.05, cap, _points_on_device(s, odd, org, 0.05, cap))
    s.close()


def test_set_halfspace_rows_equals_the_host_writer():
    """Rows of two scenes of the bitwise launch into a slack-model batch of six entries, two of them naming no scene: the parameters read
    back equal modules.halfspace_rows_set_parameters' everywhere; then first_row = 4, n_rows = 8: rows 0 - 3 keep the prefill."""
    import free_space_cases as fs
    from mpc_planner_amd import solver, modules as md
    from mpc_planner_amd.parameters import define_parameters
    want = fs.bitwise_mirror()
    pick = [5, 6]
    rows, cnt = want["rows"][pick], want["count"][pick]
    state_x = fs.bitwise_launch()["state_x"][pick]
    dims = solver.default_dims(**DIMS["slack"])
    pm = define_parameters(S, M, guidance=True, slack=True, ellipsoids=True, n_decomp=12)
    assert pm.length() == dims.npar
    scene_of = np.array([0, 1, 0, 1, -1, 2], np.int32)
    B, N = len(scene_of), 20
    p0 = np.full((B, N, dims.npar), fs.PREFILL)
    s = solver.BatchedSolver(dims, B_max=B)
    t_rows, t_sc = _up(rows), _up(scene_of)

    def write(first_row, n_rows, t_r):
        s.set_batch(np.zeros((B, dims.nx)), np.zeros((B, N + 1, dims.nvar)), p0)
        s.set_halfspace_rows(t_r.data_ptr(), n_rows, t_sc.data_ptr(), 2, first_row=first_row, disc_offset=0.125)
        s.synchronize()
        return s.debug_get_params()

    got = write(0, 12, t_rows)
    host = p0.copy()
    live = np.arange(12)[None, None, :] < cnt[:, :, None]
    for b, sc in enumerate(scene_of):
        if 0 <= sc < 2:
            nan_form = tuple(np.where(live[sc], rows[sc][:, :, w], np.nan) for w in range(3))
            md.halfspace_rows_set_parameters(pm, host[b], state_x[sc], nan_form, "disc_0_decomp", 12, disc_offset=0.125)
    assert np.array_equal(got, host)
    assert (got[4] == fs.PREFILL).all() and (got[5] == fs.PREFILL).all()  # an entry with an out-of-range scene is untouched
    sub = np.ascontiguousarray(rows[:, :, :8, :])
    got = write(4, 8, _up(sub))
    off = pm.index("ego_disc_0_offset")
    for b, sc in enumerate(scene_of[:4]):
        for j in range(12):
            ia = [pm.index(f"disc_0_decomp_{j}_{f}") for f in ("a1", "a2", "b")]
            assert np.array_equal(got[b][:, ia], sub[sc][:, j - 4, :]) if j >= 4 else (got[b][:, ia] == fs.PREFILL).all(), (b, j)
        assert (got[b][:, off] == 0.125).all()
    mask = np.ones(dims.npar, bool)
    mask[[pm.index(f"disc_0_decomp_{j}_{f}") for j in range(4, 12) for f in ("a1", "a2", "b")] + [off]] = False
    assert (got[:, :, mask] == fs.PREFILL).all()
    s.close()


# chosen on the CPU, with the mirror's rows solved by the oracle (tests/oracle_lib.py) over scenes 0 - 9: in scene 5 all 16 trajectories succeed and the
# tightest decomp row of a solution sits at a.p - b = -1.8e-8
CHAIN_SCENE = 5


@functools.lru_cache(maxsize=None)
def _chain():
    """fit_path -> track_path -> set_path_parameters -> costmap_points -> decomp_halfspaces -> set_halfspace_rows -> solve on device, nothing
    read back in between, and the same from the mirrors on the host, solved on a second handle.  One make_scene batch of 16 trajectories of
    the slack model with 12 decomp rows on its costmap; the waypoints are 25 points on the scene's own reference cubics, from 3 m behind the
    robot on, so the path parameter at the robot is about 3: the spline entry of xinit becomes the mirror's closest_s and the spline column of
    the warm start is advanced by it -- the same arrays for both handles."""
    import torch
    import free_space_cases as fs
    from mpc_planner_amd import scenes, solver, modules as md
    B, N = 16, fs.N
    sc = fs.corridor_scene(CHAIN_SCENE, n_traj=B)
    seg = sc["segments"]
    length0 = float(seg[-1, 8] + (seg[-1, 8] - seg[-2, 8]))
    ss = np.linspace(-3.0, length0, 25)
    xy = np.array([md._road_segment_eval(seg[:, :8], seg[:, 8], float(v))[:2] for v in ss])
    pos = sc["xinit"][0, :2]
    pm = sc["pm"]
    spl = [pm.index(n.format(i)) for i in range(S) for n in ("spline_x{}_a", "spline_x{}_b", "spline_x{}_c", "spline_x{}_d",
                                                              "spline_y{}_a", "spline_y{}_b", "spline_y{}_c", "spline_y{}_d", "spline{}_start")]
    dec = [pm.index(f"disc_0_decomp_{j}_{f}") for j in range(fs.N_ROWS) for f in ("a1", "a2", "b")]
    cm, org, res = sc["costmap"], sc["costmap_origin"], sc["costmap_resolution"]
    P_MAX = 4096
    # ---- host: the mirrors ----
    fit = md.fit_path(xy)
    tr = md.track_path(fit["path"], fit["length"], pos, S, segment=-1)
    xinit, x0 = sc["xinit"].copy(), sc["x0"].copy()
    xinit[:, 4] = tr["s"]; x0[:, :, md.IDX["spline"]] += tr["s"]
    pts, n_pts, overflow = md.costmap_points(cm, org, res, P_MAX)
    dc = md.decomp_halfspaces(fit["path"], fit["length"], tr["s"], x0[0, :N, md.IDX["v"]], scenes.DT, pts, fs.RANGE, fs.N_ROWS, xinit[0, 0])
    host = sc["params"].copy()
    for b in range(B):
        md.contouring_set_parameters(pm, host[b], scenes.WEIGHTS, tr["window"])
        md.halfspace_rows_set_parameters(pm, host[b], xinit[0, 0], (dc["a1"], dc["a2"], dc["b"]), "disc_0_decomp", fs.N_ROWS)
    dims = solver.default_dims(**DIMS["slack"])
    assert dims.npar == pm.length()
    ref_s = solver.BatchedSolver(dims, B_max=B)
    ref_s.set_batch(xinit, x0, host); ref_s.solve(); ref = ref_s.get()
    ref_s.close()
    # ---- device ----
    dev = torch.device("cuda")
    f64 = dict(dtype=torch.float64, device=dev); i32 = dict(dtype=torch.int32, device=dev)
    s = solver.BatchedSolver(dims, B_max=B)
    p0 = sc["params"].copy(); p0[:, :, spl + dec] = -3.0                  # the spline and decomp columns have to come from the device
    s.set_batch(xinit, x0, p0)
    P, R = 32, 40
    t_xy = torch.zeros((1, P, 2), **f64); t_xy[0, :25] = _up(xy)
    t_n = torch.full((1,), 25, **i32)
    t_path = torch.zeros((1, R, 9), **f64); t_pc = torch.zeros(1, **i32); t_len = torch.zeros(1, **f64)
    t_pos = _up(pos.copy().reshape(1, 2)); t_seg = torch.full((1,), -1, **i32); t_cs = torch.zeros(1, **f64)
    t_win = torch.zeros((1, S, 9), **f64)
    t_sc = torch.zeros(B, **i32); t_main = torch.zeros(1, **i32)
    t_cost = _up(cm[None]); t_org = _up(org.reshape(1, 2)); t_sx = _up(xinit[:1, 0].copy())
    t_pts = torch.full((1, P_MAX, 2), -3.0, **f64); t_np = torch.zeros(1, **i32); t_ov = torch.zeros(1, dtype=torch.uint8, device=dev)
    t_rows = torch.full((1, N, fs.N_ROWS, 3), -3.0, **f64); t_rc = torch.full((1, N), -3, **i32)
    t_st = torch.full((1, N), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    s.fit_path(1, P, R, t_xy.data_ptr(), t_n.data_ptr(), t_path.data_ptr(), t_pc.data_ptr(), t_len.data_ptr())
    s.track_path(1, R, t_path.data_ptr(), t_pc.data_ptr(), t_len.data_ptr(), t_pos.data_ptr(), 2, t_seg.data_ptr(), t_cs.data_ptr(), t_win.data_ptr())
    s.set_path_parameters(t_win.data_ptr(), t_sc.data_ptr(), 1)
    s.costmap_points(1, cm.shape[1], cm.shape[0], t_cost.data_ptr(), t_org.data_ptr(), res, P_MAX, t_pts.data_ptr(), t_np.data_ptr(), t_ov.data_ptr())
    s.decomp_halfspaces(t_main.data_ptr(), 1, R, t_path.data_ptr(), t_pc.data_ptr(), t_len.data_ptr(), t_cs.data_ptr(), t_sx.data_ptr(), t_pts.data_ptr(),
                        t_np.data_ptr(), P_MAX, fs.RANGE, fs.N_ROWS, t_rows.data_ptr(), t_rc.data_ptr(), t_st.data_ptr())
    s.set_halfspace_rows(t_rows.data_ptr(), fs.N_ROWS, t_sc.data_ptr(), 1)
    s.solve(sync=False)
    s.synchronize()
    out = dict(dc=dc, host=host, ref=ref, got=s.get(), p_dev=s.debug_get_params(), n_pts=n_pts, overflow=overflow, n_dev=int(t_np.item()),
               ov_dev=int(t_ov.item()), pts=pts, pts_dev=t_pts.cpu().numpy()[0], rows_dev=t_rows.cpu().numpy()[0], rc_dev=t_rc.cpu().numpy()[0],
               st_dev=t_st.cpu().numpy()[0], dec=dec, pm=pm)
    s.close()
    return out


def test_chain_costmap_to_solve_equals_the_host_mirrors():
    """Points, rows, counts, statuses and the written columns np.array_equal the mirrors'; then the solve on the device-built rows equals the
    solve on the host-built rows: every integer, and floats bitwise.  At least one trajectory succeeds, and at least one decomp row that is
    not a dummy is active or nearly so at a solution, so the rows are known to matter."""
    import free_space_cases as fs
    c = _chain()
    dc = c["dc"]
    assert c["n_dev"] == c["n_pts"] > 300 and not c["overflow"] and c["ov_dev"] == 0
    assert np.array_equal(c["pts_dev"][:c["n_pts"]], c["pts"])
    assert np.array_equal(c["rows_dev"], dc["rows"]) and np.array_equal(c["rc_dev"], dc["count"]) and np.array_equal(c["st_dev"], dc["status"])
    assert (dc["status"] == 0).all() and (dc["count"][1:] > 4).any()
    assert np.array_equal(c["p_dev"], c["host"])                          # the decomp columns, the spline columns, and nothing else moved
    got, ref = c["got"], c["ref"]
    print(f"[free space chain] {c['n_pts']} points, rows per stage {dc['count'].tolist()}, exit codes {got['exit_code'].tolist()}")
    assert (ref["exit_code"] == 1).any()
    assert sorted(got) == sorted(ref)
    for key in ref:
        a, b = np.asarray(got[key]), np.asarray(ref[key])
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), key
    worst = -np.inf
    for b in np.nonzero(ref["exit_code"] == 1)[0]:
        for k in range(1, fs.N):
            n = dc["count"][k]
            x, y = ref["xtraj"][b, k, 0], ref["xtraj"][b, k, 1]
            worst = max(worst, (dc["rows"][k, :n, 0] * x + dc["rows"][k, :n, 1] * y - dc["rows"][k, :n, 2]).max())
    print(f"[free space chain] largest a.p - b over the decomp rows of the successful trajectories: {worst:.3e}")
    assert worst >= -1e-2


def test_contract_errors_launch_nothing():
    import torch
    import free_space_cases as fs
    from mpc_planner_amd import solver
    dev = torch.device("cuda")
    f64 = dict(dtype=torch.float64, device=dev); i32 = dict(dtype=torch.int32, device=dev)
    s = solver.BatchedSolver(solver.default_dims(**DIMS["slack"]), B_max=4)
    N, R, P = 20, 12, 8
    # tmpc_costmap_points (needs no batch)
    t_cost = torch.ones((1, 4, 4), dtype=torch.uint8, device=dev); t_org = torch.zeros((1, 2), **f64)
    t_pts = torch.full((1, P, 2), -3.0, **f64); t_n = torch.full((1,), -3, **i32)
    base = dict(n_scenes=1, size_x=4, size_y=4, d_cost=t_cost.data_ptr(), d_origin=t_org.data_ptr(), resolution=0.1, n_pts_max=P,
                d_points=t_pts.data_ptr(), d_count=t_n.data_ptr())
    for kw, msg in ((dict(n_scenes=0), "n_scenes"), (dict(size_x=0), "size_x"), (dict(size_x=1025, size_y=1024), "2\\^20"), (dict(n_pts_max=0), "n_pts_max"),
                    (dict(n_pts_max=16385), "n_pts_max"), (dict(d_cost=None), "NULL input"), (dict(d_origin=None), "NULL input"),
                    (dict(d_points=None), "NULL output"), (dict(d_count=None), "NULL output")):
        with pytest.raises(solver.TmpcError, match=msg):
            s.costmap_points(**dict(base, **kw))
    s.synchronize()
    assert (t_pts == -3.0).all() and t_n.item() == -3                      # nothing ran
    assert s.lib.tmpc_costmap_points(None, 1, 4, 4, None, None, 0.1, P, None, None, None) == -1
    # tmpc_decomp_halfspaces and tmpc_set_halfspace_rows need a batch
    t_main = torch.zeros(1, **i32); t_path = torch.zeros((1, 4, 9), **f64); t_pc = torch.ones(1, **i32); t_len = torch.ones(1, **f64)
    t_s0 = torch.zeros(1, **f64); t_sx = torch.zeros(1, **f64)
    t_rows = torch.full((1, N, R, 3), -3.0, **f64); t_rc = torch.full((1, N), -3, **i32); t_st = torch.full((1, N), 7, dtype=torch.uint8, device=dev)
    dbase = dict(d_main_of=t_main.data_ptr(), n_scenes=1, n_seg_max=4, d_path=t_path.data_ptr(), d_path_count=t_pc.data_ptr(),
                 d_path_length=t_len.data_ptr(), d_s0=t_s0.data_ptr(), d_state_x=t_sx.data_ptr(), d_points=t_pts.data_ptr(), d_count=t_n.data_ptr(),
                 n_pts_max=P, decomp_range=2.0, n_rows=R, d_rows=t_rows.data_ptr(), d_row_count=t_rc.data_ptr(), d_status=t_st.data_ptr())
    t_sc = torch.zeros(4, **i32)
    with pytest.raises(solver.TmpcError, match="no batch"):
        s.decomp_halfspaces(**dbase)
    with pytest.raises(solver.TmpcError, match="no batch"):
        s.set_halfspace_rows(t_rows.data_ptr(), R, t_sc.data_ptr(), 1)
    p0 = np.full((4, N, s.dims.npar), -3.0)
    s.set_batch(np.zeros((4, s.dims.nx)), np.zeros((4, N + 1, s.dims.nvar)), p0)
    for kw, msg in ((dict(n_scenes=0), "n_scenes"), (dict(n_seg_max=0), "n_seg_max"), (dict(n_seg_max=1025), "n_seg_max"), (dict(n_pts_max=0), "n_pts_max"),
                    (dict(n_pts_max=16385), "n_pts_max"), (dict(n_rows=0), "n_rows"), (dict(n_rows=65), "n_rows"), (dict(decomp_range=-1.0), "range"),
                    (dict(decomp_range=float("nan")), "range"), (dict(decomp_range=float("inf")), "range"))\
            + tuple((dict({k: None}), "NULL input") for k in ("d_main_of", "d_path", "d_path_count", "d_path_length", "d_s0", "d_state_x", "d_points", "d_count"))\
            + tuple((dict({k: None}), "NULL output") for k in ("d_rows", "d_row_count", "d_status")):
        with pytest.raises(solver.TmpcError, match=msg):
            s.decomp_halfspaces(**dict(dbase, **kw))
    for args, kw, msg in (((None, R, t_sc.data_ptr(), 1), {}, "bad argument"), ((t_rows.data_ptr(), R, None, 1), {}, "bad argument"),
                          ((t_rows.data_ptr(), R, t_sc.data_ptr(), 0), {}, "bad argument"), ((t_rows.data_ptr(), 0, t_sc.data_ptr(), 1), {}, "do not fit"),
                          ((t_rows.data_ptr(), R, t_sc.data_ptr(), 1), dict(first_row=1), "do not fit"),
                          ((t_rows.data_ptr(), 8, t_sc.data_ptr(), 1), dict(first_row=-1), "do not fit"),
                          ((t_rows.data_ptr(), 13, t_sc.data_ptr(), 1), {}, "do not fit")):
        with pytest.raises(solver.TmpcError, match=msg):
            s.set_halfspace_rows(*args, **kw)
    s.synchronize()
    assert (t_rows == -3.0).all() and (t_rc == -3).all() and (t_st == 7).all() and np.array_equal(s.debug_get_params(), p0)      # nothing ran
    assert s.lib.tmpc_decomp_halfspaces(None, None, 1, 4, *([None] * 7), P, 2.0, R, None, None, None) == -1
    assert s.lib.tmpc_set_halfspace_rows(None, None, R, 0, None, 1, 0.0) == -1
    s.close()
    s5 = solver.BatchedSolver(solver.default_dims(**DIMS["nx5"]), B_max=4)  # a problem without slack rows has nowhere to put them
    s5.set_batch(np.zeros((4, 5)), np.zeros((4, N + 1, 7)), np.zeros((4, N, s5.dims.npar)))
    with pytest.raises(solver.TmpcError, match="do not fit"):
        s5.set_halfspace_rows(t_rows.data_ptr(), R, t_sc.data_ptr(), 1)
    s5.close()
