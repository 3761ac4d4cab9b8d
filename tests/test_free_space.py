"""CPU: the free-space decomposition's host mirror (mpc_planner_amd/modules.py costmap_points, decomp_path_points, decomp_segment,
decomp_halfspaces) -- what tmpc_costmap_points / tmpc_decomp_halfspaces and mpc_planner_modules/free_space.h are held to bit for
bit (tests/test_gpu_free_space.py, tests/test_cpp_free_space.py).  DecompUtil is not in the reference tree, so the mirror itself is pinned on
hand values and on the geometric properties any correct decomposition has; parity with the reference's own DecompUtil is not pinned."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from mpc_planner_amd import modules as md                                # noqa: E402
import free_space_cases as fs                                           # noqa: E402

P1, P2 = (0.0, 0.0), (2.0, 0.0)
BOX = [(0.0, -1.0, 2.0), (0.0, 1.0, 2.0), (1.0, 0.0, 4.0), (-1.0, 0.0, 2.0)]
DUMMY = (1.0, 0.0, 100.0)


def _seg(points, n_rows=12):
    return md.decomp_segment(P1, P2, np.array(points, float).reshape(-1, 2), 2.0, n_rows)


def _expect(got, rows, status, n_rows=12):
    out, count, st = got
    assert count == len(rows) and st == status
    for i in range(n_rows):
        assert tuple(out[i]) == (tuple(rows[i]) if i < count else DUMMY), (i, out[i])      # `==`: signed zeros may differ


def test_hand_values_of_one_segment():
    """R = 2, n_rows = 12, segment (0, 0) -> (2, 0): e = (1, 0), h = (0, -1), c = (1, 0), f = 1."""
    _expect(_seg([(1, 0.5)]), [(0, 1, 0.5)] + BOX, 0)
    _expect(_seg([(1, 0.5), (1, -0.25), (3, 1)]), [(0, -1, 0.25), (0, 1, 0.5)] + BOX, 0)
    _expect(_seg([(10, 10)]), BOX, 0)
    _expect(_seg([]), BOX, 0)
    _expect(_seg([(1, 0.5), (1, 0.5), (1, -0.5)]), [(0, 1, 0.5), (0, -1, 0.5)] + BOX, 0)       # the duplicate is removed with its twin
    _expect(_seg([(np.nan, 0.3), (1, 0.5)]), [(0, 1, 0.5)] + BOX, 0)                           # a NaN point is in no box


def test_degenerate_segments_are_reported():
    """A point on the segment makes a NaN row, which ends the copy at row 0 like the reference's (:98); p1 == p2 has no frame at all."""
    _expect(_seg([(1, 0)]), [], 2)
    _expect(_seg([(0, 0)]), [], 2)
    assert md.decomp_segment(P1, P1, np.array([[1.0, 0.5]]), 2.0, 12)[1:] == (0, 2)
    assert md.decomp_segment(P1, (np.nan, 0.0), np.zeros((0, 2)), 2.0, 12)[1:] == (0, 2)
    assert md.decomp_segment(P1, (np.inf, 0.0), np.zeros((0, 2)), 2.0, 12)[1:] == (0, 2)


def test_truncation_is_reported():
    ang = 2.0 * np.pi * np.arange(40) / 40.0
    ring = np.stack([1.0 + 1.5 * np.cos(ang), 1.5 * np.sin(ang)], 1)
    out, count, status = md.decomp_segment(P1, P2, ring, 2.0, 12)
    assert (count, status) == (12, 1)
    out6, count6, status6 = md.decomp_segment(P1, P2, ring, 2.0, 6)
    assert (count6, status6) == (6, 1) and np.array_equal(out6, out[:6])
    nrm = np.hypot(out[:, 0], out[:, 1])
    assert np.abs(nrm - 1.0).max() <= 1e-12


def test_argmin_rule_lowest_index_wins_and_nan_is_last():
    key = np.array([3.0, np.nan, 1.0, 1.0, np.inf])
    assert md._decomp_argmin(key, np.array([0, 1, 2, 3, 4])) == 2
    assert md._decomp_argmin(key, np.array([1, 4])) == 1                  # NaN counts as +inf: equal keys, the lower index
    assert md._decomp_argmin(key, np.array([4, 1][::-1])) == 1


def test_path_points_follow_the_cubics_and_continue_straight():
    fit = fs.fitted_path()
    path, length = fit["path"], fit["length"]
    pts, s = md.decomp_path_points(path, length, 1.0, [1.0, 2.0, 100.0, 1.0, 1.0], 0.2)
    assert s.tolist() == [1.0, 1.0 + 1.0 * 0.2, (1.0 + 1.0 * 0.2) + 2.0 * 0.2, ((1.0 + 1.0 * 0.2) + 2.0 * 0.2) + 100.0 * 0.2, (((1.0 + 1.0 * 0.2) + 2.0 * 0.2) + 100.0 * 0.2) + 0.2]
    for k in range(3):
        assert tuple(pts[k]) == tuple(md._road_segment_eval(path[:, :8], path[:, 8], s[k])[:2])
    ex, ey, edx, edy = md._path_end(path, length - path[-1, 8])
    assert tuple(pts[3]) == (ex + (s[3] - length) * edx, ey + (s[3] - length) * edy)
    assert abs(np.hypot(*(pts[4] - pts[3])) - 0.2 * np.hypot(edx, edy)) < 1e-12     # a straight line along the end tangent
    below, _ = md.decomp_path_points(path, length, -0.5, [0.0], 0.2)                 # below the first knot: the first cubic continued
    assert tuple(below[0]) == tuple(md._path_cubic(path[0, :8], -0.5)[:2])
    at_end, _ = md.decomp_path_points(path, length, length, [0.0], 0.2)
    assert tuple(at_end[0]) == (ex, ey)


def test_the_cases_are_what_they_are_meant_to_be():
    """The statuses of the bitwise launch, the literal list tests/test_gpu_free_space.py asserts too; the scattered launch runs the shrink loop."""
    want = fs.bitwise_mirror()
    st = want["status"]
    assert (st[:, 0] == np.where(np.isin(np.arange(len(st)), (fs.NO_MAIN, fs.NO_PATH)), 7, 0)).all()
    assert (st[fs.STILL, 1:] == 2).all() and (want["count"][fs.STILL] == 0).all()
    assert (st[fs.RING, 1:] == 1).all() and (want["count"][fs.RING, 1:] == 12).all()
    assert (st[fs.FAR, 1:] == 0).all() and (want["count"][fs.FAR, 1:] == 4).all()
    assert (st[0, 1:] == 0).all() and (want["count"][0, 1:] == 4).all()
    assert (want["rows"][fs.NO_MAIN] == fs.PREFILL).all() and (want["rows"][fs.NO_PATH] == fs.PREFILL).all()
    case = fs.bitwise_launch()
    _, s = md.decomp_path_points(case["path"][0, :11], case["path_length"][0], case["s0"][fs.PAST_END], case["v"][fs.PAST_END, :fs.N], fs.DT)
    assert s[5] < case["path_length"][0] < s[-1]                          # the polyline really leaves the path
    assert (st[fs.PAST_END, 1:] != 2).all()
    sm = fs.scattered_mirror()
    assert (sm["status"][:, 1:] == 0).mean() > 0.9 and sm["count"].max() > 8 and (sm["count"][:, 1:] >= 4).all()


def _properties(tag, pts, poly, rows, count, status, decomp_range):
    """For every stage with status 0 or 1: both end points of the segment satisfy every written row within 1e-9; every written normal has
    norm 1 within 1e-12; no box point satisfies all written rows with a margin above 1e-9.  A status-1 stage has lost at least one of its
    four box rows (found = obstacle rows + 4 > n_rows), so the last property does not apply to it: such stages are counted and printed."""
    checked = cut = 0
    worst_end, worst_norm = -np.inf, 0.0
    for k in range(1, len(poly)):
        if status[k] == 2:
            continue
        p1, p2 = poly[k - 1], poly[k]
        A, b = rows[k, :count[k], :2], rows[k, :count[k], 2]
        assert count[k] >= 1
        worst_end = max(worst_end, (A @ p1 - b).max(), (A @ p2 - b).max())
        worst_norm = max(worst_norm, np.abs(np.hypot(A[:, 0], A[:, 1]) - 1.0).max())
        if status[k] == 1:
            cut += 1
            continue
        e = (p2 - p1) / np.hypot(*(p2 - p1)); c = (p1 + p2) / 2.0; f = np.hypot(*(p2 - p1)) / 2.0
        u = (pts - c) @ e; w = (pts - c) @ np.array([e[1], -e[0]])
        box = pts[(np.abs(w) <= decomp_range + 1e-10) & (np.abs(u) <= f + decomp_range + 1e-10)]
        if len(box):
            margin = (box @ A.T - b[None, :]).max(axis=1)                 # < -1e-9: strictly inside every row
            assert margin.min() >= -1e-9, (tag, k, margin.min())
        checked += 1
    assert worst_end <= 1e-9, (tag, worst_end)
    assert worst_norm <= 1e-12, (tag, worst_norm)
    return checked, cut, worst_end, worst_norm


def test_geometric_properties_on_scattered_scenes():
    case, want = fs.scattered_launch(), fs.scattered_mirror()
    total = np.zeros(2, int); worst = [-np.inf, 0.0]
    for q in range(len(case["count"])):
        poly, _ = md.decomp_path_points(case["path"][q, :11], case["path_length"][q], case["s0"][q], case["v"][q, :fs.N], fs.DT)
        ch, cut, we, wn = _properties(("scattered", q), case["points"][q], poly, want["rows"][q], want["count"][q], want["status"][q], fs.RANGE)
        total += (ch, cut); worst = [max(worst[0], we), max(worst[1], wn)]
    print(f"[free space] scattered: {total[0]} stages checked, {total[1]} with truncated box rows, worst end-point row value {worst[0]:.3e}, "
          f"worst | |n| - 1 | {worst[1]:.3e}")
    assert total[0] > 1000


def test_geometric_properties_on_corridor_scenes():
    total = np.zeros(2, int); worst = [-np.inf, 0.0]; n_rows_seen = []
    for idx in range(64):
        sc = fs.corridor_scene(idx)
        dc = fs.corridor_decomp(sc)
        assert not dc["overflow"] and len(dc["points"]) > 100
        poly, _ = md.decomp_path_points(sc["segments"], dc["length"], sc["xinit"][0, 4], sc["x0"][0, :fs.N, md.IDX["v"]], fs.DT)
        ch, cut, we, wn = _properties(("corridor", idx), dc["points"], poly, dc["rows"], dc["count"], dc["status"], fs.RANGE)
        total += (ch, cut); worst = [max(worst[0], we), max(worst[1], wn)]
        n_rows_seen.append(dc["count"][1:].max())
    print(f"[free space] corridor: {total[0]} stages checked, {total[1]} with truncated box rows, worst end-point row value {worst[0]:.3e}, "
          f"worst | |n| - 1 | {worst[1]:.3e}, most rows in a stage {max(n_rows_seen)}")
    assert total[0] > 600 and max(n_rows_seen) >= 6


def test_costmap_points_against_nonzero():
    rng = np.random.default_rng(3)
    cost = np.where(rng.uniform(size=(37, 53)) < 0.2, rng.integers(1, 256, (37, 53)), 0).astype(np.uint8)      # [size_y = 37][size_x = 53]
    assert set(np.unique(cost)) - {0, 254} and (cost == 0).any()
    origin, res = (-3.25, 7.5), 0.05
    pts, count, overflow = md.costmap_points(cost, origin, res)
    want = [(origin[0] + (mx + 0.5) * res, origin[1] + (my + 0.5) * res) for mx in range(53) for my in range(37) if cost[my, mx] != 0]
    assert count == len(want) == int((cost != 0).sum()) and not overflow
    assert [tuple(p) for p in pts] == want
    mx, my = np.nonzero(cost.T)
    assert np.array_equal(pts, np.stack([origin[0] + (mx + 0.5) * res, origin[1] + (my + 0.5) * res], 1))
    clipped, c2, o2 = md.costmap_points(cost, origin, res, n_pts_max=100)
    assert c2 == 100 and o2 and np.array_equal(clipped, pts[:100])
    exact, c3, o3 = md.costmap_points(cost, origin, res, n_pts_max=count)
    assert c3 == count and not o3
    assert md.costmap_points(np.zeros((4, 5), np.uint8), origin, res)[1:] == (0, False)


def test_with_costmap_is_a_corridor_around_the_path():
    from mpc_planner_amd import scenes
    sc0 = scenes.make_scene(5, N=fs.N, M=8, B=1, slack=True, n_decomp=12)
    sc = fs.corridor_scene(5)
    assert np.array_equal(sc0["params"], sc["params"]) and np.array_equal(sc0["x0"], sc["x0"])     # the scene itself is left as it is
    cm = sc["costmap"]
    assert cm.shape == (100, 100) and cm.dtype == np.uint8 and set(np.unique(cm)) <= {0, 253, 254} and (cm == 254).sum() > 300
    again = scenes.with_costmap(sc0, 5005)
    assert np.array_equal(again["costmap"], cm)
    pts, _, _ = md.costmap_points(cm, sc["costmap_origin"], sc["costmap_resolution"])
    seg = sc["segments"]
    dist = np.array([min(np.hypot(p[0] - q[0], p[1] - q[1]) for q in (md._road_segment_eval(seg[:, :8], seg[:, 8], s)[:2] for s in np.arange(-3.0, 12.0, 0.05)))
                     for p in pts[::7]])
    assert dist.min() >= 0.45 - 0.1                                      # nothing closer to the path than the pillars' margin (a cell's size of slack)
    assert scenes.with_costmap(sc0, 5005, size=64, resolution=0.2)["costmap"].shape == (64, 64)


def test_rows_land_in_the_columns_the_parameter_map_names():
    sc = fs.corridor_scene(9)
    dc = fs.corridor_decomp(sc)
    pm = sc["pm"]
    params = np.full((fs.N, pm.length()), fs.PREFILL)
    md.halfspace_rows_set_parameters(pm, params, sc["xinit"][0, 0], (dc["a1"], dc["a2"], dc["b"]), "disc_0_decomp", fs.N_ROWS, disc_offset=0.25)
    cols = []
    for j in range(fs.N_ROWS):
        ia = [pm.index(f"disc_0_decomp_{j}_{f}") for f in ("a1", "a2", "b")]
        cols += ia
        assert np.array_equal(params[:, ia], dc["rows"][:, j, :])           # dummies included: the NaN form and the row form agree
    off = pm.index("ego_disc_0_offset")
    assert (params[:, off] == 0.25).all()
    rest = np.setdiff1d(np.arange(pm.length()), cols + [off])
    assert (params[:, rest] == fs.PREFILL).all()
    assert (dc["count"][1:] >= 4).all() and np.isnan(dc["a1"][0]).all() and (dc["rows"][0] == (1.0, 0.0, sc["xinit"][0, 0] + 100.0)).all()
