"""CPU: the host mirrors of Contouring's road constraints (contouring.cpp:181-262; mpc_planner_amd/modules.py road_halfspaces /
road_halfspaces_from_bounds) on hand-derived values, the two assumptions of DESIGN.md U12 (normal to the right of travel, plain piecewise
cubics) pinned by them, and generate_solver(add_halfspaces=...).  The device kernel is held to these mirrors in tests/test_gpu_road.py."""
import filecmp
import os

import numpy as np
import pytest

R = 0.325
EXACT = 1e-14          # hand-derived values: a few ulps of numbers below 10 (sums of two products)
GEOM = 1e-12           # identities on the sine paths: offsets are O(1 - 10)


def _straight(y0, S=5, seg_len=6.0):
    """P(s) = (s, y0) as S segments [ax bx cx dx ay by cy dy start]."""
    segs = np.zeros((S, 9))
    for i in range(S):
        segs[i] = [0.0, 0.0, 1.0, seg_len * i, 0.0, 0.0, 0.0, y0, seg_len * i]
    return segs


def _eval(segs, s):
    """Independent evaluation (numpy.polyval, searchsorted) of the plain piecewise cubic and its derivative."""
    i = max(int(np.searchsorted(segs[:, 8], s, side="right")) - 1, 0)
    t = s - segs[i, 8]
    px, py = np.polyval(segs[i, 0:4], t), np.polyval(segs[i, 4:8], t)
    dx, dy = np.polyval(np.polyder(segs[i, 0:4]), t), np.polyval(np.polyder(segs[i, 4:8]), t)
    return np.array([px, py]), np.array([dx, dy]), i


@pytest.mark.parametrize("y0", [0.0, 1.25, -0.7])
def test_straight_path_one_way_and_two_way(y0):
    from mpc_planner_amd import modules as md
    s_of_k = np.linspace(0.3, 17.0, 20)
    off = md.road_offsets(6.0, R)
    assert off == (3.0 - R, 3.0 - R)
    rows = md.road_halfspaces(_straight(y0), s_of_k, *off)
    assert rows.shape == (20, 2, 3)
    assert (rows[0] == 0.0).all()                                                       # stage 0 is left alone
    np.testing.assert_allclose(rows[1:, 0], np.tile([0.0, -1.0, 2.675 - y0], (19, 1)), rtol=0, atol=EXACT)
    np.testing.assert_allclose(rows[1:, 1], np.tile([0.0, 1.0, y0 + 2.675], (19, 1)), rtol=0, atol=EXACT)
    # two-way road: the 3 w / 2 side is the one row 0 bounds -- the right of travel (this pins the sign convention, U12)
    off2 = md.road_offsets(6.0, R, two_way=True)
    assert off2 == (9.0 - R, 3.0 - R)
    rows2 = md.road_halfspaces(_straight(y0), s_of_k, *off2)
    np.testing.assert_allclose(rows2[1:, 0], np.tile([0.0, -1.0, 8.675 - y0], (19, 1)), rtol=0, atol=EXACT)
    np.testing.assert_array_equal(rows2[:, 1], rows[:, 1])
    # meaning of the rows: a point 2.6 m to either side of the path satisfies both, 2.7 m to the left / right violates row 1 / row 0
    for dy, ok0, ok1 in ((2.6, True, True), (-2.6, True, True), (2.7, True, False), (-2.7, False, True)):
        p = np.array([5.0, y0 + dy])
        assert (rows[3, 0, :2] @ p <= rows[3, 0, 2]) == ok0 and (rows[3, 1, :2] @ p <= rows[3, 1, 2]) == ok1


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_sine_paths_unit_normal_and_offsets(seed):
    from mpc_planner_amd import modules as md, scenes
    rng = np.random.default_rng(seed)
    segs = scenes.reference_path_segments(rng, 5)
    s_of_k = np.concatenate([[0.0], np.sort(rng.uniform(0.0, 29.9, 19))])
    o1, o2 = 8.675, 1.675
    rows = md.road_halfspaces(segs, s_of_k, o1, o2)
    for k in range(1, 20):
        P, D, _ = _eval(segs, s_of_k[k])
        A = rows[k, 0, :2]
        assert abs(A @ A - 1.0) <= GEOM and abs(A @ D) <= GEOM * np.linalg.norm(D)      # unit, orthogonal to (x', y')
        assert A[0] * D[1] - A[1] * D[0] > 0.0                                          # to the RIGHT of travel: A x D > 0 <=> A = (y', -x') / |.|
        np.testing.assert_array_equal(rows[k, 1, :2], -A)
        assert abs(rows[k, 0, :2] @ P - rows[k, 0, 2] + o1) <= GEOM                     # a.P(s_k) - b = -offset, both rows
        assert abs(rows[k, 1, :2] @ P - rows[k, 1, 2] + o2) <= GEOM
    assert (rows[0] == 0.0).all()


def test_knots_and_extrapolation():
    from mpc_planner_amd import modules as md, scenes
    segs = scenes.reference_path_segments(np.random.default_rng(7), 5)
    segs[:, 4:8] += np.arange(5)[:, None] * 0.01          # make neighbouring cubics disagree at the knots, so the segment choice shows
    for s, seg in ((12.0, 2), (np.nextafter(12.0, 0.0), 1), (-0.5, 0), (0.0, 0), (30.0, 4), (33.5, 4)):
        rows = md.road_halfspaces(segs, np.array([0.0, s]), 2.0, 2.0)
        t = s - segs[seg, 8]
        P = np.array([np.polyval(segs[seg, 0:4], t), np.polyval(segs[seg, 4:8], t)])
        D = np.array([np.polyval(np.polyder(segs[seg, 0:4]), t), np.polyval(np.polyder(segs[seg, 4:8]), t)])
        A = np.array([D[1], -D[0]]) / np.linalg.norm(D)
        np.testing.assert_allclose(rows[1, 0], [A[0], A[1], A @ P + 2.0], rtol=0, atol=GEOM)
        np.testing.assert_allclose(rows[1, 1], [-A[0], -A[1], -(A @ P - 2.0)], rtol=0, atol=GEOM)
    # exactly on a knot the segment that STARTS there is used: the value differs from the previous segment's continuation
    on = md.road_halfspaces(segs, np.array([0.0, 12.0]), 2.0, 2.0)[1, 0, 2]
    before = md.road_halfspaces(segs, np.array([0.0, np.nextafter(12.0, 0.0)]), 2.0, 2.0)[1, 0, 2]
    assert abs(on - before) > 1e-3


@pytest.mark.parametrize("w", [2.0, 3.5])
def test_bounds_mode_on_a_straight_path_is_the_centreline_corridor(w):
    """Left bound at P - A w, right bound at P + A w (A to the right): bounds mode gives the one-way centreline rows of half = w in the other
    order -- the left bound's row comes first (contouring.cpp:252-260): row 0 there is row 1 here."""
    from mpc_planner_amd import modules as md
    y0 = 0.4
    segs = _straight(y0)
    left, right = _straight(y0 + w)[:, :8], _straight(y0 - w)[:, :8]          # A = (0, -1): P - A w = (s, y0 + w)
    s_of_k = np.linspace(0.0, 20.0, 12)
    got = md.road_halfspaces_from_bounds(segs, left, right, s_of_k, R)
    want = md.road_halfspaces(segs, s_of_k, w - R, w - R)
    assert got.shape == (12, 2, 3) and (got[0] == 0.0).all()
    np.testing.assert_allclose(got[:, 0], want[:, 1], rtol=0, atol=EXACT)
    np.testing.assert_allclose(got[:, 1], want[:, 0], rtol=0, atol=EXACT)
    np.testing.assert_allclose(got[1:, 0], np.tile([0.0, 1.0, y0 + w - R], (11, 1)), rtol=0, atol=EXACT)
    np.testing.assert_allclose(got[1:, 1], np.tile([0.0, -1.0, w - R - y0], (11, 1)), rtol=0, atol=EXACT)


def test_bounds_mode_on_a_curved_path_is_a_corridor_between_the_bounds():
    """With the normal to the right of travel the two rows admit the centreline and exclude points beyond either bound (with the other sign both
    rows would exclude the road: DESIGN.md U12)."""
    from mpc_planner_amd import modules as md, scenes
    segs = scenes.reference_path_segments(np.random.default_rng(11), 5)
    left, right = segs[:, :8].copy(), segs[:, :8].copy()
    left[:, 7] += 2.5; right[:, 7] -= 2.0                                     # the path shifted in y: bounds 2.5 m to the left, 2 m to the right
    s_of_k = np.linspace(0.0, 28.0, 15)
    rows = md.road_halfspaces_from_bounds(segs, left, right, s_of_k, R)
    for k in range(1, 15):
        P, D, _ = _eval(segs, s_of_k[k])
        for j in range(2):
            assert rows[k, j, :2] @ P < rows[k, j, 2]
        Pl, _, _ = _eval(np.column_stack([left, segs[:, 8]]), s_of_k[k]); Pr, _, _ = _eval(np.column_stack([right, segs[:, 8]]), s_of_k[k])
        assert rows[k, 0, :2] @ Pl > rows[k, 0, 2] and rows[k, 1, :2] @ Pr > rows[k, 1, 2]      # the bounds themselves are r inside the excluded side


def test_rows_feed_linearized_update_and_the_scene_helper():
    from mpc_planner_amd import modules as md, scenes
    from mpc_planner_amd.parameters import define_parameters
    N, M, B = 20, 8, 4
    sc = scenes.make_scene(80, N=N, M=M, B=B, tmpc_pp=True)
    before = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sc.items()}
    rd = scenes.add_road_constraints(sc, width=4.0)
    assert all(np.array_equal(sc[k], before[k]) for k in ("params", "x0", "xinit"))     # make_scene's output is left as it is
    pm = rd["pm"]
    assert pm.length() == define_parameters(5, 8, add_halfspaces=2).length() == sc["pm"].length() + 6 and rd["n_lin"] == 10
    rows = md.road_halfspaces(sc["segments"], sc["x0"][0, :N, 6], *md.road_offsets(4.0, scenes.ROBOT_RADIUS))
    np.testing.assert_array_equal(rd["road_rows"], rows)
    for name, idx in sc["pm"]._params.items():                                          # every old column is where the wider map puts it
        np.testing.assert_array_equal(rd["params"][:, :, pm.index(name)][:B], sc["params"][:B, :, idx])
    for b in range(B):                                                                  # guided planners: LinearizedConstraints::update + setParameters
        lin = md.linearized_update(sc["x0"][b], sc["obstacles"]["pos"], scenes.ROBOT_RADIUS, static=rows)
        want = np.zeros((N, pm.length()))
        md.linearized_set_parameters(pm, want, sc["xinit"][0, 0], lin, n_rows=M + 2)
        cols = [pm.index(f"lin_constraint_{j}_{f}") for j in range(M + 2) for f in ("a1", "a2", "b")]
        np.testing.assert_array_equal(rd["params"][b][:, cols], want[:, cols])
    # the non-guided planner sees zero obstacles: the road rows are its rows 0 and 1, dummies behind them and at stage 0
    lin = md.linearized_update(sc["x0"][B], sc["obstacles"]["pos"][:0], scenes.ROBOT_RADIUS, static=rows)
    want = np.zeros((N, pm.length()))
    md.linearized_set_parameters(pm, want, sc["xinit"][0, 0], lin, n_rows=M + 2)
    np.testing.assert_array_equal(rd["params"][B][:, cols], want[:, cols])
    assert (rd["params"][B][1:, pm.index("lin_constraint_0_a1")] == rows[1:, 0, 0]).all() and (rd["params"][B][:, pm.index("lin_constraint_9_b")] == 100.0).all()


def test_generate_solver_add_halfspaces(tmp_path):
    from mpc_planner_amd.generate_solver import generate_solver
    from mpc_planner_amd.parameters import define_parameters
    generate_solver(str(tmp_path / "road"), N=20, max_obstacles=8, num_segments=5, guidance=True, add_halfspaces=2)
    hdr = open(tmp_path / "road" / "include" / "mpc_planner_solver" / "hip_solver_dims.h").read()
    npar = define_parameters(5, 8, add_halfspaces=2).length()
    assert "#define SOLVER_NLIN 10\n" in hdr and "#define SOLVER_MAX_OBSTACLES 8\n" in hdr and f"#define SOLVER_NP {npar}\n" in hdr
    assert npar == 135 + 6
    pmap = open(tmp_path / "road" / "config" / "parameter_map.yaml").read()
    assert "lin_constraint_9_b:" in pmap and f"num parameters: {npar}" in pmap
    assert "if(index == 9)" in open(tmp_path / "road" / "src" / "mpc_planner_parameters.cpp").read().split("setSolverParameterLinConstraintB")[1]


def test_generate_solver_default_is_byte_identical(tmp_path):
    """add_halfspaces = 0 (the default) writes what the generator wrote before the argument existed: tests/golden/generate_solver_cfg2 holds
    those files for the cfg-2 solver."""
    from mpc_planner_amd.generate_solver import generate_solver
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generate_solver_cfg2")
    for name, kw in (("default", {}), ("explicit", dict(add_halfspaces=0))):
        out = str(tmp_path / name)
        generate_solver(out, N=20, max_obstacles=8, num_segments=5, guidance=True, **kw)
        for rel in ("config/parameter_map.yaml", "config/model_map.yaml", "config/solver_settings.yaml", "include/mpc_planner_solver/hip_solver_dims.h",
                    "include/mpc_planner_solver/mpc_planner_parameters.h", "src/mpc_planner_parameters.cpp"):
            assert filecmp.cmp(os.path.join(out, rel), os.path.join(golden, rel.replace("/", "__") + ".txt"), shallow=False), rel
    # without a guidance module there are no topology rows to widen
    generate_solver(str(tmp_path / "basic"), N=20, max_obstacles=4, guidance=False, add_halfspaces=2)
    assert "#define SOLVER_NLIN 0\n" in open(tmp_path / "basic" / "include" / "mpc_planner_solver" / "hip_solver_dims.h").read()
