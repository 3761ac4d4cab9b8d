"""CPU: the reference-path tracking mirrors (mpc_planner_amd/modules.py find_closest_point / path_window / track_path -- Contouring::update on
a whole path, contouring.cpp:28-48, :94-124) on hand-derived values.  RosTools::Spline2D is not in the reference tree: these tests pin what
DESIGN.md U14 assumes.  The device kernel and the C++ header are held to these mirrors bit for bit (tests/test_gpu_path.py,
tests/test_cpp_path.py)."""
import numpy as np
import pytest

from mpc_planner_amd import modules as md, scenes


def straight(n=4, L=2.0):
    """x = start + t, y = 0: n segments of L metres."""
    return np.array([[0.0, 0.0, 1.0, L * i, 0.0, 0.0, 0.0, 0.0, L * i] for i in range(n)]), L * n


# what is left of the bracket [t_{j-1}, t_{j+1}] (2 L / 8 wide) after 40 halvings, taken at its midpoint, plus four ulps of 8 for the
# evaluation of start + t and of the cubic near s = 8
TOL = (2 * 2.0 / 8) * 2.0 ** -41 + 4 * np.spacing(8.0)


@pytest.mark.parametrize("pos, kw, seg, s, exact", [
    ((-1.0, 0.5), {}, 0, 0.0, True),                                     # before the start: the end point itself
    ((9.0, 1.0), {}, 3, 8.0, True),                                      # beyond the end
    ((4.0, 1.0), {}, 1, 4.0, True),                                      # on a knot: segments 1 and 2 tie, the lower one wins
    ((3.3, 0.7), {}, 1, 3.3, False),
    ((7.1, 0.2), {}, 3, 7.1, False),
    ((7.1, 0.2), dict(segment=0, search_range=1), 1, 4.0, True),         # the local search must not see segment 3
])
def test_closest_point_on_a_straight_path(pos, kw, seg, s, exact):
    path, length = straight()
    got_seg, got_s = md.find_closest_point(path, length, pos, **kw)
    print(f"[path] {pos} {kw}: segment {got_seg}, s {got_s!r} (|s - expected| = {abs(got_s - s):.3e}, bound {TOL:.3e})")
    assert got_seg == seg
    if exact:
        assert got_s == s
    else:
        assert abs(got_s - s) <= TOL


def test_previous_segment_is_clamped_and_nonfinite_input_stays_in_range():
    path, length = straight()
    assert md.find_closest_point(path, length, (0.3, 0.0), segment=99, search_range=0)[0] == 3          # clamped to the last segment
    assert md.find_closest_point(path, length, (0.3, 0.0), segment=99, search_range=31)[0] == 0
    for bad in ((np.nan, 0.0), (np.inf, 0.0), (0.0, -np.inf)):
        assert md.find_closest_point(path, length, bad)[0] == 0                                        # the first candidate
        assert md.find_closest_point(path, length, bad, segment=3, search_range=1)[0] == 2


def test_window_pads_straight_along_the_end_tangent():
    path, length = straight()
    w = md.path_window(path, length, 2, 5)
    assert w.shape == (5, 9)
    np.testing.assert_array_equal(w[:2], path[2:])                       # two real slots
    for k in range(2, 5):                                                # three padded ones
        np.testing.assert_array_equal(w[k], [0, 0, 1, 8, 0, 0, 0, 0, 8])
    # a curved end: the pad carries the end point and the end tangent of the last cubic, the bounds their own
    path[3, :8] = [0.0, 0.0, 1.0, 6.0, 0.1, -0.2, 0.3, 0.5]
    left = path[:, :8].copy(); left[:, 7] += 2.0
    right = path[:, :8].copy(); right[:, 7] -= 1.5; right[3, 4] = 0.0
    w, wl, wr = md.path_window(path, length, 3, 3, left, right)
    y_end = ((0.1 * 2 - 0.2) * 2 + 0.3) * 2 + 0.5; dy_end = (3 * 0.1 * 2 + 2 * -0.2) * 2 + 0.3
    np.testing.assert_array_equal(w[0], path[3])
    np.testing.assert_allclose(w[1], [0, 0, 1, 8, 0, 0, dy_end, y_end, 8], rtol=0, atol=1e-15)
    np.testing.assert_array_equal(w[2], w[1])
    np.testing.assert_array_equal(wl[0], left[3]); np.testing.assert_array_equal(wr[0], right[3])
    np.testing.assert_allclose(wl[1], [0, 0, 1, 8, 0, 0, dy_end, y_end + 2.0], rtol=0, atol=1e-15)
    np.testing.assert_allclose(wr[2], [0, 0, 1, 8, 0, 0, (2 * -0.2) * 2 + 0.3, (-0.2 * 2 + 0.3) * 2 + 0.5 - 1.5], rtol=0, atol=1e-15)
    # the padded slot continues the path: value and derivative at the knot are the last cubic's, and the derivative never vanishes
    x, y, dx, dy = md._road_segment_eval(w[:, :8], w[:, 8], 8.0 + 0.25)
    assert abs(x - 8.25) < 1e-15 and abs(y - (y_end + 0.25 * dy_end)) < 1e-15 and (dx, dy) == (1.0, w[1, 6])


def test_objective_reached():
    path, length = straight()
    assert md.path_objective_reached(path, length, (7.2, 0.3)) is True
    assert md.path_objective_reached(path, length, (6.9, 0.0)) is False
    out = md.track_path(path, length, (7.2, 0.3), 5)
    assert out["reached"] and out["segment"] == 3 and out["window"].shape == (5, 9)
    assert not md.track_path(path, length, (6.9, 0.0), 5, segment=3)["reached"]


def test_never_worse_than_brute_force():
    """Seeds 0 .. 39, 12 x 2 m paths of scenes.reference_path_segments, 10 points each in [-1, 25] x [-2.5, 2.5]: D of the result is not
    above D of a dense search with 20001 samples per segment."""
    worst = -np.inf
    tt = np.linspace(0.0, 2.0, 20001)
    for seed in range(40):
        rng = np.random.default_rng(seed)
        path = scenes.reference_path_segments(rng, S=12, seg_len=2.0)
        length = 24.0
        pts = np.stack([rng.uniform(-1.0, 25.0, 10), rng.uniform(-2.5, 2.5, 10)], 1)
        c = path[:, :8, None]
        X = ((c[:, 0] * tt + c[:, 1]) * tt + c[:, 2]) * tt + c[:, 3]     # [12][20001]
        Y = ((c[:, 4] * tt + c[:, 5]) * tt + c[:, 6]) * tt + c[:, 7]
        for p in pts:
            seg, s = md.find_closest_point(path, length, p)
            D, t = md.closest_point_on_segment(path[seg, :8], 2.0, p[0], p[1])
            assert s == path[seg, 8] + t
            D_brute = ((X - p[0]) ** 2 + (Y - p[1]) ** 2).min()
            worst = max(worst, D - D_brute)
            assert D <= D_brute, (seed, p, seg, s, D, D_brute)
    print(f"[path] max D - D_brute over 400 points: {worst:.3e}")


def test_walk_with_local_search_follows_the_knots():
    """Twelve ticks of 0.4 m from x = 1.7 on the straight path, local search from the segment of the tick before: the segment never
    decreases and changes exactly where s passes a knot."""
    path, length = straight()
    seg, segs, ss = -1, [], []
    for tick in range(12):
        x = 1.7 + 0.4 * tick
        seg, s = md.find_closest_point(path, length, (x, 0.3), segment=seg, search_range=2)
        segs.append(seg); ss.append(s)
        assert abs(s - x) <= TOL
    print(f"[path] walk: segments {segs}")
    assert segs == [0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 3]
    assert all(b >= a for a, b in zip(segs, segs[1:]))
    assert segs == [min(int(s // 2.0), 3) for s in ss]


def test_long_path_scene_keeps_make_scene_and_moves_the_window():
    sc = scenes.make_scene(80, N=20, M=8, B=4)
    before = {k: np.array(v, copy=True) for k, v in sc.items() if isinstance(v, np.ndarray)}
    out = scenes.with_long_path(sc, np.random.default_rng(80), n_segments=12, seg_len=2.0, shift=2.3)
    for k, v in before.items():
        np.testing.assert_array_equal(sc[k], v)                          # the input scene is left as it is
    assert out["path"].shape == (12, 9) and out["path_length"] == 24.0
    assert out["path_segment"] == 1                                      # the robot at the origin stands 0.3 m past the knot at 2 m
    np.testing.assert_array_equal(out["segments"], md.path_window(out["path"], 24.0, 1, 5))
    pm = out["pm"]
    assert (out["params"][:, :, pm.index("spline2_start")] == out["path"][3, 8]).all()
    assert (out["params"][:, :, pm.index("contour")] == sc["params"][:, :, pm.index("contour")]).all()
    np.testing.assert_array_equal(out["xinit"][:, 4], np.full(len(out["xinit"]), out["path_s"]))
    assert abs(out["path_s"] - 2.3) < 1e-9
