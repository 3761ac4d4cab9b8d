"""CPU: the path-fit mirrors (mpc_planner_amd/modules.py path_knots / fit_cubic / fit_path / path_velocity_window -- what
Contouring::onDataReceived, contouring.cpp:126-157, and PathReferenceVelocity, path_reference_velocity.cpp:28-95, do with waypoints) on
hand-derived values and against scipy's natural cubic spline.  RosTools::Spline2D and tk::spline are not in the reference tree: these tests
pin what DESIGN.md U15 states.  The device kernel and the C++ header are held to these mirrors bit for bit (tests/test_gpu_path_fit.py,
tests/test_cpp_path_fit.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mpc_planner_amd import modules as md

import path_fit_cases as pf


def test_three_points_by_hand():
    """Knots 0, 1, 2, values 0, 1, 0: one unknown, (4 / 3) m_1 = -2, m_1 = -1.5; segments (-0.5, 0, 1.5, 0) and (0.5, -1.5, 0, 1)."""
    got = md.fit_cubic([0.0, 1.0, 2.0], [0.0, 1.0, 0.0])
    np.testing.assert_allclose(got, [[-0.5, 0.0, 1.5, 0.0], [0.5, -1.5, 0.0, 1.0]], rtol=0, atol=1e-15)


def test_two_points_give_the_line():
    got = md.fit_cubic([1.5, 4.0], [2.0, -3.0])
    assert got.shape == (1, 4)
    assert got[0].tolist() == [0.0, 0.0, (-3.0 - 2.0) / 2.5, 2.0]
    out = md.fit_path([[0.0, 0.0], [3.0, 4.0]])
    assert out["status"] == 0 and out["count"] == 1 and out["length"] == 5.0
    assert out["path"][0].tolist() == [0.0, 0.0, 3.0 / 5.0, 0.0, 0.0, 0.0, 4.0 / 5.0, 0.0, 0.0]


def test_collinear_equally_spaced_points_have_no_curvature():
    xy = np.stack([0.7 * np.arange(5), 1.0 + 0.3 * np.arange(5)], 1)
    out = md.fit_path(xy)
    assert out["count"] == 4
    assert np.abs(out["path"][:, [0, 1, 4, 5]]).max() <= 1e-14


def test_chord_knots_of_a_3_4_5_polyline():
    assert md.path_knots([[0.0, 0.0], [3.0, 4.0], [6.0, 8.0]]).tolist() == [0.0, 5.0, 10.0]
    assert md.path_knots([[1.0, 1.0], [4.0, 5.0]], s=[2.0, 9.0]).tolist() == [2.0, 9.0]          # given knots: as supplied, not shifted


def _scipy_cases():
    for n in pf.SCIPY_COUNTS:
        yield n, pf.waypoints(np.random.default_rng(150 + n), n)


def _column_errors(got, ref):
    """per coefficient column, relative to the largest |coefficient| of that column of that curve"""
    return np.abs(got - ref).max(axis=0) / np.abs(ref).max(axis=0)


# the worst column error of the mirror against scipy over _scipy_cases(), measured on the CPU (printed by the test below)
SCIPY_MEASURED = 1.8e-13
SCIPY_BOUND = min(100 * SCIPY_MEASURED, 1e-10)


def test_against_scipy_natural_cubic_spline():
    """scipy.interpolate.CubicSpline(bc_type="natural") is an independent implementation of the same spline (a banded LU solve for the
    first derivatives).  Point counts 3, 4, 5, 64, 65, 130, 1025, chord spacing 0.2 .. 3 m; the error per coefficient column relative to the
    largest |coefficient| of that column of that curve.  Measured worst: 1.8e-13 (at n = 4, the `b` column of x on a nearly straight
    path, where the largest second derivative is itself small against the slopes it is a difference of; 2e-14 and below from n = 64 on);
    asserted at 100 x that, 1.8e-11, and never looser than 1e-10."""
    from scipy.interpolate import CubicSpline
    worst = 0.0
    for n, xy in _scipy_cases():
        out = md.fit_path(xy)
        t = md.path_knots(xy)
        assert out["status"] == 0 and out["count"] == n - 1 and out["length"] == t[-1]
        assert np.array_equal(out["path"][:, 8], t[:-1])
        cs = CubicSpline(t, xy, bc_type="natural")
        for k in range(2):
            ref = cs.c[:, :, k].T                                          # scipy: c[0] t^3 + c[1] t^2 + c[2] t + c[3], the same order
            err = _column_errors(out["path"][:, 4 * k:4 * k + 4], ref)
            print(f"[fit] n = {n} curve {'xy'[k]}: column errors {err}")
            worst = max(worst, err.max())
    print(f"[fit] worst column error against scipy: {worst:.3e} (bound {SCIPY_BOUND:.3e})")
    assert worst <= SCIPY_BOUND


def test_c2_at_the_interior_knots_and_natural_ends():
    """Value, first and second derivative of neighbouring segments agree at every interior knot, to SCIPY_BOUND times the largest magnitude
    of that quantity over the curve; the second derivative at both ends is 0 (exactly at the start: b_0 = m_0 = 0)."""
    for n, xy in _scipy_cases():
        out = md.fit_path(xy, v=np.linspace(1.0, 2.0, n) ** 2)
        t = md.path_knots(xy)
        h = t[1:] - t[:-1]
        for c in (out["path"][:, 0:4], out["path"][:, 4:8], out["velocity"]):
            a, b, cc, d = c.T
            end = [((a * h + b) * h + cc) * h + d, (3 * a * h + 2 * b) * h + cc, 6 * a * h + 2 * b]
            start = [d, cc, 2 * b]
            for e, s_ in zip(end, start):
                scale = max(np.abs(e).max(), np.abs(s_).max(), 1.0)
                assert np.abs(e[:-1] - s_[1:]).max() <= SCIPY_BOUND * scale
            assert b[0] == 0.0
            assert abs(end[2][-1]) <= SCIPY_BOUND * max(np.abs(end[2]).max(), 1.0)


def test_given_s():
    xy = pf.waypoints(np.random.default_rng(7), 20)
    t = md.path_knots(xy)
    chord, given = md.fit_path(xy), md.fit_path(xy, s=t)
    assert np.array_equal(chord["path"], given["path"]) and chord["length"] == given["length"]          # bitwise
    stretched = md.fit_path(xy, s=1.5 * t + 2.0)
    assert stretched["path"][0, 8] == 2.0 and stretched["length"] == 1.5 * t[-1] + 2.0
    assert not np.array_equal(stretched["path"][:, :8], chord["path"][:, :8])
    np.testing.assert_array_equal(stretched["path"][:, [3, 7]], chord["path"][:, [3, 7]])               # d = the waypoints either way


def test_bounds_use_the_centreline_knots_and_road_width():
    xy = pf.waypoints(np.random.default_rng(8), 12)
    left, right = xy + [0.0, 2.0], xy - [0.0, 1.0]
    left[3:] += 0.4 * np.arange(9)[:, None]                              # (the left bound's own chord lengths differ from the centreline's)
    left[0], right[0] = xy[0] + [1.5, 2.0], xy[0] - [1.5, 2.0]           # |(3, 4)| = 5
    out = md.fit_path(xy, left=left, right=right)
    t = md.path_knots(xy)
    assert out["road_width"] == 5.0
    assert out["left"].shape == out["right"].shape == (11, 8)
    for side, pts in (("left", left), ("right", right)):
        assert np.array_equal(out[side][:, 0:4], md.fit_cubic(t, pts[:, 0])) and np.array_equal(out[side][:, 4:8], md.fit_cubic(t, pts[:, 1]))
    assert not np.array_equal(out["left"][:, 0:4], md.fit_cubic(md.path_knots(left), left[:, 0]))
    with pytest.raises(ValueError):
        md.fit_path(xy, left=left[:-1], right=right)
    with pytest.raises(ValueError):
        md.fit_path(xy, left=left)


@pytest.mark.parametrize("name", ["one point", "duplicate waypoint", "NaN coordinate", "decreasing s"])
def test_invalid_scenes(name):
    xy = pf.waypoints(np.random.default_rng(9), 8)
    s = None
    if name == "one point":
        xy = xy[:1]
    elif name == "duplicate waypoint":
        xy[4] = xy[3]
    elif name == "NaN coordinate":
        xy[2, 1] = np.nan
    else:
        s = md.path_knots(xy); s[5] = s[3]
    out = md.fit_path(xy, s, left=xy + 1.0, right=xy - 1.0, v=np.ones(len(xy)))
    assert out["status"] == 1 and out["count"] == 0
    assert out["path"].shape == (0, 9) and out["left"].shape == (0, 8) and out["velocity"].shape == (0, 4)
    with pytest.raises(ValueError):
        md.fit_cubic(md.path_knots(xy, s), xy[:, 0])


def test_path_velocity_window():
    xy = pf.waypoints(np.random.default_rng(10), 9)
    out = md.fit_path(xy, v=np.linspace(1.0, 2.5, 9))
    vel, count = out["velocity"], out["count"]
    assert count == 8 and vel.shape == (8, 4)
    assert np.array_equal(md.path_velocity_window(vel, count, 2, 5, 1.7), vel[2:7])                     # inside the path
    w = md.path_velocity_window(vel, count, 6, 5, 1.7)                                                  # straddling the end: brake
    assert np.array_equal(w[:2], vel[6:]) and (w[2:] == 0.0).all()
    assert md.path_velocity_window(None, 0, 3, 4, 1.7).tolist() == [[0.0, 0.0, 0.0, 1.7]] * 4            # no profile
    # into the spline_v{i}_{a..d} columns of the stack that carries them
    from mpc_planner_amd.codegen import plugin as P, stacks
    st = stacks.settings(N=20, max_obstacles=2, num_segments=5)
    _, mm = stacks.contouring_path_velocity_ellipsoids(st)
    pm = P.define_parameters(mm, P.Parameters(), st)
    params = np.full((20, pm.length()), -3.0)
    md.path_velocity_set_parameters(pm, params, w)
    cols = [pm.index(f"spline_v{i}_{k}") for i in range(5) for k in "abcd"]
    assert len(set(cols)) == 20
    assert np.array_equal(params[:, cols], np.tile(w.ravel(), (20, 1)))
    assert (np.delete(params, cols, axis=1) == -3.0).all()


def test_fit_then_track():
    """A robot standing on waypoint j of a gently curved path is found on segment j or j - 1 with |closest_s - t_j| <= 1e-9."""
    xy = pf.waypoints(np.random.default_rng(11), 30)
    out = md.fit_path(xy)
    t = md.path_knots(xy)
    for j in (0, 1, 7, 15, 28, 29):
        seg, s = md.find_closest_point(out["path"], out["length"], xy[j], segment=-1)
        print(f"[fit] waypoint {j}: segment {seg}, closest_s - t_j = {s - t[j]:.3e}")
        assert seg in (j, j - 1) and seg <= out["count"] - 1
        assert abs(s - t[j]) <= 1e-9
