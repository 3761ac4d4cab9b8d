"""The cases of the path-fit tests (helper, no tests): waypoints, and the launches of tmpc_fit_path with every case the kernel treats differently
together with the mirror's answer to them.  Shared by tests/test_path_fit.py (the mirror against scipy and hand values),
tests/test_gpu_path_fit.py (device against mirror) and tests/test_cpp_path_fit.py (the C++ header mpc_planner_modules/reference_path.h against
the same mirror, through a binary file)."""
import numpy as np

from mpc_planner_amd import modules as md

PREFILL = -3.0
SCIPY_COUNTS = (3, 4, 5, 64, 65, 130, 1025)
# one launch, n_pts_max = 1025: too short (0, 1), the line (2), the smallest systems (3, 4), around one lane stride of 64 rows (64, 65, 66), several
# strides (130), the cap (1025), a count beyond the cap (clipped), and ten points of which two coincide (invalid)
BITWISE_COUNTS = (0, 1, 2, 3, 4, 64, 65, 66, 130, 1025, 2000, 10)
BITWISE_DUPLICATE = 11                                       # the scene with the repeated waypoint
SMALL_COUNTS = (5, 3, 2, 7, 1, 4)                            # n_pts_max = 5: full, short, the line, clipped, too short, a repeated waypoint
SMALL_DUPLICATE = 5


def waypoints(rng, n):
    """n waypoints of a gently turning path, chord spacing 0.2 .. 3 m."""
    heading = np.cumsum(rng.normal(size=n) * 0.15)
    step = rng.uniform(0.2, 3.0, n)
    return np.cumsum(np.stack([np.cos(heading) * step, np.sin(heading) * step], 1), 0)


def launch(counts, n_pts_max, duplicate, seed):
    """One launch: xy, left, right [Q][n_pts_max][2], s, v [Q][n_pts_max], count [Q].  Slots behind a scene's count hold garbage that must not
    be read as waypoints.  The scene `duplicate` repeats its waypoint 2 (and its s): invalid with chord knots and with given s.  s: the chord
    knots stretched by 1.25 and moved by 3.5 (given knots are not shifted back to 0)."""
    rng = np.random.default_rng(seed)
    Q = len(counts)
    xy = rng.normal(size=(Q, n_pts_max, 2)) * 50.0
    left, right = rng.normal(size=(2, Q, n_pts_max, 2)) * 50.0
    s = rng.normal(size=(Q, n_pts_max)) * 50.0
    v = rng.normal(size=(Q, n_pts_max)) * 50.0
    for q, c in enumerate(counts):
        n = min(int(c), n_pts_max)
        if n == 0:
            continue
        p = waypoints(np.random.default_rng(seed * 1000 + q), n)
        if q == duplicate:
            p[3] = p[2]
        xy[q, :n] = p
        t = md.path_knots(p)
        s[q, :n] = 1.25 * t + 3.5
        d = np.gradient(p, axis=0) if n > 1 else np.array([[1.0, 0.0]])
        nrm = np.stack([-d[:, 1], d[:, 0]], 1) / np.maximum(np.hypot(d[:, 0], d[:, 1]), 1e-9)[:, None]
        left[q, :n] = p + (2.0 + 0.125 * q) * nrm
        right[q, :n] = p - (1.5 + 0.25 * q) * nrm
        v[q, :n] = np.random.default_rng(seed * 1000 + 500 + q).uniform(0.5, 3.0, n)
    return dict(xy=xy, left=left, right=right, s=s, v=v, count=np.array(counts, np.int32), n_pts_max=n_pts_max, duplicate=duplicate)


def bitwise_launch():
    return launch(BITWISE_COUNTS, 1025, BITWISE_DUPLICATE, 15)


def small_launch():
    return launch(SMALL_COUNTS, 5, SMALL_DUPLICATE, 16)


def mirror(case, n_seg_max, given_s, extras):
    """modules.fit_path for every scene of a launch, laid out as the device writes it into buffers prefilled with PREFILL (status with 7):
    rows at or beyond a scene's count keep the prefill, an invalid scene keeps everything but count = 0 and status = 1.  extras: with
    bounds, road width and velocity; else those stay None."""
    Q, P = len(case["count"]), case["n_pts_max"]
    out = dict(path=np.full((Q, n_seg_max, 9), PREFILL), count=np.full(Q, -3, np.int32), length=np.full(Q, PREFILL),
               status=np.full(Q, 7, np.uint8), bounds=None, velocity=None, road_width=None)
    if extras:
        out.update(bounds=np.full((Q, 2, n_seg_max, 8), PREFILL), velocity=np.full((Q, n_seg_max, 4), PREFILL), road_width=np.full(Q, PREFILL))
    for q in range(Q):
        n = min(max(int(case["count"][q]), 0), P)
        kw = dict(left=case["left"][q, :n], right=case["right"][q, :n], v=case["v"][q, :n]) if extras else {}
        fit = md.fit_path(case["xy"][q, :n], case["s"][q, :n] if given_s else None, **kw)
        out["count"][q] = fit["count"]; out["status"][q] = fit["status"]
        if fit["status"]:
            continue
        m = fit["count"]
        out["path"][q, :m] = fit["path"]; out["length"][q] = fit["length"]
        if extras:
            out["bounds"][q, 0, :m] = fit["left"]; out["bounds"][q, 1, :m] = fit["right"]
            out["velocity"][q, :m] = fit["velocity"]; out["road_width"][q] = fit["road_width"]
    return out
