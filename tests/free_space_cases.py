"""The cases of the free-space tests (helper, no tests): the launches of tmpc_decomp_halfspaces with every case the kernel treats differently,
together with the mirror's answer to them.  Shared by tests/test_free_space.py (the mirror against hand values and geometric properties),
tests/test_gpu_free_space.py (device against mirror) and tests/test_cpp_free_space.py (the C++ header mpc_planner_modules/free_space.h against
the same mirror, through a binary file)."""
import functools

import numpy as np

from mpc_planner_amd import modules as md

PREFILL = -3.0
DT = 0.2
N, RANGE, N_ROWS = 20, 2.0, 12
N_PTS_MAX = 1100                                             # more than four full sweeps of a 256-thread block, plus a tail
N_SEG_MAX = 16
# the bitwise launch: point counts around one ballot word (63, 64, 65), one sweep (257), the cap, a count beyond the cap (clipped); then points
# outside every box, a dense ring (truncates), v = 0 (degenerate), a polyline that leaves the path's end; and two scenes that must stay
# untouched: main_of = -1, path count 0
BITWISE_COUNTS = (0, 1, 63, 64, 65, 257, 1100, 2000, 40, 60, 300, 300, 300, 300)
FAR, RING, STILL, PAST_END, NO_MAIN, NO_PATH = 8, 9, 10, 11, 12, 13


def waypoints():
    """A gently turning path of 12 waypoints, about 1.1 m apart, from the origin along +x."""
    heading = 0.25 * np.sin(np.arange(12) * 0.7)
    return np.concatenate([[[0.0, 0.0]], np.cumsum(np.stack([np.cos(heading), np.sin(heading)], 1) * 1.1, 0)[:-1]])


@functools.lru_cache(maxsize=None)
def fitted_path():
    fit = md.fit_path(waypoints())
    assert fit["status"] == 0 and fit["count"] == 11
    return fit


def _launch(Q, counts, n_pts_max, points, s0, v, n_rows, decomp_range, main_of=None, path_count=None):
    fit = fitted_path()
    path = np.full((Q, N_SEG_MAX, 9), PREFILL); path[:, :fit["count"]] = fit["path"]
    return dict(path=path, path_count=np.full(Q, fit["count"], np.int32) if path_count is None else path_count,
                path_length=np.full(Q, fit["length"]), s0=np.asarray(s0, float), v=np.asarray(v, float), state_x=np.linspace(-1.0, 2.0, Q),
                points=points, count=np.asarray(counts, np.int32), n_pts_max=n_pts_max, n_seg_max=N_SEG_MAX, n_rows=n_rows, range=decomp_range,
                main_of=np.arange(Q, dtype=np.int32) if main_of is None else main_of, N=v.shape[1] - 1, dt=DT)


@functools.lru_cache(maxsize=None)
def bitwise_launch():
    """Fourteen scenes on one fitted path, one batch entry per scene.  Slots behind a scene's count hold garbage that must not be read."""
    rng = np.random.default_rng(41)
    Q = len(BITWISE_COUNTS)
    fit = fitted_path()
    points = rng.normal(size=(Q, N_PTS_MAX, 2)) * 50.0
    v = rng.uniform(0.5, 2.5, (Q, N + 1))
    s0 = np.full(Q, 1.0)
    for q, c in enumerate(BITWISE_COUNTS):
        n = min(c, N_PTS_MAX)
        points[q, :n] = np.stack([rng.uniform(-1.0, 9.0, n), rng.uniform(-2.5, 4.5, n)], 1)
    points[FAR, :BITWISE_COUNTS[FAR]] += 50.0
    v[RING] = 0.1                                                        # a short polyline: one ring of 60 points, radius 1.5, encloses every segment
    mid, _ = md.decomp_path_points(fit["path"], fit["length"], 1.19, [0.0], DT)
    ang = 2.0 * np.pi * np.arange(60) / 60.0
    points[RING, :60] = mid[0][None, :] + 1.5 * np.stack([np.cos(ang), np.sin(ang)], 1)
    v[STILL] = 0.0
    s0[PAST_END] = fit["length"] - 2.0
    main_of = np.arange(Q, dtype=np.int32); main_of[NO_MAIN] = -1
    path_count = np.full(Q, fit["count"], np.int32); path_count[NO_PATH] = 0
    return _launch(Q, BITWISE_COUNTS, N_PTS_MAX, points, s0, v, N_ROWS, RANGE, main_of, path_count)


@functools.lru_cache(maxsize=None)
def scattered_launch(Q=64):
    """400 points scattered over [-1, 9] x [-3, 3] per scene around fast segments (v in [2, 4]: 0.4 - 0.8 m long): many points fall inside
    the first ellipse, so the shrink loop runs."""
    rng = np.random.default_rng(42)
    points = np.stack([rng.uniform(-1.0, 9.0, (Q, 400)), rng.uniform(-3.0, 3.0, (Q, 400))], 2)
    v = rng.uniform(2.0, 4.0, (Q, N + 1))
    return _launch(Q, np.full(Q, 400), 400, points, rng.uniform(0.0, 1.0, Q), v, N_ROWS, RANGE)


def mirror(case):
    """modules.decomp_halfspaces for every scene of a launch, laid out as the device writes it into buffers prefilled with PREFILL (count -3,
    status 7): an untouched scene keeps the prefill."""
    Q, Nn, n_rows = len(case["count"]), case["N"], case["n_rows"]
    out = dict(rows=np.full((Q, Nn, n_rows, 3), PREFILL), count=np.full((Q, Nn), -3, np.int32), status=np.full((Q, Nn), 7, np.uint8))
    for q in range(Q):
        n = int(case["path_count"][q])
        if case["main_of"][q] < 0 or n <= 0:
            continue
        m = min(max(int(case["count"][q]), 0), case["n_pts_max"])
        r = md.decomp_halfspaces(case["path"][q, :n], case["path_length"][q], case["s0"][q], case["v"][q, :Nn], case["dt"], case["points"][q, :m],
                                 case["range"], n_rows, case["state_x"][q])
        out["rows"][q], out["count"][q], out["status"][q] = r["rows"], r["count"], r["status"]
    return out


@functools.lru_cache(maxsize=None)
def bitwise_mirror():
    return mirror(bitwise_launch())


@functools.lru_cache(maxsize=None)
def scattered_mirror(Q=64):
    return mirror(scattered_launch(Q))


@functools.lru_cache(maxsize=None)
def corridor_scene(idx, n_traj=1, size=100):
    """One make_scene scene of the slack model with 12 decomp rows, on its costmap (scenes.with_costmap)."""
    from mpc_planner_amd import scenes
    sc = scenes.make_scene(idx, N=N, M=8, B=n_traj, slack=True, n_decomp=N_ROWS)
    return scenes.with_costmap(sc, 5000 + idx, size=size)


def corridor_decomp(sc, n_pts_max=md.DECOMP_MAX_POINTS):
    """The mirror's decomposition of a corridor scene: the points of its costmap, the polyline along the main solver's warm start."""
    pts, count, overflow = md.costmap_points(sc["costmap"], sc["costmap_origin"], sc["costmap_resolution"], n_pts_max)
    seg = sc["segments"]
    length = float(2.0 * seg[-1, 8] - seg[-2, 8])
    out = md.decomp_halfspaces(seg, length, sc["xinit"][0, 4], sc["x0"][0, :N, md.IDX["v"]], DT, pts, RANGE, N_ROWS, sc["xinit"][0, 0])
    out.update(points=pts, overflow=overflow, length=length)
    return out


def x0_of(case, nvar):
    """A warm start [Q][N + 1][nvar] that carries the launch's speeds in its v column and garbage elsewhere."""
    Q, Np1 = case["v"].shape
    x0 = np.random.default_rng(7).normal(size=(Q, Np1, nvar))
    x0[:, :, md.IDX["v"]] = case["v"]
    return x0
