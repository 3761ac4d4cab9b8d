"""The scenes of the bitwise path-tracking tests (helper, no tests): one launch of tmpc_track_path with every case the kernel treats
differently, and the mirror's answer to it.  Shared by tests/test_gpu_path.py (device against mirror) and tests/test_cpp_path.py (the C++ header
mpc_planner_modules/reference_path.h against the same mirror, through a binary file)."""
import numpy as np

from mpc_planner_amd import modules as md, scenes

S = 5
N_SEG_MAX = 70
SEARCH_RANGE = 2


def straight(n, L=2.0):
    return np.array([[0.0, 0.0, 1.0, L * i, 0.0, 0.0, 0.0, 0.0, L * i] for i in range(n)])


def bitwise_scenes():
    """Seven scenes, n_seg_max = 70.  count: 1, 3 (fewer than S), 12, 70 (more than one candidate per lane in the global search), 0 (nothing
    is written), 12 with the previous segment 99 (clamped), 75 (clipped to n_seg_max).  Previous segments -1, -1, 4, -1, -1, 99, 68.  Positions:
    before the start, beyond the end, on a knot (an exact tie of two segments), generic.  Slots behind count hold garbage that must not be read
    as path.  Returns dict(path [7][70][9], count, length, bounds [7][2][70][8], pos [7][4], segment)."""
    rng = np.random.default_rng(14)
    n_sc = 7
    count = np.array([1, 3, 12, 70, 0, 12, 75], np.int32)
    prev = np.array([-1, -1, 4, -1, -1, 99, 68], np.int32)
    path = rng.normal(size=(n_sc, N_SEG_MAX, 9)) * 50.0                  # garbage behind count
    length = np.zeros(n_sc)
    for q in range(n_sc):
        n = min(int(count[q]), N_SEG_MAX)
        if n == 0:
            length[q] = 3.0
            continue
        path[q, :n] = straight(n) if q == 2 else scenes.reference_path_segments(np.random.default_rng(100 + q), S=n, seg_len=2.0)
        length[q] = 2.0 * n
    bounds = rng.normal(size=(n_sc, 2, N_SEG_MAX, 8)) * 50.0
    for q in range(n_sc):
        n = min(int(count[q]), N_SEG_MAX)
        bounds[q, 0, :n] = path[q, :n, :8]; bounds[q, 0, :n, 7] += 1.5 + 0.25 * q
        bounds[q, 1, :n] = path[q, :n, :8]; bounds[q, 1, :n, 7] -= 2.0 + 0.125 * q
        bounds[q, 1, :n, 5] += 0.01                                      # (the right bound is not parallel to the path: its own end tangent)
    pos = np.array([[-1.3, 0.4, 0.1, 1.0],                               # before the start
                    [7.5, -0.8, 0.0, 1.5],                               # beyond the end of a 6 m path
                    [10.0, 0.7, 0.0, 2.0],                               # on the knot between segments 4 and 5: the lower one wins
                    [133.1, 0.8, 0.0, 1.2],                              # generic, segment 66: the second candidate of lane 2
                    [1.0, 1.0, 0.0, 1.0],
                    [20.6, -0.3, 0.0, 1.0],                              # generic, inside the clamped range [9, 11]
                    [139.3, 0.2, 0.0, 1.0]])
    pos[6, :2] = np.add(md._path_end(path[6, :N_SEG_MAX], 2.0)[:2], (-0.7, 0.2))      # within 1 m of the end of the path: objective reached
    return dict(path=path, count=count, length=length, bounds=bounds, pos=pos, segment=prev)


def mirror(case, with_bounds, S_=S, search_range=SEARCH_RANGE, prefill=-3.0):
    """modules.track_path for every scene of bitwise_scenes(); scenes with count <= 0 keep the prefill and their segment."""
    n_sc = len(case["count"])
    seg = case["segment"].copy(); s = np.full(n_sc, prefill); window = np.full((n_sc, S_, 9), prefill)
    bw = np.full((n_sc, 2, S_, 8), prefill); reached = np.full(n_sc, 7, np.uint8)
    for q in range(n_sc):
        n = min(int(case["count"][q]), case["path"].shape[1])
        if n <= 0:
            continue
        kw = dict(left=case["bounds"][q, 0, :n], right=case["bounds"][q, 1, :n]) if with_bounds else {}
        out = md.track_path(case["path"][q, :n], case["length"][q], case["pos"][q, :2], S_, segment=int(case["segment"][q]),
                            search_range=search_range, **kw)
        seg[q] = out["segment"]; s[q] = out["s"]; window[q] = out["window"]; reached[q] = int(out["reached"])
        if with_bounds:
            bw[q, 0] = out["left"]; bw[q, 1] = out["right"]
    return dict(segment=seg, s=s, window=window, bound_window=bw, reached=reached)
