"""bench.py's roofline model is SURVEY.md 8(d)'s: compulsory bytes and algorithmic flops per solve, checked against the
figures stated there (cfg 2: 23,976 B; ~1.06e7 flop at 10 RTI x 10 IPM iterations).  No GPU needed."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench


def test_bytes_per_solve_is_the_survey_figure():
    assert bench.bytes_per_solve() == 8 * (2700 + 147 + 5 + 105 + 40) == 23976           # cfg 2
    assert bench.bytes_per_solve(npar=83) == 15656                                        # cfg 1
    assert bench.bytes_per_solve(npar=175) == 30376                                       # cfg 4


def test_flops_per_solve_is_the_survey_model():
    f = bench.flops_per_solve(10, 10)
    assert abs(f - 1.06e7) / 1.06e7 < 0.01
    # linear in the RTI count, affine in the IPM count
    assert bench.flops_per_solve(5, 10) * 2 == f
    assert bench.flops_per_solve(10, 4) < f


def test_usable_cpus_is_positive_and_bounded_by_the_visible_cpus():
    n = bench.usable_cpus()
    assert 1 <= n <= (os.cpu_count() or 1)


def test_write_outputs_float64_whole_or_one_seeded_sample(tmp_path):
    """--dump-outputs: float64 files; under the cap every array whole, over it the same seeded sample of trajectories in every per-trajectory
    array (plus trajectory_index) -- the same files from run to run."""
    import numpy as np
    B = 1000
    arrays = {"xtraj": np.arange(B * 6, dtype=np.float64).reshape(B, 3, 2), "exit_code": np.arange(B, dtype=np.int32) % 5,
              "best_index": np.array([3, -1], np.int32)}
    shapes = bench.write_outputs(str(tmp_path / "whole"), arrays, B)
    assert shapes == {"xtraj": [B, 3, 2], "exit_code": [B], "best_index": [2]}
    for k, v in arrays.items():
        got = np.load(tmp_path / "whole" / f"{k}.npy")
        assert got.dtype == np.float64 and np.array_equal(got, v)
    limit = 8 * 2000                                            # room for 2000 float64 values: 7 per trajectory kept -> 285 trajectories
    for run in ("a", "b"):
        shapes = bench.write_outputs(str(tmp_path / run), arrays, B, limit=limit)
        assert sum(int(np.prod(s)) for s in shapes.values()) * 8 <= limit
    idx = np.load(tmp_path / "a" / "trajectory_index.npy").astype(int)
    assert 0 < len(idx) < B and np.all(np.diff(idx) > 0)
    for k in ("xtraj", "exit_code", "best_index", "trajectory_index"):
        a, b = np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy")
        assert a.dtype == np.float64 and np.array_equal(a, b)
    assert np.array_equal(np.load(tmp_path / "a" / "xtraj.npy"), arrays["xtraj"][idx])
    assert np.array_equal(np.load(tmp_path / "a" / "best_index.npy"), arrays["best_index"])
