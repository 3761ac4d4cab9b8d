"""The forward Riccati sweep's two lane groups (csrc/tmpc_riccati.hpp, riccati_sweeps_rows) at the smallest shapes at which a lane role can go wrong.

What the sweep does: group A (lanes 0..6 of the 16-lane row) is the stage vector [u; x]; group B (lanes 8..14) shadows it for the second column of
Lxu -- lane 8 holds (y1, 1/L11), lanes 10..14 a copy of dx with Lxu_i1, the same rb_i and the same row of [B E] --, one product and one chain of five
row shifts reduce both columns (lane 0 sums lanes 2..6, lane 8 lanes 10..14), u1 is broadcast from lane 8, and the compact layouts read E = A - I from
the constant table.  A wrong base, stride or lane set of the per-lane loads, a shift that crosses the groups, or a shadow dx that drifts from group A's
shows as a wrong iterate.  So every shape below is solved by the fast kernel and by its compact twin (another LDS layout: other strides per lane, the
table instead of the dense [B A]; the same arithmetic), which must agree bit for bit on every output field, and both are compared with the CPU oracle as
tests/test_gpu_parity._compare does: exit codes, SQP counts, QP status and interior-point counts equal, iterates and objectives within 1e-8 relative.
B = 128 trajectories of scenes.make_batch per shape (two scenes of 64), with seeds at which the oracle ends at least one trajectory with an exit code
other than 1 (the failure path leaves the sweeps early) and at least 90 % with exit code 1; both are asserted on the oracle's answer.  The shapes:
  (8,8) N = 20             the benchmark's shape
  (8,8) N = 19             an odd horizon: the by-two loop's tail stage
  (8,8) N = 2              the shortest by-two trip (tmpc_create refuses N = 1)
  (12,12) N = 20           compact layout 3: y inside the stage's 30-double block (lane 8 reads y1 at another base and stride)
  (8,8) N = 30             the one-wave kernels at two lanes per stage
  (8,8) N = 30 two-wave    NTH = 128: the sweeping wave alternates, the other wave's lanes take no role
  (8,8) N = 20, riccati_form = 1    the square-root form shares the sweeps (fast kernels only: no compact twin to compare with)"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_dispatch_matrix import CP0, CP2_0, FIELDS, _dims, _problem, _running, _scenes, _slots, case

B = 128
TWO_WAVE = {"TMPC_NO_ONE_WAVE_N30": "1"}
# (case of the fast kernel with the scene seeds and the lab switches it needs, instantiation of the compact twin or None, the twin's lab switches)
SHAPES = [
    (case("(8,8) N=20", "fast<8,8,3,64,Solo,0>", 20, 8, 8, ids=(31, 32), B=B), "compact<8,8,3,64,0>", CP0),
    (case("(8,8) N=19", "fast<8,8,3,64,Solo,0>", 19, 8, 8, ids=(25, 26), B=B), "compact<8,8,3,64,0>", CP0),
    (case("(8,8) N=2", "fast<8,8,3,64,Solo,0>", 2, 8, 8, ids=(13, 14), B=B), "compact<8,8,3,64,0>", CP0),
    (case("(12,12) N=20", "fast<12,12,3,64,Solo,0>", 20, 12, 12, ids=(15, 16), B=B), "compact<12,12,3,64,0>", CP0),
    (case("(8,8) N=30", "fast<8,8,2,64,Solo,0>", 30, 8, 8, ids=(11, 12), B=B), "compact<8,8,2,64,0>", CP0),
    (case("(8,8) N=30 two-wave", "fast<8,8,4,128,Solo,0>", 30, 8, 8, ids=(11, 12), B=B, lab=TWO_WAVE), "compact<8,8,4,128,0>", {**TWO_WAVE, **CP2_0}),
    (case("sqrt (8,8) N=20", "fast<-1,13,3,64,SoloSqrt,0>", 20, 8, 8, rf=1, ids=(31, 32), B=B), None, None),
]


@functools.lru_cache(maxsize=None)
def _oracle(N, n_lin, M, rf, ids):
    """Scenes and the oracle's answer, computed once per (shape, seeds) and shared (the two N = 30 cases)."""
    import oracle_lib as O
    c = case("", "", N, n_lin, M, rf=rf, ids=ids, B=B)
    sc = _scenes(c, B)
    xt, ut, info = O.solve_batch(_problem(c), sc["xinit"], sc["x0"].reshape(B, -1), sc["params"].reshape(B, -1))
    for a in (xt, ut, *info.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return sc, xt, ut, info


def _run(c, sc, expect):
    from mpc_planner_amd import solver
    s = solver.BatchedSolver(_dims(c), B_max=B)
    slots, th = _slots(s.kernel_info())
    assert slots.get(_running(slots, 0, B, th)) == expect, (expect, slots)
    s.set_batch(sc["xinit"], sc["x0"], sc["params"]); s.solve()
    got = s.get(); s.close()
    return got


@pytest.mark.parametrize("c,twin,lab", SHAPES, ids=[s[0]["id"] for s in SHAPES])
def test_forward_sweep_half_row(c, twin, lab, lab_library, monkeypatch):
    from test_gpu_parity import _compare
    sc, xt, ut, info = _oracle(c["N"], c["n_lin"], c["M"], c["rf"], tuple(c["ids"]))
    ok = info["exit_code"] == 1
    assert ok.sum() < B, "no trajectory of these seeds leaves the solve early"
    assert ok.sum() >= 0.9 * B, (int(ok.sum()), B)                 # the comparison is not made on failures
    for k, v in c["lab"].items():
        monkeypatch.setenv(k, v)
    fast = _run(c, sc, c["expect"])
    worst = max(_compare(fast, xt, ut, info))
    if twin is not None:
        for k, v in lab.items():
            monkeypatch.setenv(k, v)
        compact = _run(c, sc, twin)
        for f in FIELDS:
            assert np.array_equal(fast[f], compact[f], equal_nan=True), f
        worst = max(worst, *_compare(compact, xt, ut, info))
    print(f"[forward sweep] {c['id']}: successes {int(ok.sum())}/{B}, exit codes {sorted(set(info['exit_code'].tolist()))}, "
          f"worst rel diff {worst:.2e}, twin {twin}")
