"""The per-stage operand addresses of the sequential Riccati loops (csrc/tmpc_riccati.hpp: riccati_factor_rows, riccati_sweeps_rows) at the smallest
shapes at which a base, a stride or a clamp can be wrong.

Every operand stream of the three stage loops -- the factorisation's Hh row / gh load, its table / rb loads, the P-row store at k + 1, the Lxu / y
pair store and lane 1's pivot store; the sweeps' gh / q and y / rb loads, their table column / row, the lane's pair of the stage's factor block and
the stores of y, p, du and dx -- is a per-lane (base pointer, stride in bytes) pair evaluated once, and the stage's address is one multiply-add
(at8, csrc/tmpc_kernels.hpp).  A wrong base, a stride left in elements, a clamp lost at stage 0 or a store one stage off shows as a wrong iterate or
a wrong exit code.  So every shape below is solved by the fast kernel and by its compact twin where it has one (another LDS layout: another block
stride, the constant table instead of the dense [B A], y inside the block for layout 3; the same arithmetic): the two must agree bit for bit on
every output field, and both are compared with the CPU oracle as tests/test_gpu_parity._compare does: exit codes, SQP counts, QP status and
interior-point counts equal, iterates and objectives within 1e-8 relative.
B = 128 trajectories of scenes.make_batch per shape, with seeds at which the oracle ends at least one trajectory with an exit code other than 1 (the
failure path leaves the loops early) and at least 90 % with exit code 1; both are asserted on the oracle's answer.  (Two scenes of 64, except N = 3:
at that horizon a scene's trajectories end alike -- of 4000 scenes none ends with 1 to 63 successes --, so the batch is sixteen scenes of 8, one of
which fails.)  The shapes:
  (8,8) N = 2              k + 1 = N and the stage-0 clamp in the same trip (tmpc_create refuses N = 1)
  (8,8) N = 3, N = 19      the odd tail of the by-two loops
  (8,8) N = 20             the benchmark's shape: compact layout 2, block stride 29
  (12,12) N = 20           compact layout 3: stride 30, y inside the stage's block
  <-1,7,3> nr = 21         a run-time-shape kernel: compact layout 1, stride 28
  (8,8) N = 30             one wave at two lanes per stage
  (8,8) N = 30 two-wave    NTH = 128: one wave sweeps, layout 1 on the compact side
  (8,8) N = 20, riccati_form = 1    the square-root form (SQ path; fast kernels only: no compact twin)
  N = 20 nr = 40, curvature-aware cost    the generic kernel: the non-VEC factorisation and the predictor's own backward sweep (no twin: oracle only)"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_dispatch_matrix import CP0, CP2_0, FIELDS, _dims, _problem, _running, _scenes, _slots, case

B = 128
TWO_WAVE = {"TMPC_NO_ONE_WAVE_N30": "1"}
# (case of the fast / generic kernel with the scene seeds and the lab switches it needs, instantiation of the compact twin or None, the twin's lab switches)
SHAPES = [
    (case("(8,8) N=2", "fast<8,8,3,64,Solo,0>", 2, 8, 8, ids=(13, 14), B=B), "compact<8,8,3,64,0>", CP0),
    (case("(8,8) N=3", "fast<8,8,3,64,Solo,0>", 3, 8, 8, ids=(582, *range(1, 16)), B=B), "compact<8,8,3,64,0>", CP0),
    (case("(8,8) N=19", "fast<8,8,3,64,Solo,0>", 19, 8, 8, ids=(25, 26), B=B), "compact<8,8,3,64,0>", CP0),
    (case("(8,8) N=20", "fast<8,8,3,64,Solo,0>", 20, 8, 8, ids=(31, 32), B=B), "compact<8,8,3,64,0>", CP0),
    (case("(12,12) N=20", "fast<12,12,3,64,Solo,0>", 20, 12, 12, ids=(15, 16), B=B), "compact<12,12,3,64,0>", CP0),
    (case("<-1,7,3> nr=21", "fast<-1,7,3,64,Solo,0>", 20, 3, 4, ids=(9, 10), B=B), "compact<-1,7,3,64,0>", CP0),
    (case("(8,8) N=30", "fast<8,8,2,64,Solo,0>", 30, 8, 8, ids=(11, 12), B=B), "compact<8,8,2,64,0>", CP0),
    (case("(8,8) N=30 two-wave", "fast<8,8,4,128,Solo,0>", 30, 8, 8, ids=(11, 12), B=B, lab=TWO_WAVE), "compact<8,8,4,128,0>", {**TWO_WAVE, **CP2_0}),
    (case("sqrt (8,8) N=20", "fast<-1,13,3,64,SoloSqrt,0>", 20, 8, 8, rf=1, ids=(31, 32), B=B), None, None),
    (case("generic N=20 nr=40", "generic<1>", 20, 13, 13, cm=1, ids=(45, 46), B=B), None, None),
]


@functools.lru_cache(maxsize=None)
def _oracle(N, n_lin, M, cm, rf, ids):
    """Scenes and the oracle's answer, computed once per (shape, seeds) and shared (the two N = 30 cases)."""
    import oracle_lib as O
    c = case("", "", N, n_lin, M, cm=cm, rf=rf, ids=ids, B=B)
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
def test_riccati_stage_addresses(c, twin, lab, lab_library, monkeypatch):
    from test_gpu_parity import _compare
    sc, xt, ut, info = _oracle(c["N"], c["n_lin"], c["M"], c["cm"], c["rf"], tuple(c["ids"]))
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
    print(f"[stage addresses] {c['id']}: successes {int(ok.sum())}/{B}, exit codes {sorted(set(info['exit_code'].tolist()))}, "
          f"worst rel diff {worst:.2e}, twin {twin}")
