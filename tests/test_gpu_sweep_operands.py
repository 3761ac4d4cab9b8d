"""The operand loads of the sequential Riccati loops (csrc/tmpc_riccati.hpp) at the smallest shapes at which they can go wrong.

Disjoint lane sets of the factorisation and the two vector sweeps share LDS loads through per-lane addresses: the pivot pair of lanes 0, 1 with the
Lxu pair of lanes 2..6 (both sweeps), y of lanes 0, 1 with rb of lanes 2..6 (forward sweep), a column's (x, y) and (psi, v, s) entries of [B A] as
neighbours of the table (factorisation, backward sweep), its rows at stride 2 (forward sweep).  A wrong base, stride or lane set shows as a wrong
iterate, so every shape below is solved by the fast kernel and by its compact twin (another LDS layout, the same arithmetic), which must agree
bit for bit, and both are compared with the CPU oracle as tests/test_gpu_parity._compare does: no mismatch in exit codes, SQP counts, QP status and
interior-point counts, iterates and objectives within 1e-8 relative.  B = 16 per case.  The shapes:
  (8,8) N = 2            the by-two unrolled sweeps run one pass and no remainder; N = 3: one pass and the odd remainder
  (8,8) N = 20           the benchmark's shape
  (12,12) N = 20         compact layout 3: y lives inside the stage's 30-double block (another base and stride of the merged y / rb load)
  (0,4) N = 20           no packed topology rows
  <-1,7,3> N = 20        a runtime-shape instantiation
  <-1,6,4> N = 22        two waves per trajectory (NTH = 128): the sweeps run on the other wave
  (8,8) N = 20, riccati_form = 1    the square-root form shares the sweeps (fast kernels only: no compact twin to compare with)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_dispatch_matrix import CP0, CP2_0, FIELDS, _dims, _problem, _running, _scenes, _slots, case

B = 16
# (case of the fast kernel, instantiation of the compact twin or None, lab switches that make the twin run at B = 16)
SHAPES = [
    (case("(8,8) N=2", "fast<8,8,3,64,Solo,0>", 2, 8, 8, B=B), "compact<8,8,3,64,0>", CP0),
    (case("(8,8) N=3", "fast<8,8,3,64,Solo,0>", 3, 8, 8, B=B), "compact<8,8,3,64,0>", CP0),
    (case("(8,8) N=20", "fast<8,8,3,64,Solo,0>", 20, 8, 8, B=B), "compact<8,8,3,64,0>", CP0),
    (case("(12,12) N=20", "fast<12,12,3,64,Solo,0>", 20, 12, 12, B=B), "compact<12,12,3,64,0>", CP0),
    (case("(0,4) N=20", "fast<0,4,3,64,Solo,0>", 20, 0, 4, ids=range(50, 66), B=B), "compact<0,4,3,64,0>", CP0),
    (case("<-1,7,3> N=20", "fast<-1,7,3,64,Solo,0>", 20, 3, 4, B=B), "compact<-1,7,3,64,0>", CP0),
    (case("<-1,6,4> N=22 two-wave", "fast<-1,6,4,128,Solo,0>", 22, 5, 5, S=3, B=B), "compact<-1,6,4,128,0>", CP2_0),
    (case("sqrt (8,8) N=20", "fast<-1,13,3,64,SoloSqrt,0>", 20, 8, 8, rf=1, B=B), None, None),
]


def _oracle(c):
    import oracle_lib as O
    sc = _scenes(c, B)
    xt, ut, info = O.solve_batch(_problem(c), sc["xinit"], sc["x0"].reshape(B, -1), sc["params"].reshape(B, -1))
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
def test_sweep_operand_loads(c, twin, lab, lab_library, monkeypatch):
    from test_gpu_parity import _compare
    sc, xt, ut, info = _oracle(c)
    ok = info["exit_code"] == 1
    assert ok.sum() >= B / 2, (int(ok.sum()), B)                   # the comparison is not made on failures alone
    fast = _run(c, sc, c["expect"])
    worst = max(_compare(fast, xt, ut, info))
    if twin is not None:
        for k, v in lab.items():
            monkeypatch.setenv(k, v)
        compact = _run(c, sc, twin)
        for f in FIELDS:
            assert np.array_equal(fast[f], compact[f], equal_nan=True), f
        worst = max(worst, *_compare(compact, xt, ut, info))
    print(f"[sweep operands] {c['id']}: successes {int(ok.sum())}/{B}, worst rel diff {worst:.2e}, twin {twin}")
