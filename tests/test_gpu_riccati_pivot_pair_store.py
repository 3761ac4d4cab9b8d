"""The merged stores of the sequential Riccati stage loops (csrc/tmpc_riccati.hpp) at the smallest shapes at which a store lane, base or stride can go wrong.

What the loops do: every store of a stage is a store of EVERY lane of the 16-lane row through a per-lane (base, stride) pair, and lanes that write to
different arrays share one instruction.
  factorisation (riccati_factor_rows, store_pairs): one pair store per stage -- lanes 2..6 the Lxu row of the stage's factor block, the extra row [y0 y1],
      lane 0 (1/L00, L10) at FB_R0 and lane 1 (L10, 1/L11) at FB_L10, both at the block stride; slot FB_L10 is written by both lanes with the same bits.
      Before, lane 1 stored the three pivot doubles in two instructions of its own through a second address.
  backward sweep (riccati_sweeps_rows): one store per stage -- lane 0 y0 to y_k[0], lane 1 y1 to y_k[1] (compact layout 3: inside the stage's 30-double
      block, at the block stride), lanes 2..6 p to pr[k NX + i].  Before, lane 0 stored the pair and lanes 2..6 p in a second instruction.
A wrong base or stride of lanes 0 / 1, a select that takes the wrong register, or a pivot that lands in a neighbouring block shows as a wrong iterate, a
NaN (QP status 4) or another iteration count: the forward sweep reads (1/L00, L10) on lane 0 and 1/L11 on lane 8, the backward sweep (1/L00, L10) and
(L10, 1/L11) on lanes 0 and 1, and both read y.  So every shape below is solved by the fast kernel and by its compact twin (another LDS layout: other
block strides, y in another place; the same arithmetic), which must agree bit for bit on every output field, and both are compared with the CPU oracle
as tests/test_gpu_parity._compare does: exit codes, SQP counts, QP status and interior-point counts equal, iterates and objectives within 1e-8 relative.
The oracle runs the recursion in the form the kernel runs; the two sides number the option the other way round (include/tmpc_hip.h: 0 = Schur
complement, 1 = square root; oracle/tmpc_oracle.h: 0 = square root, 1 = Schur complement), so _oracle sets 1 - rf, as tests/test_gpu_tight.py does.
B = 128 trajectories of scenes.make_batch per shape (two scenes of 64), with seeds at which the oracle ends at least one trajectory with an exit code
other than 1 and at least 90 % with exit code 1; both are asserted on the oracle's answer.  The shapes:
  (8,8) N = 20             the benchmark's shape
  (8,8) N = 19             an odd horizon: the by-two tail stage of the sweep
  (8,8) N = 2              the shortest trip
  (12,12) N = 20           compact layout 3: y inside the stage's block, so lanes 0 / 1 of the backward store use the block stride
  (8,8) N = 30             one wave at two lanes per stage
  (8,8) N = 30 two-wave    NTH = 128: one wave factorises, the other sweeps
  (8,8) N = 20, riccati_form = 1    the square-root form: seven columns through chol_rows<0>, the same pair store (fast kernels only: no compact twin)
test_pivot_verdicts_unchanged: the N = 2 batch of tests/test_gpu_riccati_fused_broadcast.py (seed 14, B = 64) in which the square-root form meets
non-positive pivots in eleven QPs and the Schur-complement form in none: the pair store carries the reciprocal pivots of exactly those stages (NaN or
infinite where the pivot is not positive), and the status-4 verdict of every kernel must stay the oracle's, trajectory by trajectory."""
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
# the batch with non-positive pivots: (id, case of the fast kernel, compact twin, the twin's lab switches, QPs the oracle ends with status 4)
PB = 64
PIVOT_BATCHES = [
    ("seed 14, Schur complement", case("(8,8) N=2", "fast<8,8,3,64,Solo,0>", 2, 8, 8, ids=(14,), B=PB), "compact<8,8,3,64,0>", CP0, 0),
    ("seed 14, square root", case("sqrt (8,8) N=2", "fast<-1,13,3,64,SoloSqrt,0>", 2, 8, 8, rf=1, ids=(14,), B=PB), None, None, 11),
]


@functools.lru_cache(maxsize=None)
def _oracle(N, n_lin, M, rf, ids, nb):
    """Scenes and the oracle's answer in the kernel's own form, computed once per (shape, form, seeds) and shared (the two N = 30 cases).
    rf is the kernels' numbering (tmpc_dims.riccati_form); the oracle gets the same form under its own number, 1 - rf."""
    import oracle_lib as O
    c = case("", "", N, n_lin, M, rf=rf, ids=ids, B=nb)
    sc = _scenes(c, nb)
    pb = _problem(c)
    pb.riccati_form = 1 - rf
    xt, ut, info = O.solve_batch(pb, sc["xinit"], sc["x0"].reshape(nb, -1), sc["params"].reshape(nb, -1))
    for a in (xt, ut, *info.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return sc, xt, ut, info


def _run(c, sc, expect, nb):
    from mpc_planner_amd import solver
    s = solver.BatchedSolver(_dims(c), B_max=nb)
    slots, th = _slots(s.kernel_info())
    assert slots.get(_running(slots, 0, nb, th)) == expect, (expect, slots)
    s.set_batch(sc["xinit"], sc["x0"], sc["params"]); s.solve()
    got = s.get(); s.close()
    return got


@pytest.mark.parametrize("c,twin,lab", SHAPES, ids=[s[0]["id"] for s in SHAPES])
def test_riccati_pivot_pair_store(c, twin, lab, lab_library, monkeypatch):
    from test_gpu_parity import _compare
    sc, xt, ut, info = _oracle(c["N"], c["n_lin"], c["M"], c["rf"], tuple(c["ids"]), B)
    ok = info["exit_code"] == 1
    assert ok.sum() < B, "no trajectory of these seeds fails"
    assert ok.sum() >= 0.9 * B, (int(ok.sum()), B)                 # the comparison is not made on failures
    for k, v in c["lab"].items():
        monkeypatch.setenv(k, v)
    fast = _run(c, sc, c["expect"], B)
    worst = max(_compare(fast, xt, ut, info))
    if twin is not None:
        for k, v in lab.items():
            monkeypatch.setenv(k, v)
        compact = _run(c, sc, twin, B)
        for f in FIELDS:
            assert np.array_equal(fast[f], compact[f], equal_nan=True), f
        worst = max(worst, *_compare(compact, xt, ut, info))
    print(f"[pivot pair store] {c['id']}: successes {int(ok.sum())}/{B}, exit codes {sorted(set(info['exit_code'].tolist()))}, "
          f"worst rel diff {worst:.2e}, twin {twin}")


@pytest.mark.parametrize("c,twin,lab,n_bad", [p[1:] for p in PIVOT_BATCHES], ids=[p[0] for p in PIVOT_BATCHES])
def test_pivot_verdicts_unchanged(c, twin, lab, n_bad, lab_library, monkeypatch):
    """QP status 4 (a non-positive pivot, or a negative diagonal entry of P) on exactly the oracle's trajectories, for the fast kernel and its twin."""
    sc, xt, ut, info = _oracle(c["N"], c["n_lin"], c["M"], c["rf"], tuple(c["ids"]), PB)
    bad = info["qp_status"] == 4
    assert int(bad.sum()) == n_bad, int(bad.sum())
    assert 0 < (info["exit_code"] != 1).sum() < PB
    for k, v in c["lab"].items():
        monkeypatch.setenv(k, v)
    got = {"fast": _run(c, sc, c["expect"], PB)}
    if twin is not None:
        for k, v in lab.items():
            monkeypatch.setenv(k, v)
        got["compact"] = _run(c, sc, twin, PB)
    for name, g in got.items():
        print(f"[pivot pair store] verdicts, {c['id']}, {name}: oracle {n_bad} of {PB} with QP status 4, device {int((g['qp_status'] == 4).sum())}")
    for name, g in got.items():
        assert np.array_equal(g["exit_code"], info["exit_code"]), name
        assert np.array_equal(g["qp_status"] == 4, bad), name
