"""The row broadcasts that the sequential Riccati stage loops fold into their multiply-adds (csrc/tmpc_riccati.hpp: chol_column_update, w_chains_update,
f_row_update in riccati_factor_rows / chol_rows, bwd_chain_update in riccati_sweeps_rows; TMPC_FMAC_BCAST16 in csrc/tmpc_kernels.hpp).

What changed: where a v_mov_b64_dpp row_newbcast fed one multiplicand of a v_fma_f64, one v_fmac_f64_dpp does both -- the same operands, the same single
rounding --, written as groups of inline assembly behind one hazard pad.  The compiler sees neither the lane numbers nor the hazards of such a group:
a wrong lane, a source and an accumulator exchanged, a term left out of a chain, a pad that is missing where the source was just written, or a path that
was meant to keep the plain broadcast and did not shows as a wrong iterate, a NaN (QP status 4) or another iteration count.  So every shape below is
solved by the fast kernel and by its compact twin where it has one (they share the loops' source and differ in the LDS layout, in the unrolling of the
factorisation and in the registers around the groups): the two must agree bit for bit on every output field, and each is compared with the CPU oracle
as tests/test_gpu_parity._compare does: exit codes, SQP counts, QP status and interior-point counts equal, iterates and objectives within 1e-8 relative.
The oracle runs the recursion in the form the kernel runs: the two sides number the option the other way round (include/tmpc_hip.h: tmpc_dims.riccati_form
0 = Schur complement, 1 = square root; oracle/tmpc_oracle.h: 0 = square root, 1 = Schur complement), so _oracle sets 1 - rf, as tests/test_gpu_tight.py
does.  On QPs that converge the forms agree to 4e-11; on QPs that diverge they end differently (test_non_positive_pivot_verdict).
B = 64 trajectories of scenes.make_batch per shape (one scene of 64; N = 3: two of 32, because at that horizon a scene's trajectories end alike), with
seeds at which the oracle ends at least one trajectory with an exit code other than 1 and at least half with exit code 1; both are asserted on the
oracle's answer.  The shapes:
  (8,8) N = 2              k + 1 = N and stage 0 in the same trip of the factorisation; eleven QPs of this batch diverge, and the square-root form
                           meets NON-POSITIVE PIVOTS in them (test_non_positive_pivot_verdict: the oracle's trace against the device's verdict)
  (8,8) N = 3, N = 19      the odd tail of the by-two loops
  (8,8) N = 20             the benchmark's shape: compact layout 2
  (12,12) N = 20           compact layout 3
  (8,8) N = 30             one wave at two lanes per stage
  (8,8) N = 30 two-wave    NTH = 128: one wave factorises, the other sweeps; layout 1 on the compact side
  (8,8) N = 20, riccati_form = 1    the square-root form: its seven-column elimination and its G products keep the plain broadcasts, its sweeps take the
                           folded chain (fast kernels only: no compact twin)
  (8,8) N = 20 generic     the generic kernel (lab switch TMPC_FORCE_GENERIC): the non-VEC factorisation and the predictor's own backward sweep (oracle only)"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_dispatch_matrix import CP0, CP2_0, FIELDS, _dims, _problem, _running, _scenes, _slots, case

B = 64
TWO_WAVE = {"TMPC_NO_ONE_WAVE_N30": "1"}
GENERIC = {"TMPC_FORCE_GENERIC": "1"}
PIVOT_CASE = "(8,8) N=2"
# (case of the fast / generic kernel with the scene seeds and the lab switches it needs, instantiation of the compact twin or None, the twin's lab switches)
SHAPES = [
    (case(PIVOT_CASE, "fast<8,8,3,64,Solo,0>", 2, 8, 8, ids=(14,), B=B), "compact<8,8,3,64,0>", CP0),
    (case("(8,8) N=3", "fast<8,8,3,64,Solo,0>", 3, 8, 8, ids=(582, 1), B=B), "compact<8,8,3,64,0>", CP0),
    (case("(8,8) N=19", "fast<8,8,3,64,Solo,0>", 19, 8, 8, ids=(26,), B=B), "compact<8,8,3,64,0>", CP0),
    (case("(8,8) N=20", "fast<8,8,3,64,Solo,0>", 20, 8, 8, ids=(31,), B=B), "compact<8,8,3,64,0>", CP0),
    (case("(12,12) N=20", "fast<12,12,3,64,Solo,0>", 20, 12, 12, ids=(16,), B=B), "compact<12,12,3,64,0>", CP0),
    (case("(8,8) N=30", "fast<8,8,2,64,Solo,0>", 30, 8, 8, ids=(12,), B=B), "compact<8,8,2,64,0>", CP0),
    (case("(8,8) N=30 two-wave", "fast<8,8,4,128,Solo,0>", 30, 8, 8, ids=(12,), B=B, lab=TWO_WAVE), "compact<8,8,4,128,0>", {**TWO_WAVE, **CP2_0}),
    (case("sqrt (8,8) N=20", "fast<-1,13,3,64,SoloSqrt,0>", 20, 8, 8, rf=1, ids=(31,), B=B), None, None),
    (case("generic (8,8) N=20", "generic<0>", 20, 8, 8, ids=(31,), B=B, lab=GENERIC), None, None),
]


@functools.lru_cache(maxsize=None)
def _oracle(N, n_lin, M, rf, ids):
    """Scenes, the oracle's problem and its answer, computed once per (shape, form, seeds) and shared (N = 30 twice, N = 2 with the pivot test).
    rf is the kernels' numbering (tmpc_dims.riccati_form); the oracle gets the same form under its own number, 1 - rf."""
    import oracle_lib as O
    c = case("", "", N, n_lin, M, rf=rf, ids=ids, B=B)
    sc = _scenes(c, B)
    pb = _problem(c)
    pb.riccati_form = 1 - rf
    xt, ut, info = O.solve_batch(pb, sc["xinit"], sc["x0"].reshape(B, -1), sc["params"].reshape(B, -1))
    for a in (xt, ut, *info.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return sc, pb, xt, ut, info


def _run(c, sc, expect):
    from mpc_planner_amd import solver
    s = solver.BatchedSolver(_dims(c), B_max=B)
    slots, th = _slots(s.kernel_info())
    assert slots.get(_running(slots, 0, B, th)) == expect, (expect, slots)
    s.set_batch(sc["xinit"], sc["x0"], sc["params"]); s.solve()
    got = s.get(); s.close()
    return got


@pytest.mark.parametrize("c,twin,lab", SHAPES, ids=[s[0]["id"] for s in SHAPES])
def test_riccati_fused_broadcast(c, twin, lab, lab_library, monkeypatch):
    from test_gpu_parity import _compare
    sc, _, xt, ut, info = _oracle(c["N"], c["n_lin"], c["M"], c["rf"], tuple(c["ids"]))
    ok = info["exit_code"] == 1
    assert ok.sum() < B, "no trajectory of these seeds fails"
    assert ok.sum() >= B / 2, (int(ok.sum()), B)                   # the comparison is not made on failures alone
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
    print(f"[fused broadcast] {c['id']}: successes {int(ok.sum())}/{B}, exit codes {sorted(set(info['exit_code'].tolist()))}, "
          f"worst rel diff {worst:.2e}, twin {twin}")


# (id, case of the fast kernel, compact twin or None, the twin's lab switches, whether the oracle meets non-positive pivots in the batch)
PIVOT_BATCHES = [
    ("seed 14, Schur complement", SHAPES[0][0], SHAPES[0][1], SHAPES[0][2], False),
    ("seed 14, square root", case("sqrt (8,8) N=2", "fast<-1,13,3,64,SoloSqrt,0>", 2, 8, 8, rf=1, ids=(14,), B=B), None, None, True),
]
assert PIVOT_BATCHES[0][1]["id"] == PIVOT_CASE


@pytest.mark.parametrize("c,twin,lab,pivots", [p[1:] for p in PIVOT_BATCHES], ids=[p[0] for p in PIVOT_BATCHES])
def test_non_positive_pivot_verdict(c, twin, lab, pivots, lab_library, monkeypatch, capfd):
    """Batches in which the factorisation meets non-positive pivots: the oracle says so on its trace (`riccati: Fuu not PD`, once per QP that it ends
    with status 4 for that reason).  The device's exit code and its verdict -- chol_rows' `bad`, or the sign test of P's diagonal, either of which ends
    the QP with status 4 -- must be the oracle's on every trajectory, for the fast kernel and for its compact twin.

    Both sides run the same form of the recursion (_oracle), because the two forms test different pivots: the square-root form all seven of a stage,
    the Schur-complement form the two input pivots and the sign bits of the five diagonal entries of P_{k+1}.  N = 2 with seed 14 is the failing batch
    of tests/test_gpu_forward_sweep_half_row.py: eleven of its QPs diverge.  The oracle's square-root form finds a non-positive pivot in each of the
    eleven (after 8 .. 11 interior-point iterations); its Schur-complement form finds none and ends the eleven with status 3 (step length below
    1e-12).  So that batch is solved in both forms: by the SoloSqrt kernel, whose verdicts must be the eleven, and by the fast and
    compact kernels of the default form, which must find none either.  (Compared with the oracle's OTHER form, as an earlier version of this test
    did by passing rf through unchanged, the default kernels' status 3 looks like eleven missed verdicts.)

    No batch in which the Schur-complement form itself meets a non-positive pivot is here, because none was found whose verdict the oracle itself
    holds on to.  The stage-loop tests' scenes have none; among scenes.make_batch's seeds 0 .. 699 at N = 2 .. 5 (and 0 .. 119 at N = 20), run on the
    oracle alone, seeds 470 and 664 at N = 2 have one such QP each.  In the one of seed 470 the interior-point method has diverged when the pivot
    test fails (iteration 16: stationarity residual 3e27; the pivot is -1.858e39 where the Hessian's entry is 1.870e39; the two steps before were
    1.2e-12 and 2.8e-12 long, and below 1e-12 the QP ends with status 3), and the oracle built with -ffp-contract=off ends both QPs with status 3
    (as the fast and the compact kernel end the one of seed 470, measured on an MI355X; exit codes and SQP counts of that batch equal the oracle's):
    their verdict is the rounding of one build of the oracle, not a property of the QP, so no kernel can be held to it.  The verdicts of seed 14
    are the same eleven (square root) and none (Schur complement) in both builds of the oracle."""
    import oracle_lib as O
    sc, pb, xt, ut, info = _oracle(c["N"], c["n_lin"], c["M"], c["rf"], tuple(c["ids"]))
    capfd.readouterr()
    monkeypatch.setenv("ORC_IPM_TRACE", "1")                       # (the trace is read per call: the cached answer above was computed without it)
    _, _, traced = O.solve_batch(pb, sc["xinit"], sc["x0"].reshape(B, -1), sc["params"].reshape(B, -1))
    monkeypatch.delenv("ORC_IPM_TRACE")
    n_pivot = capfd.readouterr().err.count("riccati: Fuu not PD")
    assert np.array_equal(traced["exit_code"], info["exit_code"]) and np.array_equal(traced["qp_status"], info["qp_status"])
    bad = info["qp_status"] == 4
    assert (n_pivot > 0) == pivots, n_pivot
    assert n_pivot == int(bad.sum()), (n_pivot, int(bad.sum()))   # every status-4 end of this batch is a pivot verdict (none is a non-finite residual)
    assert 0 < (info["exit_code"] != 1).sum() < B and bad.sum() < B
    got = {"fast": _run(c, sc, c["expect"])}
    if twin is not None:
        for k, v in lab.items():
            monkeypatch.setenv(k, v)
        got["compact"] = _run(c, sc, twin)
    for name, g in got.items():
        print(f"[fused broadcast] non-positive pivots, {c['id']}, {name}: oracle {n_pivot} of {B} with QP status 4, device QP status on those "
              f"{sorted(set(g['qp_status'][bad].tolist()))}, on the others {sorted(set(g['qp_status'][~bad].tolist()))}; exit codes equal "
              f"{bool(np.array_equal(g['exit_code'], info['exit_code']))}, SQP counts equal {bool(np.array_equal(g['sqp_iter'], info['sqp_iter']))}, "
              f"QP status equal {bool(np.array_equal(g['qp_status'], info['qp_status']))}")
    for name, g in got.items():
        assert np.array_equal(g["exit_code"], info["exit_code"]), name
    for name, g in got.items():
        assert np.array_equal(g["qp_status"] == 4, bad), name     # the `bad` verdict
