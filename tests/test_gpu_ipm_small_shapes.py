"""The interior-point iteration (csrc/tmpc_fast.hpp ipm_fast; the generic kernel's own loop) of every kernel family the dispatcher can pick, at small
horizons, on batches that hold the inputs its maxima, selects and wave reductions treat specially.

Families and horizons (the instantiation each case must report, as tests/test_gpu_dispatch_matrix.py does):
  one-wave compact and its fast twin        (8,8) N = 20      compact<8,8,3,64,0> / fast<8,8,3,64,Solo,0>          bitwise twins
  the same pair at the shortest horizon     (8,8) N = 2
  one-wave, more than ten rows per lane     (12,12) N = 20    compact<12,12,3,64,0> / fast<12,12,3,64,Solo,0>      bitwise twins
        (the two-waves-per-SIMD form that keeps fmax in its row passes: SLIM off in ipm_fast; its fast twin has it on)
  two waves                                 (8,8) N = 22      fast<8,8,4,128,Solo,0> / compact<8,8,4,128,0>        bitwise twins; N = 22 is the first two-wave horizon
  four-wave tick kernel (latency mode 3)    (8,8) N = 2       fast<8,8,12,256,ScanQuad,0>
  run-time shape                            (3,4) N = 2       fast<-1,7,3,64,Solo,0> / compact<-1,7,3,64,0>        bitwise twins (one arithmetic, two layouts)
  generic                                   (13,13) N = 21    generic<0>: 40 rows per stage is past every one-wave register-row kernel; at N <= 20 the
                                                              generic kernel starts at 55 rows, which needs the slack model's rows -- N = 21 is its smallest
                                                              horizon on the plain model
The twins are the pairs tests/test_gpu_riccati_pivot_pair_store.py and tests/test_gpu_dispatch_matrix.py already hold to equal bits.

Every batch is B = 32 trajectories (two scenes of 16) solved with qp_iter_max = 6, so that ordinary trajectories end interior-point loops at the
limit (QP status 2: the SQP loop goes on), plus
  entry 3:  contradictory topology rows (x <= x_k - gap and x >= x_k + gap at every stage, test_gpu_parity._make_infeasible's rows): the QP diverges.  The
            gap is the family's (FAMILIES), chosen from the ORACLE's run so that the divergence ends in a failure verdict before the iteration limit:
            at N >= 20 the factorisation meets a non-positive pivot in interior-point iteration 5 or 6 (QP status 4; the oracle's trace, ORC_IPM_TRACE,
            says "Fuu not PD" there: gap 5, and 100 for (12,12), whose gap-5 QP is still running at the limit); the two-stage problems never get that far
            at any gap from 5 to 1e8 -- theirs, at gap 1e8, ends with a step length below 1e-12 in iteration 3 (QP status 3);
  entry 5:  a NaN in one parameter (the right-hand side of topology row 0 at stage 1).
Checks, against the CPU oracle with the same options (the Riccati form the kernels run: 1 - rf in the oracle's numbering): exit codes and SQP counts of
every entry, QP status and interior-point counts of every entry the oracle ends with exit code 1, iterates and objectives within
test_gpu_parity._compare's tolerance (1e-8 relative next to the 1e-4 contract); entries 3 and 5 must fail (exit code other than 1) in the oracle
and so on the device; entry 3 must end with the family's failure verdict (PIVOT = 4 or STEP = 3) in the oracle and with a failure verdict in
every kernel -- PIVOT in the PIVOT families --, and at least one family must be a PIVOT one; at least one entry must end an interior-point loop
at the limit and at least a quarter must succeed.  The interior-point count of entry 3 is printed, not compared: a diverging QP amplifies rounding,
and the (8,8) N = 20 kernels meet their non-positive pivot one iteration after the oracle (6 against 5), as test_gpu_parity._compare allows for
entries the oracle does not end with exit code 1."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_dispatch_matrix import CP0, CP2_0, FIELDS, _dims, _problem, _running, _scenes, _slots, case

B = 32
QP_ITER_MAX = 6
DOOMED, NAN_ENTRY = 3, 5
PIVOT, STEP = 4, 3                 # QP status: non-positive pivot (or a NaN: not on this entry, whose inputs are finite), step length below 1e-12
TWO_WAVE = {"TMPC_NO_ONE_WAVE_N30": "1"}
# (case of the first kernel, instantiation of its bitwise twin or None, the twin's lab switches, entry 3's gap and the verdict it must end with)
FAMILIES = [
    (case("one wave (8,8) N=20", "fast<8,8,3,64,Solo,0>", 20, 8, 8, ids=(31, 32), B=B), "compact<8,8,3,64,0>", CP0, 5.0, PIVOT),
    (case("one wave (8,8) N=2", "fast<8,8,3,64,Solo,0>", 2, 8, 8, ids=(13, 14), B=B), "compact<8,8,3,64,0>", CP0, 1e8, STEP),
    (case("one wave (12,12) N=20", "fast<12,12,3,64,Solo,0>", 20, 12, 12, ids=(15, 16), B=B), "compact<12,12,3,64,0>", CP0, 100.0, PIVOT),
    (case("two waves (8,8) N=22", "fast<8,8,4,128,Solo,0>", 22, 8, 8, ids=(11, 12), B=B, lab=TWO_WAVE), "compact<8,8,4,128,0>", {**TWO_WAVE, **CP2_0}, 5.0, PIVOT),
    (case("four waves (8,8) N=2", "fast<8,8,12,256,ScanQuad,0>", 2, 8, 8, mode=3, ids=(13, 14), B=B), None, None, 1e8, STEP),
    (case("run-time shape (3,4) N=2", "fast<-1,7,3,64,Solo,0>", 2, 3, 4, ids=(11, 12), B=B), "compact<-1,7,3,64,0>", CP0, 1e8, STEP),
    (case("generic (13,13) N=21", "generic<0>", 21, 13, 13, ids=(1, 2), B=B), None, None, 5.0, PIVOT),
]


@functools.lru_cache(maxsize=None)
def _batch_and_oracle(N, n_lin, M, ids, gap):
    """The batch with its special entries and the oracle's answer: computed once per shape, shared by the cases of the shape, read-only."""
    import oracle_lib as O
    from test_gpu_parity import _make_infeasible
    c = case("", "", N, n_lin, M, ids=ids, B=B)
    sc = _scenes(c, B)
    sc["params"] = sc["params"].copy()
    sc = _make_infeasible(sc, [DOOMED])                                 # the rows, at gap 5
    pm = sc["pm"]
    sc["params"][DOOMED, 1:, pm.index("lin_constraint_0_b")] = sc["x0"][DOOMED, 1:-1, 2] - gap
    sc["params"][DOOMED, 1:, pm.index("lin_constraint_1_b")] = -sc["x0"][DOOMED, 1:-1, 2] - gap
    sc["params"][NAN_ENTRY, 1, sc["pm"].index("lin_constraint_0_b")] = np.nan
    pb = _problem(c)
    pb.riccati_form = 1 - c["rf"]
    pb.qp_iter_max = QP_ITER_MAX
    xt, ut, info = O.solve_batch(pb, sc["xinit"], sc["x0"].reshape(B, -1), sc["params"].reshape(B, -1))
    for a in (sc["xinit"], sc["x0"], sc["params"], xt, ut, *info.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return sc, xt, ut, info


def _run(c, sc, expect):
    from mpc_planner_amd import solver
    d = _dims(c)
    d.qp_iter_max = QP_ITER_MAX
    s = solver.BatchedSolver(d, B_max=B)
    if c["mode"]:
        assert s.set_latency_mode(c["mode"])
    slots, th = _slots(s.kernel_info())
    assert slots.get(_running(slots, c["mode"], B, th)) == expect, (expect, slots)
    s.set_batch(sc["xinit"], sc["x0"], sc["params"]); s.solve()
    got = s.get(); s.close()
    return got


def test_some_family_meets_a_non_positive_pivot():
    assert any(f[4] == PIVOT for f in FAMILIES)


@pytest.mark.parametrize("c,twin,lab,gap,verdict", FAMILIES, ids=[f[0]["id"] for f in FAMILIES])
def test_ipm_small_shapes(c, twin, lab, gap, verdict, lab_library, monkeypatch):
    from test_gpu_parity import _compare
    sc, xt, ut, info = _batch_and_oracle(c["N"], c["n_lin"], c["M"], tuple(c["ids"]), gap)
    ok = info["exit_code"] == 1
    assert info["exit_code"][DOOMED] != 1 and info["exit_code"][NAN_ENTRY] != 1, info["exit_code"]
    assert info["qp_status"][DOOMED] == verdict, (info["qp_status"][DOOMED], verdict)
    assert ok.sum() >= B // 4, int(ok.sum())
    assert (info["qp_status"] == 2).any(), "no entry ends an interior-point loop at the limit"
    for k, v in c["lab"].items():
        monkeypatch.setenv(k, v)
    got = {c["expect"]: _run(c, sc, c["expect"])}
    if twin is not None:
        for k, v in lab.items():
            monkeypatch.setenv(k, v)
        got[twin] = _run(c, sc, twin)
        for f in FIELDS:
            assert np.array_equal(got[c["expect"]][f], got[twin][f], equal_nan=True), f
    worst = 0.0
    for name, g in got.items():
        print(f"[ipm small shapes] {c['id']} {name}: doomed entry (exit, QP status, SQP, IPM) {tuple(int(g[f][DOOMED]) for f in ('exit_code', 'qp_status', 'sqp_iter', 'qp_iter_total'))}"
              f" oracle {tuple(int(info[f][DOOMED]) for f in ('exit_code', 'qp_status', 'sqp_iter', 'qp_iter_total'))};"
              f" NaN entry {tuple(int(g[f][NAN_ENTRY]) for f in ('exit_code', 'qp_status', 'sqp_iter', 'qp_iter_total'))}"
              f" oracle {tuple(int(info[f][NAN_ENTRY]) for f in ('exit_code', 'qp_status', 'sqp_iter', 'qp_iter_total'))}")
    for name, g in got.items():
        worst = max(worst, *_compare(g, xt, ut, info))                  # exit codes and SQP counts of all, status / counts / iterates of the successes
        assert g["exit_code"][DOOMED] != 1 and g["exit_code"][NAN_ENTRY] != 1, name
        assert g["qp_status"][DOOMED] in (STEP, PIVOT) and (verdict != PIVOT or g["qp_status"][DOOMED] == PIVOT), (name, int(g["qp_status"][DOOMED]), verdict)
    print(f"[ipm small shapes] {c['id']}: successes {int(ok.sum())}/{B}, exit codes {sorted(set(info['exit_code'].tolist()))}, "
          f"QP status at the limit on {int((info['qp_status'] == 2).sum())}, worst rel diff {worst:.2e}, twin {twin}")
