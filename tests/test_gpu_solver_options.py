"""GPU: every solve-kernel family with model bounds that bind and with solver options off their defaults, against the CPU oracle under the same options.

The dispatch matrix, the closed loops and the parity tests run at the tmpc_dims that tmpc_default_dims* writes, on scenes whose solutions stay clear of
every model bound: the 14 box rows per stage -- cold start, ratio test, multipliers, once per kernel family -- only ever act as far-away barrier terms,
most bound pairs are symmetric (ub[i] read for lb[i] returns the same bits), and dt, erk_steps, reg_eps, ipm_mu0, ipm_thr0, n_sqp never leave their
defaults.  The cases, the bound values per shape and the oracle runs are tests/solver_option_cases.py; tests/test_solver_option_cases.py (no GPU) holds
them to their preconditions.  Each (family, option case) asserts
  1. tmpc_kernel_info names the expected instantiation for the slot the launch runs;
  2. the oracle's exit code, SQP count, QP status and interior-point count of every entry (all succeed; latency mode 2 keeps its interior-point rule,
     test_gpu_parity._compare_relaxed_iterations), trajectories and objective within 1e-4 and within the 1e-8 regression line;
  3. discrimination: on the entries where the option moves the oracle (>= 1e-7, or an integer), the device is at least 10 x closer to the oracle under the
     option than the oracle's baseline run is, or its integers are the option run's and not the baseline's -- a kernel that ignores the option fails;
  4. bound cases: the device's own solution has the named sides active (< 1e-4) in the entries the oracle's has, and violates no bound by more than 1e-6;
  5. the same launch twice gives the same bits.
Measured on an MI355X, worst relative difference per stage between device and oracle over a case's families -- all below 1e-9, so every case is
held to the 1e-8 line: bounds upper 4.4e-11, bounds x 2.5e-11, bounds psi lower 1.3e-11, bounds w lower 5.5e-10, bounds w upper 8.7e-11, bounds a lower 5.4e-10,
bounds asymmetric inactive 5.3e-11, dt 0.25 9.8e-11, erk 1 at dt 0.4 8.9e-10, reg 1e-6 2.6e-10, reg 1e-2 2.7e-11, mu0 only 0.1 1.2e-11, thr0 only 0.1 8.5e-11,
mu0 thr0 (1, 1) 1.5e-10, n_sqp 3 1.2e-11, n_sqp 25 2.9e-12, all off + bounds upper 2.3e-10."""
import numpy as np
import pytest

import solver_option_cases as SC

pytestmark = pytest.mark.gpu

FIELDS = ("xtraj", "utraj", "pobj", "exit_code", "qp_status", "sqp_iter", "qp_iter_total", "res_eq")
TIGHT, HARD = 1e-8, 1e-6
# (family, option case) -> its line where a correct kernel measures above 1e-9: 1000 x the measured value, never above HARD (none so far)
LINES = {}

MATRIX = SC.matrix()


@pytest.mark.parametrize("fid,oid", MATRIX, ids=[f"{f}: {o}" for f, o in MATRIX])
def test_option_case(fid, oid, request, monkeypatch):
    import test_gpu_dispatch_matrix as T
    from mpc_planner_amd import solver
    from test_gpu_parity import _compare, _compare_relaxed_iterations
    c = SC.dispatch_case(fid)
    o = SC.OPTION[oid]
    if c["lab"]:
        for k, v in c["lab"].items():
            monkeypatch.setenv(k, v)
        request.getfixturevalue("lab_library")
    r = SC.oracle_runs(SC.shape_of(fid), oid, c["rf"])
    sc, opts, xt, ut, info = r["sc"], r["opts"], r["xt"], r["ut"], r["info"]
    B = sc["xinit"].shape[0]
    assert (info["exit_code"] == 1).all() and r["mask"].mean() >= 0.25            # (tests/test_solver_option_cases.py, once more where it is used)
    dims = T._dims(c)
    for k, v in opts.items():
        setattr(dims, k, v)
    s = solver.BatchedSolver(dims, B_max=B)
    assert s.set_latency_mode(c["mode"]) or c["mode"] == 0
    slots, th = T._slots(s.kernel_info())
    slot = T._running(slots, c["mode"], B, th)
    # 1. the instantiation that runs
    assert slots.get(slot) == c["expect"], (slot, slots)
    assert sc["params"].shape[2] == s.npar
    got = T._solve(s, sc)
    # 2. against the oracle under the same options
    line = LINES.get((fid, oid), TIGHT)
    assert line <= HARD
    dist = SC.distance(got["xtraj"], got["utraj"], xt, ut)
    pobj = np.abs(got["pobj"] - info["pobj"]) / np.maximum(np.abs(info["pobj"]), 1.0)
    if slot == "lat2":                                             # (the regression line where the interior-point counts agree, as in the dispatch matrix)
        _compare_relaxed_iterations(got, xt, ut, info)
        same = got["qp_iter_total"] == info["qp_iter_total"]
        worst = max(dist[same].max(initial=0.0), pobj[same].max(initial=0.0))
    else:
        _compare(got, xt, ut, info, tight=line)
        worst = max(dist.max(), pobj.max())
    print(f"[options] {fid}: {oid}: {slot}={c['expect']} B {B} worst rel diff {worst:.2e} (line {line:.0e})")
    assert worst < line, worst
    # 3. discrimination
    mask = r["mask"]
    base = r["moved"]                                               # the oracle's baseline run against its run under the option, per entry
    ints_option = np.ones(B, bool); ints_base = np.ones(B, bool)
    for k in SC.VERDICT:
        ints_option &= got[k] == info[k]; ints_base &= got[k] == r["ib"][k]
    told = (10.0 * dist <= base) | (ints_option & ~ints_base)
    print(f"[options] {fid}: {oid}: the option matters on {int(mask.sum())}/{B} entries; closest call: device {dist[mask].max():.1e} against baseline "
          f"{base[mask].min():.1e}")
    assert told[mask].all(), (np.flatnonzero(mask & ~told), dist[mask], base[mask])
    # 4. the bound cases: active where the oracle's are, none violated
    lb, ub = opts.get("lb", SC.DEFAULT_LB), opts.get("ub", SC.DEFAULT_UB)
    lo, hi = SC.gaps(got["xtraj"], got["utraj"], lb, ub)
    assert min(lo.min(), hi.min()) > -SC.VIOLATED, (lo.min(axis=0), hi.min(axis=0))
    for side, var in o["active"]:
        want = SC.active_entries(xt, ut, opts, side, var)
        have = SC.active_entries(got["xtraj"], got["utraj"], opts, side, var)
        assert want.sum() >= 2 and np.array_equal(want, have), (side, var, np.flatnonzero(want), np.flatnonzero(have))
    if o["inactive"]:
        assert min(lo.min(), hi.min()) > SC.INACTIVE
    # 5. launch to launch
    s.solve(); again = s.get()
    for k in FIELDS:
        assert np.array_equal(again[k], got[k]), k
    s.close()
