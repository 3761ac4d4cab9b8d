"""The matrix of tests/test_gpu_solver_options.py without a GPU: what every (shape, option case) of tests/solver_option_cases.py has to give on the oracle
alone, so that the device comparison cannot fail for a reason that is no bug -- every entry succeeds; the oracle's integers are those of its other Riccati
form and of ulp-moved inputs; the sides a bound case names are active; the option moves the result; and the coverage ratchet -- every (kind, lanes per
stage, threads, team) among the instantiations the pick_*_kernel functions of csrc/tmpc_capi.hip name runs the matrix, or has a reason."""
import numpy as np
import pytest

import solver_option_cases as SC


def test_the_table_knows_the_default_bounds():
    import oracle_lib as O
    from mpc_planner_amd import solver
    pb, d = O.problem(), solver.default_dims()
    assert tuple(pb.lb) == SC.DEFAULT_LB == tuple(d.lb) and tuple(pb.ub) == SC.DEFAULT_UB == tuple(d.ub)
    for name in ("dt", "erk_steps", "reg_eps", "ipm_mu0", "ipm_thr0", "n_sqp"):
        assert getattr(pb, name) == getattr(d, name), name
    for o in SC.OPTION_CASES:                                     # every override is a field of both structures, and off its default
        for k, v in {**o["opts"], **o["baseline"]}.items():
            assert getattr(pb, k) != v and hasattr(d, k), (o["id"], k)
    for lbd, ubd in SC.ASYM_SETS.values():                          # all 14 changed, no two of one magnitude
        box = SC._box(lbd, ubd)
        mags = [abs(v) for v in box["lb"] + box["ub"]]
        assert len(set(mags)) == 14 and all(a != b for a, b in zip(box["lb"] + box["ub"], SC.DEFAULT_LB + SC.DEFAULT_UB)), box
        assert all(l < u for l, u in zip(box["lb"], box["ub"]))


SHAPE_MATRIX = SC.shape_matrix()


@pytest.mark.parametrize("shape,oid,fid", SHAPE_MATRIX, ids=[f"{s}: {o}" for s, o, _ in SHAPE_MATRIX])
def test_preconditions_on_the_oracle(shape, oid, fid):
    o = SC.OPTION[oid]
    r = SC.oracle_runs(shape, oid)
    info, opts, n = r["info"], r["opts"], len(r["moved"])
    assert n == SC.B_PER_SCENE * len(r["ids"])
    # success: every entry, under the option and under its baseline
    assert (info["exit_code"] == 1).all(), info["exit_code"]
    assert (r["ib"]["exit_code"] == 1).all(), r["ib"]["exit_code"]
    # activity
    counts = {f"{side} {var}": int(SC.active_entries(r["xt"], r["ut"], opts, side, var).sum()) for side, var in o["active"]}
    assert all(c >= 2 for c in counts.values()), counts
    lo, hi = SC.gaps(r["xt"], r["ut"], opts.get("lb", SC.DEFAULT_LB), opts.get("ub", SC.DEFAULT_UB))
    for side, var in o["active"]:                                   # (the device is asked for the same entries: none may sit on the threshold itself)
        gap = (lo if side == "lb" else hi)[:, SC.VARS.index(var)]
        assert (np.abs(np.abs(gap) - SC.ACTIVE) > SC.THRESHOLD_GUARD).all(), (side, var, gap)
    assert min(lo.min(), hi.min()) > -SC.VIOLATED
    if o["inactive"]:
        assert min(lo.min(), hi.min()) > SC.INACTIVE, (lo.min(axis=0), hi.min(axis=0))
        for k in SC.VERDICT:                                        # bounds nobody touches leave the oracle's integers where its default bounds do
            np.testing.assert_array_equal(info[k], r["ib"][k], err_msg=k)
    # the option matters
    share = r["mask"].mean()
    assert share >= 0.25, (share, np.sort(r["moved"]))
    # stability: the other Riccati form, ulp-moved inputs in either form
    sc = r["sc"]
    runs = [("other form", SC.oracle_solve(fid, sc, opts, rf=1))]
    runs += [(f"draw {d}", SC.oracle_solve(fid, sc, opts, rf=0, moved=100 + d)) for d in range(SC.DRAWS)]
    runs.append(("draw in the other form", SC.oracle_solve(fid, sc, opts, rf=1, moved=200)))
    worst = 0.0
    for what, (x2, u2, i2) in runs:
        for k in SC.VERDICT:
            np.testing.assert_array_equal(i2[k], info[k], err_msg=f"{what}: {k}")
        worst = max(worst, SC.distance(x2, u2, r["xt"], r["ut"]).max())
    print(f"[options] {shape}: {oid}: scenes {r['ids']} successes {int((info['exit_code'] == 1).sum())}/{n} active {counts} the option matters on "
          f"{int(r['mask'].sum())}/{n} (median move {np.median(r['moved']):.1e}, integers differ on {int(r['ints_differ'].sum())}) rounding sensitivity {worst:.1e}")
    assert worst < 1e-8, worst                                      # what the device is held to must not hang on the oracle's own rounding


def test_every_family_runs_the_four_common_cases():
    fams = SC.families()
    assert len(set(fams)) == len(fams) and set(SC.REDUCED) <= set(fams)
    for fid in fams:
        shape, got = SC.shape_of(fid), SC.options_of(fid)
        for oid in ("bounds upper", "bounds asymmetric inactive", "all off + bounds upper"):
            assert oid in got or (shape, oid) in SC.EXCLUDED, (fid, oid, got)
        assert any(oid in SC.LOWER_CASES for oid in got) or all((shape, oid) in SC.EXCLUDED for oid in SC.LOWER_CASES), (fid, got)
        assert not any((shape, oid) in SC.EXCLUDED for oid in got), (fid, got)
        if fid in SC.REDUCED:                                       # every option case, or a reason
            missing = [o["id"] for o in SC.OPTION_CASES if o["id"] not in got and (shape, o["id"]) not in SC.EXCLUDED]
            assert not missing, (fid, missing)
    assert all(reason.strip() for reason in SC.EXCLUDED.values())
    assert all(s in SC.shapes() and o in SC.OPTION for s, o in SC.EXCLUDED)


def test_every_kernel_family_runs_the_matrix():
    import test_gpu_carried_state as CS
    from test_dispatch_table import pick_instantiations
    named = {CS.family(n) for n in pick_instantiations() if "tmpc_gen::" not in n} | {("generic", 0, 64, "")}
    covered = {CS.family(SC.dispatch_case(fid)["expect"]) for fid in SC.families()}
    covered.add(CS.family(CS.GENERATED_DEFAULT))                     # tests/test_gpu_generated_tick.py: the cfg 2 library under two option cases
    orphans = sorted(named - covered - set(SC.FAMILY_EXCLUDED))
    assert not orphans, "kernel families (kind, lanes per stage, threads, team) without a row in tests/solver_option_cases.py (or FAMILY_EXCLUDED): " + repr(orphans)
    assert not sorted(set(SC.FAMILY_EXCLUDED) - named) and all(reason.strip() for reason in SC.FAMILY_EXCLUDED.values())
