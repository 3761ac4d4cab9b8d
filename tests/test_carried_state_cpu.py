"""The closed loop of tests/test_gpu_carried_state.py without a GPU: what its scene has to give on every case's shape, the oracle against itself in both
Riccati forms (each form carrying its own multipliers), and the coverage ratchet -- every (kind, lanes per stage, threads, team) among the
instantiations the pick_*_kernel functions of csrc/tmpc_capi.hip name has a closed-loop case, or a reason in EXCLUDED."""
import numpy as np
import pytest

import test_gpu_carried_state as CS

def _shapes():
    """One case id per distinct oracle problem (the Riccati form aside) among the loop cases."""
    seen = {}
    for cid in CS.LOOP_CASES:
        seen.setdefault(CS._shape_key(CS._case(cid), 0), cid)
    return list(seen.values())


@pytest.mark.parametrize("cid", _shapes())
def test_scene_supports_the_loop_and_the_oracle_agrees_with_itself_in_both_forms(cid):
    (schur, differs), (sqrt, differs_sq) = CS.oracle_loop(cid, rf=0), CS.oracle_loop(cid, rf=1)
    CS.check_loop_inputs(cid, schur, differs)
    CS.check_loop_inputs(cid, sqrt, differs_sq)
    worst = 0.0
    for t, (a, b) in enumerate(zip(schur, sqrt)):
        # what the GPU test asserts against the oracle must not hang on the oracle's own rounding: exit code and SQP count of every entry, QP status,
        # interior-point count and trajectory of the successful ones.  (A failed entry's QP diverges: whether it ends as status 3 or 4, and after how many
        # interior-point iterations, differs between the two forms on half of the shapes)
        ok = a["exit_code"] == 1
        for k in ("exit_code", "sqp_iter"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{cid}: tick {t}: {k}")
        for k in ("qp_status", "qp_iter_total"):
            np.testing.assert_array_equal(a[k][ok], b[k][ok], err_msg=f"{cid}: tick {t}: {k}")
        worst = max(worst, np.abs(a["xtraj"][ok] - b["xtraj"][ok]).max(), np.abs(a["utraj"][ok] - b["utraj"][ok]).max())
    print(f"[carried] {cid}: Schur against square-root form over {CS.TICKS} ticks {worst:.2e}; carried multipliers move the oracle by {differs:.2e}; "
          f"entry {CS.DOOMED} after its failure: {[int(r['exit_code'][CS.DOOMED]) for r in schur]}")
    assert worst < 1e-8, worst                                      # (observed: at most 5.6e-9, on the Gaussian rows at N = 30; 1.5e-9 elsewhere)


@pytest.mark.parametrize("cid", sorted(CS.BOUNDED_LOOPS))
def test_scene_supports_the_loop_with_active_bounds(cid):
    """The loop of CS.BOUNDED_LOOPS (no doomed entry): every entry succeeds at every tick with the three upper bounds active, in both Riccati forms, with the
    same integers and the same active sets."""
    import solver_option_cases as SC
    scene, _ = CS.BOUNDED_LOOPS[cid]
    opts = CS.bounded_options(cid)
    (schur, differs), (sqrt, differs_sq) = CS.oracle_loop(cid, rf=0, opts=opts, scene=scene), CS.oracle_loop(cid, rf=1, opts=opts, scene=scene)
    CS.check_bounded_loop_inputs(cid, schur, differs)
    CS.check_bounded_loop_inputs(cid, sqrt, differs_sq)
    worst = 0.0; counts = []
    for t, (a, b) in enumerate(zip(schur, sqrt)):
        for k in ("exit_code", "sqp_iter", "qp_status", "qp_iter_total"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{cid}: tick {t}: {k}")
        for var in CS.BOUNDED_LOOPS[cid][1]:
            np.testing.assert_array_equal(SC.active_entries(a["xtraj"], a["utraj"], opts, "ub", var), SC.active_entries(b["xtraj"], b["utraj"], opts, "ub", var))
        counts.append({var: int(SC.active_entries(a["xtraj"], a["utraj"], opts, "ub", var).sum()) for var in CS.BOUNDED_LOOPS[cid][1]})
        worst = max(worst, np.abs(a["xtraj"] - b["xtraj"]).max(), np.abs(a["utraj"] - b["utraj"]).max())
    print(f"[carried] {cid} with active bounds: scene {scene}: active entries per tick {counts}; Schur against square-root form {worst:.2e}; carried multipliers "
          f"move the oracle by {differs:.2e}")
    assert worst < 1e-8, worst
    assert set(CS.BOUNDED_LOOPS) <= set(CS.LOOP_CASES)


def test_every_kernel_family_has_a_closed_loop_case():
    import test_gpu_dispatch_matrix as T
    from test_dispatch_table import pick_instantiations
    named = {CS.family(n) for n in pick_instantiations() if "tmpc_gen::" not in n} | {("generic", 0, 64, "")}
    covered = {CS.family(CS._case(cid)["expect"]) for cid in CS.LOOP_CASES}
    covered.add(CS.family(CS.GENERATED_DEFAULT))                     # test_closed_loop_on_the_generated_cfg2_library
    orphans = sorted(named - covered - set(CS.EXCLUDED))
    assert not orphans, "kernel families (kind, lanes per stage, threads, team) without a closed loop in tests/test_gpu_carried_state.py LOOP_CASES (or EXCLUDED): " + repr(orphans)
    stale = sorted(set(CS.EXCLUDED) - named)
    assert not stale, stale
    assert all(reason.strip() for reason in CS.EXCLUDED.values())
    assert len(set(CS.LOOP_CASES)) == len(CS.LOOP_CASES) and set(CS.LOOP_CASES) <= {c["id"] for c in T.DISPATCH_CASES}


def test_family_of_an_instantiation_name():
    assert CS.family("fast<-1,12,4,128,ScanSoloT<2>,0>") == ("fast", 4, 128, "ScanSoloT<2>")
    assert CS.family("fast<8,8,3,64,Solo,0>") == ("fast", 3, 64, "Solo")
    assert CS.family("compact<20,8,4,128,1>") == ("compact", 4, 128, "")
    assert CS.family("generic<2>") == ("generic", 0, 64, "")
