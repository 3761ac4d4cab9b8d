"""Every handle keeps its inputs, the slot map and its outputs in ONE device allocation each (csrc/tmpc_handle_layout.hpp).  Control-tick handles mirror both
in pinned host memory (round 6: tmpc_set_batch = one asynchronous H2D copy, tmpc_set_slots without a stream synchronisation, tmpc_get = one D2H copy;
csrc/tmpc_capi.hip).  Larger handles have no mirrors: the runtime's own path for pageable memory and a stream synchronisation.  Both must be the same
function of the caller's arrays: bit for bit, for every batch size up to B_max and every transfer path, with and without a slot map, when the caller reuses
or overwrites its arrays right after the call, and when only some outputs are asked for."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("xtraj", "utraj", "pobj", "exit_code", "qp_status", "sqp_iter", "res_eq", "qp_iter_total")


def _scene(B, scene=4):
    from mpc_planner_amd import scenes
    return scenes.make_scene(scene, B=B, N=20, M=8)


def _dims():
    from mpc_planner_amd import solver
    return solver.default_dims(N=20, S=5, n_lin=8, M=8)


def _small_dims():
    from mpc_planner_amd import solver
    return solver.default_dims(N=20, S=1, n_lin=2, M=2)         # npar 39: 7456 B of inputs per trajectory


def _small_scene(B):
    from mpc_planner_amd import scenes
    return scenes.make_scene(4, N=20, M=2, B=B, S=1)


# (dims, scene, B_max of the small handle, batch sizes, share of the last batch that has to end with exit code 1, or None).  cfg 2 takes 22 816 B of inputs per
# trajectory: 22 trajectories are the last batch through the mirror (<= 512 KiB), 23 the first copied directly INTO the mirrored handle's allocation.
CASES = {
    # inputs 1.4 MB, outputs 90 KB: params start below 256 KiB (one H2D copy), the output block is one D2H copy
    "cfg2-64": (_dims, _scene, 64, (1, 5, 8, 22, 23, 64), None),
    "cfg2-91-largest-mirrored": (_dims, _scene, 91, (1, 22, 23, 91), None),
    "cfg2-92-first-without-mirrors": (_dims, _scene, 92, (1, 92), None),
    # params start at 331 008 B (> 256 KiB: three H2D copies out of the mirror), outputs 325 376 B (> 256 KiB: per-array D2H copies into the mirror);
    # 70 x 7456 B is the last batch through the mirror.  The CPU oracle ends 270 of these 272 with exit code 1 (two with 4)
    "npar39-272-three-copies-per-array-download": (_small_dims, _small_scene, 272, (1, 70, 71, 272), 0.5),
}


@pytest.mark.parametrize("case", list(CASES))
def test_small_and_large_handles_agree_bitwise(case):
    from mpc_planner_amd import solver
    dims, scene, B_max, sizes, solved_share = CASES[case]
    sc = scene(B_max)
    small = solver.BatchedSolver(dims(), B_max=B_max)
    large = solver.BatchedSolver(dims(), B_max=4096)            # tens of MB of inputs: no mirrors
    for B in sizes:
        res = []
        for s in (small, large):
            s.set_batch(sc["xinit"][:B], sc["x0"][:B], sc["params"][:B]); s.solve(); res.append(s.get())
        for k in KEYS:
            assert res[0][k].shape[0] == B and np.array_equal(res[0][k], res[1][k]), (B, k)
    if solved_share is not None:                                # (of the last, largest batch: not a comparison of failed solves)
        solved = int((res[0]["exit_code"] == 1).sum())
        print(f"[{case}] exit code 1: {solved} of {sizes[-1]}")
        assert solved >= solved_share * sizes[-1]
    small.close(); large.close()


def test_the_callers_arrays_may_change_right_after_the_call():
    """tmpc_set_batch / tmpc_set_slots return before the copy has run (pinned mirror): they must have taken their own copy of the caller's data."""
    from mpc_planner_amd import solver
    sc = _scene(8)
    ref = solver.BatchedSolver(_dims(), B_max=8)
    ref.set_batch(sc["xinit"], sc["x0"], sc["params"]); ref.solve(); want = ref.get(); ref.close()
    s = solver.BatchedSolver(_dims(), B_max=8)
    xi, x0, pa = sc["xinit"].copy(), sc["x0"].copy(), sc["params"].copy()
    s.set_batch(xi, x0, pa)
    xi[:] = np.nan; x0[:] = np.nan; pa[:] = np.nan              # the caller's buffers are gone
    s.solve(); got = s.get()
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), k
    # two set_batch calls back to back: the second rewrites the mirror only after the first copy has left it; the last one wins
    s.set_batch(sc["xinit"][::-1].copy(), sc["x0"][::-1].copy(), sc["params"][::-1].copy())
    s.set_batch(sc["xinit"], sc["x0"], sc["params"])
    s.solve(); got = s.get()
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), k
    s.close()


def test_slot_map_through_the_mirror():
    """Capsule state per slot (tmpc_set_slots + tmpc_solve_iterations with kept multipliers): a tick-size handle and a large one, the same permuted slot map,
    three ticks -- bit for bit."""
    from mpc_planner_amd import solver
    sc = _scene(8)
    slots = np.array([5, 0, 7, 2, 6, 1, 4, 3], np.int32)
    out = []
    for B_max in (8, 4096):
        s = solver.BatchedSolver(_dims(), B_max=B_max)
        ticks = []
        for t in range(3):
            s.set_batch(sc["xinit"], sc["x0"], sc["params"])
            m = slots.copy(); s.set_slots(m); m[:] = -1         # (the map is copied by the call)
            s.solve_iterations(4, keep_multipliers=True, complete=True, new_solve=True)
            ticks.append(s.get())
        out.append(ticks); s.close()
    for t in range(3):
        for k in KEYS:
            assert np.array_equal(out[0][t][k], out[1][t][k]), (t, k)
    assert not np.array_equal(out[0][0]["xtraj"], out[0][1]["xtraj"]) or (out[0][0]["qp_iter_total"] != out[0][1]["qp_iter_total"]).any()   # the kept multipliers act


def test_partial_outputs():
    from mpc_planner_amd import solver
    sc = _scene(5)
    s = solver.BatchedSolver(_dims(), B_max=8)
    s.set_batch(sc["xinit"], sc["x0"], sc["params"]); s.solve(); full = s.get()
    ec = np.zeros(5, np.int32); pobj = np.zeros(5)
    null = C.c_void_p(None)
    rc = s.lib.tmpc_get(s._h, null, null, pobj.ctypes.data_as(C.c_void_p), ec.ctypes.data_as(C.c_void_p), null, null, null, null)
    assert rc == 0 and np.array_equal(ec, full["exit_code"]) and np.array_equal(pobj, full["pobj"])
    s.close()
