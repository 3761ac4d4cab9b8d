"""Pins the wide build of the CPU oracle (oracle/Makefile: liboracle_tmpc_wide.so, liboracle_tmpc_slack_wide.so -- the same sources and
flags with ORC_MAX_N = 62, ORC_MAX_NH = 98), the reference of the GPU tests past 32 stages or 40 rows per stage:

  * on the five BASELINE shapes it is the default build BIT FOR BIT -- trajectories, every info field, a debug capture field by field over the
    used extents, carried multipliers.  The two builds differ in array strides only, so no tolerance is in place;
  * past the default build's capacity, where there is nothing to be bitwise equal to, its RTI iterate equals the independent active-set
    solver's (tests/independent_rti.py) to the 1e-6 that tests/test_independent_rti.py asserts on the BASELINE shapes;
  * either build refuses a problem past its arrays (exit code O.EXIT_CAPACITY, nothing solved) rather than index past them.
"""
import numpy as np
import pytest

import independent_rti as I
import oracle_lib as O
from mpc_planner_amd import scenes
from test_independent_rti import CASES

INFO_FIELDS = ("pobj", "res_eq", "exit_code", "qp_status", "sqp_iter", "qp_iter_total")


def _bits(a, b, what):
    a = np.asarray(a); b = np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert a.tobytes() == b.tobytes(), (what, float(np.abs(a.astype(float) - b.astype(float)).max()))   # bytes: -0.0 != 0.0, NaN == the same NaN


def _debug_used(pb, dbg):
    """The entries of an orc_debug capture that a solve of pb writes, with the capacity-dependent strides taken out."""
    N, nh = pb.N, pb.nh
    cn, cnh = pb.capacity
    rows = lambda a, tail=(): np.array(a).reshape((cn, cnh) + tail)[:N, :nh]
    flat = lambda a, n: np.array(a)[:n]
    return dict(W=flat(dbg.W, (N + 1) * 49), g=flat(dbg.g, (N + 1) * 7), BA=flat(dbg.BA, N * 35), b=flat(dbg.b, N * 5), h=rows(dbg.h), D=rows(dbg.D, (7,)),
                W_raw=flat(dbg.W_raw, (N + 1) * 49), z_in=flat(dbg.z_in, (N + 1) * 7), pi_in=flat(dbg.pi_in, (N + 1) * 5), lamh_in=rows(dbg.lamh_in),
                dz=flat(dbg.dz, (N + 1) * 7), pi=flat(dbg.pi, (N + 1) * 5), qp_iters=np.array(dbg.qp_iters))


@pytest.mark.parametrize("cfg", sorted(CASES))
def test_wide_build_is_bitwise_the_default_build(cfg):
    skw, pkw, _ = CASES[cfg]
    narrow = O.problem(**pkw); wide = O.problem(wide=True, **pkw)
    assert narrow.capacity == (O.MAX_N, O.MAX_NH) and wide.capacity == (O.WIDE_N, O.WIDE_NH) and O.lib_of(narrow) is not O.lib_of(wide)
    assert narrow.npar == wide.npar
    sc = scenes.make_scene(70, **skw)
    B = sc["xinit"].shape[0]
    flat = (sc["xinit"], sc["x0"].reshape(B, -1), sc["params"].reshape(B, -1))
    xn, un, fn = O.solve_batch(narrow, *flat)
    xw, uw, fw = O.solve_batch(wide, *flat)
    _bits(xn, xw, "xtraj"); _bits(un, uw, "utraj")
    for f in INFO_FIELDS:
        _bits(fn[f], fw[f], f)
    assert (fn["exit_code"] == 1).any()
    b = int(np.argmax(fn["exit_code"] == 1))
    one = (sc["xinit"][b], sc["x0"][b], sc["params"][b])
    # the second linearisation of a solve: non-zero multipliers in the Lagrangian Hessian
    dn = O.solve(narrow, *one, debug_iter=1); dw = O.solve(wide, *one, debug_iter=1)
    _bits(dn[0], dw[0], "debug xtraj"); _bits(dn[1], dw[1], "debug utraj"); _bits(dn[0], xn[b], "debug solve == batch solve")
    for f in INFO_FIELDS:
        assert getattr(dn[2], f) == getattr(dw[2], f), f
    un_, uw_ = _debug_used(narrow, dn[3]), _debug_used(wide, dw[3])
    for f in un_:
        _bits(un_[f], uw_[f], "debug " + f)
    assert np.abs(un_["lamh_in"]).max() > 0 or narrow.nh == 0
    assert np.abs(un_["pi_in"]).max() > 0 and np.abs(un_["dz"]).max() > 0
    # carried multipliers, two solves in a row: the second reads what the first stored, at the library's own stride
    N, nh = narrow.N, narrow.nh
    pin = np.zeros((N + 1) * 5); piw = np.zeros((N + 1) * 5); ln = np.zeros(N * O.MAX_NH); lw = np.zeros(N * O.WIDE_NH)
    for tick in range(2):
        cn = O.solve_carry(narrow, *one, 10, pin, ln); cw = O.solve_carry(wide, *one, 10, piw, lw)
        _bits(cn[0], cw[0], f"carry xtraj {tick}"); _bits(cn[1], cw[1], f"carry utraj {tick}")
        for f in INFO_FIELDS:
            assert getattr(cn[2], f) == getattr(cw[2], f), (f, tick)
        _bits(pin, piw, f"carry pi {tick}")
        _bits(ln.reshape(N, O.MAX_NH)[:, :nh], lw.reshape(N, O.WIDE_NH)[:, :nh], f"carry lamh {tick}")
        assert not lw.reshape(N, O.WIDE_NH)[:, nh:].any() and not ln.reshape(N, O.MAX_NH)[:, nh:].any()
    assert pin.any() and (ln.any() or nh == 0)
    print(f"[oracle wide] {cfg}: B {B}, successes {int((fn['exit_code'] == 1).sum())}, bitwise equal; debug / carry on trajectory {b}")


WIDE_CASES = {
    "N=40 (8,8)": (dict(N=40, M=8, B=8), dict(N=40, S=5, n_lin=8, M=8)),
    "N=62 (6,6)": (dict(N=62, M=6, B=8), dict(N=62, S=5, n_lin=6, M=6)),
    "N=20 (24,24)": (dict(N=20, M=24, B=8), dict(N=20, S=5, n_lin=24, M=24)),
}


@pytest.mark.parametrize("name", list(WIDE_CASES))
def test_wide_oracle_rti_iterate_matches_active_set_solver(name):
    skw, pkw = WIDE_CASES[name]
    tight = O.problem(qp_tol=1e-9, **pkw)
    assert tight._wide and tight.capacity == (O.WIDE_N, O.WIDE_NH)
    n = 0; worst = 0.0
    for scene in (70, 71):
        sc = scenes.make_scene(scene, **skw)
        B = sc["xinit"].shape[0]
        xt, ut, info = O.solve_batch(tight, sc["xinit"], sc["x0"].reshape(B, -1), sc["params"].reshape(B, -1))
        for b in range(B):
            if info["exit_code"][b] != 1 or info["sqp_iter"][b] != tight.n_sqp:       # only full-length solves are comparable (test_independent_rti.py)
                continue
            xa, ua, pobj, _ = I.rti_solve(tight, sc["xinit"][b], sc["x0"][b], sc["params"][b])
            worst = max(worst, np.abs(xa - xt[b]).max(), np.abs(ua - ut[b]).max())
            assert abs(pobj - info["pobj"][b]) <= 1e-7 * max(1.0, abs(pobj))
            n += 1
            if n >= 6:
                break
        if n >= 6:
            break
    print(f"[oracle wide] {name}: {n} trajectories, worst |oracle - active set| {worst:.2e}")
    assert n >= 4, n
    assert worst < 1e-6, worst


@pytest.mark.parametrize("wide,pkw,fits", [
    (False, dict(N=32, n_lin=20, M=20), True), (False, dict(N=33), False), (False, dict(N=20, n_lin=20, M=21), False),
    (False, dict(N=30, n_lin=8, M=8, n_slk=25, slack=1), False),
    (True, dict(N=62, n_lin=6, M=6), True), (True, dict(N=20, n_lin=49, M=49), True), (True, dict(N=63), False), (True, dict(N=20, n_lin=49, M=50), False),
    (True, dict(N=20, n_lin=40, M=40, n_slk=19, slack=1), False),
])
def test_a_problem_past_the_capacity_is_refused(wide, pkw, fits):
    """N = 33 and 41 rows on the default build, N = 63 and 99 rows on the wide one: exit code EXIT_CAPACITY from every solve entry point, outputs
    untouched; the largest problems that fit are solved."""
    pb = O.problem(wide=wide, **pkw)
    assert pb._wide == wide and pb.capacity == ((O.WIDE_N, O.WIDE_NH) if wide else (O.MAX_N, O.MAX_NH))
    assert fits == (pb.N <= pb.capacity[0] and pb.nh <= pb.capacity[1])
    N = pb.N
    xinit = np.zeros(pb.nxe); x0 = np.zeros((N + 1, pb.nve)); x0[:, 5] = 1.0; params = np.ones((N, pb.npar))
    xt, ut, info = O.solve(pb, xinit, x0, params)
    xb, ub, ib = O.solve_batch(pb, xinit[None], x0.reshape(1, -1), params.reshape(1, -1), num_threads=1)
    pi = np.full((N + 1) * 5, 0.5); lamh = np.full(N * pb.capacity[1], 0.5)
    xc, uc, ic = O.solve_carry(pb, xinit, x0, params, 2, pi, lamh)
    xd, ud, idb, dbg = O.solve(pb, xinit, x0, params, debug_iter=0)
    codes = (info.exit_code, int(ib["exit_code"][0]), ic.exit_code, idb.exit_code)
    if fits:
        assert O.EXIT_CAPACITY not in codes, codes
        assert info.sqp_iter >= 1
    else:
        assert codes == (O.EXIT_CAPACITY,) * 4, codes
        assert info.sqp_iter == 0 and info.qp_iter_total == 0
        assert not xt.any() and not ut.any() and not xb.any() and not xc.any() and not xd.any()
        assert (pi == 0.5).all() and (lamh == 0.5).all() and not np.array(dbg.W).any()


def test_problem_picks_the_build_by_size():
    assert not O.problem(N=32, n_lin=20, M=20)._wide and not O.problem(N=30, n_lin=8, M=8, n_slk=12, slack=1)._wide
    assert O.problem(N=33)._wide and O.problem(N=20, n_lin=20, M=21)._wide and O.problem(N=20, n_lin=12, M=12, n_slk=17, slack=1)._wide
    assert O.problem(N=30, n_lin=0, M=0, n_gauss=41)._wide and O.problem(N=20, wide=True)._wide and not O.problem(N=33, wide=False)._wide
    assert O.lib() is O.lib(0) and O.lib(1) is O.lib_of(O.problem(N=20, n_lin=0, M=0, n_slk=24, slack=1)) and (O.MAX_N, O.MAX_NH) == (32, 40)
    assert O.Debug is O.debug_struct(32, 40)
