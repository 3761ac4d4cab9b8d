"""GPU: the two entry points of every row writer -- the hand-written layout's (include/tmpc_hip.h) and the column form of generated stacks
(tmpc_hip_stack*.h) -- are one body behind two thin entries (csrc/tmpc_row_entries.hpp).  On libtmpc_hip.so, where the column entries work
with the layout's own columns (define_parameters(...)._params): N = 20, S = 3, 4 topology rows, 2 obstacles, 4 slack rows, slack model
(76 parameters), 2 entries over 2 scenes, every row and buffer prefilled with sentinels.  No solve is launched.

  (a) both entries refuse the same destination-independent mistakes, each message starting with its own entry's name and continuing in the
      same words;
  (b) no refused call changes a parameter row or an output buffer;
  (c) the accepted layout call and the accepted column call on the layout's own columns leave bit-identical parameter rows (and buffers)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
N, S, N_LIN, M, N_SLK, B, Q, N_PTS = 20, 3, 4, 2, 4, 2, 2, 6


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda"))


def _message(call, entry, named=None):
    """The library's message of a refused call: behind "<entry> failed (-1): ", and itself starting with the entry's name."""
    from mpc_planner_amd import solver
    with pytest.raises(solver.TmpcError) as e:
        call()
    head, named = f"{entry} failed (-1): ", (named or entry) + ": "
    text = str(e.value)
    assert text.startswith(head + named), text
    return text[len(head + named):]


def test_twin_entries_refuse_alike_write_nothing_when_refusing_and_write_the_same_rows():
    from mpc_planner_amd import solver
    from mpc_planner_amd.parameters import define_parameters
    from mpc_planner_amd.stack_env import StackEnvironment, decomp_columns, path_columns
    from mpc_planner_amd.stack_scenario import StackScenario
    from mpc_planner_amd.stack_writers import StackWriters, obstacle_columns, topology_columns
    dims = solver.default_dims(N=N, S=S, n_lin=N_LIN, M=M, n_slk=N_SLK, slack=1)
    pm = define_parameters(S, M, add_halfspaces=2, slack=True, n_decomp=N_SLK)._params
    assert len(pm) == dims.npar == 76 and dims.nvar == 8
    ocols, tcols, pcols, dcols = obstacle_columns(pm, M, 0), topology_columns(pm, N_LIN), path_columns(pm, S), decomp_columns(pm, N_SLK)
    rng = np.random.default_rng(5)
    xinit, x0 = rng.normal(size=(B, 6)), rng.normal(size=(B, N + 1, 8))
    x0[:, :, 6] = 0.3 * np.arange(N + 1)                                       # the spline state runs through the window's knots
    start = -(1.0e3 + np.arange(B * N * dims.npar, dtype=np.float64)).reshape(B, N, dims.npar)
    window = rng.normal(size=(Q, S, 9)); window[:, :, 8] = 2.0 * np.arange(S)
    host = dict(o_pos=rng.normal(size=(Q, M, N, 2)) + 6.0, o_shape=rng.uniform(0.1, 0.4, (Q, M, N, 3)), o_radius=rng.uniform(0.3, 0.6, (Q, M)),
                o_gauss=np.array([[1, 0], [0, 1]], np.uint8), scene_of=np.arange(B, dtype=np.int32) % Q, main_of=np.arange(Q, dtype=np.int32),
                state=rng.normal(size=(Q, 4)), state_x=rng.normal(size=Q), static=rng.normal(size=(Q, N, 2, 3)), window=window,
                closest_s=rng.uniform(0.0, 1.0, Q), rows=rng.normal(size=(Q, N, N_SLK, 3)), samples=rng.normal(0.0, 8.0, (Q, N, N_PTS, 2)),
                xstate=-(7.0 + np.arange(B * 6, dtype=np.float64)).reshape(B, 6), road=np.full((Q, N, 3, 3), -5.0),
                out=np.full((2, B), -9, np.int32))
    outputs = ("xstate", "road", "out")                                        # what an entry may write besides the parameter rows
    t = {k: _up(v) for k, v in host.items()}
    p = {k: v.data_ptr() for k, v in t.items()}

    s = solver.BatchedSolver(dims, B_max=B)
    w, env, scn = StackWriters(s), StackEnvironment(s), StackScenario(s)
    obst = dict(d_obstacle_pos=p["o_pos"], d_obstacle_shape=p["o_shape"], d_obstacle_radius=p["o_radius"], d_obstacle_gaussian=p["o_gauss"],
                d_scene_of=p["scene_of"], d_state=p["state"], robot_radius=0.325, disc_offset=0.03, risk=0.05, obstacle_radius=0.4)
    topo = dict(d_obstacle_pos=p["o_pos"], n_obstacles=2, d_scene_of=p["scene_of"], d_state_x=p["state_x"], robot_radius=0.325,
                d_obstacle_radius=p["o_radius"], d_static_halfspaces=p["static"], n_static=2)
    path = dict(d_window=p["window"], d_scene_of=p["scene_of"], n_scenes=Q, d_closest_s=p["closest_s"], d_state=p["xstate"])
    road = dict(d_main_of=p["main_of"], n_scenes=Q, offset_first=1.5, offset_second=1.25, d_static_halfspaces=p["road"], n_static=3, first_row=1)
    half = dict(d_rows=p["rows"], d_scene_of=p["scene_of"], n_scenes=Q, disc_offset=0.07)
    poly = dict(d_samples=p["samples"], n_pts=N_PTS, d_scene_of=p["scene_of"], d_state_x=p["state_x"], radius=0.725)
    sup = dict(n_scenarios=3, tol=1e-3, d_support=t["out"][0].data_ptr(), d_active_rows=t["out"][1].data_ptr())
    # writer -> (layout entry, its call, column entry, its call, the required device pointers, further mistakes both refuse in the same words)
    twins = {
        "obstacles": ("tmpc_set_obstacle_parameters", lambda **kw: s.set_obstacle_parameters(**dict(obst, **kw)),
                      "tmpc_stack_set_obstacle_columns", lambda **kw: w.set_obstacle_columns(ocols, 0, M, **dict(obst, **kw)),
                      ["d_obstacle_pos", "d_obstacle_shape", "d_obstacle_radius", "d_obstacle_gaussian", "d_scene_of", "d_state"], []),
        "topology": ("tmpc_linearize_topology_ex", lambda **kw: s.linearize_topology_ex(**dict(topo, **kw)),
                     "tmpc_stack_linearize_topology_columns", lambda **kw: w.linearize_topology_columns(tcols, **dict(topo, **kw)),
                     ["d_scene_of", "d_state_x", "d_obstacle_pos", "d_static_halfspaces"],
                     [dict(n_obstacles=3), dict(n_obstacles=-1), dict(n_static=-1), dict(n_obstacles=2 ** 31 - 1, n_static=2 ** 31 - 1)]),
        "path": ("tmpc_set_path_parameters", lambda **kw: s.set_path_parameters(**dict(path, **kw)),
                 "tmpc_stack_set_path_columns", lambda **kw: env.set_path_columns(pcols, **dict(path, **kw)),
                 ["d_window", "d_scene_of"], [dict(n_scenes=0), dict(d_closest_s=None), dict(d_state=None)]),
        "road": ("tmpc_road_halfspaces", lambda **kw: s.road_halfspaces(**dict(road, **kw)),
                 "tmpc_stack_road_halfspaces", lambda **kw: env.road_halfspaces(pcols, **dict(road, **kw)),
                 ["d_main_of", "d_static_halfspaces"],
                 [dict(n_scenes=0), dict(first_row=-1), dict(n_static=2, first_row=1), dict(first_row=2 ** 31 - 1), dict(n_scenes=2 ** 31 - 1)]),
        "halfspace rows": ("tmpc_set_halfspace_rows", lambda **kw: s.set_halfspace_rows(n_rows=N_SLK, **dict(half, **kw)),
                           "tmpc_stack_set_halfspace_columns", lambda **kw: env.set_halfspace_columns(dcols, **dict(half, **kw)),
                           ["d_rows", "d_scene_of"], [dict(n_scenes=0)]),
        "scenario rows": ("tmpc_scenario_halfspaces", lambda **kw: s.scenario_halfspaces(n_rows=N_SLK, **dict(poly, **kw)),
                          "tmpc_stack_scenario_halfspaces", lambda **kw: scn.halfspaces(dcols, **dict(poly, **kw)),
                          ["d_samples", "d_scene_of", "d_state_x"], [dict(n_pts=0)]),
        "scenario support": ("tmpc_scenario_support", lambda **kw: s.scenario_support_async(**dict(sup, **kw)),
                             "tmpc_stack_scenario_support", lambda **kw: scn.support_async(dcols, **dict(sup, **kw)),
                             ["d_support"], [dict(n_scenarios=0), dict(n_scenarios=8193), dict(tol=-1.0), dict(tol=float("nan"))]),
    }
    named = {"tmpc_linearize_topology_ex": "tmpc_linearize_topology"}           # tmpc_linearize_topology and its _ex form speak under one name

    def both_refuse(writer, expect=None, **kw):
        """(a) for one mistake: both entries refuse, under their own names, in the same words."""
        lay, lay_call, col, col_call, _, _ = twins[writer]
        said = [_message(lambda: lay_call(**kw), lay, named.get(lay)), _message(lambda: col_call(**kw), col)]
        if writer == "scenario support":                                       # each names the builder of its own destination
            said = [m.replace("tmpc_stack_scenario_halfspaces", "tmpc_scenario_halfspaces") for m in said]
        assert said[0] == said[1], (writer, kw, said)
        assert expect is None or expect in said[0], (writer, kw, said)

    # ---- (a) no batch yet
    for writer in twins:
        both_refuse(writer, "not built by" if writer == "scenario support" else "no batch")
    s.set_batch(xinit, x0, start)
    # ---- (a) each required pointer NULL in turn, n_scenes = 0 and the writer's other destination-independent mistakes
    for writer, (_, _, _, _, pointers, mistakes) in twins.items():
        for name in pointers:
            both_refuse(writer, "NULL", **{name: None})
        for kw in mistakes:
            both_refuse(writer, **kw)
    both_refuse("path", "n_scenes", n_scenes=0); both_refuse("road", "n_scenes", n_scenes=0); both_refuse("halfspace rows", "n_scenes", n_scenes=0)
    both_refuse("road", "do not fit", first_row=-1); both_refuse("road", "do not fit", n_static=2, first_row=1)
    both_refuse("road", "too large", n_scenes=2 ** 31 - 1)
    both_refuse("scenario support", "not built by")                            # support before the rows were built
    # more halfspace rows than fit: each destination's own limit (the problem's 4 slack rows; the 128 columns of a table)
    assert "do not fit" in _message(lambda: s.set_halfspace_rows(n_rows=N_SLK + 1, **half), "tmpc_set_halfspace_rows")
    assert "do not fit" in _message(lambda: s.set_halfspace_rows(n_rows=N_SLK, first_row=1, **half), "tmpc_set_halfspace_rows")
    assert "at most 128" in _message(lambda: env.set_halfspace_columns(list(range(1 + 3 * 43)), **half), "tmpc_stack_set_halfspace_columns")
    # ---- (b) none of the refused calls wrote a parameter row or an output buffer
    s.synchronize()
    assert np.array_equal(s.debug_get_params(), start)
    for k in outputs:
        assert np.array_equal(t[k].cpu().numpy(), host[k]), k
    # ---- (c) the same rows when accepted: every writer through its layout entry, then through its column entry on the layout's own columns
    got = {}
    for form in (0, 2):                                                        # the layout's call, the column call of each twins[...]
        for k in outputs:
            t[k].copy_(_up(host[k]))
        s.set_batch(xinit, x0, start)
        for writer in ("obstacles", "topology", "path", "road", "halfspace rows"):
            twins[writer][form + 1]()
        s.synchronize()
        first = s.debug_get_params()
        twins["scenario rows"][form + 1](); twins["scenario support"][form + 1]()
        s.synchronize()
        got[form] = dict(first=first, second=s.debug_get_params(), **{k: t[k].cpu().numpy() for k in outputs})
    lay, col = got[0], got[2]
    for k in lay:
        assert np.array_equal(lay[k], col[k]), k
    named_cols = sorted(set(ocols + tcols + pcols + dcols))
    rest = np.setdiff1d(np.arange(dims.npar), named_cols)
    assert (lay["first"][:, :, named_cols] != start[:, :, named_cols]).all()   # every named column was written, by both
    assert np.array_equal(lay["first"][:, :, rest], start[:, :, rest]) and len(rest) > 0
    assert not np.array_equal(lay["second"][:, :, dcols], lay["first"][:, :, dcols])              # the scenario rows replaced the halfspace rows
    assert (lay["road"][:, 1:, 1:3] != -5.0).all() and (lay["road"][:, :, 0] == -5.0).all() and (lay["out"] >= 0).all()
    assert np.array_equal(lay["xstate"][:, 4], host["closest_s"][host["scene_of"]])
    s.close()
