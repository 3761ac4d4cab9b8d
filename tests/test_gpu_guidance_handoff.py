"""GPU: the guidance hand-off on device (tmpc_sample_guidance, tmpc_guidance_plan, tmpc_guidance_decide; csrc/tmpc_aux_kernels.hpp; DESIGN.md
U18) against the host mirrors (mpc_planner_amd/modules.py sample_guidance / guidance_plan / guidance_decide, pinned on hand values in
tests/test_guidance_handoff.py).  Equality is bitwise, floats included: kernels and mirrors share the operation order and use neither fused
multiply-adds nor transcendental functions.  Then the whole tick chain plan -> warmstart -> sample -> init_with_guidance ->
linearize_topology_ex -> solve -> decide -> gather_best without a host round trip, against the same ticks whose hand-off the mirrors do."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, S, M = 20, 5, 8
SENTINEL = -3.0


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda"))


def _full(shape, value, dtype):
    import torch
    return torch.full(shape, value, dtype=dtype, device=torch.device("cuda"))


def _bits(a):
    """The bit patterns of an array; every NaN becomes one pattern: IEEE 754 leaves a NaN's sign and payload to the implementation (x86
    keeps the operand's, gfx950's subtraction -- an addition with a negated source -- flips its sign), so "the same NaN" means NaN in the
    same place.  Every other value, signed zeros and infinities included, keeps its bits."""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float64:
        return a
    bits = a.view(np.uint64).copy()
    bits[np.isnan(a)] = np.uint64(0x7ff8000000000000)
    return bits


def _same(a, b):
    """Bitwise equality; a NaN equals a NaN in the same place (_bits)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _solver(B_max=12):
    from mpc_planner_amd import solver
    return solver.BatchedSolver(solver.default_dims(N=N, S=S, n_lin=M, M=M), B_max=B_max)


def _random_nodes(rng, n, t0=0.0, span=4.0):
    t = t0 + np.sort(np.concatenate([[0.0, span], rng.uniform(0.05 * span, 0.95 * span, max(n - 2, 0))]))[:n]
    heading = np.cumsum(rng.normal(size=n) * 0.3)
    xy = np.cumsum(np.stack([np.cos(heading), np.sin(heading)], 1) * rng.uniform(0.3, 1.5, (n, 1)), 0)
    return np.concatenate([t[:, None], xy], 1)


def test_sample_guidance_equals_the_mirror_bitwise():
    """n_nodes_max = 9 and 64.  Node counts 0, 1, 2, 3, 5 and n_nodes_max; t_0 = 0.7 (the first samples lie before the first knot) and
    t_0 = -1.3; a span of 1.1 s, shorter than N dt = 4 s (most samples continue the last cubic); a repeated t, a decreasing t, a NaN knot, an
    infinite knot, a count beyond n_nodes_max and a negative one.  Rows behind the count hold a value that would win any `<=` test.  The
    outputs are prefilled with a sentinel: every entry of the launch is written, nothing behind it."""
    import torch
    from mpc_planner_amd import modules as md
    s = _solver()
    dt = s.dims.dt
    for R in (9, 64):
        rng = np.random.default_rng(100 + R)
        lists = [np.zeros((0, 3)), _random_nodes(rng, 1), _random_nodes(rng, 2), _random_nodes(rng, 3), _random_nodes(rng, 5), _random_nodes(rng, R),
                 _random_nodes(rng, 4, t0=0.7), _random_nodes(rng, 6, t0=-1.3), _random_nodes(rng, 5, span=1.1), _random_nodes(rng, 2, t0=0.5, span=0.3)]
        bad = _random_nodes(rng, 5); bad[3, 0] = bad[2, 0]; lists.append(bad)                       # a repeated t
        bad = _random_nodes(rng, 5); bad[[2, 3], 0] = bad[[3, 2], 0]; lists.append(bad)             # a decreasing t
        bad = _random_nodes(rng, 4); bad[1, 0] = np.nan; lists.append(bad)
        bad = _random_nodes(rng, 3); bad[2, 0] = np.inf; lists.append(bad)
        nan_value = _random_nodes(rng, 4); nan_value[2, 1] = np.nan; lists.append(nan_value)        # a NaN position is no invalid list: it propagates
        J = len(lists) + 2
        nodes = np.full((J, R, 3), -9e9)
        counts = np.zeros(J, np.int32)
        for j, l in enumerate(lists):
            nodes[j, :len(l)] = l; counts[j] = len(l)
        nodes[J - 2, :3] = _random_nodes(rng, 3); counts[J - 2] = R + 1                              # more nodes than the buffer holds
        nodes[J - 1, :3] = _random_nodes(rng, 3); counts[J - 1] = -2
        want = [md.sample_guidance(nodes[j, :counts[j]] if 0 <= counts[j] <= R else np.zeros((R + 1, 3)), N, dt, n_nodes_max=R) for j in range(J)]
        want_pos, want_vel = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
        want_status = np.array([w[2] for w in want], np.int32)
        assert want_status.tolist() == [1, 1] + [0] * 8 + [1, 1, 1, 1, 0, 1, 1]
        assert np.isnan(want_pos[14]).any() and not want_pos[[0, 1, 10, 11, 12, 13, 15, 16]].any()
        t_nodes, t_counts = _up(nodes), _up(counts)
        t_pos, t_vel = _full((J + 1, N + 1, 2), SENTINEL, torch.float64), _full((J + 1, N + 1, 2), SENTINEL, torch.float64)
        t_status = _full((J + 1,), -7, torch.int32)
        s.sample_guidance(J, R, t_nodes.data_ptr(), t_counts.data_ptr(), t_pos.data_ptr(), t_vel.data_ptr(), t_status.data_ptr())
        s.synchronize()
        got_pos, got_vel, got_status = t_pos.cpu().numpy(), t_vel.cpu().numpy(), t_status.cpu().numpy()
        with np.errstate(all="ignore"):
            print(f"[sample R={R}] status {got_status[:J].tolist()}, max |pos - mirror| {np.nanmax(np.abs(got_pos[:J] - want_pos)):.3e}, "
                  f"max |vel - mirror| {np.nanmax(np.abs(got_vel[:J] - want_vel)):.3e}")
        assert np.array_equal(got_status[:J], want_status)
        assert _same(got_pos[:J], want_pos) and _same(got_vel[:J], want_vel)
        assert (got_pos[J] == SENTINEL).all() and (got_vel[J] == SENTINEL).all() and got_status[J] == -7
        assert _same(t_nodes.cpu().numpy(), nodes)                                                   # inputs are inputs
    s.close()


def _solved_batch(n_scenes, P, seed):
    """A handle holding a SOLVED batch of n_scenes x P entries (any solution will do: decide reads v of node 1 and w of node 0 from it)."""
    from mpc_planner_amd import scenes
    s = _solver(B_max=n_scenes * P)
    scs = [scenes.make_scene(seed + q, N=N, M=M, B=P) for q in range(n_scenes)]
    s.set_batch(np.concatenate([sc["xinit"] for sc in scs]), np.concatenate([sc["x0"] for sc in scs]), np.concatenate([sc["params"] for sc in scs]))
    s.solve()
    return s, s.get()


@pytest.mark.parametrize("n_paths,tmpcpp,warm,shift,explicit", [(2, True, True, True, False), (4, True, True, False, True), (3, False, False, True, False)])
def test_plan_and_decide_equal_the_mirrors_over_six_ticks(n_paths, tmpcpp, warm, shift, explicit):
    """3 scenes, P = 3 (2 + 1), P = 5 (4 + 1) and P = 3 without a non-guided planner; 6 ticks of changing classes and counts, the cross-tick
    state carried on the device and compared after every tick.  pobj / exit_code are synthetic device arrays: small integers (ties), tick 1
    fails every planner of scene 0, tick 2 ties the weighted objectives of scene 1 throughout (4 x 0.75 = 3 x 1), tick 3 gives the lowest objective of scene 2 to a disabled planner.
    plan is called twice per tick (it is pure).  With `explicit` the previously_selected flags are an input, else they come from the state."""
    import torch
    from mpc_planner_amd import modules as md, solver
    Q, P, ticks = 3, n_paths + int(tmpcpp), 6
    B = Q * P
    s, sol = _solved_batch(Q, P, 300)
    opt = solver.guidance_options(n_paths, tmpcpp, warm, shift, 0.75)
    rng = np.random.default_rng(17 * n_paths + int(explicit))
    ids, sel = np.full((Q, P), -1, np.int32), np.tile(np.array([-1, 0, -1], np.int32), (Q, 1))
    t_ids, t_sel = _up(ids), _up(sel)
    state = rng.normal(size=(Q, 5)); state[:, 3] = (0.05, 1.0, 2.0)
    t_state = _up(state)
    i32, u8, f64 = torch.int32, torch.uint8, torch.float64
    t_out = dict(mode=_full((B + 1,), -7, i32), src=_full((B + 1,), -7, i32), init_enabled=_full((B + 1,), 9, u8), rows_dummy=_full((B + 1,), 9, u8),
                 disabled=_full((B + 1,), 9, u8), guidance_id=_full((B + 1,), -7, i32), weight=_full((B + 1,), SENTINEL, f64))
    t_best, t_exit, t_cmd = _full((Q + 1,), -7, i32), _full((Q + 1,), -7, i32), _full((Q + 1, 2), SENTINEL, f64)
    seen = dict(tie=False, none=False, disabled_best=False, existing=False, weighted=False, disabled=False)
    classes = rng.integers(0, 4, (Q, n_paths)).astype(np.int32)
    for tick in range(ticks):
        keep = rng.uniform(size=(Q, n_paths)) < 0.6                                                  # most classes survive a tick: existing guidance
        classes = np.where(keep, classes, rng.integers(0, 4, (Q, n_paths))).astype(np.int32)
        counts = rng.integers(0, n_paths + 1, Q).astype(np.int32)
        if tick == 2:
            counts[1] = n_paths
        if tick == 3:
            counts[2] = 1
        if tick == 5:
            counts[:] = (n_paths + 3, -1, n_paths)                                                   # clipped to [0, n_paths]
        prev = rng.integers(0, 2, (Q, n_paths)).astype(np.uint8) if explicit else None
        t_cls, t_cnt, t_prev = _up(classes), _up(counts), (_up(prev) if explicit else None)
        want = md.guidance_plan(counts, classes, ids, sel, n_paths, tmpcpp, warm, shift, 0.75, prev)
        for _ in range(2):
            s.guidance_plan(Q, opt, t_cnt.data_ptr(), t_cls.data_ptr(), t_ids.data_ptr(), t_sel.data_ptr(),
                            *(t_out[k].data_ptr() for k in ("mode", "src", "init_enabled", "rows_dummy", "disabled", "guidance_id", "weight")),
                            d_previously_selected=t_prev.data_ptr() if explicit else None)
            s.synchronize()
            for k, t in t_out.items():
                got = t.cpu().numpy()
                assert _same(got[:B], want[k]), (tick, k, got[:B].tolist(), want[k].tolist())
                assert got[B] == (SENTINEL if k == "weight" else 9 if t.dtype == u8 else -7)
            assert np.array_equal(t_ids.cpu().numpy(), ids) and np.array_equal(t_sel.cpu().numpy(), sel)      # plan does not touch the state
        assert ((want["src"] >= 0) & (want["src"] < B)).all()
        seen["existing"] |= bool(warm and ((want["init_enabled"] == 0) & (want["rows_dummy"] == 0)).any())
        seen["weighted"] |= bool((want["weight"] == 0.75).any())
        seen["disabled"] |= bool(want["disabled"].any())
        # ---- synthetic verdicts
        pobj = rng.integers(1, 4, B).astype(np.float64)
        code = rng.choice(np.array([1, 1, 1, 0, -1, 2], np.int32), B).astype(np.int32)
        if tick == 1:
            code[:P] = (0, -1, 2, 3, 0)[:P]
        if tick == 2:
            pobj[P:2 * P] = np.where(want["weight"][P:2 * P] == 0.75, 4.0, 3.0); code[P:2 * P] = 1
        if tick == 3:
            pobj[2 * P + 1] = 0.25; code[2 * P + 1] = 1                                              # disabled (count 1) when n_paths >= 2
        dec = md.guidance_decide(pobj, code, want["disabled"], want["guidance_id"], want["weight"], state, sol["xtraj"], sol["utraj"], ids, sel,
                                 n_paths, tmpcpp, deceleration=2.5, control_dt=0.04, enable_output=tick != 4)
        t_pobj, t_code = _up(pobj), _up(code)
        s.guidance_decide(Q, opt, t_pobj.data_ptr(), t_code.data_ptr(), t_out["disabled"].data_ptr(), t_out["guidance_id"].data_ptr(),
                          t_out["weight"].data_ptr(), t_state.data_ptr(), t_best.data_ptr(), t_exit.data_ptr(), t_cmd.data_ptr(), t_ids.data_ptr(),
                          t_sel.data_ptr(), deceleration=2.5, control_dt=0.04, enable_output=tick != 4)
        s.synchronize()
        got_best, got_exit, got_cmd = t_best.cpu().numpy(), t_exit.cpu().numpy(), t_cmd.cpu().numpy()
        print(f"[plan/decide P={P}] tick {tick}: counts {counts.tolist()}, best {got_best[:Q].tolist()}, exit {got_exit[:Q].tolist()}, "
              f"selection {t_sel.cpu().numpy().tolist()}")
        assert np.array_equal(got_best[:Q], dec["best"]) and np.array_equal(got_exit[:Q], dec["exit"]) and _same(got_cmd[:Q], dec["cmd"])
        assert got_best[Q] == -7 and got_exit[Q] == -7 and (got_cmd[Q] == SENTINEL).all()
        assert np.array_equal(t_ids.cpu().numpy(), dec["planner_ids"]) and np.array_equal(t_sel.cpu().numpy(), dec["selection"])
        eff = np.where((code == 1) & (want["disabled"] == 0), pobj * want["weight"], np.inf).reshape(Q, P)
        seen["tie"] |= bool(((eff == eff.min(1, keepdims=True)) & np.isfinite(eff)).sum(1).max() >= 2)
        seen["none"] |= bool((dec["best"] < 0).any())
        raw = np.where(code == 1, pobj * want["weight"], np.inf).reshape(Q, P)
        seen["disabled_best"] |= bool((want["disabled"].reshape(Q, P)[np.arange(Q), raw.argmin(1)] == 1).any())
        for q in range(Q):                                                                           # the command really is the winner's solution
            b = q * P + int(dec["best"][q])
            if dec["best"][q] >= 0 and tick != 4:
                assert got_cmd[q, 0] == sol["xtraj"][b, 1, 3] and got_cmd[q, 1] == sol["utraj"][b, 0, 1]
            else:
                assert got_cmd[q, 1] == 0.0 and got_cmd[q, 0] == max(state[q, 3] - 2.5 * 0.04, 0.0)
        ids, sel = dec["planner_ids"], dec["selection"]
    need = ["tie", "none", "disabled"] + (["disabled_best"] if n_paths >= 2 else []) + (["existing"] if warm else []) + ([] if explicit else ["weighted"])
    assert all(seen[k] for k in need), seen
    s.close()


def test_every_refusal():
    import torch
    from mpc_planner_amd import solver
    Q, n_paths, P = 2, 2, 3
    B = Q * P
    s = _solver()
    i32, u8, f64 = torch.int32, torch.uint8, torch.float64
    z = lambda n, dt: _full((n,), 0, dt)
    opt = solver.guidance_options(n_paths)
    # ---- tmpc_sample_guidance
    t_nodes, t_cnt, t_pos, t_vel, t_st = _full((2, 4, 3), 0.0, f64), z(2, i32), _full((2, N + 1, 2), SENTINEL, f64), _full((2, N + 1, 2), SENTINEL, f64), z(2, i32)
    sample = lambda **kw: s.sample_guidance(**dict(dict(n_traj=2, n_nodes_max=4, d_nodes=t_nodes.data_ptr(), d_node_count=t_cnt.data_ptr(),
                                                        d_gpos=t_pos.data_ptr(), d_gvel=t_vel.data_ptr(), d_status=t_st.data_ptr()), **kw))
    for kw, msg in ((dict(n_traj=0), "n_traj"), (dict(n_nodes_max=1), "n_nodes_max"), (dict(n_nodes_max=65), "n_nodes_max"), (dict(d_nodes=None), "NULL input"),
                    (dict(d_node_count=None), "NULL input"), (dict(d_gpos=None), "NULL output"), (dict(d_gvel=None), "NULL output"), (dict(d_status=None), "NULL output")):
        with pytest.raises(solver.TmpcError, match=msg):
            sample(**kw)
    s.synchronize()
    assert (t_pos.cpu().numpy() == SENTINEL).all() and (t_st.cpu().numpy() == 0).all()              # nothing was launched
    sample()                                                                                         # accepted, and without a batch
    # ---- tmpc_guidance_plan
    t_tc, t_cls, t_ids, t_sel = z(Q, i32), z(Q * n_paths, i32), _full((B,), -1, i32), _up(np.tile(np.array([-1, 0, -1], np.int32), (Q, 1)))
    names = ("d_mode", "d_src", "d_init_enabled", "d_rows_dummy", "d_disabled", "d_guidance_id", "d_weight")
    outs = dict(d_mode=_full((B,), -7, i32), d_src=z(B, i32), d_init_enabled=z(B, u8), d_rows_dummy=z(B, u8), d_disabled=z(B, u8), d_guidance_id=z(B, i32), d_weight=z(B, f64))
    plan = lambda **kw: s.guidance_plan(**dict(dict(n_scenes=Q, options=opt, d_traj_count=t_tc.data_ptr(), d_topology_class=t_cls.data_ptr(),
                                                    d_planner_ids=t_ids.data_ptr(), d_selection=t_sel.data_ptr(),
                                                    **{k: outs[k].data_ptr() for k in names}), **kw))
    short = solver.guidance_options(n_paths); short.size = C.sizeof(short) - 8
    long_dirty = (C.c_char * (C.sizeof(opt) + 8)).from_buffer_copy(bytes(opt) + b"\0\0\0\1\0\0\0\0")
    C.cast(long_dirty, C.POINTER(solver.TmpcGuidanceOptions)).contents.size = C.sizeof(opt) + 8
    dirty = C.cast(long_dirty, C.POINTER(solver.TmpcGuidanceOptions)).contents
    bad_options = [(dict(options=solver.guidance_options(0)), "n_paths"), (dict(options=solver.guidance_options(64)), "n_paths"), (dict(options=None), "NULL options"),
                   (dict(options=short), "smaller"), (dict(options=dirty), "non-zero field")]
    for kw, msg in [(dict(n_scenes=0), "n_scenes"), (dict(d_traj_count=None), "NULL input"), (dict(d_topology_class=None), "NULL input"),
                    (dict(d_planner_ids=None), "NULL input"), (dict(d_selection=None), "NULL input")] + [(dict([(k, None)]), "NULL output") for k in names] + bad_options:
        with pytest.raises(solver.TmpcError, match=msg):
            plan(**kw)
    s.synchronize()
    assert (outs["d_mode"].cpu().numpy() == -7).all()
    plan()                                                                                           # accepted without a batch and without previously_selected
    long_clean = (C.c_char * (C.sizeof(opt) + 8)).from_buffer_copy(bytes(opt) + b"\0" * 8)            # a newer, longer header with a zero tail
    clean = C.cast(long_clean, C.POINTER(solver.TmpcGuidanceOptions)).contents; clean.size = C.sizeof(opt) + 8
    plan(options=clean)
    s.synchronize()
    assert (outs["d_mode"].cpu().numpy() == 3).all()                                                 # no previous solution: braking
    # ---- tmpc_guidance_decide
    t_pobj, t_code, t_state = z(B, f64), z(B, i32), z(Q * 5, f64)
    t_best, t_exit, t_cmd = _full((Q,), -7, i32), z(Q, i32), z(Q * 2, f64)
    args = dict(n_scenes=Q, options=opt, d_pobj=t_pobj.data_ptr(), d_exit_code=t_code.data_ptr(), d_disabled=outs["d_disabled"].data_ptr(),
                d_guidance_id=outs["d_guidance_id"].data_ptr(), d_weight=outs["d_weight"].data_ptr(), d_state=t_state.data_ptr(), d_best=t_best.data_ptr(),
                d_exit=t_exit.data_ptr(), d_cmd=t_cmd.data_ptr(), d_planner_ids=t_ids.data_ptr(), d_selection=t_sel.data_ptr())
    decide = lambda **kw: s.guidance_decide(**dict(args, **kw))
    with pytest.raises(solver.TmpcError, match="no solved batch"):
        decide()                                                                                     # no batch at all
    from mpc_planner_amd import scenes
    scs = [scenes.make_scene(310 + q, N=N, M=M, B=P) for q in range(Q)]
    batch = [np.concatenate([sc[k] for sc in scs]) for k in ("xinit", "x0", "params")]
    s.set_batch(*batch)
    with pytest.raises(solver.TmpcError, match="no solved batch"):
        decide()                                                                                     # a batch, but not solved
    s.solve()
    for kw, msg in [(dict(n_scenes=0), "n_scenes"), (dict(n_scenes=3), "n_scenes x P"), (dict(options=solver.guidance_options(n_paths, use_tmpcpp=False)), "n_scenes x P")] + \
                   [(dict([(k, None)]), "NULL input") for k in ("d_pobj", "d_exit_code", "d_disabled", "d_guidance_id", "d_weight", "d_state")] + \
                   [(dict([(k, None)]), "NULL output") for k in ("d_best", "d_exit", "d_cmd", "d_planner_ids", "d_selection")] + bad_options:
        with pytest.raises(solver.TmpcError, match=msg):
            decide(**kw)
    s.synchronize()
    assert (t_best.cpu().numpy() == -7).all() and (t_ids.cpu().numpy() == -1).all()
    decide()                                                                                         # the same call on the solved batch: accepted
    s.set_batch(*batch)
    with pytest.raises(solver.TmpcError, match="no solved batch"):
        decide()                                                                                     # new inputs: the solution is the old batch's
    null = None
    assert s.lib.tmpc_sample_guidance(null, 1, 4, null, null, null, null, null) == -1                # no handle: TMPC_ERR_INVALID
    assert s.lib.tmpc_guidance_plan(null, 1, C.byref(opt), *([null] * 12)) == -1
    assert s.lib.tmpc_guidance_decide(null, 1, C.byref(opt), *([null] * 6), 1.0, 1.0, 1, *([null] * 5)) == -1
    s.close()


# the script of the end-to-end test: per tick and scene the number of guidance trajectories and their classes (n_paths = 2)
E2E_SEEDS = (80, 81)
E2E_COUNTS = [(2, 2), (2, 1), (1, 2), (2, 2), (0, 2), (2, 2)]
E2E_CLASSES = [((0, 1), (3, 2)), ((0, 1), (3, 2)), ((1, 0), (2, 3)), ((1, 0), (2, 3)), ((1, 0), (5, 3)), ((0, 1), (3, 5))]
E2E_NODE_STAGES = ((0, 5, 10, 15, 20), (0, 7, 14, 20))                                               # the nodes of planner 0 / 1: guidance_pos at these stages


def test_end_to_end_six_ticks_equal_the_host_hand_off(seeds=E2E_SEEDS):
    """2 scenes x (2 + 1) planners, 6 ticks.  Handle A runs plan -> warmstart -> sample -> init_with_guidance -> linearize_topology_ex -> solve
    -> decide -> gather_best stream-ordered, the robot's state advanced on the device to node 1 of the winner (kept without one), the nodes
    moved with the robot.  Handle B runs the same ticks with the hand-off done by the mirrors on the host -- plan, samples and decision
    uploaded / downloaded around the existing calls, the batch given through set_batch.  Both see bit-identical inputs, so xtraj, utraj, pobj,
    exit codes, best, cmd and the state arrays are equal bit for bit every tick.  The script makes a disabled planner,
    warmstart_with_mpc_solution && existing_guidance and a previously selected class with the non-unit weight occur: asserted."""
    import torch
    from mpc_planner_amd import modules as md, scenes, solver
    Q, n_paths, P, ticks, R = 2, 2, 3, 6, 6
    B = Q * P
    scs = [scenes.make_scene(seed, N=N, M=M, B=n_paths, tmpc_pp=True) for seed in seeds]
    xinit = np.concatenate([sc["xinit"] for sc in scs]); params = np.concatenate([sc["params"] for sc in scs])
    x0 = np.full((B, N + 1, 7), SENTINEL)                                                            # every warm start is the device's
    obst = np.ascontiguousarray(np.stack([sc["obstacles"]["pos"] for sc in scs]))
    scene_of = np.repeat(np.arange(Q, dtype=np.int32), P)
    r, decel, cdt, w_cons = scenes.ROBOT_RADIUS, 3.0, 0.05, 0.8
    kw = dict(use_tmpcpp=True, warmstart_with_mpc_solution=True, shift_previous_solution_forward=True, selection_weight_consistency=w_cons)
    opt = solver.guidance_options(n_paths, **kw)
    # the nodes relative to the robot: (t, x, y) of the scene's guidance trajectories at a few stages; none for the non-guided planner
    base_nodes, node_count = np.full((B, R, 3), -9e9), np.zeros(B, np.int32)
    for q, sc in enumerate(scs):
        for p in range(n_paths):
            st = np.array(E2E_NODE_STAGES[p])
            base_nodes[q * P + p, :len(st)] = np.concatenate([st[:, None] * 0.2, sc["guidance_pos"][p][st] - xinit[q * P, None, 0:2]], 1)
            node_count[q * P + p] = len(st)
    dev = torch.device("cuda")
    A, Bh = _solver(B), _solver(B)
    i32, u8, f64 = torch.int32, torch.uint8, torch.float64
    # ---- handle A: everything on the device
    t_xinit, t_x0, t_params = _up(xinit), _up(x0), _up(params)
    A.set_batch_device(B, t_xinit.data_ptr(), t_x0.data_ptr(), t_params.data_ptr())
    t_state = _up(xinit[::P].copy()); t_stateB = _up(xinit.copy()); t_sx = _up(xinit[::P, 0].copy())
    t_base, t_nodes, t_ncnt = _up(base_nodes), _up(base_nodes), _up(node_count)
    t_ob, t_sc = _up(obst), _up(scene_of)
    t_ids, t_sel = _full((Q, P), -1, i32), _up(np.tile(np.array([-1, 0, -1], np.int32), (Q, 1)))
    t_mode, t_src, t_gid = _full((B,), -7, i32), _full((B,), -7, i32), _full((B,), -7, i32)
    t_init, t_dummy, t_dis, t_w = _full((B,), 9, u8), _full((B,), 9, u8), _full((B,), 9, u8), _full((B,), SENTINEL, f64)
    t_gpos, t_gvel, t_status = _full((B, N + 1, 2), SENTINEL, f64), _full((B, N + 1, 2), SENTINEL, f64), _full((B,), -7, i32)
    t_best, t_exit, t_cmd = _full((Q,), -7, i32), _full((Q,), -7, i32), _full((Q, 2), SENTINEL, f64)
    t_wx, t_wu = _full((Q, (N + 1) * 5), SENTINEL, f64), _full((Q, N * 2), SENTINEL, f64)
    d_pobj, d_code = A.result_device_ptrs()
    hs = torch.cuda.ExternalStream(A.stream_ptr(), device=dev)
    # ---- handle B: the hand-off on the host
    Bh.set_batch(xinit, x0, params)
    state = xinit[::P].copy()
    ids, sel = np.full((Q, P), -1, np.int32), np.tile(np.array([-1, 0, -1], np.int32), (Q, 1))
    ref = None
    seen = dict(disabled=False, existing=False, weighted=False, winner=False)
    torch.cuda.synchronize()
    for tick in range(ticks):
        counts = np.array(E2E_COUNTS[tick], np.int32); classes = np.array(E2E_CLASSES[tick], np.int32)
        t_cnt, t_cls = _up(counts), _up(classes)
        torch.cuda.synchronize()
        # ---- A: one stream, nothing read back before gather_best is enqueued
        with torch.cuda.stream(hs):
            if tick > 0:
                node1 = t_wx.view(Q, N + 1, 5)[:, 1, :]
                t_state.copy_(torch.where((t_best >= 0)[:, None], node1, t_state))
                t_stateB.copy_(t_state.repeat_interleave(P, 0)); t_sx.copy_(t_state[:, 0])
            t_nodes.copy_(t_base); t_nodes[:, :, 1:3] += t_stateB[:, None, 0:2]
            A.guidance_plan(Q, opt, t_cnt.data_ptr(), t_cls.data_ptr(), t_ids.data_ptr(), t_sel.data_ptr(), t_mode.data_ptr(), t_src.data_ptr(),
                            t_init.data_ptr(), t_dummy.data_ptr(), t_dis.data_ptr(), t_gid.data_ptr(), t_w.data_ptr())
            A.warmstart(t_stateB.data_ptr(), t_mode.data_ptr(), t_src.data_ptr(), deceleration=decel)
            A.sample_guidance(B, R, t_nodes.data_ptr(), t_ncnt.data_ptr(), t_gpos.data_ptr(), t_gvel.data_ptr(), t_status.data_ptr())
            A.init_with_guidance(t_gpos.data_ptr(), t_gvel.data_ptr(), t_init.data_ptr())
            A.linearize_topology_ex(t_ob.data_ptr(), M, t_sc.data_ptr(), t_sx.data_ptr(), r, d_is_original=t_dummy.data_ptr())
            A.solve(sync=False)
            A.guidance_decide(Q, opt, d_pobj, d_code, t_dis.data_ptr(), t_gid.data_ptr(), t_w.data_ptr(), t_state.data_ptr(), t_best.data_ptr(),
                              t_exit.data_ptr(), t_cmd.data_ptr(), t_ids.data_ptr(), t_sel.data_ptr(), deceleration=decel, control_dt=cdt)
            A.gather_best(t_best.data_ptr(), Q, P, t_wx.data_ptr(), t_wu.data_ptr())
        A.synchronize()
        got = A.get()
        # ---- B: the same tick, the hand-off by the mirrors
        if tick > 0:
            for q in range(Q):
                if dec["best"][q] >= 0:
                    state[q] = ref["xtraj"][q * P + int(dec["best"][q]), 1]
        stateB = np.repeat(state, P, axis=0)
        plan = md.guidance_plan(counts, classes, ids, sel, n_paths, **kw)
        nodes = base_nodes.copy(); nodes[:, :, 1:3] += stateB[:, None, 0:2]
        samples = [md.sample_guidance(nodes[b, :node_count[b]], N, Bh.dims.dt, n_nodes_max=R) for b in range(B)]
        gpos, gvel = np.stack([sm[0] for sm in samples]), np.stack([sm[1] for sm in samples])
        h_state, h_mode, h_src, h_init, h_dummy = _up(stateB), _up(plan["mode"]), _up(plan["src"]), _up(plan["init_enabled"]), _up(plan["rows_dummy"])
        h_gpos, h_gvel, h_sx = _up(gpos), _up(gvel), _up(state[:, 0].copy())
        torch.cuda.synchronize()
        Bh.warmstart(h_state.data_ptr(), h_mode.data_ptr(), h_src.data_ptr(), deceleration=decel)
        Bh.init_with_guidance(h_gpos.data_ptr(), h_gvel.data_ptr(), h_init.data_ptr())
        Bh.linearize_topology_ex(t_ob.data_ptr(), M, t_sc.data_ptr(), h_sx.data_ptr(), r, d_is_original=h_dummy.data_ptr())
        Bh.solve()
        ref = Bh.get()
        dec = md.guidance_decide(ref["pobj"], ref["exit_code"], plan["disabled"], plan["guidance_id"], plan["weight"], state, ref["xtraj"], ref["utraj"],
                                 ids, sel, n_paths, True, deceleration=decel, control_dt=cdt)
        ids, sel = dec["planner_ids"], dec["selection"]
        # ---- equal, bit for bit
        print(f"[hand-off loop] tick {tick}: counts {counts.tolist()}, exit codes {got['exit_code'].tolist()} (host {ref['exit_code'].tolist()}), best "
              f"{t_best.cpu().numpy().tolist()} (host {dec['best'].tolist()}), weights {plan['weight'].tolist()}, existing {plan['existing_guidance'].tolist()}, "
              f"selection {sel.tolist()}, cmd {t_cmd.cpu().numpy().tolist()}")
        for k, t in (("mode", t_mode), ("src", t_src), ("init_enabled", t_init), ("rows_dummy", t_dummy), ("disabled", t_dis), ("guidance_id", t_gid), ("weight", t_w)):
            assert _same(t.cpu().numpy(), plan[k]), (tick, k)
        assert _same(t_gpos.cpu().numpy(), gpos) and _same(t_gvel.cpu().numpy(), gvel)
        assert t_status.cpu().numpy().tolist() == [sm[2] for sm in samples] == [0, 0, 1] * Q
        x0_a, xinit_a = A.debug_get_x0(); x0_b, xinit_b = Bh.debug_get_x0()
        assert _same(x0_a, x0_b) and _same(xinit_a, xinit_b) and _same(A.debug_get_params(), Bh.debug_get_params())
        for k in ("xtraj", "utraj", "pobj", "exit_code"):
            assert _same(got[k], ref[k]), (tick, k)
        assert np.array_equal(t_best.cpu().numpy(), dec["best"]) and np.array_equal(t_exit.cpu().numpy(), dec["exit"]) and _same(t_cmd.cpu().numpy(), dec["cmd"])
        assert np.array_equal(t_ids.cpu().numpy(), ids) and np.array_equal(t_sel.cpu().numpy(), sel)
        assert _same(t_state.cpu().numpy(), state)
        wx = t_wx.cpu().numpy().reshape(Q, N + 1, 5)
        for q in range(Q):
            if dec["best"][q] >= 0:
                assert _same(wx[q], ref["xtraj"][q * P + int(dec["best"][q])])
            else:
                assert np.isnan(wx[q]).all()
        guided = (plan["rows_dummy"] == 0)
        seen["disabled"] |= bool(plan["disabled"].any())
        seen["existing"] |= bool((guided & (plan["existing_guidance"] == 1) & (plan["init_enabled"] == 0) & (plan["src"] == np.arange(B))).any())
        seen["weighted"] |= bool((plan["weight"] == w_cons).any())
        seen["winner"] |= bool((dec["best"] >= 0).any())
    assert all(seen.values()), seen
    A.close(); Bh.close()
