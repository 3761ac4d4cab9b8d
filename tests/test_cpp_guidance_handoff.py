"""C++ guidance hand-off (mpc_planner_modules/guidance_handoff.h: GuidanceSpline, guidancePlan, guidanceDecide; guidance_handoff_batch.h:
BatchedGuidanceHandoff) against the numpy mirrors (mpc_planner_amd/modules.py sample_guidance / guidance_plan / guidance_decide), values
bitwise (%.17g round-trips a double).  CPU: the Solver-free header alone, no generated header, nothing touches a GPU.  GPU: the batched twin
equals the same calls made through the C-ABI byte for byte, and both equal the mirrors."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "mpc_planner_amd", "cpp")
SRC = os.path.join(ROOT, "tests", "cpp", "test_guidance_handoff.cpp")
BIN = os.path.join(ROOT, "build", "test_guidance_handoff")
N, DT, R, NX = 20, 0.2, 6, 5
DECEL, CDT, W = 2.5, 0.04, 0.75


def _build():
    """The program, unless it is there and newer than everything it is made of (the library included); build() first, for the library."""
    deps = [SRC, os.path.join(ROOT, "mpc_planner_amd", "libtmpc_hip.so")] + [os.path.join(CPP, "include", d, f) for d, f in (
        ("mpc_planner_modules", "guidance_handoff.h"), ("mpc_planner_modules", "guidance_handoff_batch.h"), ("mpc_planner_modules", "reference_path.h"),
        ("mpc_planner_types", "prep_arithmetic.h"), ("mpc_planner_solver", "device_plumbing.h"))]
    if os.path.exists(BIN) and all(os.path.exists(d) and os.path.getmtime(d) <= os.path.getmtime(BIN) for d in deps):
        return
    import __graft_entry__ as g
    g.build()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(CPP, "include"),
                           "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include", SRC, "-L", os.path.join(ROOT, "mpc_planner_amd"), "-ltmpc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "mpc_planner_amd"), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-o", BIN])


def _nodes(rng, n):
    """n nodes in a buffer of R: times that start away from 0 and end before N dt = 4 s (both continuations are sampled)."""
    out = np.full((R, 3), -9e9)
    if n > 0:
        out[:n, 0] = rng.uniform(-0.5, 0.5) + np.cumsum(rng.uniform(0.2, 0.9, n))
        out[:n, 1:] = np.cumsum(rng.normal(size=(n, 2)), 0)
    return out


def _script(rng, n_paths, Q, ticks):
    """Per tick: enable_output, counts [Q], classes / previously_selected / node counts [Q][n_paths], nodes [Q][n_paths][R][3].  Most classes
    survive a tick (existing guidance); node counts 0 .. R, and one list with a repeated time."""
    classes = rng.integers(0, 4, (Q, n_paths))
    out = []
    for t in range(ticks):
        classes = np.where(rng.uniform(size=(Q, n_paths)) < 0.6, classes, rng.integers(0, 4, (Q, n_paths)))
        counts = rng.integers(0, n_paths + 1, Q)
        if t == 0:
            counts[:] = n_paths
        n_nodes = rng.integers(2, R + 1, (Q, n_paths))
        if t == 1:
            n_nodes[0, 0] = 1
        nodes = np.stack([np.stack([_nodes(rng, n_nodes[q, i]) for i in range(n_paths)]) for q in range(Q)])
        if t == 2:
            nodes[1, 0, 1, 0] = nodes[1, 0, 0, 0]
        out.append(dict(enable_output=t != 3, counts=counts.astype(np.int32), classes=classes.astype(np.int32), prev=rng.integers(0, 2, (Q, n_paths)).astype(np.uint8),
                        n_nodes=n_nodes, nodes=nodes))
    return out


def _case_file(path, cfg, Q, state, script, host=None, device=None):
    n_paths, tmpcpp, warm, shift, explicit = cfg
    P = n_paths + int(tmpcpp)
    vals = [N, DT, R, n_paths, int(tmpcpp), int(warm), int(shift), W, int(explicit), Q, len(script), NX, DECEL, CDT] + list(state.ravel())
    if host is not None:
        vals += list(host["xtraj"].ravel()) + list(host["utraj"].ravel())
    else:
        vals += list(device["dims"]) + list(device["xinit"].ravel()) + list(device["x0"].ravel()) + list(device["params"].ravel())
    for t, tick in enumerate(script):
        vals += [int(tick["enable_output"])] + list(tick["counts"])
        for q in range(Q):
            for i in range(n_paths):
                vals += [tick["classes"][q, i], tick["prev"][q, i], tick["n_nodes"][q, i]] + list(tick["nodes"][q, i].ravel())
        if host is not None:
            vals += list(host["pobj"][t]) + list(host["code"][t])
    np.array(vals, float).tofile(path)
    return P


def _parse(stdout):
    ticks = []
    for l in stdout.splitlines():
        w = l.split()
        if w[0] == "tick":
            ticks.append({})
        else:
            ticks[-1][w[0]] = np.array([float(x) for x in w[1:]])
    return ticks


def _check_against_mirrors(ticks, cfg, Q, state, script, dt):
    """Every printed array of every tick against the mirrors; pobj / code / v1 / w0 are the program's (the host case's inputs, the device
    case's solve).  Returns what the ticks covered."""
    from mpc_planner_amd import modules as md
    n_paths, tmpcpp, warm, shift, explicit = cfg
    P = n_paths + int(tmpcpp); B = Q * P
    ids, sel = np.full((Q, P), -1, np.int32), np.tile(np.array([-1, 0, -1], np.int32), (Q, 1))
    seen = dict(disabled=False, existing=False, invalid=False, none=False)
    assert len(ticks) == len(script)
    for t, (got, tick) in enumerate(zip(ticks, script)):
        plan = md.guidance_plan(tick["counts"], tick["classes"], ids, sel, n_paths, tmpcpp, warm, shift, W, tick["prev"] if explicit else None)
        for k in ("mode", "src", "init_enabled", "rows_dummy", "disabled", "guidance_id", "weight"):
            assert np.array_equal(got[k], plan[k].astype(float)), (t, k)
        gpos, gvel, status = np.zeros((B, N + 1, 2)), np.zeros((B, N + 1, 2)), np.ones(B)
        for q in range(Q):
            for i in range(min(max(int(tick["counts"][q]), 0), n_paths)):
                gpos[q * P + i], gvel[q * P + i], status[q * P + i] = md.sample_guidance(tick["nodes"][q, i, :tick["n_nodes"][q, i]], N, dt, n_nodes_max=R)
        assert np.array_equal(got["status"], status), t
        assert np.array_equal(got["gpos"], gpos.ravel()) and np.array_equal(got["gvel"], gvel.ravel()), t
        xtraj, utraj = np.zeros((B, N + 1, NX)), np.zeros((B, N, 2))
        xtraj[:, 1, 3], utraj[:, 0, 1] = got["v1"], got["w0"]
        dec = md.guidance_decide(got["pobj"], got["code"].astype(np.int32), plan["disabled"], plan["guidance_id"], plan["weight"], state, xtraj, utraj, ids, sel,
                                 n_paths, tmpcpp, deceleration=DECEL, control_dt=CDT, enable_output=tick["enable_output"])
        assert np.array_equal(got["best"], dec["best"]) and np.array_equal(got["exit"], dec["exit"]) and np.array_equal(got["cmd"], dec["cmd"].ravel()), t
        assert np.array_equal(got["ids"], dec["planner_ids"].ravel()) and np.array_equal(got["sel"], dec["selection"].ravel()), t
        ids, sel = dec["planner_ids"], dec["selection"]
        seen["disabled"] |= bool(plan["disabled"].any())
        seen["existing"] |= bool(warm and ((plan["init_enabled"] == 0) & (plan["rows_dummy"] == 0)).any())
        seen["invalid"] |= bool((status[plan["rows_dummy"] == 0] == 1).any())
        seen["none"] |= bool((dec["best"] < 0).any())
    return seen


@pytest.mark.parametrize("cfg", [(2, True, True, True, False), (3, True, True, False, True), (3, False, False, True, False)])
def test_header_equals_the_mirrors_bitwise(tmp_path, cfg):
    """3 scenes, 6 ticks; P = 3, 4 and 3 (no non-guided planner); previously_selected from the state and as an input; synthetic objectives (small
    integers: ties) and exit codes; node lists of 1 .. 6 nodes and one with a repeated time."""
    _build()
    Q, ticks = 3, 6
    rng = np.random.default_rng(11 + cfg[0] + int(cfg[4]))
    script = _script(rng, cfg[0], Q, ticks)
    P = cfg[0] + int(cfg[1]); B = Q * P
    state = rng.normal(size=(Q, NX)); state[:, 3] = (0.05, 1.0, 2.0)
    host = dict(xtraj=rng.normal(size=(B, N + 1, NX)), utraj=rng.normal(size=(B, N, 2)), pobj=rng.integers(1, 4, (ticks, B)).astype(float),
                code=rng.choice(np.array([1, 1, 1, 0, -1, 2]), (ticks, B)))
    host["code"][1, :P] = 0                                                # scene 0 has no winner at tick 1
    f = str(tmp_path / "case.bin")
    _case_file(f, cfg, Q, state, script, host=host)
    out = subprocess.run([BIN, "host", f], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = _parse(out.stdout)
    for t in range(ticks):                                                 # the program printed the inputs it was given
        assert np.array_equal(got[t]["pobj"], host["pobj"][t]) and np.array_equal(got[t]["v1"], host["xtraj"][:, 1, 3])
    seen = _check_against_mirrors(got, cfg, Q, state, script, DT)
    assert seen["disabled"] and seen["invalid"] and seen["none"] and (seen["existing"] or not cfg[2]), seen


@pytest.mark.gpu
def test_batched_twin_equals_the_c_abi_path(tmp_path):
    """2 scenes x (2 + 1) planners on a solved batch of the small hand-written shape, 4 ticks: BatchedGuidanceHandoff (one upload, plan, sample,
    decide, its own state) against tmpc_guidance_plan / tmpc_sample_guidance / tmpc_guidance_decide called with buffers of the program's own
    -- byte for byte, state included --, and against the mirrors."""
    from mpc_planner_amd import scenes, solver
    _build()
    cfg, Q, ticks, M, S = (2, True, True, True, False), 2, 4, 8, 5
    P = 3
    rng = np.random.default_rng(23)
    script = _script(rng, cfg[0], Q, ticks)
    scs = [scenes.make_scene(320 + q, N=N, M=M, B=P) for q in range(Q)]
    dims = solver.default_dims(N=N, S=S, n_lin=M, M=M)
    state = np.stack([sc["xinit"][0] for sc in scs])
    device = dict(dims=[S, M, M, dims.npar], xinit=np.concatenate([sc["xinit"] for sc in scs]), x0=np.concatenate([sc["x0"] for sc in scs]),
                  params=np.concatenate([sc["params"] for sc in scs]))
    f = str(tmp_path / "case.bin")
    _case_file(f, cfg, Q, state, script, device=device)
    out = subprocess.run([BIN, "device", f], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.count("equal 1") == ticks and "equal 0" not in out.stdout
    got = _parse("\n".join(l for l in out.stdout.splitlines() if not l.startswith("equal")))
    print(f"[twin] best per tick {[g['best'].tolist() for g in got]}, exit codes {got[0]['code'].tolist()}")
    seen = _check_against_mirrors(got, cfg, Q, state, script, dims.dt)
    assert seen["existing"], seen
