#!/usr/bin/env python3
"""bench.py -- MPC solves/s of the batched T-MPC solve path on MI355X (BASELINE.json metric).

A "step" = one pass of the hot path over one launch batch: `scenes` scenes x 64 guidance trajectories
(configs[1]: Jackal MPCC, N=20, 8 obstacles, 64 T-MPC guidance trajectories per control tick), i.e. the batched
counterpart of GuidanceConstraints::optimize (guidance_constraints.cpp:264-388): one solve launch over all
trajectories + record packing + (N>1: ONE RCCL all-gather of the 16-byte records) + FindBestPlanner per scene.
Inputs are resident in HBM before the timed region.  One solve = one trajectory's full Solver::solve()
(n_sqp = 10 RTI iterations).  Weak scaling: every rank owns `scenes` x 64 trajectories of each scene's
(64 x world_size)-trajectory guidance set.

Usage: python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
A plain run sets up, warms up, times the K steps and prints the result line (plus DIR/<name>.npy: what the last timed step computed).
--full adds everything else: the CPU baseline, the oracle parity and FindBestPlanner checks of the launch, the tight-tolerance leg, the
end-to-end leg and the control-tick latencies.
N > 1: either under `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...` (one rank per GPU; RANK / LOCAL_RANK /
WORLD_SIZE / MASTER_* from the environment), or the plain command -- without WORLD_SIZE in the environment bench.py re-executes itself
under torch.distributed.run on 127.0.0.1 (self_launch below); either way rank 0 prints exactly ONE JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

N_H, M_OBS, S_SEG, TRAJ = 20, 8, 5, 64          # configs[1]
NV, NX, NU = 7, 5, 2
HBM_PEAK_GBS = 8000.0                           # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
FP64_VALU_PEAK_TFLOPS = 78.6                    # MI355X FP64 vector peak (AMD spec; f64 MFMA has the same rate)


# BASELINE.json configs as bench workloads.  configs[1] (cfg2) is what the metric is quoted on and the default; cfg4 / cfg5 are the
# multi-GPU configurations (one guidance / scenario set split over the ranks): `--workload cfg4` under torch.distributed.run.
WORKLOADS = {
    "cfg2": dict(dims=dict(N=20, S=5, n_lin=8, M=8), scene=dict(N=20, M=8), traj=64, nh=16, npar=135,
                 what="configs[1]: Jackal MPCC N=20, 8 obstacles, 64 T-MPC guidance trajectories per scene"),
    "cfg3": dict(dims=dict(N=30, S=5, n_lin=8, M=8, n_slk=12, slack=1, cost_model=1), scene=dict(N=30, M=8, slack=True, n_decomp=12), traj=512, nh=28, npar=172,
                 one_set=True, what="configs[2] as named: Jackal CA-MPC (curvature_aware_contouring.py:48-105, spline ODE s' = v) + guidance + 8 ellipsoids + 12 decomp "
                                    "(static) rows, slack model, N=30, ONE set of 512 trajectories"),
    "cfg3_mpcc": dict(dims=dict(N=30, S=5, n_lin=8, M=8, n_slk=12, slack=1), scene=dict(N=30, M=8, slack=True, n_decomp=12), traj=512, nh=28, npar=172,
                      one_set=True, what="the rosnavigation T-MPC stack (MPCC contouring instead of the curvature-aware cost; rounds 1-3 ran configs[2] as this), "
                                         "slack model + guidance + 8 ellipsoids + 12 decomp rows, N=30, ONE set of 512 trajectories"),
    "jackal": dict(dims=dict(N=30, S=3, n_lin=5, M=5, row_model=1), oracle_dims=dict(N=30, S=3, n_lin=5, M=0, n_gauss=5), scene=dict(N=30, M=5, S=3, chance=True),
                   traj=64, nh=10, npar=82,
                   what="mpc_planner_jackal's default (generate_jackal_solver.py:53-73; not a BASELINE config): T-MPC with Gaussian chance constraints "
                        "(gaussian_constraints.py:66-113) as collision avoidance, N=30, 5 obstacles, 3 spline segments, 64 guidance trajectories per scene"),
    "cfg4": dict(dims=dict(N=20, S=5, n_lin=12, M=12), scene=dict(N=20, M=12), traj=4096, nh=24, npar=175, one_set=True,
                 what="configs[3]: T-MPC++ 4096 guidance trajectories, N=20, 12 obstacles, ONE guidance set split over the ranks"),
    "cfg5": dict(dims=dict(N=20, S=5, n_lin=0, M=0, n_slk=24, slack=1), scene=dict(N=20, M=8, slack=True, n_scenario=24), traj=32, nh=24,
                 npar=127, one_set=True, scenario=dict(n_obstacles=8, n_scenarios=256, n_rows=24),
                 what="configs[4]: SH-MPC, per step: every scenario solver samples 8 obstacles x 256 scenarios on device (tmpc_sample_scenarios), reduces them to "
                      "24 halfspaces per stage (tmpc_scenario_halfspaces), solves, counts its support (tmpc_scenario_support); 32 scenario solvers split over the ranks"),
}


def library_sha256():
    """Identity of the kernels a profile was taken on: sha256 over the library's sources (csrc/*.hip, *.hpp, include/tmpc_hip.h) --
    stable across rebuilds of the same sources on different machines, unlike a hash of the binary."""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "mpc_planner_amd", "csrc")
    for f in sorted(os.listdir(csrc)) + [os.path.join(ROOT, "include", "tmpc_hip.h")]:
        path = f if os.path.isabs(f) else os.path.join(csrc, f)
        if path.endswith((".hip", ".hpp", ".h")):
            with open(path, "rb") as fh:
                h.update(fh.read())
    return h.hexdigest()


def flops_per_solve(n_sqp_mean, n_ipm_per_qp, N=N_H, nv=NV, nx=NX, nh=2 * M_OBS):
    """SURVEY.md 8(d) algorithmic FP64 flop model, with MEASURED iteration counts."""
    f_dyn = 12 * (2 * nx * nx * nv + 2 * nx * nv * nv + 20)
    f_cost = 927
    f_con = 43 * nh
    f_reg = 10 * nv ** 3
    f_ric = 2 * nh * nv * nv + 2 * nv ** 3 + 12 * nv * nv + 40 * (nv + nh)
    return n_sqp_mean * (N * (f_dyn + f_cost + f_con + f_reg) + n_ipm_per_qp * N * f_ric)


def bytes_per_solve(N=N_H, npar=135, nv=NV, nx=NX, nu=NU):
    """SURVEY.md 8(d) compulsory HBM bytes: parameters + warm start + xinit in, trajectories out."""
    return 8 * (N * npar + (N + 1) * nv + nx + (N + 1) * nx + N * nu)


def usable_cpus():
    """CPUs this process can actually run on: scheduler affinity capped by the cgroup CPU quota (the bench box shows 256
    logical CPUs to a container whose quota is 16)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as fh:                         # cgroup v2: "<quota> <period>" or "max <period>"
            q, per = fh.read().split()
            if q != "max":
                n = min(n, max(1, int(float(q) / float(per))))
    except OSError:
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as fq, open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as fp:
                q, per = int(fq.read()), int(fp.read())
                if q > 0:
                    n = min(n, max(1, q // per))
        except OSError:
            pass
    return n


def cpu_baseline(n_scenes, quick=False):
    """Reported baseline (NOT the target): the restated acados-equivalent CPU path (oracle/, kind 'port'), OpenMP over trajectories like
    guidance_constraints.cpp:279, on all host cores.  Protocol = BASELINE.md section 3: steady clock around the whole batch call, 20 warm-up
    calls, 200 timed repetitions, p50 / p90, solves/s = B / p50 -- on a BOUNDED batch (16 solves per core per call, tiled from `n_scenes`
    scenes of the bench workload) so that the 220 calls stay within ~20 s of CPU work; the literal 64-trajectory tick and the one-thread
    single-solve latency beside it."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as O
    from mpc_planner_amd import scenes
    pb = O.problem(N=N_H, S=S_SEG, n_lin=M_OBS, M=M_OBS)
    cores = usable_cpus()
    batch = scenes.make_batch(range(n_scenes), N=N_H, M=M_OBS, B=TRAJ)
    B = 16 * cores
    n_have = batch["xinit"].shape[0]
    import math
    stride = next(c for c in (7, 11, 13, 17, 19, 23, 1) if math.gcd(c, n_have) == 1)    # coprime to the sample size: every scene is visited
    pick = (np.arange(B) * stride) % n_have
    args = (pb, batch["xinit"][pick], batch["x0"][pick].reshape(B, -1), batch["params"][pick].reshape(B, -1))

    def timed(call, warm, reps, budget_s):
        for _ in range(warm):
            call()
        ts, t_start = [], time.perf_counter()
        for _ in range(reps):
            t1 = time.perf_counter(); call(); ts.append(time.perf_counter() - t1)
            if time.perf_counter() - t_start > budget_s:                  # slow host: keep the bench within minutes, say how many were taken
                break
        return np.array(ts)

    warm, reps = (1, 3) if quick else (20, 200)                      # quick: the launcher self-test (tests/test_bench_launcher.py), not a measurement
    ts = timed(lambda: O.solve_batch(*args, num_threads=cores), warm, reps, 40.0)
    sl = slice(0, TRAJ)
    tick = timed(lambda: O.solve_batch(pb, batch["xinit"][sl], batch["x0"][sl].reshape(TRAJ, -1), batch["params"][sl].reshape(TRAJ, -1), num_threads=cores), warm, reps, 15.0)
    one = []                                                         # single-thread latency of ONE Solver::solve()
    for i in range(4 if quick else 64):
        s1 = slice(i, i + 1)
        t1 = time.perf_counter(); O.solve_batch(pb, args[1][s1], args[2][s1], args[3][s1], num_threads=1); one.append(time.perf_counter() - t1)
    p50, p90 = float(np.percentile(ts, 50)), float(np.percentile(ts, 90))
    return {"value": B / p50, "unit": "solves/s", "cores": cores, "kind": "port",
            "protocol": f"BASELINE.md section 3: {warm} warm-up calls, {reps} repetitions of the whole batch call, solves/s = B / p50",
            "batch": B, "repetitions": int(len(ts)), "batch_ms_p50": p50 * 1e3, "batch_ms_p90": p90 * 1e3,
            "tick_b64": {"repetitions": int(len(tick)), "ms_p50": float(np.percentile(tick, 50) * 1e3), "ms_p90": float(np.percentile(tick, 90) * 1e3),
                         "solves_per_s": float(TRAJ / np.percentile(tick, 50)), "what": "one 64-trajectory guidance set per call (the reference's OpenMP loop as it runs per control tick)"},
            "single_thread_solve_ms_p50": float(np.percentile(one, 50) * 1e3),
            "sample": f"{B} solves per call (16 per core) drawn from {n_scenes} scenes x {TRAJ} trajectories of the same workload, {len(ts)} timed calls after {warm} warm-ups "
                      f"({float(ts.sum()):.1f} s), restated acados-equivalent C oracle (oracle/), OpenMP over trajectories on the {cores} CPUs usable by this "
                      f"process (affinity / cgroup quota; {os.cpu_count()} logical CPUs visible)"}


def parity_block(O, wl, batch, res, n_check, opts):
    """Compare `n_check` trajectories of a launch, spread evenly over the whole batch (first and last scene included), with the CPU oracle."""
    B = batch["xinit"].shape[0]
    idx = np.unique(np.linspace(0, B - 1, min(n_check, B)).round().astype(int))
    n = len(idx)
    pbo = O.problem(**wl.get("oracle_dims", wl["dims"]), **opts)
    xt, ut, info = O.solve_batch(pbo, batch["xinit"][idx], batch["x0"][idx].reshape(n, -1), batch["params"][idx].reshape(n, -1),
                                 num_threads=usable_cpus())
    both = (info["exit_code"] == 1) & (res["exit_code"][idx] == 1)
    sx = np.maximum(np.abs(xt[both]).max(axis=2, keepdims=True), 1.0)
    su = np.maximum(np.abs(ut[both]).max(axis=2, keepdims=True), 1.0)
    return {"trajectories": int(n), "sample": f"every {max(1, (B - 1) // max(1, n - 1))}-th trajectory of the {B} in the timed launch (first and last included)",
            "parity_max_rel": float(max((np.abs(res["xtraj"][idx][both] - xt[both]) / sx).max(),
                                        (np.abs(res["utraj"][idx][both] - ut[both]) / su).max())) if both.any() else None,
            "exit_code_mismatch": int((res["exit_code"][idx] != info["exit_code"]).sum()),
            "sqp_iter_mismatch": int((res["sqp_iter"][idx] != info["sqp_iter"]).sum()),
            "ipm_iter_mismatch": int((res["qp_iter_total"][idx][both] != info["qp_iter_total"][both]).sum()),
            "against": "oracle/ (restated acados-equivalent CPU path), same options"}


def best_index_block(O, wl, batch, res, best, set_size, max_sets):
    """FindBestPlanner per set of the timed launch: the device's index against (i) the reference's rule (strict '<', lowest index, init
    1e10: orc_find_best) applied to the DEVICE's objectives -- integer work, must be 0 mismatches -- and (ii) the index the ORACLE picks from
    its own solves of the same sets.  (ii) can differ without either being wrong: guidance trajectories that reach the same optimum have
    objectives that tie to rounding, and then the lowest index among the tied ones is decided by the last bits; such cases are counted as
    ties (|objective difference| <= 1e-9 relative), anything else as a true mismatch."""
    B = batch["xinit"].shape[0]
    n_sets = min(B // set_size, max_sets)
    which = np.unique(np.linspace(0, B // set_size - 1, n_sets).round().astype(int))
    idx = (which[:, None] * set_size + np.arange(set_size)[None, :]).ravel()
    n = len(idx)
    pbo = O.problem(**wl.get("oracle_dims", wl["dims"]))
    _, _, info = O.solve_batch(pbo, batch["xinit"][idx], batch["x0"][idx].reshape(n, -1), batch["params"][idx].reshape(n, -1), num_threads=usable_cpus())
    mism_rule = mism_oracle = ties = 0
    worst = 0.0
    for j, sset in enumerate(which):
        sl = slice(j * set_size, (j + 1) * set_size)
        dsl = slice(sset * set_size, (sset + 1) * set_size)
        dev_best = int(best[sset])                                                     # (index inside the set, -1: no successful trajectory)
        rule = O.find_best(res["pobj"][dsl], res["exit_code"][dsl])
        ref = O.find_best(info["pobj"][sl], info["exit_code"][sl])
        mism_rule += int(dev_best != rule)
        if dev_best != ref:
            mism_oracle += 1
            if dev_best >= 0 and ref >= 0:
                a, b = float(res["pobj"][dsl][dev_best]), float(info["pobj"][sl][ref])
                rel = abs(a - b) / max(1.0, abs(b))
                worst = max(worst, rel)
                ties += int(rel <= 1e-9)
    return {"sets_checked": int(len(which)), "set_size": int(set_size), "trajectories_solved_by_the_oracle": int(n),
            "best_index_mismatch_vs_rule_on_device_objectives": mism_rule,
            "best_index_mismatch_vs_oracle": mism_oracle, "of_which_objective_ties_at_rounding": ties,
            "true_mismatches": mism_oracle - ties, "worst_relative_objective_gap_among_mismatches": worst,
            "what": "device FindBestPlanner index per set vs orc_find_best on the device's objectives (integer work: must be 0) and vs the index the oracle "
                    "picks from its own solves (ties at rounding counted separately)"}



def end_to_end_leg(a, dims, sv, batch, t_xinit, t_x0, t_params, dev, n_sets, traj, res_resident, best_resident, batch_in=None):
    """`value_end_to_end` (round-3 verdict item 6): the step as a control tick pays for it.  Per step the host hands over only what a tick
    changes -- per scene: the state (xinit), the main solver's warm start, the parameter rows the shared modules write (weights, path, obstacle
    ellipsoids: ONE row block per scene, the set's planners read it through the parameter-sharing hint), the obstacle predictions; per
    trajectory: the guidance trajectory (position / velocity at t = k dt) -- and the device does the rest on the handle's stream:
    `*solver = *_solver` (broadcast of the warm start), initializeSolverWithGuidance (tmpc_init_with_guidance), LinearizedConstraints::update +
    setParameters (tmpc_linearize_topology), the solve, FindBestPlanner per scene, the winners' trajectories gathered (tmpc_gather_best) and
    copied back.  Uploads of step i + 1 run on a second stream under the solve of step i (double-buffered staging).  cfg 2, one GPU."""
    import torch
    from mpc_planner_amd import scenes, solver
    B = n_sets * traj
    N, npar, nv = dims.N, dims.npar, dims.nvar
    lead = np.arange(0, B, traj)
    host = {"xinit": batch["xinit"], "gpos": batch["guidance_pos"], "gvel": batch["guidance_vel"], "obst": batch["obstacle_pos"],
            "lead_rows": batch["params"][lead].reshape(n_sets, -1), "main_x0": None, "state_x": batch["xinit"][lead, 0].copy()}
    # the main solver's warm start of a scene: a planner's x0 differs from it in (x, y, psi, v) of nodes 1 .. N-1 only (guidance_constraints.cpp:401-413)
    host["main_x0"] = batch["x0"][lead].reshape(n_sets, -1).copy()
    # THREE distinct input sets rotate through the two staging buffers (round-4 verdict, weak #6: the same pinned buffers every step never
    # showed the device-built rows on changing inputs): set r = the launch's scenes rolled by r, so that every step's x0 / halfspace rows are
    # built from inputs that differ from the previous two steps' in every scene, and the last step's results have a known counterpart in the
    # resident step's (rolled the same way).
    N_ROT = 3
    per_traj = ("xinit", "gpos", "gvel")
    def rolled(k, v, r):
        return np.ascontiguousarray(np.roll(v, r * (traj if k in per_traj else 1), axis=0))
    pinned_sets = [{k: torch.from_numpy(rolled(k, v, r)).pin_memory() for k, v in host.items()} for r in range(N_ROT)]
    pinned = pinned_sets[0]
    # Inputs on which LinearizedConstraints::projectToSafety is NOT the identity (round-4 verdict, next-8): the first n_in scenes of rotation set 1
    # are replaced by scenes whose guidance has ~10 % of its trajectories carrying one point inside an obstacle's disc (scenes.make_scene(inside_share)).
    # They run through the timed loop like every other input; after timing one more step on set 1 is compared with the host mirror (below).
    n_in = 0
    if batch_in is not None:
        n_in = batch_in["xinit"].shape[0] // traj
        lead_in = np.arange(0, n_in * traj, traj)
        over = {"xinit": batch_in["xinit"], "gpos": batch_in["guidance_pos"], "gvel": batch_in["guidance_vel"], "obst": batch_in["obstacle_pos"],
                "lead_rows": batch_in["params"][lead_in].reshape(n_in, -1), "main_x0": None, "state_x": batch_in["xinit"][lead_in, 0].copy()}
        # the main solver's warm start: the scene's forward propagation = a planner's x0 outside (x, y, psi, v) of nodes 1 .. N-1; rebuilt like scenes.make_scene does
        from mpc_planner_amd import modules as _md
        over["main_x0"] = np.stack([_md.initialize_with_forward_propagation(batch_in["xinit"][i], N, scenes.DT, nv) for i in lead_in]).reshape(n_in, -1)
        for k, v in over.items():
            pinned_sets[1][k][:v.shape[0]].copy_(torch.from_numpy(np.ascontiguousarray(v)))
    stage = [{k: torch.empty(v.shape, dtype=v.dtype, device=dev) for k, v in pinned.items()} for _ in range(2)]
    h2d_bytes = sum(v.numel() * v.element_size() for v in pinned.values())
    t_scene_of = torch.arange(B, dtype=torch.int32, device=dev) // traj
    t_rec = torch.zeros((B, 2), dtype=torch.int64, device=dev)
    t_best = torch.full((n_sets,), -2, dtype=torch.int32, device=dev)
    nxd, nud = (N + 1) * dims.nx, N * NU
    t_wx = torch.empty((n_sets, nxd), dtype=torch.float64, device=dev); t_wu = torch.empty((n_sets, nud), dtype=torch.float64, device=dev)
    h_wx = torch.empty((n_sets, nxd), dtype=torch.float64).pin_memory(); h_wu = torch.empty((n_sets, nud), dtype=torch.float64).pin_memory()
    h_best = torch.empty((n_sets,), dtype=torch.int32).pin_memory()
    copy_stream = torch.cuda.Stream(device=dev)
    hs = torch.cuda.ExternalStream(sv.stream_ptr(), device=dev)
    uploaded = [torch.cuda.Event() for _ in range(2)]; consumed = [torch.cuda.Event() for _ in range(2)]
    x0v = t_x0.view(n_sets, traj, -1); pv = t_params.view(n_sets, traj, -1)

    def upload(i):
        sl = i % 2
        with torch.cuda.stream(copy_stream):
            if i >= 2:
                copy_stream.wait_event(consumed[sl])
            src = pinned_sets[i % N_ROT]
            for k in src:
                stage[sl][k].copy_(src[k], non_blocking=True)
            uploaded[sl].record(copy_stream)

    def step(i):
        sl = i % 2
        st = stage[sl]
        with torch.cuda.stream(hs):
            hs.wait_event(uploaded[sl])
            t_xinit.copy_(st["xinit"], non_blocking=True)
            x0v.copy_(st["main_x0"][:, None, :].expand(-1, traj, -1))            # *solver = *_solver (warm start part)
            pv[:, 0, :].copy_(st["lead_rows"])                                   # the scene's shared parameter rows: one block per set
        sv.init_with_guidance(st["gpos"].data_ptr(), st["gvel"].data_ptr())
        sv.linearize_topology(st["obst"].data_ptr(), t_scene_of.data_ptr(), st["state_x"].data_ptr(), scenes.ROBOT_RADIUS)
        consumed[sl].record(hs)
        sv.solve(sync=False)
        sv.pack_records(t_rec.data_ptr())
        sv.select_best_records(t_rec.data_ptr(), 1, n_sets, traj, t_best.data_ptr())
        sv.gather_best(t_best.data_ptr(), n_sets, traj, t_wx.data_ptr(), t_wu.data_ptr())
        with torch.cuda.stream(hs):
            h_wx.copy_(t_wx, non_blocking=True); h_wu.copy_(t_wu, non_blocking=True); h_best.copy_(t_best, non_blocking=True)

    steps, warm = a.steps, max(a.warmup, 2)
    upload(0)
    for i in range(warm):
        upload(i + 1); step(i)
    sv.synchronize(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(warm, warm + steps):
        upload(i + 1); step(i)
    sv.synchronize(); torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    # the uploads alone (what the second stream has to hide)
    t1 = time.perf_counter()
    for i in range(4):
        with torch.cuda.stream(copy_stream):
            for k in pinned:
                stage[0][k].copy_(pinned[k], non_blocking=True)
    copy_stream.synchronize()
    h2d_ms = (time.perf_counter() - t1) / 4 * 1e3
    k_ms = sv.get_timings()
    k_avg = float(np.mean(k_ms)) if len(k_ms) else None
    res = sv.get()
    ok = res["exit_code"] == 1
    r_last = (warm + steps - 1) % N_ROT                                   # the input set the last step solved: the resident results rolled the same way
    res_resident = {k: np.roll(v, r_last * traj, axis=0) for k, v in res_resident.items() if isinstance(v, np.ndarray) and v.shape[:1] == (B,)}
    best_resident = np.roll(best_resident, r_last)
    cmp = np.ones(B, bool)                                                # (the inside scenes replaced set 1's first n_in scenes: no resident counterpart there)
    if r_last == 1 and n_in:
        cmp[:n_in * traj] = False
    both = ok & (res_resident["exit_code"] == 1) & cmp
    best = h_best.numpy().copy()
    # FindBestPlanner: where the index differs from the resident step's, is it a tie at rounding (the two picks' objectives equal to 1e-9
    # relative: the device-built x0 differs from the host-built one in the last bit of atan2) or a true split?
    diff = np.flatnonzero((best != best_resident) & cmp[::traj])
    ties, worst_gap = 0, 0.0
    for sset in diff:
        if best[sset] >= 0 and best_resident[sset] >= 0:
            oa = float(res["pobj"][sset * traj + best[sset]]); ob = float(res_resident["pobj"][sset * traj + best_resident[sset]])
            gap = abs(oa - ob) / max(1.0, abs(ob))
            worst_gap = max(worst_gap, gap); ties += int(gap <= 1e-9)
    wx = h_wx.numpy().reshape(n_sets, N + 1, dims.nx)
    sel = np.flatnonzero(best >= 0)
    winners_ok = bool(np.array_equal(wx[sel], res["xtraj"][sel * traj + best[sel]])) if sel.size else None
    ms = elapsed / steps * 1e3
    projection = None
    if n_in:
        # one more step on rotation set 1 (multiple of N_ROT away from any assumption: upload it explicitly), then the device-built x0 / rows / results
        # of the inside scenes against the host mirror (modules.linearized_update with the Douglas-Rachford restatement) and a resident solve of the
        # host-built copies
        i_v = 1
        while i_v % N_ROT != 1 or i_v % 2 != 0:
            i_v += 1                                                    # a step index whose input set is 1 and whose staging buffer is 0
        upload(i_v); step(i_v)
        sv.synchronize(); torch.cuda.synchronize()
        nb = n_in * traj
        dev_par = t_params[:nb].cpu().numpy().reshape(nb, N, npar); dev_x0 = t_x0[:nb].cpu().numpy().reshape(nb, N + 1, nv)
        resv = sv.get()
        own = solver.own_parameter_columns(dims)
        want_par = batch_in["params"].reshape(nb, N, npar); want_x0 = batch_in["x0"].reshape(nb, N + 1, nv)
        ins = batch_in["inside"]
        rows_diff = float(np.abs(dev_par[:, :, own] - want_par[:, :, own]).max())
        rows_diff_inside = float(np.abs(dev_par[ins][:, :, own] - want_par[ins][:, :, own]).max()) if ins.any() else None
        # geometry on the DEVICE output: recover the projected point p of every perturbed (trajectory, stage) from two of its rows
        # (a_j = (o_j - p) / |o_j - p|  =>  p = o_j - d_j a_j, two rows give d) and check |p - o_j| >= r for every obstacle
        r_disc = 1e-3 + scenes.ROBOT_RADIUS
        worst_clear, moved_min = np.inf, np.inf
        M_l = dims.n_lin
        for bq in np.flatnonzero(ins):
            kq = int(batch_in["inside_at"][bq, 0])
            o = batch_in["obstacle_pos"][bq // traj][:, kq - 1]                      # [M][2]
            rowp = dev_par[bq, kq, own].reshape(M_l, 3)
            A2 = np.array([[-rowp[0, 0], rowp[1, 0]], [-rowp[0, 1], rowp[1, 1]]]); rhs = o[1] - o[0]
            if abs(np.linalg.det(A2)) < 1e-9:
                continue
            d01 = np.linalg.solve(A2, rhs)
            pq = o[0] - d01[0] * rowp[0, :2]
            worst_clear = min(worst_clear, float((np.hypot(*(pq[None] - o).T) - r_disc).min()))
            moved_min = min(moved_min, float(np.hypot(*(pq - want_x0[bq, kq, 2:4]))))
        chk = solver.BatchedSolver(dims, B_max=nb, device=dev.index or 0)
        chk.set_batch(batch_in["xinit"], batch_in["x0"], batch_in["params"])
        chk.set_param_sharing(solver.param_sharing_map(batch_in["params"], dims, traj))
        chk.solve(); rh = chk.get(); chk.close()
        okv = (rh["exit_code"] == 1) & (resv["exit_code"][:nb] == 1)
        projection = {"scenes": int(n_in), "trajectories": int(nb), "trajectories_with_a_point_inside_a_disc": int(ins.sum()),
                      "device_rows_vs_host_mirror_max_abs": rows_diff, "same_on_the_perturbed_trajectories": rows_diff_inside,
                      "device_x0_vs_host_max_abs": float(np.abs(dev_x0 - want_x0).max()),
                      "projected_points_min_clearance_from_any_disc": (worst_clear if np.isfinite(worst_clear) else None),
                      "projection_moved_every_perturbed_point_by_at_least": (moved_min if np.isfinite(moved_min) else None),
                      "exit_code_mismatch_vs_resident_solve_of_host_built_copies": int((resv["exit_code"][:nb] != rh["exit_code"]).sum()),
                      "ipm_iter_mismatch": int((resv["qp_iter_total"][:nb][okv] != rh["qp_iter_total"][okv]).sum()),
                      "max_abs_xtraj_diff": float(np.abs(resv["xtraj"][:nb][okv] - rh["xtraj"][okv]).max()) if okv.any() else None,
                      "success_fraction_perturbed": float((rh["exit_code"][ins] == 1).mean()) if ins.any() else None,
                      "what": "LinearizedConstraints::projectToSafety acting inside the end-to-end step: scenes with ~10 % of the guidance trajectories carrying one point "
                              "inside an obstacle's disc occupy the first scenes of rotation set 1 (timed like the rest); device-built rows vs the host mirror, "
                              "|p - o| >= r recovered from the device's rows, results vs a resident solve of the host-built copies"}
    return {"value_end_to_end": float(B * steps * ok.mean() / elapsed), "unit": "successful solves/s", "ms_per_step": ms,
            "h2d_bytes_per_step": int(h2d_bytes), "h2d_ms_alone": h2d_ms, "d2h_bytes_per_step": int((nxd + nud) * 8 * n_sets + 4 * n_sets),
            "step": ["H2D on a second stream (double-buffered): xinit, main warm start and shared parameter rows per scene, obstacle predictions, guidance trajectories",
                     "broadcast of the warm start to the set's planners", "tmpc_init_with_guidance", "tmpc_linearize_topology", "tmpc_solve", "tmpc_pack_records",
                     "tmpc_select_best_records", "tmpc_gather_best", "D2H of the winners' trajectories and indices"],
            "solve_kernel_ms_avg": k_avg,
            "bounded_by": ("the solve kernel (uploads hidden under it on the second stream; the device-side x0 / halfspace-row build, selection, gather and "
                           "the copy back add the difference)") if (k_avg and ms < 1.2 * k_avg) else "not the solve kernel alone: compare ms_per_step with solve_kernel_ms_avg and h2d_ms_alone",
            "vs_resident_step": {"exit_code_mismatch": int(((res["exit_code"] != res_resident["exit_code"]) & cmp).sum()), "trajectories_compared": int(cmp.sum()),
                                 "ipm_iter_mismatch": int((res["qp_iter_total"][both] != res_resident["qp_iter_total"][both]).sum()),
                                 "max_abs_xtraj_diff": float(np.abs(res["xtraj"][both] - res_resident["xtraj"][both]).max()) if both.any() else None,
                                 "best_index_mismatch": int(diff.size), "of_which_objective_ties_at_rounding": int(ties),
                                 "true_mismatches": int(diff.size - ties), "worst_relative_objective_gap_among_mismatches": worst_gap,
                                 "what": "the device rebuilt x0 and the halfspace rows from the uploaded guidance / obstacles; the resident step solved the host-built copies "
                                         "(compared after rolling the resident results like the last step's input set)"},
            "input_rotation": {"distinct_input_sets": N_ROT, "last_step_set": int(r_last),
                               "what": "set r = the launch's scenes rolled by r; the sets rotate through the two staging buffers, so consecutive steps build x0 / rows from different inputs"},
            "projection_exercise": projection,
            "winners_copied_back_equal_device_trajectories": winners_ok}


# keys every bench line carries, at every N (the driver's contract + this tier's roofline / cpu_baseline objects; cpu_baseline only when it
# was measured: --full without --no-cpu-baseline)
REQUIRED_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
                 "config", "roofline", "cpu_baseline", "parity")

DUMP_LIMIT_BYTES = 64 << 20                     # --dump-outputs: at most this much in all


def write_outputs(out_dir, arrays, per_traj, limit=DUMP_LIMIT_BYTES, seed=0):
    """--dump-outputs: every array as out_dir/<name>.npy in float64 (the integer outputs are exact in it).  Arrays whose first axis is the
    trajectory (`per_traj` rows) are cut to a fixed, seeded sample of trajectories -- the same rows in every such array, saved as
    trajectory_index.npy -- when the whole set would exceed `limit` bytes.  Returns {name: shape}."""
    arrays = {k: np.asarray(v) for k, v in arrays.items()}
    fixed = sum(v.size for v in arrays.values() if v.shape[:1] != (per_traj,))
    row = sum(v.size // per_traj for v in arrays.values() if v.shape[:1] == (per_traj,))
    if 8 * (fixed + row * per_traj) > limit:
        n_keep = max(1, (limit // 8 - fixed) // (row + 1))                     # (+1: the index array itself)
        idx = np.sort(np.random.default_rng(seed).choice(per_traj, n_keep, replace=False))
        arrays = {k: (v[idx] if v.shape[:1] == (per_traj,) else v) for k, v in arrays.items()}
        arrays["trajectory_index"] = idx
    os.makedirs(out_dir, exist_ok=True)
    shapes = {}
    for k, v in arrays.items():
        np.save(os.path.join(out_dir, f"{k}.npy"), np.ascontiguousarray(v, dtype=np.float64))
        shapes[k] = list(v.shape)
    return shapes


def gathered_index_inputs(dist, host_pg, batch, n_traj, rank, world):
    """Every rank's first n_traj trajectories (inputs) -> rank 0, over the host (gloo) group.  Returns on rank 0 a list over ranks of
    (xinit, x0, params) arrays, None elsewhere."""
    import torch
    parts = [np.ascontiguousarray(batch[k][:n_traj]).reshape(n_traj, -1) for k in ("xinit", "x0", "params")]
    mine = torch.from_numpy(np.concatenate(parts, axis=1))
    into = [torch.empty_like(mine) for _ in range(world)] if rank == 0 else None
    dist.gather(mine, into, dst=0, group=host_pg)
    if rank != 0:
        return None
    w = [p.shape[1] for p in parts]
    return [tuple(np.ascontiguousarray(a) for a in np.split(t.numpy(), np.cumsum(w)[:-1], axis=1)) for t in into]


def best_index_block_gathered(O, wl, inputs, rec, best, world, per_rank, n_chk):
    """FindBestPlanner on the all-gathered records (N > 1).  rec: [world][n_sets][per_rank] tmpc_record as the collective left them on rank 0;
    best: the device's index per set in the gathered numbering (rank * per_rank + t).  (i) the reference's rule (orc_find_best: init 1e10,
    strict '<', lowest index) on the gathered DEVICE objectives, ALL sets: integer work, must be 0 mismatches; (ii) the oracle's own pick
    from its solves of every rank's inputs, first n_chk sets; ties at rounding counted separately (see best_index_block)."""
    n_sets = rec.shape[1]
    obj = np.transpose(rec["objective"], (1, 0, 2)).reshape(n_sets, world * per_rank)
    ec = np.transpose(rec["exit_code"], (1, 0, 2)).reshape(n_sets, world * per_rank)
    mism_rule = sum(int(int(best[s]) != O.find_best(obj[s], ec[s])) for s in range(n_sets))
    pbo = O.problem(**wl.get("oracle_dims", wl["dims"]))
    pobj_o, ec_o = [], []
    for xi, x0, pr in inputs:                                   # one oracle batch per rank
        _, _, info = O.solve_batch(pbo, xi, x0, pr, num_threads=usable_cpus())
        pobj_o.append(info["pobj"].reshape(n_chk, per_rank)); ec_o.append(info["exit_code"].reshape(n_chk, per_rank))
    pobj_o = np.concatenate(pobj_o, axis=1); ec_o = np.concatenate(ec_o, axis=1)        # [n_chk][world * per_rank]: the gathered numbering
    mism_oracle = ties = 0
    worst = 0.0
    for s in range(n_chk):
        dev_best, ref = int(best[s]), O.find_best(pobj_o[s], ec_o[s])
        if dev_best != ref:
            mism_oracle += 1
            if dev_best >= 0 and ref >= 0:
                rel = abs(float(obj[s][dev_best]) - float(pobj_o[s][ref])) / max(1.0, abs(float(pobj_o[s][ref])))
                worst = max(worst, rel); ties += int(rel <= 1e-9)
    return {"on": "the all-gathered records (selection domain = world x per-rank trajectories per set)", "sets_checked_vs_rule": int(n_sets),
            "sets_checked_vs_oracle": int(n_chk), "set_size": int(world * per_rank), "trajectories_solved_by_the_oracle": int(n_chk * world * per_rank),
            "best_index_mismatch_vs_rule_on_device_objectives": mism_rule, "best_index_mismatch_vs_oracle": mism_oracle,
            "of_which_objective_ties_at_rounding": ties, "true_mismatches": mism_oracle - ties, "worst_relative_objective_gap_among_mismatches": worst}


def _free_port():
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def self_launch_command(n, argv, port=None):
    """The command `python bench.py --gpus N ...` turns itself into when it was started WITHOUT a torch.distributed environment: the
    driver's own N > 1 form (one rank per GPU, rendezvous on 127.0.0.1 -- the container's hostname may not resolve)."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
            "--master-port", str(port or _free_port()), os.path.abspath(__file__), *argv]


def self_launch(n, argv):
    """Re-execute under torch.distributed.run and pass the ranks' output through: rank 0's JSON line is the only line on stdout that
    starts with '{' (torchrun's own messages go to stderr).  The exit code is the job's."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")                     # dmabuf IPC only on this driver (RCCL needs it)
    env.setdefault("OMP_NUM_THREADS", str(max(1, usable_cpus() // n)))
    env["TMPC_BENCH_SELF_LAUNCHED"] = "1"
    return subprocess.call(self_launch_command(n, argv), env=env)


def launcher_selftest(a, world, rank):
    """`--launcher-selftest`: the N > 1 control flow of main() without a GPU (gloo in RCCL's place): scene-generation workers divided by the world
    size, the host group's barriers around rank 0's CPU baseline, `steps` timed all-gathers of 16-byte records the way a step does them, the
    selection rule on the gathered records, the gather of every rank's inputs to rank 0, the ranks held at the host barrier until rank 0 is
    done -- and rank 0 prints ONE JSON line with the full key set of a real line (REQUIRED_KEYS; the values that need a GPU are null and the line
    says so).  tests/test_bench_launcher.py drives this at N = 2 through the plain command."""
    import datetime
    import torch
    import torch.distributed as dist
    from mpc_planner_amd import distributed as D, scenes
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29511")
    gen_workers = a.gen_workers or max(1, usable_cpus() // world)
    n_sets, per = 2, 8
    batch = scenes.make_batch(range(100000 * rank, 100000 * rank + n_sets), workers=min(gen_workers, n_sets), N=N_H, M=M_OBS, B=per)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    host_pg = dist.new_group(backend="gloo", timeout=datetime.timedelta(minutes=60))
    cpu_base = None
    if a.full and not a.no_cpu_baseline:
        dist.barrier(group=host_pg)
        if rank == 0:
            cpu_base = cpu_baseline(1, quick=True)
        dist.barrier(group=host_pg)
    # stand-in records (no solve without a GPU): a deterministic objective per (rank, set, trajectory), every fifth trajectory failed
    g = np.arange(n_sets * per).reshape(n_sets, per)
    objective = 50.0 + ((g * 37 + 11 * rank) % 23).astype(np.float64)
    exit_code = np.where((g + rank) % 5 == 0, 4, 1).astype(np.int32)
    rec = D.pack_records_host(objective.ravel(), exit_code.ravel(), (g + n_sets * per * rank).ravel())
    t = torch.from_numpy(rec.view(np.int64).reshape(n_sets * per, 2).copy())
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        gathered = D.all_gather_records(t, world)
    dist.barrier()
    elapsed = time.perf_counter() - t0
    allrec = gathered.numpy().reshape(-1).view(D.RECORD_DTYPE).reshape(world, n_sets, per)
    best = D.find_best_planner_records(allrec)                  # what tmpc_select_best_records computes on device
    blk = gathered_index_inputs(dist, host_pg, batch, n_sets * per, rank, world)
    if rank == 0:
        obj = np.transpose(allrec["objective"], (1, 0, 2)).reshape(n_sets, world * per)
        ec = np.transpose(allrec["exit_code"], (1, 0, 2)).reshape(n_sets, world * per)
        rule = [int(np.argmin(np.where((ec[s] == 1) & (obj[s] < 1e10), obj[s], np.inf))) if ((ec[s] == 1) & (obj[s] < 1e10)).any() else -1 for s in range(n_sets)]
        out = {"launcher_selftest": True, "self_launched": os.environ.get("TMPC_BENCH_SELF_LAUNCHED") == "1",
               "metric": "launcher self-test (no GPU: records all-gathered per second over gloo; NOT the benchmark)", "value": world * n_sets * per * a.steps / elapsed,
               "unit": "records/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": elapsed / a.steps * 1e3, "higher_is_better": True,
               "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
               "config": {"workload": f"launcher self-test: {n_sets} sets x {per} stand-in records per rank", "gen_workers_per_rank": gen_workers,
                          "omp_num_threads": os.environ.get("OMP_NUM_THREADS")},
               "roofline": None, "records": int(allrec.size), "best": [int(b) for b in best],
               "parity": {"best_index": {"on": "the all-gathered records", "sets_checked_vs_rule": n_sets,
                                         "best_index_mismatch_vs_rule_on_device_objectives": int(sum(int(best[s]) != rule[s] for s in range(n_sets))),
                                         "inputs_gathered_from_ranks": len(blk), "input_shapes_rank_last": [list(x.shape) for x in blk[-1]]}}}
        if cpu_base is not None:
            out["cpu_baseline"] = cpu_base
        missing = [k for k in REQUIRED_KEYS if k not in out and not (k == "cpu_baseline" and cpu_base is None)]
        assert not missing, missing
        print(json.dumps(out))
    dist.barrier(group=host_pg)
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sets", type=int, default=1, help="one-set workloads (cfg3, cfg4, cfg5): K independent sets per launch instead of the one BASELINE names "
                                                         "(single GPU; shows the shape's kernels on a saturated GPU)")
    ap.add_argument("--scenes", type=int, default=512,
                    help="scenes (control ticks) per launch per GPU; 512 x 64 = 32768 trajectories keep the tail of uneven solve "
                         "times small (256 scenes: 497k solves/s, 1024: 514k, 2048: 516k on one MI355X)")
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="cfg2")
    ap.add_argument("--lanes", action="store_true", help="also measure the lane-per-trajectory variant (tmpc_set_throughput_mode; loses on every shape, "
                                                        "round 2 -- out of the default run since round 4)")
    ap.add_argument("--no-lanes", action="store_true", help="(accepted for old command lines; the lanes leg is off unless --lanes)")
    ap.add_argument("--no-end-to-end", action="store_true", help="skip the end-to-end leg (value_end_to_end; cfg2 on one GPU)")
    ap.add_argument("--index-check-sets", type=int, default=512,
                    help="sets of the timed launch whose FindBestPlanner index is compared with the oracle's pick after timing (0 = skip)")
    ap.add_argument("--no-tight", action="store_true", help="skip the qp_tol = 1e-9 leg")
    ap.add_argument("--share-of", type=int, default=0,
                    help="one-set workloads on ONE GPU: solve rank 0's share of a split over this many ranks (what one GPU of such a node "
                         "does, without the collective) instead of the whole set")
    ap.add_argument("--gen-workers", type=int, default=0, help="processes that generate the scenes (0 = all usable CPUs; 1 = no fork, e.g. under a profiler)")
    ap.add_argument("--scene-cache", default="", help="npz file to keep the generated batch in (repeated profiler passes)")
    ap.add_argument("--cpu-scenes", type=int, default=16)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-param-sharing", action="store_true",
                    help="do not give the tmpc_set_param_sharing hint (A/B: every trajectory reads its own copy of its set's parameter rows)")
    ap.add_argument("--latency-reps", type=int, default=100)
    ap.add_argument("--latency-mode", type=int, default=0, choices=[0, 1, 2, 3],
                    help="kernel variant of the timed launch (tmpc_set_latency_mode): 0 throughput kernels (default, what `value` of cfg 2 is quoted on), "
                         "1 two waves per trajectory, 2 parallel-in-time Newton solve, 3 four waves per trajectory (N <= 20) -- for the small one-set workloads "
                         "(cfg 4 share, cfg 5), which are one dependent chain deep")
    ap.add_argument("--parity-check", type=int, default=256,
                    help="trajectories of the timed launch re-solved by the CPU oracle after timing (0 = skip)")
    ap.add_argument("--launcher-selftest", action="store_true", help="exercise the N > 1 launch path on CPU (gloo) and exit; no GPU needed")
    ap.add_argument("--full", action="store_true",
                    help="besides the timed steps: CPU baseline, parity and FindBestPlanner checks against the oracle, the tight-tolerance, end-to-end "
                         "and control-tick latency legs (the --no-* / --lanes / --*-check options choose among them); a plain run only times the steps")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what the last one computed (trajectories, objectives, exit codes, iteration counts, best index per "
                         "set) as DIR/<name>.npy in float64, at most 64 MB in all (a fixed, seeded sample of the trajectories beyond that); rank 0's share at N > 1")
    a = ap.parse_args()

    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        # the plain command at N > 1 (how the driver starts N = 1): become the torch.distributed.run job, one rank per GPU
        raise SystemExit(self_launch(a.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus != world:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}: the launcher's --nproc-per-node and --gpus must agree")
    if a.launcher_selftest:
        return launcher_selftest(a, world, rank)
    wl = WORKLOADS[a.workload]
    TRAJ_SET = wl["traj"]                                 # trajectories of one guidance / scenario set (one FindBestPlanner domain)
    gen_workers = a.gen_workers or max(1, usable_cpus() // world)      # the ranks of one node generate their scenes side by side: share the host cores

    # ---- synthetic inputs, generated before the GPU runtime is touched (forked workers) -------------------------
    from mpc_planner_amd import scenes
    if wl.get("one_set") and a.sets > 1:
        # NOT the BASELINE configuration (which names one set): `--sets K` independent sets of the same shape in one launch, to show the kernels
        # of the shape on a saturated GPU (cfg 3: the two-wave compact kernel, four trajectories per CU, takes launches of more than 512)
        batch = scenes.make_batch(range(7, 7 + a.sets), workers=gen_workers, B=TRAJ_SET, **wl["scene"])
        n_sets, traj_local = a.sets, TRAJ_SET
    elif wl.get("one_set"):
        # one set split over the ranks: every rank builds the same scene and keeps its contiguous share
        per_rank = TRAJ_SET // (a.share_of if (a.share_of > 0 and world == 1) else world)
        full = scenes.make_scene(7, B=TRAJ_SET, **wl["scene"])
        sl = slice(rank * per_rank, (rank + 1) * per_rank)
        batch = {k: full[k][sl] for k in ("xinit", "x0", "params", "guidance_id")}
        n_sets, traj_local = 1, per_rank
    else:
        # weak scaling: rank r owns trajectories [64 r, 64 (r+1)) of every scene's guidance set -> different seeds per rank
        first_scene = 100000 * rank
        cache = f"{a.scene_cache}.{a.workload}.{a.scenes}.{rank}.npz" if a.scene_cache else ""
        if cache and os.path.exists(cache):
            batch = dict(np.load(cache))
        else:
            batch = scenes.make_batch(range(first_scene, first_scene + a.scenes), workers=gen_workers, B=TRAJ_SET, **wl["scene"])
            if cache:
                np.savez(cache, **{k: batch[k] for k in ("xinit", "x0", "params", "guidance_id", "guidance_pos", "guidance_vel", "obstacle_pos") if k in batch})
        n_sets, traj_local = a.scenes, TRAJ_SET
    B = batch["xinit"].shape[0]
    batch_in = None
    if a.full and a.workload == "cfg2" and not a.no_end_to_end and world == 1 and "RANK" not in os.environ and a.scenes >= 32 and not a.latency_mode:
        # scenes on which projectToSafety acts, for the end-to-end leg (generated before the GPU runtime is touched: forked workers)
        batch_in = scenes.make_batch(range(900000, 900016), workers=gen_workers, B=TRAJ_SET, inside_share=0.1, **wl["scene"])

    import torch
    import torch.distributed as dist
    from mpc_planner_amd import solver, distributed as D

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the product path has no CPU fallback")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    use_dist = world > 1 or "RANK" in os.environ           # under torch.distributed.run the collective path runs even for N=1
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    # Host-side waits (rank 0's CPU baseline before the timed region, its oracle legs after it) go through a gloo group with a long timeout:
    # the other ranks block on sockets there, nothing is left pending on the GPUs and nothing depends on RCCL's watchdog.
    import datetime
    host_pg = dist.new_group(backend="gloo", timeout=datetime.timedelta(minutes=60)) if use_dist else None

    def host_barrier():
        if use_dist:
            dist.barrier(group=host_pg)

    # ---- reported CPU baseline (rank 0, at every N): before the timed region, while the other ranks wait and the host cores are free -------
    cpu_base = None
    if a.full and not a.no_cpu_baseline:
        host_barrier()                                      # every rank's scene generation is done
        if rank == 0:
            cpu_base = cpu_baseline(a.cpu_scenes)
        host_barrier()

    t_xinit = torch.from_numpy(batch["xinit"]).to(dev)
    t_x0 = torch.from_numpy(batch["x0"].reshape(B, -1)).to(dev)
    t_params = torch.from_numpy(batch["params"].reshape(B, -1)).to(dev)
    t_gid = torch.from_numpy(batch["guidance_id"].astype(np.int32) + traj_local * rank).to(dev)
    t_rec = torch.zeros((B, 2), dtype=torch.int64, device=dev)              # 16-byte tmpc_record each
    t_best = torch.full((n_sets,), -2, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    dims = solver.default_dims(**wl["dims"])
    sv = solver.BatchedSolver(dims, B_max=B, device=local_rank)
    sv.set_batch_device(B, t_xinit.data_ptr(), t_x0.data_ptr(), t_params.data_ptr())
    sv.enable_timing(a.steps + a.warmup + 4)
    kernel_info = sv.kernel_info()                        # which solve kernel the handle dispatches (fast / compact / ...), from the library
    lat_mode_ok = sv.set_latency_mode(a.latency_mode) if a.latency_mode else None
    # A guidance set's planners carry copies of the main solver's parameters and differ in their own halfspace rows only
    # (guidance_constraints.cpp:300-318): tell the library which entries are such copies (checked on the host, entry by entry)
    share_map = None
    if not a.no_param_sharing:
        share_map = solver.param_sharing_map(batch["params"], dims, traj_local)
        sv.set_param_sharing(share_map)

    # SH-MPC (cfg 5): the scenario pipeline runs inside the timed step -- every scenario solver draws its own 8 x 256 scenarios from the
    # obstacles' Gaussian-mixture predictions (new seed every step), builds its <= 24 halfspaces per stage around its warm start and, after
    # the solve, counts the support of its solution; all on the handle's stream, no host synchronisation
    scn = None
    if wl.get("scenario"):
        sk = wl["scenario"]
        Mo, Sc, Rr = sk["n_obstacles"], sk["n_scenarios"], sk["n_rows"]
        pred = np.repeat(scenes.mixture_prediction(full["obstacles"]["pos"], 0)[None], B, 0)          # [P][M][3][N][6]: every solver sees the same prediction
        prob = np.tile(scenes.MIXTURE_WEIGHTS, (B, Mo, 1))
        scn = dict(pred=torch.from_numpy(pred).to(dev), prob=torch.from_numpy(prob).to(dev), Mo=Mo, Sc=Sc, Rr=Rr,
                   samples=torch.empty((B, dims.N, Mo * Sc, 2), dtype=torch.float64, device=dev),
                   scene_of=torch.arange(B, dtype=torch.int32, device=dev), state_x=torch.from_numpy(np.ascontiguousarray(batch["xinit"][:, 0])).to(dev),
                   support=torch.zeros((2, B), dtype=torch.int32, device=dev), radius=scenes.OBSTACLE_RADIUS + scenes.ROBOT_RADIUS, n=0)
        torch.cuda.synchronize()

    # The whole step is stream-ordered on the handle's stream: solve -> pack -> (N > 1: the all-gather, issued with that stream as
    # torch's current stream, so RCCL waits for the records and the selection waits for RCCL) -> FindBestPlanner.  No host
    # synchronisation inside a step.
    ext_stream = torch.cuda.ExternalStream(sv.stream_ptr(), device=dev) if use_dist else None

    def step():
        if scn is not None:
            scn["n"] += 1
            sv.sample_scenarios(scn["pred"].data_ptr(), scn["prob"].data_ptr(), B, scn["Mo"], 3, scn["Sc"], 1000 + 131 * rank + scn["n"], scn["samples"].data_ptr())
            sv.scenario_halfspaces(scn["samples"].data_ptr(), scn["Mo"] * scn["Sc"], scn["Rr"], scn["scene_of"].data_ptr(), scn["state_x"].data_ptr(), scn["radius"])
        sv.solve(sync=False)                                                # the dominant kernel
        if scn is not None:
            sv.scenario_support_async(scn["Sc"], 1e-6, scn["support"][0].data_ptr(), scn["support"][1].data_ptr())
        sv.pack_records(t_rec.data_ptr(), t_gid.data_ptr())
        if use_dist:
            with torch.cuda.stream(ext_stream):
                gathered = D.all_gather_records(t_rec, world)               # ONE RCCL all-gather, 16 B x B per rank
            sv.select_best_records(gathered.data_ptr(), world, n_sets, traj_local, t_best.data_ptr())
            step.keep = gathered
        else:
            sv.select_best_records(t_rec.data_ptr(), 1, n_sets, traj_local, t_best.data_ptr())

    for _ in range(a.warmup):
        step()
    sv.synchronize()
    sv.get_timings()                                                        # drop warm-up timings
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    sv.synchronize()
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if use_dist:
        te = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(te, op=dist.ReduceOp.MAX)
        elapsed = float(te.item())
    kernel_ms = sv.get_timings()                                            # HIP events on the launch stream

    res = sv.get()
    best = t_best.cpu().numpy()
    ok = res["exit_code"] == 1
    full_iter = res["sqp_iter"] == dims.n_sqp
    dumped = None
    if a.dump_outputs and rank == 0:
        # what the last timed step hands its caller: every trajectory's solution and status, the best index per set (and, cfg 5, the support counts)
        arrays = dict(res, best_index=best)
        if scn is not None:
            arrays["scenario_support"] = scn["support"].cpu().numpy().T
        dumped = {"dir": os.path.abspath(a.dump_outputs), "arrays": write_outputs(a.dump_outputs, arrays, B)}
    scenario_info = None
    if scn is not None:
        # the rows the last step built on device are what its solve saw: the parity block below re-solves exactly those
        batch = dict(batch, params=sv.debug_get_params())
        sup = scn["support"].cpu().numpy()
        scenario_info = {"pipeline_in_timed_step": ["tmpc_sample_scenarios", "tmpc_scenario_halfspaces", "tmpc_solve", "tmpc_scenario_support", "tmpc_pack_records", "tmpc_select_best_records"],
                         "scenarios_per_solver_per_stage": scn["Mo"] * scn["Sc"], "rows_per_stage": scn["Rr"], "support_mean": float(sup[0][ok].mean()) if ok.any() else None,
                         "support_max": int(sup[0][ok].max()) if ok.any() else None, "empty_polygon_stages": int(sv.scenario_empty_stages().sum()),
                         "new_scenarios_every_step": True}

    # ---- parity spot check of THIS launch against the CPU oracle (outside the timed region; rank 0) ---------------------
    parity = None
    if rank == 0 and a.full and a.parity_check > 0:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import oracle_lib as O
        parity = parity_block(O, wl, batch, res, a.parity_check, {})
        if a.index_check_sets > 0 and not use_dist:
            parity["best_index"] = best_index_block(O, wl, batch, res, best, traj_local, a.index_check_sets)
    if use_dist and a.full and a.index_check_sets > 0:
        # N > 1 (and N = 1 under the launcher): the selection ran on the GATHERED records -- check it there.  Every rank hands rank 0 the inputs of
        # its first sets over the host group; rank 0 re-solves them with the oracle and applies the reference's rule to the gathered records.
        n_chk = min(n_sets, 16)
        blk = gathered_index_inputs(dist, host_pg, batch, n_chk * traj_local, rank, world)
        if rank == 0:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import oracle_lib as O
            rec_host = step.keep.cpu().numpy().reshape(-1).view(D.RECORD_DTYPE).reshape(world, n_sets, traj_local)
            bi = best_index_block_gathered(O, wl, blk, rec_host, best, world, traj_local, n_chk)
            if parity is None:
                parity = {}
            parity["best_index"] = bi
    n_sqp_mean = float(res["sqp_iter"].mean())
    ipm_per_qp = float(res["qp_iter_total"].sum() / max(res["sqp_iter"].sum(), 1))

    # ---- the same launch at a tight QP tolerance: the RTI iterate no longer depends on how the QP solver reaches its tolerance ------
    # (tests/test_independent_rti.py).  1e-8 since round 6: at 1e-9 a float64 interior-point method is below the noise floor of its own stationarity
    # residual on these QPs and two correct implementations disagree on integers in ~0.6 % of the solves, in either Riccati form
    # (profiles/round6_tight_tolerance_study.json names trajectory, iteration, stopping test and both sides' residuals); the 1e-9 numbers stay beside it
    tight = None
    if rank == 0 and a.full and not a.no_tight and not use_dist:
        def tight_leg(tol):
            dims_t = solver.default_dims(**wl["dims"], qp_tol=tol)
            st = solver.BatchedSolver(dims_t, B_max=B, device=local_rank)
            st.set_batch_device(B, t_xinit.data_ptr(), t_x0.data_ptr(), t_params.data_ptr())
            st.solve(); ms_t = st.time_solve(3); rt = st.get(); st.close()
            okt = rt["exit_code"] == 1
            blk = {"qp_tol": tol, "kernel_ms": float(np.median(ms_t)), "success_fraction": float(okt.mean()),
                   "value": float(B * okt.mean() / (np.median(ms_t) * 1e-3)), "unit": "successful solves/s (kernel time, same resident batch)",
                   "mean_ipm_iter_per_qp": float(rt["qp_iter_total"].sum() / max(rt["sqp_iter"].sum(), 1))}
            if a.parity_check > 0:
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                import oracle_lib as O
                # like for like: the oracle runs the kernels' Riccati form (its option riccati_form 1: the elimination stops after the input block)
                blk["parity"] = parity_block(O, wl, batch, rt, min(a.parity_check, 128), {"qp_tol": tol, "riccati_form": 1})
                blk["parity"]["against"] += " (oracle option riccati_form = 1: the same recursion form as the kernels)"
            return blk
        tight = tight_leg(1e-8)
        tight["why_1e_8"] = "the tightest tolerance above the float64 noise floor of the interior-point method on these QPs: profiles/round6_tight_tolerance_study.json"
        tight["beyond_the_noise_floor_1e_9"] = tight_leg(1e-9)
        tight["beyond_the_noise_floor_1e_9"]["note"] = ("integer disagreements here are the stopping test deciding on rounding noise (res_g ~ 1e-9 from terms of magnitude 1e6 .. 1e7), "
                                                        "at the same rate in both Riccati forms; both sides also break down on ~0.5 % of the solves: see the study")

    # ---- end to end: per-tick inputs uploaded every step, x0 / halfspace rows built on device, winners copied back ----------
    e2e = None
    if rank == 0 and a.full and not use_dist and a.workload == "cfg2" and not a.no_end_to_end and "guidance_pos" in batch and share_map is not None and not a.latency_mode:
        sv.get_timings()
        sv.set_param_sharing(share_map, copies_not_maintained=True)      # this leg writes a set's shared rows into the base entry only: say so (strict mode)
        e2e = end_to_end_leg(a, dims, sv, batch, t_xinit, t_x0, t_params, dev, n_sets, traj_local, res, best, batch_in)

    # ---- p50 latency of one control tick (64 trajectories, host call -> best index on host) --------------
    lat = None
    lat5 = None
    lat5_n30 = None
    lanes = None
    if rank == 0 and a.full and a.lanes and not use_dist and not dims.cost_model and not dims.row_model and solver.has_lane_kernels():
        # the lane-per-trajectory variant (tmpc_set_throughput_mode) on the same resident batch: the measured alternative design
        sv.set_throughput_mode(True)
        sv.solve(); sv.solve(sync=False)
        ms_l = sv.time_solve(3)
        rl = sv.get()
        sv.set_throughput_mode(False)
        okl = (rl["exit_code"] == 1) & ok
        lanes = {"kernel": "lanes_solve_kernel (one lane per trajectory, state streamed from a lane-major HBM workspace)",
                 "kernel_ms": float(np.median(ms_l)), "solves_per_s": float(B / (np.median(ms_l) * 1e-3)),
                 "exit_code_mismatch_vs_default": int((rl["exit_code"] != res["exit_code"]).sum()),
                 "ipm_iter_mismatch_vs_default": int((rl["qp_iter_total"][okl] != res["qp_iter_total"][okl]).sum()),
                 "max_abs_traj_diff_vs_default": float(np.abs(rl["xtraj"][okl] - res["xtraj"][okl]).max()) if okl.any() else None}
    if rank == 0 and a.full and a.latency_reps > 0 and a.workload == "cfg2":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import oracle_lib as O
        VARIANT = {1: "latency 1 (two waves per trajectory, sequential Riccati recursion)",
                   2: "latency 2 (two waves per trajectory, parallel-in-time Newton solve: Schur complement + block cyclic reduction)",
                   3: "latency 3 (FOUR waves per trajectory: stage evaluation split four ways, row passes at twelve lanes per stage, the wide phases of the "
                      "parallel-in-time factorisation on all four waves)"}

        def tick_block(nb, label, dims=dims, batch=batch, wl=wl):
            """One control tick of `nb` planners, host call -> best index on host, in every kernel variant the library offers for it."""
            one = solver.BatchedSolver(dims, B_max=nb, device=local_rank)
            hx, h0, hp = batch["xinit"][:nb], batch["x0"][:nb], batch["params"][:nb]
            out_modes, res_modes, best_modes = {}, {}, {}
            for mode in (1, 2, 3):
                if not one.set_latency_mode(mode):
                    continue
                ts = []
                for i in range(a.latency_reps + 10):
                    t1 = time.perf_counter()
                    one.set_batch(hx, h0, hp); one.solve(sync=False); b_ = one.select_best()
                    ts.append(time.perf_counter() - t1)
                ts = np.array(ts[10:]) * 1e3
                one.get_timings(); one.enable_timing(32)
                for _ in range(20):
                    one.solve(sync=False)
                k_ms = one.get_timings()
                r_ = one.get()
                res_modes[mode], best_modes[mode] = r_, b_
                out_modes[mode] = {"p50_ms": float(np.percentile(ts, 50)), "p90_ms": float(np.percentile(ts, 90)), "kernel_ms": float(np.median(k_ms)),
                                   "solves_per_s": float(nb / (np.percentile(ts, 50) * 1e-3)), "kernel_variant": VARIANT[mode]}
                if a.parity_check > 0:
                    out_modes[mode]["parity"] = parity_block(O, wl, {"xinit": hx, "x0": h0, "params": hp}, r_, min(a.parity_check, nb), {})
            one.close()
            if not out_modes:
                return None
            fastest = min(out_modes, key=lambda m: out_modes[m]["p50_ms"])
            blk = {"planners": nb, "what": label, "includes": "H2D of params/warm start, solve kernel, FindBestPlanner, D2H of the index",
                   **{k: out_modes[fastest][k] for k in ("p50_ms", "p90_ms", "kernel_ms", "solves_per_s", "kernel_variant")},
                   "fastest_mode": fastest, "by_mode": {f"mode_{m}": v for m, v in out_modes.items()},
                   "best_index_equal_across_modes": bool(len(set(best_modes.values())) == 1)}
            if 1 in res_modes:
                r1 = res_modes[1]
                blk["vs_mode_1"] = {}
                for m, r2 in res_modes.items():
                    if m == 1:
                        continue
                    both = (r1["exit_code"] == 1) & (r2["exit_code"] == 1)
                    blk["vs_mode_1"][f"mode_{m}"] = {"exit_code_mismatch": int((r1["exit_code"] != r2["exit_code"]).sum()),
                                                     "ipm_iter_mismatch": int((r1["qp_iter_total"] != r2["qp_iter_total"]).sum()),
                                                     "max_abs_xtraj_diff": float(np.abs(r1["xtraj"][both] - r2["xtraj"][both]).max()) if both.any() else None}
            return blk

        lat = tick_block(TRAJ, "configs[1] as named: one 64-trajectory guidance set per tick")
        if lat is not None:
            lat["kernel_ms_b64"] = lat["kernel_ms"]; lat["solves_per_s_b64"] = lat["solves_per_s"]          # (the key names of rounds 1-5)
        # the reference's DEPLOYED size: 4 guidance planners + the non-guided T-MPC++ planner (mpc_planner_jackalsimulator/config/guidance_planner.yaml:11,
        # guidance_constraints.cpp:40-52): the first five trajectories of the same set
        lat5 = tick_block(5, "the reference's deployed size: n_paths = 4 guidance planners + the non-guided planner (guidance_planner.yaml:11)")
        # ... and at the horizon the reference SHIPS for this stack (mpc_planner_jackalsimulator/config/settings.yaml N: 30; BASELINE's configs[1] says N = 20):
        # the same module stack, N = 30, 4 guidance planners + the non-guided one
        from mpc_planner_amd import scenes
        wl30 = dict(dims=dict(N=30, S=5, n_lin=8, M=8), scene=dict(N=30, M=8, tmpc_pp=True))
        sc30 = scenes.make_scene(11, B=4, **wl30["scene"])
        lat5_n30 = tick_block(5, "the reference's deployed size AND shipped horizon: 4 + 1 planners, N = 30 (settings.yaml; module stack and obstacle count of configs[1]: 8 + 8 rows; settings.yaml's max_obstacles 12 -> tools/tick_shapes.py)",
                              dims=solver.default_dims(**wl30["dims"]), batch=sc30, wl=wl30)

    if rank == 0:
        solves = B * world * a.steps
        attempted = solves / elapsed
        value = attempted * float(ok.mean())               # successful solves only (rank 0's success fraction; same workload on every rank)
        k_avg = float(np.mean(kernel_ms)) * 1e-3
        fl = flops_per_solve(n_sqp_mean, ipm_per_qp, N=dims.N, nh=wl["nh"])
        by = bytes_per_solve(N=dims.N, npar=wl["npar"], nv=dims.nvar, nx=dims.nx)
        tflops = B * fl / k_avg / 1e12
        gbs = B * by / k_avg / 1e9
        # HBM traffic comes from rocprofv3 PMC passes (tools/collect_profiles.py), which cannot run inside this process: it is
        # reported only if the committed counters were collected on THIS build of the library and this launch size
        traffic, traffic_note, lib_hash = None, None, library_sha256()
        import glob
        if a.workload == "cfg2":
            seen = []
            for pmc in sorted(glob.glob(os.path.join(ROOT, "profiles", "round*_pmc.json")), reverse=True):
                try:
                    pj = json.load(open(pmc))
                except Exception:
                    continue
                if pj.get("library_sha256") == lib_hash and pj.get("trajectories_per_launch") == B \
                        and ("--no-param-sharing" in pj.get("extra_bench_args", [])) == a.no_param_sharing:
                    traffic = pj.get("hbm_bytes_per_launch")
                    traffic_note = f"rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this build ({lib_hash[:12]}), profiles/{os.path.basename(pmc)}"
                    break
                seen.append(f"{os.path.basename(pmc)}: build {str(pj.get('library_sha256'))[:12]} / {pj.get('trajectories_per_launch')} per launch")
            if traffic is None:
                traffic_note = f"no committed PMC passes for this build ({lib_hash[:12]}) at {B} trajectories per launch; found " + "; ".join(seen[:3])
        out = {
            "metric": "MPC solves/s (Jackal N=20, 8 obs)" if a.workload == "cfg2" else f"MPC solves/s ({a.workload})", "value": value, "unit": "solves/s",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": elapsed / a.steps * 1e3,
            "higher_is_better": True, "scaling": "strong" if wl.get("one_set") else "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"{wl['what']}; {n_sets} set(s) x {traj_local} = {B} trajectories per launch per GPU, n_sqp=10, qp_tol=1e-5"
                                   + (f" (rank 0's share of a {a.share_of}-rank split, solved on one GPU without the collective)" if a.share_of > 0 and world == 1 else "")
                                   + (f" (--sets {a.sets}: NOT the BASELINE configuration, which names ONE set; the shape on a saturated GPU)" if wl.get("one_set") and a.sets > 1 else ""),
                       "trajectories_per_launch_per_gpu": B, "scenes_per_launch": n_sets,
                       "success_fraction": float(ok.mean()), "mean_sqp_iter": n_sqp_mean, "mean_ipm_iter_per_qp": ipm_per_qp,
                       "value_counts": "successful solves (exit_code == 1) only",
                       "param_sharing": {"hint": share_map is not None, "entries_reading_a_shared_row": int((share_map != np.arange(B)).sum()) if share_map is not None else 0,
                                         "what": "tmpc_set_param_sharing: a set's copies of the obstacle / spline / weight rows are read from the set's first entry (checked equal on the host); results bitwise unchanged"},
                       "kernel_variant": {"latency_mode": a.latency_mode, "accepted": lat_mode_ok,
                                          "what": ["throughput kernels", "two waves per trajectory", "parallel-in-time Newton solve (csrc/tmpc_scan.hpp)",
                                                   "four waves per trajectory (parallel-in-time solve, split stage evaluation, twelve lanes per stage)"][a.latency_mode]},
                       "parallelism": f"trajectory-sharded x{world}, one 16 B/trajectory all-gather" if world > 1 else "single GPU"},
            "roofline": {"bound": "fp64_valu", "bound_detail": "FP64 vector (VALU) peak; the kernel issues no MFMA instruction (the dense f64 MFMA peak is the same 78.6 TFLOP/s on MI355X, so the schema's 'mfma' label would give the same number)", "achieved": tflops, "peak": FP64_VALU_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": tflops / FP64_VALU_PEAK_TFLOPS, "traffic": traffic, "traffic_source": traffic_note,
                         "library_sha256": lib_hash,
                         "kernel": kernel_info, "kernel_ms_avg": k_avg * 1e3, "flops_per_solve": fl,
                         "note": "compute roofline for dtype f64: on MI355X the dense f64 MFMA peak equals the f64 vector (VALU) "
                                 "peak, 78.6 TFLOP/s (AMD spec); the kernel issues FP64 VALU (7x7 stage blocks, SURVEY 8d), so "
                                 "this is the binding roofline; achieved = algorithmic flops (SURVEY 8d model x measured "
                                 "iteration counts) / HIP-event kernel time; HBM term alongside",
                         "hbm": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                 "frac": gbs / HBM_PEAK_GBS, "bytes_per_solve": by}},
            "success_solves_per_s": value, "attempted_solves_per_s": attempted,
            "value_all_10_iter": attempted * float(full_iter.mean()),
            "parity": parity,
            "value_end_to_end": e2e["value_end_to_end"] if e2e else None,
            "end_to_end": e2e,
            "value_qp_tol_1e_8": tight["value"] if tight else None,
            "qp_tol_1e_8": tight,
            "value_qp_tol_1e_9": tight["beyond_the_noise_floor_1e_9"]["value"] if tight else None,
            "lanes_variant": lanes,
            "latency_b64": lat,
            "latency_b5": lat5,
            "latency_b5_n30": lat5_n30,
            "best_index_sample": best[:4].tolist(),
            "scenario_pipeline": scenario_info,
            "full": bool(a.full),
            "dumped_outputs": dumped,
        }
        if cpu_base is not None:                                      # reported baseline: rank 0's host cores, measured before the timed region (at every N)
            out["cpu_baseline"] = cpu_base
        missing = [k for k in REQUIRED_KEYS if k not in out and not (k == "cpu_baseline" and cpu_base is None)]
        assert not missing, missing
        print(json.dumps(out))
    sv.close()
    host_barrier()                                          # ranks != 0 wait HERE (gloo, on sockets) while rank 0 runs its oracle / latency legs
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
