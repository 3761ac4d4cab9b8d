"""What the two road rows of `contouring/add_road_constraints` (linearized_constraints/add_halfspaces: 2) cost the solve: the cfg-2 shape
(n_lin, M) = (8, 8) against (10, 8) on the same scenes -- saturated launches (kernel time by HIP events, the shapes alternating; the road rows once of a 4 m
road, where they bind and 29 % of the guidance guesses are infeasible, and once of a 50 m road, where they never bind: the shape's cost alone) and the
reference's deployed tick of 4 guided + 1 non-guided planners (p50 of 200 launches, the highest latency mode whose capacity holds the tick).
One JSON line per measurement; tmpc_kernel_info names the kernel that ran."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def _scene(idx):
    from mpc_planner_amd import scenes
    sc = scenes.make_scene(idx, N=20, M=8, B=64)
    return sc["xinit"], sc["x0"], sc["params"], scenes.add_road_constraints(sc, 4.0)["params"], scenes.add_road_constraints(sc, 50.0)["params"]


def main():
    n_scenes = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    import multiprocessing as mp
    with mp.get_context("fork").Pool(min(16, n_scenes)) as pool:          # before anything initialises the GPU runtime in this process
        parts = pool.map(_scene, range(500, 500 + n_scenes))
    import torch
    torch.cuda.init()
    from mpc_planner_amd import scenes, solver
    xinit = np.concatenate([p[0] for p in parts]); x0 = np.concatenate([p[1] for p in parts])
    legs = {"no road rows": (8, np.concatenate([p[2] for p in parts])), "road 4 m": (10, np.concatenate([p[3] for p in parts])),
            "road 50 m (rows never bind)": (10, np.concatenate([p[4] for p in parts]))}
    B = len(xinit)
    sol = {n: solver.BatchedSolver(solver.default_dims(N=20, S=5, n_lin=n, M=8), B_max=B) for n in (8, 10)}
    ms = {leg: [] for leg in legs}
    res = {}
    for rep in range(6):
        for leg, (n, p) in legs.items():
            sol[n].set_batch(xinit, x0, p); sol[n].solve()
            t = sol[n].time_solve(5)
            res[leg] = sol[n].get()
            if rep:                                                       # (the first round warms up)
                ms[leg].append(float(np.median(t)))
    for leg, (n, p) in legs.items():
        r = res[leg]
        print(json.dumps(dict(leg="saturated, " + leg, n_lin=n, M=8, B=B, kernel_ms=float(np.median(ms[leg])), kernel_ms_all=ms[leg],
                              solves_per_s=B / (float(np.median(ms[leg])) * 1e-3), success=float((r["exit_code"] == 1).mean()),
                              ipm_per_qp=float(r["qp_iter_total"].sum() / r["sqp_iter"].sum()), kernel_info=sol[n].kernel_info())), flush=True)
    for n in sol:
        sol[n].close()
    # the deployed tick: 4 guided planners + the non-guided one
    sc = scenes.make_scene(500, N=20, M=8, B=4, tmpc_pp=True)
    rd = scenes.add_road_constraints(sc, 4.0)
    for n, p in ((8, sc["params"]), (10, rd["params"])):
        s = solver.BatchedSolver(solver.default_dims(N=20, S=5, n_lin=n, M=8), B_max=5)
        caps = {m: s.latency_mode_capacity(m) for m in (0, 1, 2, 3)}
        mode = max(m for m in (0, 1, 2, 3) if caps[m] >= 5)
        honoured = s.set_latency_mode(mode) if mode else True
        s.set_batch(sc["xinit"], sc["x0"], p); s.solve(); s.solve()
        t = np.concatenate([s.time_solve(100) for _ in range(2)])
        res = s.get()
        print(json.dumps(dict(leg="tick 4+1", n_lin=n, M=8, B=5, latency_mode=mode, mode_honoured=bool(honoured), capacity=caps,
                              kernel_ms_p50=float(np.median(t)), kernel_ms_p90=float(np.percentile(t, 90)), exit_codes=res["exit_code"].tolist(),
                              kernel_info=s.kernel_info())), flush=True)
        s.close()


if __name__ == "__main__":
    main()
