#!/usr/bin/env python3
"""Kernel times of the control-tick kernels of generated solver libraries (latency mode 3; profiles/generated_tick_kernels.json).

    python tools/bench_generated_tick.py [--baseline DIR] [--unsplit DIR] [--out FILE]

Shapes: tmpc_cfg2 at N = 20 and jackal_tmpc at N = 30, 64 trajectories and the deployed 4 + 1 / 5.  Variants: the libraries of build/generated in
modes 0, 2 and 3 (a mode the library does not offer is reported and left out); --baseline: a directory with the same two libraries of another commit,
run in mode 0; --unsplit: a directory with the two libraries built with build_generated_solver(..., _tick_split=0), whose tick kernels evaluate every
stage in one piece on all waves; the product library's hand-written kernels of the same shapes for information.  Instrument: time_solve(30) per run
(HIP events around the launch, warm), five alternating runs per variant in one process; ms per launch."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpc_planner_amd import scenes, solver  # noqa: E402

REPS, RUNS = 30, 5
BASE = "baseline (parent library, default kernel)"


def _jackal(B):
    sc = scenes.make_scene(1, N=30, M=5, S=3, B=max(B, 16), chance=True)
    return {k: sc[k][:B] for k in ("xinit", "x0", "params")}


SHAPES = {
    "tmpc_cfg2 N=20 B=64": ("tmpc_cfg2", dict(N=20), lambda: scenes.make_scene(1, N=20, M=8, B=64), dict(N=20, S=5, n_lin=8, M=8)),
    "tmpc_cfg2 N=20 B=5": ("tmpc_cfg2", dict(N=20), lambda: scenes.make_scene(5, N=20, M=8, B=4, tmpc_pp=True), dict(N=20, S=5, n_lin=8, M=8)),
    "jackal_tmpc N=30 B=5": ("jackal_tmpc", dict(N=30, S=3), lambda: _jackal(5), dict(N=30, S=3, n_lin=5, M=5, row_model=1)),
    "jackal_tmpc N=30 B=64": ("jackal_tmpc", dict(N=30, S=3), lambda: _jackal(64), dict(N=30, S=3, n_lin=5, M=5, row_model=1)),
}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--baseline"); ap.add_argument("--unsplit"); ap.add_argument("--out")
    args = ap.parse_args()
    new = os.path.join(ROOT, "build", "generated")
    out = {"instrument": f"time_solve({REPS}) per run, HIP events, warm; {RUNS} alternating runs per variant; ms per launch (median of the run)", "shapes": {}}
    for label, (name, dkw, mk, prod_kw) in SHAPES.items():
        sc = mk()
        B = sc["xinit"].shape[0]
        handles = {}

        def add(tag, lib, mode, kw):
            s = solver.BatchedSolver(solver.default_dims(lib_path=lib, **kw), B_max=B, lib_path=lib)
            if mode and not s.set_latency_mode(mode):
                print(f"{label}: {tag}: mode not offered")
                s.close()
                return
            s.set_batch(sc["xinit"], sc["x0"], sc["params"]); s.solve()
            handles[tag] = (s, s.get(), s.kernel_info().split("kernels:")[-1].strip())

        if args.baseline:
            add(BASE, os.path.join(args.baseline, f"libtmpc_hip_{name}.so"), 0, dkw)
        for mode in (0, 2, 3):
            add(f"this change, mode {mode}", os.path.join(new, f"libtmpc_hip_{name}.so"), mode, dkw)
        if args.unsplit:
            for mode in (2, 3):
                add(f"unsplit linearisation, mode {mode}", os.path.join(args.unsplit, f"libtmpc_hip_{name}.so"), mode, dkw)
        for mode in (0, 2, 3):
            add(f"product hand-written kernels, mode {mode} (information)", None, mode, prod_kw)
        for s, _, _ in handles.values():
            s.time_solve(REPS)                                   # warm
        runs = {tag: [] for tag in handles}
        for _ in range(RUNS):
            for tag, (s, _, _) in handles.items():
                runs[tag].append(float(np.median(s.time_solve(REPS))))
        rec = {"B": int(B), "runs_ms": runs, "kernels": {t: h[2] for t, h in handles.items()},
               "successes": {t: int((h[1]["exit_code"] == 1).sum()) for t, h in handles.items()}}
        if BASE in handles:
            a, b = handles[BASE][1], handles["this change, mode 0"][1]
            rec["mode0_bitwise_equals_baseline"] = bool(all(np.array_equal(a[k], b[k]) for k in ("xtraj", "utraj", "pobj", "exit_code", "sqp_iter", "qp_iter_total")))
        out["shapes"][label] = rec
        print(label)
        for tag, v in runs.items():
            print(f"   {tag:62s} min {min(v):.4f} med {np.median(v):.4f} max {max(v):.4f}")
        for s, _, _ in handles.values():
            s.close()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
