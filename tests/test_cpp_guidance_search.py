"""C++ guidance search (mpc_planner_modules/guidance_search.h: MPCPlanner::guidanceSearch) against the numpy mirror
(mpc_planner_amd/modules.py guidance_search) on the scenes of tests/guidance_search_cases.py: every output and every carried array after every
tick, bit for bit (%.17g round-trips a double).  And the stand-alone program under -fsanitize=address,undefined.  The Solver-free header
alone, host code only: nothing touches a GPU, nothing loaded into Python is sanitized."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import guidance_search_cases as gc  # noqa: E402

CPP = os.path.join(ROOT, "mpc_planner_amd", "cpp")
SRC = os.path.join(ROOT, "tests", "cpp", "test_guidance_search.cpp")
BIN = os.path.join(ROOT, "build", "test_guidance_search")
BIN_SAN = os.path.join(ROOT, "build", "test_guidance_search_san")
NAMES = gc.OUTPUTS + gc.CARRIED


def _build(out=BIN, extra=()):
    """The program, unless it is there and newer than everything it is made of."""
    deps = [SRC, os.path.join(CPP, "include", "mpc_planner_modules", "guidance_search.h"),
            os.path.join(CPP, "include", "mpc_planner_types", "prep_arithmetic.h")]
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", *extra, "-I", os.path.join(CPP, "include"), SRC, "-o", out])


def case_file(path, case):
    opt, t0 = case["opt"], case["ticks"][0]
    Q, G, M = len(t0["state4"]), t0["goals"].shape[1], t0["selected"].shape[1]
    vals = [Q, G, M, case["N"], len(case["ticks"]), opt["n_paths"], opt["n_samples"], opt["n_nodes_max"], opt["max_expansions"], opt["seed"],
            opt["robot_radius"], opt["max_velocity"], opt["margin"], opt["weight_length"], case["dt"]]
    arrays = [t[k] for t in case["ticks"] for k in ("state4", "goals", "obstacle_pos", "obstacle_radius", "selected", "was_reset")]
    np.concatenate([np.array(vals, float)] + [np.asarray(a, float).ravel() for a in arrays]).tofile(path)


def parse(stdout):
    ticks = []
    for line in stdout.splitlines():
        w = line.split()
        if w[0] == "tick":
            ticks.append({})
        else:
            ticks[-1][w[0]] = np.array([float(x) for x in w[1:]])
    return ticks


def run_twin(tmp_path, case, binary=BIN):
    f = str(tmp_path / "case.bin")
    case_file(f, case)
    return subprocess.run([binary, f], capture_output=True, text=True, timeout=120)


CASES = [("one_obstacle_%d" % s, lambda s=s: gc.one_obstacle(s)) for s in range(16)] + \
        [("no_obstacle", gc.no_obstacle), ("identity", gc.identity_run), ("identity_reset", lambda: gc.identity_run(reset_at=3)),
         ("no_samples", lambda: gc.one_obstacle(0, n_samples=0)), ("working", lambda: gc.working_case(seed=1, n_samples=30, Q=4))] + \
        [("flag_%d" % flag, fn) for flag, fn in gc.FLAG_CASES] + \
        [("smallest_%d" % i, lambda i=i: gc.smallest_cases()[i]) for i in range(5)] + [("chain", gc.chain_case), ("limits", gc.limits_case)]


@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
def test_header_equals_the_mirror_bitwise(tmp_path, name, make):
    _build()
    case = make()
    history = gc.run_mirror(case)
    out = run_twin(tmp_path, case)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = parse(out.stdout)
    assert len(got) == len(history) == len(case["ticks"])
    for tick, (g, want) in enumerate(zip(got, history)):
        for k in NAMES:
            assert gc.same(g[k], np.asarray(want[k], float).ravel()), (tick, k)


def test_the_header_refuses_what_the_entry_point_refuses(tmp_path):
    _build()
    for change in (dict(n_paths=0), dict(n_paths=17), dict(n_samples=-1), dict(n_samples=257), dict(n_nodes_max=1), dict(n_nodes_max=65),
                   dict(max_expansions=0), dict(max_expansions=65537), dict(robot_radius=-0.1), dict(max_velocity=0.0),
                   dict(max_velocity=float("inf")), dict(weight_length=0.0), dict(weight_length=float("nan")), dict(margin=-1.0),
                   dict(margin=float("inf"))):
        out = run_twin(tmp_path, gc.one_obstacle(0, **change))
        assert out.returncode == 3 and out.stdout == "refused\n", (change, out.returncode, out.stdout[-200:])


def test_sanitized_program_runs_clean(tmp_path):
    """A stand-alone program with its own main, -fsanitize=address,undefined: no samples, no real obstacle, and full tables (the guard
    table, the connector table, the kept list at n_paths = 16)."""
    _build(BIN_SAN, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    for make in (lambda: gc.one_obstacle(0, n_samples=0), gc.no_obstacle, gc.flag_guards_full, gc.flag_connectors_full, gc.identity_run):
        out = run_twin(tmp_path, make(), BIN_SAN)
        assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-3000:]
