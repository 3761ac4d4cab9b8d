"""C++ episode step (mpc_planner/episode.h: MPCPlanner::episodeStep) against the numpy mirror (mpc_planner_amd/modules.py episode_step) on the
script of the GPU equality test (tests/episode_cases.py): every array after every tick, bit for bit (%.17g round-trips a double; a NaN equals
a NaN in the same place).  The Solver-free header alone, host code only: nothing touches a GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import episode_cases as ec  # noqa: E402

CPP = os.path.join(ROOT, "mpc_planner_amd", "cpp")
SRC = os.path.join(ROOT, "tests", "cpp", "test_episode.cpp")
BIN = os.path.join(ROOT, "build", "test_episode")
NAMES = ec.IN_OUT + ec.OUTPUTS


def _build():
    """The program, unless it is there and newer than everything it is made of."""
    deps = [SRC, os.path.join(CPP, "include", "mpc_planner", "episode.h"), os.path.join(CPP, "include", "mpc_planner_types", "prep_arithmetic.h")]
    if os.path.exists(BIN) and all(os.path.getmtime(d) <= os.path.getmtime(BIN) for d in deps):
        return
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(CPP, "include"), SRC, "-o", BIN])


def case_file(path, case, opt, n_slots=ec.N_SLOTS):
    ticks = len(case["commands"])
    vals = [len(case["plant0"]), n_slots, ec.P, case["nx"], ticks, opt["substeps"], opt["timeout_ticks"], opt["max_episodes"], opt["control_dt"],
            opt["max_acceleration"], opt["max_angular_velocity"], opt["robot_radius"], opt["goal_x"], int(case["box"] is not None), int(case["goal"] is not None)]
    arrays = [case["plant0"], case["count"], case["raw_pos0"], case["raw_vel0"], case["raw_radius"]] + \
             [case[k] for k in ("box", "goal") if case[k] is not None] + [case["commands"]]
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


def _same(a, b):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


@pytest.mark.parametrize("config", ec.CONFIGS)
def test_header_equals_the_mirror_bitwise(tmp_path, config):
    """6 scenes, 70 slots, counts (0, 1, 3, 64, 70, 70), 40 ticks; substeps 1 and 4, box given and absent, acceleration limit on and off.  The
    script's events (completions of both kinds, timeouts, the NaN scene, collisions, reflections, the log overflow, a clipped w) are asserted
    in tests/test_episode_mirror.py."""
    _build()
    substeps, boxed, acc = config
    case, opt = ec.make_case(7, boxed), ec.options(substeps, acc)
    history, _ = ec.run_mirror(case, opt)
    f = str(tmp_path / "case.bin")
    case_file(f, case, opt)
    out = subprocess.run([BIN, f], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = parse(out.stdout)
    assert len(got) == len(history) == ec.TICKS
    for tick, (g, want) in enumerate(zip(got, history)):
        for k in NAMES:
            assert _same(g[k], want[k]), (tick, k)


def test_the_header_refuses_what_the_entry_point_refuses(tmp_path):
    _build()
    case = ec.make_case(7, True, ticks=1)
    for change in (dict(substeps=0), dict(substeps=17), dict(control_dt=0.0), dict(control_dt=float("inf")), dict(max_angular_velocity=0.0),
                   dict(max_angular_velocity=2.6), dict(max_episodes=4097), dict(timeout_ticks=-1), dict(robot_radius=-0.1)):
        f = str(tmp_path / "case.bin")
        case_file(f, case, dict(ec.options(1, 0.0), **change))
        out = subprocess.run([BIN, f], capture_output=True, text=True, timeout=60)
        assert out.returncode == 3 and out.stdout == "refused\n", (change, out.returncode, out.stdout[-200:])
