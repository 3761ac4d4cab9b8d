"""The numpy mirror of the guidance search (mpc_planner_amd/modules.py guidance_search) on properties stated here, without a
GPU: the winding number against the sum of atan2 increments, the one-obstacle scene (two trajectories, one each side, every leg valid by a
check restated here), the scene without a real obstacle, class identity across ticks, and the four capacity flags."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import guidance_search_cases as gc  # noqa: E402
from mpc_planner_amd import modules  # noqa: E402


def _angle_winding(poly):
    """The independent statement: the sum of the signed angle increments of the closed polygon about the origin, in turns, rounded."""
    total = 0.0
    for u, w in zip(poly, np.roll(poly, -1, axis=0)):
        total += math.atan2(u[0] * w[1] - u[1] * w[0], u[0] * w[0] + u[1] * w[1])
    return int(round(total / (2.0 * math.pi)))


def test_winding_number_equals_the_angle_sum():
    """400 random closed polygons of 3 .. 40 vertices that keep at least 0.1 from the origin, half of them built to wind several times."""
    rng = np.random.default_rng(0)
    seen = set()
    for i in range(400):
        n = int(rng.integers(3, 41))
        if i % 2:
            turns = int(rng.integers(-3, 4))
            ang = np.sort(rng.uniform(0.0, 1.0, n)) * 2.0 * math.pi * turns + rng.uniform(0, 6.28)
            rad = rng.uniform(0.1, 3.0, n)
            poly = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
        else:
            poly = rng.uniform(-2.0, 2.0, (n, 2))
            norm = np.hypot(poly[:, 0], poly[:, 1])
            poly = np.where((norm < 0.1)[:, None], poly / np.maximum(norm, 1e-9)[:, None] * 0.1001, poly)
        assert np.all(np.hypot(poly[:, 0], poly[:, 1]) >= 0.1)
        want = _angle_winding(poly)
        assert modules.winding_number(poly) == want, (i, poly)
        seen.add(want)
    assert len(seen) >= 5                                                                   # the polygons do wind: the test is not 0 == 0


def _leg_valid(a, b, obstacle, rr, max_velocity, dt):
    """The validity of a connection, restated: speed, then the clearance at every stage >= 1 of the leg."""
    (ta, xa, ya), (tb, xb, yb) = a, b
    ka, kb = int(round(ta / dt)), int(round(tb / dt))
    if not ka < kb or math.hypot(xb - xa, yb - ya) > max_velocity * (kb - ka) * dt * (1 + 1e-12):
        return False
    for k in range(max(ka, 1), kb + 1):
        f = (k - ka) / (kb - ka)
        ox, oy = obstacle(k)
        if math.hypot(xa + (xb - xa) * f - ox, ya + (yb - ya) * f - oy) < rr * (1 - 1e-12):
            return False
    return True


def _dense(nodes, N, dt):
    """A trajectory's nodes as one point per stage (linear between the nodes)."""
    ks = np.rint(nodes[:, 0] / dt).astype(int)
    return np.stack([np.interp(np.arange(N + 1), ks, nodes[:, 1]), np.interp(np.arange(N + 1), ks, nodes[:, 2])], 1)


@pytest.mark.parametrize("seed", range(16))
def test_one_static_obstacle_gives_one_trajectory_each_side(seed):
    """Radius 0.5 midway between the start and a single goal 6 m apart, N = 20, dt = 0.2, max_velocity 3.  With n_samples = 64 and
    margin = 2 the mirror found both sides for 7 of the 16 seeds only (measured before the scene was fixed): the sampling box is 4 m high, a
    disc of 0.825 fills much of it, and too few samples see both the start and the goal.  Raising n_samples alone does not help (128 and
    256 at margin 3: seeds 6 and 12 keep one side); n_samples = 128 with margin = 6 gives exactly two for all sixteen.  No seed was
    dropped, nothing but n_samples and margin was changed."""
    case = gc.one_obstacle(seed)
    assert case["opt"]["n_samples"] == 128 and case["opt"]["margin"] == 6.0 and case["opt"]["max_velocity"] == 3.0
    assert case["N"] == 20 and case["dt"] == 0.2
    out = gc.run_mirror(case)[-1]
    gc.well_formed(case, out)
    assert out["traj_count"][0] == 2 and out["status"][0] == 0
    N, dt, opt = case["N"], case["dt"], case["opt"]
    lines = []
    for i in range(2):
        n = int(out["node_count"][i])
        nodes = out["nodes"][i][:n]
        for a, b in zip(nodes[:-1], nodes[1:]):
            assert _leg_valid(a, b, lambda k: (3.0, 0.0), 0.5 + opt["robot_radius"], opt["max_velocity"], dt)
        lines.append(_dense(nodes, N, dt))
    poly = np.concatenate([lines[0], lines[1][::-1]]) - np.array([3.0, 0.0])
    assert abs(_angle_winding(poly)) == 1
    assert np.array_equal(out["prev_traj"][0][0], lines[0]) or np.allclose(out["prev_traj"][0][0], lines[0], rtol=0, atol=1e-12)
    assert out["topology_class"][0][:2].tolist() == [0, 1] and out["next_class"][0] == 2


def test_without_a_real_obstacle_one_direct_trajectory_to_the_cheapest_reachable_goal():
    case = gc.no_obstacle()
    out = gc.run_mirror(case)[-1]
    gc.well_formed(case, out)
    assert out["traj_count"][0] == 1 and out["node_count"][0] == 2 and out["status"][0] == 0
    # the goal of cost -5 is 40 m away, out of reach in N dt = 4 s at 3 m/s; of the two others the third is the cheaper
    assert np.array_equal(out["nodes"][0][:2], np.array([[0.0, 0.0, 0.0], [20 * 0.2, 5.0, -1.0]]))
    assert np.all(out["nodes"][0][2:] == gc.NODE_SENTINEL)


def test_class_identity_across_ticks():
    """Six ticks of the one-obstacle scene, the start advancing along the cheapest trajectory, the obstacle at a constant velocity: both classes
    keep their ids while both are found, whichever is the cheaper; then the obstacle has been passed, the two merge into the id of the lower
    previous index and no id is reused."""
    case = gc.identity_run()
    hist = gc.run_mirror(case)
    side = []
    for t, out in enumerate(hist[:6]):
        assert out["traj_count"][0] == 2 and sorted(out["topology_class"][0][:2].tolist()) == [0, 1] and out["next_class"][0] == 2
        first = out["nodes"][0][:out["node_count"][0]]
        ob = case["ticks"][t]["obstacle_pos"][0, 0, 0]
        above = bool(np.interp(ob[0], first[:, 1], first[:, 2]) > ob[1])
        side.append(above == (out["topology_class"][0][0] == hist[0]["topology_class"][0][0]))
    assert len(set(side)) == 1                                                              # an id stays on its side of the obstacle
    assert len({tuple(out["topology_class"][0][:2].tolist()) for out in hist[:6]}) == 2     # and the cost order did change along the way
    last, before = hist[6], hist[5]
    assert last["traj_count"][0] == 1 and last["node_count"][0] == 2
    assert last["topology_class"][0][0] == before["topology_class"][0][0] and last["next_class"][0] == 2
    assert last["prev_class"][0].tolist() == [int(before["topology_class"][0][0]), -1, -1, -1]


def test_a_reset_restarts_the_ids():
    case = gc.identity_run(reset_at=3)
    hist = gc.run_mirror(case)
    plain = gc.run_mirror(gc.identity_run())
    # the ids before the reset are those of the plain run; at the reset the cheapest trajectory is class 0 again whatever it was
    for t in range(3):
        assert np.array_equal(hist[t]["topology_class"], plain[t]["topology_class"])
    assert hist[3]["topology_class"][0][:2].tolist() == [0, 1] and hist[3]["next_class"][0] == 2
    assert plain[3]["topology_class"][0][:2].tolist() == [1, 0]
    for k in ("nodes", "node_count", "traj_count", "prev_traj"):
        assert gc.same(hist[3][k], plain[3][k])


@pytest.mark.parametrize("flag,make", gc.FLAG_CASES, ids=["guards", "connectors", "expansions", "nodes"])
def test_capacity_flags(flag, make):
    case = make()
    out = gc.run_mirror(case)[-1]
    assert out["status"][0] & flag
    gc.well_formed(case, out)


def test_smallest_shapes_and_the_chain_scene_yield_their_trajectories():
    """Each of the smallest shapes yields the trajectories it was built for -- N = 2 a 3-node trajectory through stage 1, the start inside an
    obstacle trajectories that leave it -- and the chain scene a path through two connectors: the device comparison of these scenes is a
    comparison of nodes, classes and carried trajectories, not of empty results."""
    cases = gc.smallest_cases() + [gc.chain_case()]
    for case in cases:
        out = gc.run_mirror(case)[-1]
        gc.well_formed(case, out)
        want = case["want"]
        assert out["traj_count"][0] == want["count"] and out["node_count"][:want["count"]].tolist() == want["nodes"] and out["status"][0] == 0
    two, inside = cases[0], cases[4]
    assert gc.run_mirror(two)[-1]["nodes"][0][1, 0] == 1 * two["dt"]                          # the middle node is at stage 1
    tick, rr = inside["ticks"][0], 0.2 + inside["opt"]["robot_radius"]
    d0 = np.hypot(*(tick["obstacle_pos"][0, 0, 0] - tick["state4"][0, 0:2]))
    assert d0 < rr                                                                          # the start is inside at stage 0 (prepared step 0)
    out = gc.run_mirror(inside)[-1]
    for i in range(3):
        line = _dense(out["nodes"][i][:out["node_count"][i]], inside["N"], inside["dt"])
        assert np.hypot(*(line[1] - tick["obstacle_pos"][0, 0, 0])) >= rr                   # and every trajectory has left it by stage 1
    assert max(gc.run_mirror(gc.chain_case())[-1]["node_count"]) >= 5
