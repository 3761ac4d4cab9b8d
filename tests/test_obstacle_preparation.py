"""CPU: the numpy mirrors of mpc_planner/src/data_preparation.cpp (mpc_planner_amd/modules.py: define_robot_area, constant_velocity_prediction,
propagate_prediction_uncertainty, remove_distant_obstacles, ensure_obstacle_size, prepare_obstacles) on hand-derived values, and their
composition against what scenes.make_scene builds with its own three lines.  The device kernels (tests/test_gpu_obstacles.py) and the C++
header (tests/test_cpp_data_preparation.py) are held to these mirrors bit for bit."""
import numpy as np

from mpc_planner_amd import modules as md, scenes

DT, N = 0.2, 20


def _cv_set(pos, vel, radius=0.4, probabilistic=False):
    pos = np.asarray(pos, float); vel = np.asarray(vel, float)
    cvs = [md.constant_velocity_prediction(p, v, DT, N, probabilistic, propagate=False) for p, v in zip(pos, vel)]
    return dict(position=pos, pos=np.stack([c["pos"] for c in cvs]), angle=np.zeros((len(pos), N)),
                major=np.stack([c["major"] for c in cvs]), minor=np.stack([c["minor"] for c in cvs]),
                radius=np.full(len(pos), radius), gaussian=np.full(len(pos), probabilistic))


def test_define_robot_area():
    off, r = md.define_robot_area(1.0, 0.5, 3)                # data_preparation.cpp:32-41: back -0.5 + 0.25, front -0.5 + 1 - 0.25, one between
    assert off.tolist() == [-0.25, 0.0, 0.25] and r == 0.25
    off, r = md.define_robot_area(1.0, 0.5, 1)                # (:25-28): one disc at offset 0 with radius width / 2
    assert off.tolist() == [0.0] and r == 0.25


def test_selection_distance_by_hand():
    """state (0, 0, 0, 1), obstacle at (4, 1) with velocity (-0.5, 0), dt = 0.2: prediction step k = (4 - 0.1 k, 1), the robot's point of
    step k is (k, 0) -- `v k` without dt, as the reference has it -- so the key of step k is (k + 1) 0.6 sqrt((4 - 1.1 k)^2 + 1): 2.4739 at
    k = 0, 3.70 at k = 2 (3 x 0.6 x sqrt(1.8^2 + 1)), 2.93 at k = 3, 3.23 at k = 4 and growing: the minimum is step 0's, 0.6 sqrt(17)."""
    obs = _cv_set([[4.0, 1.0], [4.0, -1.0]], [[-0.5, 0.0], [-0.5, 0.0]])
    d = md.obstacle_selection_distance(obs["pos"], (0.0, 0.0, 0.0, 1.0))
    # 0.6 sqrt(17) = 2.47386337537059633...; the double next to it is 2.4738633753705965.  Evaluated in the reference's order the key passes
    # three roundings (the square root, the constant 0.6, the product) and lands one ulp below it: held to two ulps of the real number,
    # and to the bit of the reference's own expression
    assert abs(d[0] - 2.4738633753705965) <= 2.0 * np.spacing(2.4738633753705965)
    assert d[0] == (1.0 * 0.6) * np.sqrt(4.0 * 4.0 + 1.0 * 1.0)
    assert d[1] == d[0]                                       # the mirrored obstacle: IDENTICAL, not merely close
    # a key above the start value 1e5 is never taken (:116)
    far = _cv_set([[4.0e5, 0.0]], [[0.0, 0.0]])
    assert md.obstacle_selection_distance(far["pos"], (0.0, 0.0, 0.0, 1.0))[0] == 1e5


def _mirrored_pairs():
    """Three pairs (x, +1) / (x, -1) with equal keys inside a pair; the pairs in descending raw order of distance."""
    pos = [[6.0, 1.0], [6.0, -1.0], [4.0, 1.0], [4.0, -1.0], [5.0, 1.0], [5.0, -1.0]]
    return _cv_set(pos, [[-0.5, 0.0]] * 6)


def test_ties_keep_the_lower_raw_index():
    obs = _mirrored_pairs()
    state = (0.0, 0.0, 0.0, 1.0)
    d = md.obstacle_selection_distance(obs["pos"], state)
    assert d[0] == d[1] and d[2] == d[3] and d[4] == d[5] and d[2] < d[4] < d[0]
    out, sel = md.ensure_obstacle_size(obs, state, 3, DT)
    assert sel.tolist() == [2, 3, 4]                          # ascending distance; of the cut pair (4, 5) the lower raw index stays
    np.testing.assert_array_equal(out["pos"], obs["pos"][[2, 3, 4]])
    full = md.prepare_obstacles(state, obs["position"], obs["radius"], 3, N, DT, raw_vel=np.tile([-0.5, 0.0], (6, 1)))
    assert full["selected"].tolist() == [2, 3, 4]


def test_fewer_obstacles_keep_raw_order_and_get_dummies():
    state = (1.5, -2.0, 0.3, 0.8)
    pos = np.array([[9.0, 1.0], [2.0, 0.5], [5.0, -3.0]]); vel = np.array([[0.1, 0.2], [-0.3, 0.0], [0.0, 0.4]])
    out = md.prepare_obstacles(state, pos, [0.4, 0.5, 0.6], 5, N, DT, raw_vel=vel)
    assert out["selected"].tolist() == [0, 1, 2, -1, -1]      # raw order although obstacle 1 is the closest
    assert out["radius"].tolist() == [0.4, 0.5, 0.6, 0.0, 0.0]
    np.testing.assert_array_equal(out["pos"][3:], np.broadcast_to([101.5, 98.0], (2, N, 2)))
    np.testing.assert_array_equal(out["pos"][1, 7], pos[1] + (vel[1] * DT) * 7.0)
    assert not out["gaussian"].any() and (out["major"] == 0.0).all() and (out["chi"] == 1.0).all()
    exact = md.prepare_obstacles(state, pos, [0.4, 0.5, 0.6], 3, N, DT, raw_vel=vel)
    assert exact["selected"].tolist() == [0, 1, 2]            # exactly M: untouched
    # no obstacle at all: M dummies; in probabilistic mode a dummy is a GAUSSIAN constant-velocity obstacle with the noise
    none = md.prepare_obstacles(state, np.zeros((0, 2)), np.zeros(0), 2, N, DT, raw_vel=np.zeros((0, 2)), probabilistic=True)
    assert none["selected"].tolist() == [-1, -1] and none["gaussian"].all() and (none["shape"][:, :, 1] == 0.3).all()


def test_distance_filter_sees_the_current_position_only():
    state = (0.0, 0.0, 0.0, 1.0)
    pos = np.array([[7.0, 0.0], [3.0, 4.0], [5.9, 0.0], [0.0, -6.0]])            # distances 7, 5, 5.9, 6 (not closer than 6: dropped)
    vel = np.array([[-5.0, 0.0], [0.0, 0.0], [9.0, 0.0], [0.0, 0.0]])            # obstacle 0 approaches, obstacle 2 leaves: irrelevant (:88)
    out = md.prepare_obstacles(state, pos, np.full(4, 0.4), 3, N, DT, raw_vel=vel, max_obstacle_distance=6.0)
    assert out["selected"].tolist() == [1, 2, -1]
    obs, keep = md.remove_distant_obstacles(_cv_set(pos, vel), state, 6.0)
    assert keep.tolist() == [1, 2] and obs["pos"].shape == (2, N, 2)


def test_given_predictions_and_their_type():
    """ros1_jackalsimulator.cpp:331-334: GAUSSIAN iff probabilistic and the last step's major != 0."""
    state = (0.0, 0.0, 0.0, 1.0)
    pred = np.zeros((2, N, 5))
    pred[:, :, 0] = 3.0 + 0.1 * np.arange(N); pred[:, :, 1] = [[1.0], [-2.0]]; pred[:, :, 2] = 0.25
    pred[0, :, 3] = 0.2; pred[0, :, 4] = 0.1                                     # obstacle 1: zero uncertainty
    pred[1, :N - 1, 3] = 0.3                                                     # ... except before the last step: still DETERMINISTIC
    out = md.prepare_obstacles(state, pred[:, 0, :2], [0.4, 0.4], 3, N, DT, raw_pred=pred, probabilistic=True, propagate_passes=1)
    assert out["gaussian"].tolist() == [True, False, True]                       # the dummy: a probabilistic constant-velocity obstacle
    assert out["chi"][1] == 1.0 and out["chi"][0] == -np.log(0.05) / 0.5
    np.testing.assert_array_equal(out["shape"][1, :, 1], pred[1, :, 3])          # as given, untouched by the pass
    assert (out["major"][1] == 0.0).all()                                        # what the ellipsoid rows take (ellipsoid_constraints.cpp:72-77)
    assert out["major"][0, 0] == np.sqrt(0.0 + (0.2 * DT) * (0.2 * DT)) and (out["angle"][:2] == 0.25).all()
    det = md.prepare_obstacles(state, pred[:, 0, :2], [0.4, 0.4], 3, N, DT, raw_pred=pred, probabilistic=False, propagate_passes=2)
    assert not det["gaussian"].any()
    np.testing.assert_array_equal(det["shape"][0, :, 1], pred[0, :, 3])


def test_uncertainty_propagation():
    """One pass over sigma = 0.3 is the scene generator's Gaussian prediction (a cumulative sum under one square root there: equal to rounding,
    not bitwise); two passes -- what ros1_jackal.cpp:324-332 does -- pinned by hand for k = 0, 1."""
    sc = scenes.make_scene(3, N=N, M=8, B=1, gaussian=True)
    one, one_minor = md.propagate_prediction_uncertainty(np.full(N, 0.3), np.full(N, 0.3), DT)
    np.testing.assert_allclose(one, sc["obstacles"]["major"][0], rtol=1e-14, atol=0.0)
    np.testing.assert_array_equal(one, one_minor)
    a0 = np.sqrt(0.0 * 0.0 + (0.3 * DT) * (0.3 * DT)); a1 = np.sqrt(a0 * a0 + (0.3 * DT) * (0.3 * DT))
    assert one[0] == a0 == 0.06 and one[1] == a1
    two, _ = md.propagate_prediction_uncertainty(one, one_minor, DT)
    b0 = np.sqrt(0.0 + (a0 * DT) * (a0 * DT)); b1 = np.sqrt(b0 * b0 + (a1 * DT) * (a1 * DT))
    assert two[0] == b0 and two[1] == b1 and abs(b0 - 0.012) < 1e-17 and abs(b1 - 0.012 * np.sqrt(3.0)) < 1e-16
    cv = md.constant_velocity_prediction([1.0, 2.0], [0.5, -0.5], DT, N, probabilistic=True)       # (:75-76: one pass inside)
    np.testing.assert_array_equal(cv["major"], one)
    out = md.prepare_obstacles((0.0, 0.0, 0.0, 1.0), [[1.0, 2.0]], [0.4], 2, N, DT, raw_vel=[[0.5, -0.5]], probabilistic=True, propagate_passes=2)
    np.testing.assert_array_equal(out["major"], np.tile(two, (2, 1)))                               # the dummy gets the passes like any other


def _scene_velocities(scene_idx, M):
    """The obstacle velocities make_scene draws (its first random numbers; it does not return them)."""
    rng = np.random.Generator(np.random.PCG64(1000 + scene_idx))
    rng.uniform(0.5, 2.0)
    scenes.reference_path_segments(rng, 5)
    speed = rng.uniform(0.6, 1.6, M)
    heading = np.where(rng.uniform(size=M) < 0.5, 1.0, -1.0) * np.pi / 2 + rng.uniform(-0.5, 0.5, M)
    return np.stack([speed * np.cos(heading), speed * np.sin(heading)], 1)


def test_composition_reproduces_the_scene():
    """R = M raw constant-velocity obstacles (a scene's pos0 and vel): prepare_obstacles gives the scene's predictions bit for bit, and
    ellipsoid_set_parameters on its result the scene's parameter rows bit for bit."""
    for idx in (3, 11):
        sc = scenes.make_scene(idx, N=N, M=8, B=2)
        vel = _scene_velocities(idx, 8)
        pos0 = sc["obstacles"]["pos"][:, 0]
        state = (sc["xinit"][0, 0], sc["xinit"][0, 1], sc["xinit"][0, 2], sc["xinit"][0, 3])
        out = md.prepare_obstacles(state, pos0, sc["obstacles"]["radius"], 8, N, DT, raw_vel=vel)
        np.testing.assert_array_equal(out["pos"], sc["obstacles"]["pos"])
        assert out["selected"].tolist() == list(range(8))
        pm = sc["pm"]
        params = sc["params"][0].copy()
        cols = [pm.index(f"ellipsoid_obst_{j}_{f}") for j in range(8) for f in ("x", "y", "psi", "major", "minor", "chi", "r")]
        cols += [pm.index("ego_disc_radius"), pm.index("ego_disc_0_offset")]
        params[:, cols] = -7.0
        md.ellipsoid_set_parameters(pm, params, state[:2], out, scenes.ROBOT_RADIUS)
        np.testing.assert_array_equal(params, sc["params"][0])
