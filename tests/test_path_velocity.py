"""CPU: the velocity-profile mirrors (mpc_planner_amd/modules.py path_velocity_at, path_velocity_window, scatter_parameters -- what
PathReferenceVelocity::setParameters, path_reference_velocity.cpp:59-95, writes and what GuidanceConstraints::update hands to the guidance
planner, guidance_constraints.cpp:91-94) on hand values, and the emitted stage cost of the `path_velocity` stack of build() on a window the
mirrors wrote.  tk::spline::operator() is not in the reference tree: these tests pin what DESIGN.md U17 states.  The device kernels are held
to these mirrors bit for bit (tests/test_gpu_path_velocity.py)."""
import numpy as np
import pytest

from mpc_planner_amd import modules as md

# two segments on the knots 0, 2, 5 (length 5): v(s) = ((a t + b) t + c) t + d on t = s - start
VEL = np.array([[0.125, -0.5, 0.25, 1.5], [-0.0625, 0.75, 2.0, 0.75]])
PATH = np.zeros((2, 9)); PATH[:, 8] = (0.0, 2.0)


def test_path_velocity_at_hand_values():
    at = lambda s: md.path_velocity_at(VEL, PATH, 2, 5.0, s, 1.7)
    assert at(1.0) == 0.125 - 0.5 + 0.25 + 1.5                                        # t = 1 on segment 0
    assert at(4.0) == ((-0.0625 * 2.0 + 0.75) * 2.0 + 2.0) * 2.0 + 0.75                # t = 2 on segment 1
    assert at(2.0) == 0.75                                                             # on a knot: the RIGHT segment's d, exactly
    assert at(np.nextafter(2.0, 0.0)) != 0.75                                          # just before it: still segment 0
    assert at(0.0) == 1.5
    assert at(-1.0) == ((0.125 * -1.0 - 0.5) * -1.0 + 0.25) * -1.0 + 1.5              # below the first knot: segment 0, t < 0
    assert at(5.0) == ((-0.0625 * 3.0 + 0.75) * 3.0 + 2.0) * 3.0 + 0.75                # s = length: the last cubic at t = L_last
    assert at(5.5) == ((-0.0625 * 3.5 + 0.75) * 3.5 + 2.0) * 3.5 + 0.75                # beyond: it continues (U17)
    # the Horner form, not the power form: the two differ in the last bits for these coefficients
    a, b, c, d = 0.1, 0.7, -0.3, 1.1
    got = md.path_velocity_at(np.array([[a, b, c, d]]), PATH[:1], 1, 3.0, 1.3, 0.0)
    assert got == ((a * 1.3 + b) * 1.3 + c) * 1.3 + d
    # only the first `count` rows are looked at
    assert md.path_velocity_at(VEL, PATH, 1, 2.0, 4.0, 1.7) == ((0.125 * 4.0 - 0.5) * 4.0 + 0.25) * 4.0 + 1.5
    assert np.isnan(md.path_velocity_at(VEL, PATH, 2, 5.0, np.nan, 1.7))               # no knot is <= NaN: segment 0, t = NaN


def test_no_profile_falls_back_to_the_reference_velocity():
    assert md.path_velocity_at(None, PATH, 2, 5.0, 1.0, 1.7) == 1.7
    assert md.path_velocity_at(VEL, PATH, 0, 5.0, 1.0, 1.7) == 1.7
    assert md.path_velocity_window(None, 2, 0, 3, 1.7).tolist() == [[0.0, 0.0, 0.0, 1.7]] * 3


def test_window_on_a_fitted_profile_agrees_with_the_value():
    """fit_path's velocity cubics interpolate the waypoints' v: path_velocity_at on knot i is v_i exactly (the cubic's d), and the window's
    first slot is the cubic that path_velocity_at evaluates for any s inside the segment."""
    xy = np.stack([np.linspace(0.0, 7.0, 8), np.sin(np.linspace(0.0, 2.0, 8))], 1)
    v = np.array([1.0, 1.2, 1.5, 1.4, 1.0, 0.8, 0.9, 0.5])
    fit = md.fit_path(xy, v=v)
    for i in range(7):
        assert md.path_velocity_at(fit["velocity"], fit["path"], 7, fit["length"], fit["path"][i, 8], 9.9) == v[i]
    s = 0.5 * (fit["path"][3, 8] + fit["path"][4, 8])
    a, b, c, d = md.path_velocity_window(fit["velocity"], 7, 3, 2, 9.9)[0]
    t = s - fit["path"][3, 8]
    assert md.path_velocity_at(fit["velocity"], fit["path"], 7, fit["length"], s, 9.9) == ((a * t + b) * t + c) * t + d
    assert abs(md.path_velocity_at(fit["velocity"], fit["path"], 7, fit["length"], fit["length"], 9.9) - v[-1]) < 1e-12


@pytest.mark.parametrize("per_stage", [False, True])
def test_scatter_parameters_against_a_plain_loop(per_stage):
    rng = np.random.default_rng(3)
    B, N, npar, n_scenes = 7, 4, 11, 3
    cols = [9, 0, 4, 10]
    scene_of = np.array([0, 2, -1, 1, 3, 2, 0])                                        # -1 and 3: outside [0, 3)
    values = rng.normal(size=(n_scenes, N, len(cols)) if per_stage else (n_scenes, len(cols)))
    params = rng.normal(size=(B, N, npar)); before = params.copy()
    md.scatter_parameters(params, cols, values, scene_of, per_stage)
    want = before.copy()
    for b in range(B):
        if scene_of[b] in (0, 1, 2):
            for k in range(N):
                for c in range(len(cols)):
                    want[b, k, cols[c]] = values[scene_of[b], k, c] if per_stage else values[scene_of[b], c]
    assert np.array_equal(params, want)
    assert np.array_equal(params[[2, 4]], before[[2, 4]])                              # entries outside the scene range: untouched
    assert np.array_equal(np.delete(params, cols, axis=2), np.delete(before, cols, axis=2))
    assert not np.array_equal(params[0], before[0])
    for bad in ([1, 1], [], [11], [-1], list(range(11)) * 12):
        with pytest.raises(ValueError):
            md.scatter_parameters(params, bad, np.zeros((n_scenes, N, len(bad)) if per_stage else (n_scenes, len(bad))), scene_of, per_stage)


def test_scatter_with_the_spline_columns_is_the_path_writer():
    """With the spline_v columns of the stack's parameter map, scatter_parameters writes what path_velocity_set_parameters writes."""
    from mpc_planner_amd.codegen import plugin as P, stacks
    st = stacks.settings(N=20, max_obstacles=2, num_segments=3)
    _, mm = stacks.contouring_path_velocity_ellipsoids(st)
    pm = P.define_parameters(mm, P.Parameters(), st)
    window = md.path_velocity_window(np.arange(8.0).reshape(2, 4) + 1.0, 2, 1, 3, 0.0)
    want = np.full((20, pm.length()), -3.0)
    md.path_velocity_set_parameters(pm, want, window)
    got = np.full((1, 20, pm.length()), -3.0)
    cols = [pm.index(f"spline_v{i}_{k}") for i in range(3) for k in "abcd"]
    md.scatter_parameters(got, cols, window.reshape(1, 12), [0])
    assert np.array_equal(got[0], want)


def test_stage_cost_of_the_path_velocity_stack_on_a_mirror_window():
    """The emitted stage cost of build()'s `path_velocity` stack (dynamic velocity reference, three segments), evaluated on the host with the
    spline and spline_v columns the mirrors write for a window that STRADDLES THE PATH'S END: a straight path x(s) = s on the knots 0, 2, 4, 6
    with v = 1 + 0.25 s at the waypoints (a natural spline through collinear values is that line), tracked from segment 1.  Slots: segments
    1 and 2, then the end padding, whose velocity slot is (0, 0, 0, 0).  By hand: lag error x - s, contour error -y, and v_ref the
    sigmoid glue (spline.py:25-50) of the three slots' values -- near the last knot the zero slot pulls v_ref down: the brake."""
    from mpc_planner_amd.codegen import emit, stacks
    from mpc_planner_amd.codegen.hostlib import HostStageFunctions
    st = stacks.settings(N=20, max_obstacles=2, num_segments=3); st["contouring"]["dynamic_velocity_reference"] = True
    model, mm = stacks.contouring_path_velocity_ellipsoids(st)
    gen = emit.generate(mm, model, st, "path_velocity", method="jets")
    pm, hs = gen["params"], HostStageFunctions(gen["header"])
    knots = np.array([0.0, 2.0, 4.0, 6.0])
    fit = md.fit_path(np.stack([knots, np.zeros(4)], 1), v=1.0 + 0.25 * knots)
    assert fit["count"] == 3 and np.array_equal(fit["velocity"][:, :2], np.zeros((3, 2)))
    S, seg = 3, 1
    window = md.path_window(fit["path"], fit["length"], seg, S)
    vwin = md.path_velocity_window(fit["velocity"], fit["count"], seg, S, 1.7)
    assert np.array_equal(vwin[:2], fit["velocity"][1:]) and (vwin[2] == 0.0).all() and window[2, 8] == 6.0
    p = np.zeros((1, 1, hs.npar))
    for n, v in dict(acceleration=0.3, angular_velocity=0.8, contour=0.05, lag=0.75, velocity=0.55, ego_disc_radius=0.3).items():
        p[0, 0, pm.index(n)] = v
    for j in range(2):
        for n, v in dict(x=50.0, y=50.0, r=0.1, chi=1.0).items():
            p[0, 0, pm.index(f"ellipsoid_obst_{j}_{n}")] = v
    names = ("spline_x{}_a", "spline_x{}_b", "spline_x{}_c", "spline_x{}_d", "spline_y{}_a", "spline_y{}_b", "spline_y{}_c", "spline_y{}_d", "spline{}_start")
    md.scatter_parameters(p, [pm.index(n.format(i)) for i in range(S) for n in names], window.reshape(1, -1), [0])
    md.scatter_parameters(p, [pm.index(f"spline_v{i}_{k}") for i in range(S) for k in "abcd"], vwin.reshape(1, -1), [0])
    for s in (3.0, 4.9, 5.95, 6.0):
        z = np.array([0.4, -0.2, s + 0.3, 0.6, 0.1, 1.2, s])                           # a, w, x, y, psi, v, s
        lam = [1.0 / (1.0 + np.exp((s - start + 0.02) / 0.1)) for start in (4.0, 6.0)]
        slot = [md.path_velocity_at(vwin[i:i + 1], window[i:i + 1], 1, 0.0, s, 0.0) for i in range(S)]
        assert slot[2] == 0.0 and abs(slot[0] - (1.0 + 0.25 * s)) < 1e-12
        v_ref = lam[0] * slot[0] + (1.0 - lam[0]) * (lam[1] * slot[1] + (1.0 - lam[1]) * slot[2])
        want = 0.3 * 0.16 + 0.8 * 0.04 + 0.75 * 0.3 ** 2 + 0.05 * 0.6 ** 2 + 0.55 * (1.2 - v_ref) ** 2
        got, _, _ = hs.cost(z, p[0, 0])
        assert abs(got - want) < 1e-9, (s, got, want)
    assert v_ref < 0.5 * (1.0 + 0.25 * 6.0)                                             # at the end the brake has taken more than half
