"""Host-side mirror of the C++ modules' parameter writers on the T-MPC path (numpy, per trajectory).

Each function cites the reference method it restates; they fill one solver's `all_parameters[N][npar]`
(acados_solver_interface.h:56) and warm start `x0[(N+1)][nvar]` (:54) exactly like the reference's
`setParameters(k)` / `initializeSolverWithGuidance` do, so the parity tests read like the reference flow.
"""
import numpy as np

NU, NX, NV = 2, 5, 7
IDX = dict(a=0, w=1, x=2, y=3, psi=4, v=5, spline=6)   # model_map.yaml order (solver_model.py:118-128)


def mpc_base_set_parameters(pm, params, weights):
    """MPCBaseModule::setParameters (mpc_planner_modules/src/mpc_base.cpp:23-35): every stage k."""
    for name in ("acceleration", "angular_velocity", "slack", "velocity", "reference_velocity"):
        if pm.has_parameter(name):
            params[:, pm.index(name)] = weights[name]


def contouring_set_parameters(pm, params, weights, segments):
    """Contouring::setParameters + setSplineParameters (contouring.cpp:50-124): weights and the S
    segments starting at the closest one, identical for every stage k.
    segments: array [S][9] = (xa,xb,xc,xd, ya,yb,yc,yd, start)."""
    for name in ("contour", "lag", "terminal_angle", "terminal_contouring"):
        params[:, pm.index(name)] = weights[name]
    names = ["spline_x{}_a", "spline_x{}_b", "spline_x{}_c", "spline_x{}_d",
             "spline_y{}_a", "spline_y{}_b", "spline_y{}_c", "spline_y{}_d", "spline{}_start"]
    for i in range(segments.shape[0]):
        for w, n in enumerate(names):
            params[:, pm.index(n.format(i))] = segments[i, w]


def ellipsoid_set_parameters(pm, params, state_xy, obstacles, robot_radius, disc_offset=0.0):
    """EllipsoidConstraints::update/setParameters (ellipsoid_constraints.cpp:24-90).
    obstacles: dict(pos [M][N][2], angle [M][N], radius [M], major [M][N], minor [M][N], chi [M])."""
    N = params.shape[0]
    M = obstacles["pos"].shape[0]
    params[:, pm.index("ego_disc_radius")] = robot_radius
    params[:, pm.index("ego_disc_0_offset")] = disc_offset
    for j in range(M):
        ix = [pm.index(f"ellipsoid_obst_{j}_{f}") for f in ("x", "y", "psi", "major", "minor", "chi", "r")]
        # k == 0: dummies (:42-56)
        params[0, ix] = [state_xy[0] + 50.0, state_xy[1] + 50.0, 0.0, 0.0, 0.0, 1.0, 0.1]
        # k >= 1: prediction step k-1 (:62-85)
        params[1:, ix[0]] = obstacles["pos"][j, :N - 1, 0]
        params[1:, ix[1]] = obstacles["pos"][j, :N - 1, 1]
        params[1:, ix[2]] = obstacles["angle"][j, :N - 1]
        params[1:, ix[3]] = obstacles["major"][j, :N - 1]
        params[1:, ix[4]] = obstacles["minor"][j, :N - 1]
        params[1:, ix[5]] = obstacles["chi"][j]
        params[1:, ix[6]] = obstacles["radius"][j]


def gaussian_set_parameters(pm, params, state_xy, obstacles, robot_radius, risk, disc_offset=0.0):
    """GaussianConstraints::update/setParameters (gaussian_constraints.cpp:22-79): stage 0 dummies (x + 100, y + 100,
    0.1, 0.1, 0.05, 0.1), stages k >= 1 the Gaussian prediction step k-1 with CONFIG probabilistic/risk and obstacle_radius."""
    N = params.shape[0]
    M = obstacles["pos"].shape[0]
    params[:, pm.index("ego_disc_radius")] = robot_radius
    params[:, pm.index("ego_disc_0_offset")] = disc_offset
    for j in range(M):
        ix = [pm.index(f"gaussian_obst_{j}_{f}") for f in ("x", "y", "major", "minor", "risk", "r")]
        params[0, ix] = [state_xy[0] + 100.0, state_xy[1] + 100.0, 0.1, 0.1, 0.05, 0.1]
        params[1:, ix[0]] = obstacles["pos"][j, :N - 1, 0]
        params[1:, ix[1]] = obstacles["pos"][j, :N - 1, 1]
        params[1:, ix[2]] = obstacles["major"][j, :N - 1]
        params[1:, ix[3]] = obstacles["minor"][j, :N - 1]
        params[1:, ix[4]] = risk
        params[1:, ix[5]] = obstacles["radius"][j]


def _outside_disc(qx, qy, cx, cy, r):
    """Nearest point of the closed outside of the disc (c, r)."""
    dx, dy = qx - cx, qy - cy
    dist = np.sqrt(dx * dx + dy * dy)
    if dist >= r:
        return qx, qy
    if dist > 1e-12:
        s = r / dist
        return cx + dx * s, cy + dy * s
    return cx, cy + r


def project_to_safety(pos, obstacles_k, r):
    """(r: one radius for every obstacle, or one per obstacle -- the `_use_guidance == false` branch uses each obstacle's own.)"""
    return _project_to_safety(pos, obstacles_k, np.broadcast_to(np.asarray(r, float), (len(obstacles_k),)))


def _project_to_safety(pos, obstacles_k, radii):
    """LinearizedConstraints::projectToSafety (linearized_constraints.cpp:130-148): at most 3 sweeps over the obstacles of
    ros_tools' Douglas-Rachford projection, with obstacle 0 as the anchor.  The ros_tools source is not in the reference tree
    (DESIGN.md U10); restated from the published Douglas-Rachford operator p <- (p + R_delta R_anchor p) / 2 with reflections
    R = 2 P - I, P = nearest point outside the disc of radius r, applied when p is inside the obstacle's disc -- the call order of
    the reference (anchor first, then the obstacle).  The identity for a guess clear of every obstacle.  Same arithmetic as
    tmpc_linearize_topology_kernel (csrc/tmpc_aux_kernels.hpp) and the C++ DouglasRachford (modules_hip.h)."""
    px, py = float(pos[0]), float(pos[1])
    if len(obstacles_k) == 0:
        return np.array([px, py])
    ax, ay = float(obstacles_k[0][0]), float(obstacles_k[0][1])
    for _ in range(3):
        for o, r in zip(obstacles_k, radii):
            dx, dy = px - o[0], py - o[1]
            if np.sqrt(dx * dx + dy * dy) < r:
                qx, qy = _outside_disc(px, py, ax, ay, r)
                rx, ry = 2.0 * qx - px, 2.0 * qy - py
                bx, by = _outside_disc(rx, ry, float(o[0]), float(o[1]), r)
                sx, sy = 2.0 * bx - rx, 2.0 * by - ry
                px, py = (px + sx) / 2.0, (py + sy) / 2.0
    return np.array([px, py])


def _road_segment_eval(coef, starts, s):
    """Point and derivative of the plain piecewise cubic at s (assumption 2): the segment i = max{j : start_j <= s}
    (i = 0 below the first knot; beyond the last knot the last segment's cubic continues), t = s - start_i, Horner form -- no sigmoid
    glue, that belongs to the NLP's spline.  coef [S][8] = (ax bx cx dx ay by cy dy); starts [S].  Same operation order as
    tmpc_arith::road_frame, which tmpc_road_halfspaces_kernel and the C++ Contouring compile."""
    i = 0
    for j in range(len(starts)):
        if starts[j] <= s:
            i = j
    t = s - starts[i]
    c = coef[i]
    px = ((c[0] * t + c[1]) * t + c[2]) * t + c[3]
    py = ((c[4] * t + c[5]) * t + c[6]) * t + c[7]
    dx = (3.0 * c[0] * t + 2.0 * c[1]) * t + c[2]
    dy = (3.0 * c[4] * t + 2.0 * c[5]) * t + c[6]
    return px, py, dx, dy


def _road_orthogonal(dx, dy):
    """getOrthogonal (assumption 1): the unit normal pointing to the RIGHT of travel, (y', -x') / |(x', y')|."""
    n = np.sqrt(dx * dx + dy * dy)
    return dy / n, -dx / n


def road_offsets(width, radius, two_way=False):
    """(offset_first, offset_second) of the centreline mode (contouring.cpp:203,216-220,229-230): times * width / 2 - r with
    times = 3 on a two-way road (the side row 0 bounds, the right of travel under U12), and width / 2 - r."""
    half = width / 2.0
    return (3.0 if two_way else 1.0) * half - radius, half - radius


def road_halfspaces(segments, s_of_k, offset_first, offset_second):
    """Contouring::constructRoadConstraintsFromCenterline (contouring.cpp:191-235): for stage k = 1 .. N-1 (N = len(s_of_k); stage 0
    gets nothing and stays zero here) with s_k = the MAIN solver's warm-start spline state, P the path point and A the unit normal
    (_road_orthogonal) at s_k:  row 0 (A, A.(P + A offset_first)),  row 1 (-A, -A.(P - A offset_second)),  each meaning a.p <= b;
    offsets from road_offsets.  segments [S][9] = (ax bx cx dx ay by cy dy start), the window the parameter rows carry.
    RosTools::Spline2D is not in the reference tree: normal direction and spline evaluation are the assumptions U12 of DESIGN.md.
    Returns [N][2][3] = (a1, a2, b), directly usable as linearized_update(static=...)."""
    segments = np.asarray(segments, float)
    N = len(s_of_k)
    out = np.zeros((N, 2, 3))
    for k in range(1, N):
        px, py, dx, dy = _road_segment_eval(segments[:, :8], segments[:, 8], float(s_of_k[k]))
        ax, ay = _road_orthogonal(dx, dy)
        b0 = ax * (px + ax * offset_first) + ay * (py + ay * offset_first)
        b1 = ax * (px - ax * offset_second) + ay * (py - ay * offset_second)
        out[k, 0] = (ax, ay, b0)
        out[k, 1] = (-ax, -ay, -b1)
    return out


def road_halfspaces_from_bounds(segments, left, right, s_of_k, radius):
    """Contouring::constructRoadConstraintsFromBounds (contouring.cpp:237-262): P_l, A_l / P_r, A_r point and normal of the left /
    right bound spline at the same s_k -- the bound splines live on the centreline's knot vector (:142-149), so only `segments`'
    start column is used --:  row 0 (-A_l, -A_l.(P_l + A_l r)),  row 1 (A_r, A_r.(P_r - A_r r)).
    left, right [S][8] = (ax bx cx dx ay by cy dy).  Returns [N][2][3]."""
    starts = np.asarray(segments, float)[:, 8]
    left = np.asarray(left, float); right = np.asarray(right, float)
    N = len(s_of_k)
    out = np.zeros((N, 2, 3))
    for k in range(1, N):
        s = float(s_of_k[k])
        px, py, dx, dy = _road_segment_eval(left[:, :8], starts, s)
        ax, ay = _road_orthogonal(dx, dy)
        bl = ax * (px + ax * radius) + ay * (py + ay * radius)
        out[k, 0] = (-ax, -ay, -bl)
        px, py, dx, dy = _road_segment_eval(right[:, :8], starts, s)
        ax, ay = _road_orthogonal(dx, dy)
        br = ax * (px - ax * radius) + ay * (py - ay * radius)
        out[k, 1] = (ax, ay, br)
    return out


def linearized_update(x0, obstacle_pos, robot_radius, obstacle_radius=None, static=None):
    """LinearizedConstraints::update (linearized_constraints.cpp:49-123).  x0: warm start [N+1][nvar]; obstacle_pos [M][N][2].
    obstacle_radius None: guidance mode, radius 1e-3 (:99); else [M], the `_use_guidance == false` branch with each obstacle's own radius.
    static: [N][n_static][3] static halfspaces (a1, a2, b) per stage, appended behind the obstacle rows as they are (:107-123).
    Returns a1, a2, b [N][M + n_static] (row k = 0 unused)."""
    Np1 = x0.shape[0]; N = Np1 - 1; M = obstacle_pos.shape[0]
    n_static = 0 if static is None else static.shape[1]
    a1 = np.zeros((N, M + n_static)); a2 = np.zeros((N, M + n_static)); b = np.zeros((N, M + n_static))
    radii = (np.full(M, 1e-3) if obstacle_radius is None else np.asarray(obstacle_radius, float)) + robot_radius   # _use_guidance (:99, :140)
    for k in range(1, N):
        pos = project_to_safety(x0[k, [IDX["x"], IDX["y"]]], obstacle_pos[:, k - 1], radii) if M else x0[k, [IDX["x"], IDX["y"]]]
        for j in range(M):
            o = obstacle_pos[j, k - 1]
            diff = o - pos
            dist = np.sqrt(diff[0] * diff[0] + diff[1] * diff[1])
            a1[k, j] = diff[0] / dist
            a2[k, j] = diff[1] / dist
            b[k, j] = a1[k, j] * o[0] + a2[k, j] * o[1] - radii[j]
        if n_static:
            a1[k, M:] = static[k, :, 0]; a2[k, M:] = static[k, :, 1]; b[k, M:] = static[k, :, 2]
    return a1, a2, b


def linearized_set_parameters(pm, params, state_x, lin=None, n_rows=None):
    """LinearizedConstraints::setParameters (linearized_constraints.cpp:150-189).  lin=None writes the
    all-dummy rows of the non-guided T-MPC++ planner (guidance_constraints.cpp:301-305,323-324)."""
    N = params.shape[0]
    dummy = (1.0, 0.0, state_x + 100.0)                       # _dummy_a1,_dummy_a2 (header), _dummy_b (:54)
    for j in range(n_rows):
        ia = [pm.index(f"lin_constraint_{j}_{f}") for f in ("a1", "a2", "b")]
        params[:, ia] = dummy                                 # k == 0 and unused rows
        if lin is not None and j < lin[0].shape[1]:
            params[1:, ia[0]] = lin[0][1:, j]
            params[1:, ia[1]] = lin[1][1:, j]
            params[1:, ia[2]] = lin[2][1:, j]


def halfspace_rows_set_parameters(pm, params, state_x, rows, prefix, n_rows, disc_offset=0.0):
    """DecompConstraints::setParameters (decomp_constraints.cpp:150-187) and the scenario_module's parameter writer
    (scenario_constraints.cpp:76-79; same layout, scenario_constraints.py:40-49): ego disc offset at every stage,
    k = 0 all dummies (1, 0, x + 100), stages k >= 1 the rows computed by update(), padded with dummies.
    rows: (a1, a2, b) each [N][n] with row k = 0 unused, or None; prefix: "disc_0_decomp" | "disc_0_scenario_constraint"."""
    params[:, pm.index("ego_disc_0_offset")] = disc_offset
    dummy = (1.0, 0.0, state_x + 100.0)
    for j in range(n_rows):
        ia = [pm.index(f"{prefix}_{j}_{f}") for f in ("a1", "a2", "b")]
        params[:, ia] = dummy
        if rows is not None and j < rows[0].shape[1]:
            ok = ~np.isnan(rows[0][1:, j])                   # NaN = no row computed for this slot: stays a dummy
            for w in range(3):
                col = params[1:, ia[w]]
                col[ok] = rows[w][1:, j][ok]
                params[1:, ia[w]] = col


POLY_EPS_PARALLEL = 1e-12       # |sin| below which two halfspace boundaries count as parallel
POLY_TOL_EDGE = 1e-9            # minimal length [m] of the piece of a boundary line that lies on the polygon
POLY_SEED_MARGIN = 1e-6         # slack of the candidate filter
POLY_BINS = (4, 32, 256)        # sector resolution (bins per octant) of the three filter rounds


def _poly_sector(ax, ay, bins):
    """Direction sector 0..8*bins-1 of unit vectors (octant x bins of min(|ax|,|ay|)/max(|ax|,|ay|)): only comparisons, one divide
    and one multiply by a power of two, so host and device classify identically."""
    u, v = np.abs(ax), np.abs(ay)
    steep = v > u
    octant = (ax < 0).astype(int) | ((ay < 0).astype(int) << 1) | (steep.astype(int) << 2)
    t = np.where(steep, u, v) / np.where(steep, v, u)
    return octant * bins + np.minimum((t * float(bins)).astype(int), bins - 1)


def _poly_clip(ax, ay, dm, rows, cols, kill_below, dedup):
    """Clip the boundary line of every halfspace in `rows` (q_i + t perp_i, q_i = p + dm_i a_i) with the halfspaces in `cols`:
    (a_j . perp_i) t <= dm_j - dm_i (a_j . a_i).  Returns lo, hi (the interval of t left) and kill (a parallel halfspace
    excludes the whole line -- kill_below <= 0 is the slack of that decision; with dedup, of identical halfspaces only the
    lowest index survives)."""
    a1i, a2i, di = ax[rows][:, None], ay[rows][:, None], dm[rows][:, None]
    a1j, a2j, dj = ax[cols][None, :], ay[cols][None, :], dm[cols][None, :]
    c = a1j * (-a2i) + a2j * a1i
    dot = a1j * a1i + a2j * a2i
    rhs = dj - di * dot
    other = np.asarray(rows)[:, None] != np.asarray(cols)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = rhs / c
    hi = np.where(other & (c > POLY_EPS_PARALLEL), ratio, np.inf).min(axis=1, initial=np.inf)
    lo = np.where(other & (c < -POLY_EPS_PARALLEL), ratio, -np.inf).max(axis=1, initial=-np.inf)
    par = other & (np.abs(c) <= POLY_EPS_PARALLEL)
    same = dot > 0.0                                   # same direction: the closer one wins; opposite: an empty strip kills both
    k = par & np.where(same, dj < di + kill_below, rhs < kill_below)
    if dedup:
        k |= par & same & (dj == di) & (np.asarray(cols)[None, :] < np.asarray(rows)[:, None])
    return lo, hi, k.any(axis=1)


def polygon_edges(ax, ay, dm):
    """Which of the halfspaces  a_i . (q - p) <= dm_i  (unit normals a_i = (ax, ay), margins dm_i measured from the point p they
    were linearised around) form the boundary of their intersection polygon: halfspace i is an edge iff the piece of its boundary
    line inside all other halfspaces has positive length (every other halfspace is redundant -- removing it changes nothing).
    A filter comes first -- free to be anything conservative, since a halfspace whose boundary line misses the polygon of SOME of
    the halfspaces (the seeds) cannot touch the smaller polygon of all, and dropping it changes neither the polygon nor its edges:
    here three rounds at sector resolution POLY_BINS, the closest halfspace of each direction sector a seed (lowest index on ties),
    every seed clipping; tmpc_scenario_halfspaces_kernel filters differently (neighbouring seeds only, no division).  Then the edge
    test above among the candidates, which the kernel runs with the same per-pair arithmetic -- the rows are equal bit for bit.
    Returns a bool array."""
    n = len(dm)
    cand = np.arange(n)
    for bins in POLY_BINS:
        sec = _poly_sector(ax[cand], ay[cand], bins)
        order = np.lexsort((cand, dm[cand]))                    # by margin, then index
        seeds = np.sort(cand[order[np.unique(sec[order], return_index=True)[1]]])
        lo, hi, kill = _poly_clip(ax, ay, dm, cand, seeds, -POLY_SEED_MARGIN, False)
        cand = cand[~kill & (hi - lo > -POLY_SEED_MARGIN)]
    lo, hi, kill = _poly_clip(ax, ay, dm, cand, cand, 0.0, True)
    edge = np.zeros(n, bool)
    edge[cand] = ~kill & (hi - lo > POLY_TOL_EDGE)
    return edge


# ---- SH-MPC scenario sampler: host mirror of tmpc_sample_scenarios_kernel, bit for bit -------------------------------------------
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _smp_mix(z):
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _smp_uniform(key, ctr):
    with np.errstate(over="ignore"):
        r = _smp_mix(np.uint64(key) + (np.asarray(ctr, np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15))
    return ((r >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def _det_log(x):
    """Natural logarithm from +, x, / only, in the operation order of the device's det_log (no library call: reproducible)."""
    m, e = np.frexp(x)
    small = m < 0.70710678118654752
    m = np.where(small, m * 2.0, m); e = np.where(small, e - 1, e)
    f = (m - 1.0) / (m + 1.0); w = f * f
    p = np.full_like(f, 1.0 / 19.0)
    for c in (17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        p = p * w + 1.0 / c
    p = p * w + 1.0
    return e.astype(np.float64) * 0.69314718055994531 + 2.0 * f * p


def _smp_normal(u):
    """Inverse normal CDF (Acklam's rational approximation), same polynomials and operation order as the device."""
    a = (-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02, 1.383577518672690e+02, -3.066479806614716e+01, 2.506628277459239e+00)
    b = (-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02, 6.680131188771972e+01, -1.328068155288572e+01)
    c = (-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00, -2.549732539343734e+00, 4.374664141464968e+00, 2.938163982698783e+00)
    dd = (7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00, 3.754408661907416e+00)
    u = np.asarray(u, np.float64)
    lo = 0.02425

    def tail(p):
        q = np.sqrt(-2.0 * _det_log(p))
        return (((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5]) / ((((dd[0] * q + dd[1]) * q + dd[2]) * q + dd[3]) * q + 1.0)

    q = u - 0.5; r = q * q
    mid = (((((a[0] * r + a[1]) * r + a[2]) * r + a[3]) * r + a[4]) * r + a[5]) * q / (((((b[0] * r + b[1]) * r + b[2]) * r + b[3]) * r + b[4]) * r + 1.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        low = tail(np.where(u < lo, u, 0.5)); high = -tail(np.where(u > 1.0 - lo, 1.0 - u, 0.5))
    return np.where(u < lo, low, np.where(u > 1.0 - lo, high, mid))


def sample_scenarios(pred, prob, n_scenarios, seed):
    """Scenario sampler of SH-MPC (scenario_constraints.cpp:121-131; the scenario_module that implements it is absent -- restated from
    the call: IntegrateAndTranslateToMeanAndVariance): per solver q, obstacle m and scenario s a mode of the obstacle's Gaussian
    mixture is drawn from prob [Q][M][n_modes] and ONE standard-normal pair places the obstacle on every prediction step of that
    mode, o_k = mean_k + R(angle_k) (major_k xi1, minor_k xi2); pred [Q][M][n_modes][N][6] = (x, y, cos angle, sin angle, major, minor).
    Returns samples [Q][N][M * n_scenarios][2] -- equal bit for bit to tmpc_sample_scenarios (counter-based splitmix64 bits, inverse
    normal CDF from +, x, /, sqrt only)."""
    pred = np.asarray(pred, np.float64); prob = np.asarray(prob, np.float64)
    Q, M, n_modes, N, _ = pred.shape
    S = int(n_scenarios)
    out = np.zeros((Q, N, M * S, 2))
    mm, ss = np.meshgrid(np.arange(M), np.arange(S), indexing="ij")
    ctr = ((mm.astype(np.uint64) * np.uint64(S) + ss.astype(np.uint64)) * np.uint64(4))
    for q in range(Q):
        with np.errstate(over="ignore"):
            key = _smp_mix(np.uint64(seed) ^ _smp_mix(np.uint64(q) + np.uint64(0x51ED270B1)))
        um = _smp_uniform(key, ctr)
        mode = np.full((M, S), n_modes - 1)
        cum = np.zeros((M, 1)); done = np.zeros((M, S), bool)
        for j in range(n_modes):
            cum = cum + prob[q, :, j:j + 1]
            hit = (um < cum) & ~done
            mode[hit] = j; done |= hit
        xi1 = _smp_normal(_smp_uniform(key, ctr + np.uint64(1))); xi2 = _smp_normal(_smp_uniform(key, ctr + np.uint64(2)))
        e = pred[q][np.arange(M)[:, None], mode]                       # [M][S][N][6]
        a = e[..., 4] * xi1[..., None]; b = e[..., 5] * xi2[..., None]
        ox = (e[..., 0] + e[..., 2] * a) - e[..., 3] * b
        oy = (e[..., 1] + e[..., 3] * a) + e[..., 2] * b
        out[q, :, :, 0] = ox.transpose(2, 0, 1).reshape(N, M * S)
        out[q, :, :, 1] = oy.transpose(2, 0, 1).reshape(N, M * S)
    return out


def scenario_discard(x0, samples, radius, n_discard):
    """Scenario removal (host mirror of tmpc_scenario_discard_kernel): the n_discard scenarios with the smallest clearance
    min over obstacles m, stages k >= 1 of |o_{m,s,k-1} - p_k| - radius  from the guess (lowest scenario index on ties).
    x0 [N+1][nv]; samples [M][S][N][2].  Returns a bool mask [S] (True = discarded); they count into the bound:
    scenario_risk(S, support, removed=n_discard)."""
    M, S, N, _ = samples.shape
    p = x0[1:N, [IDX["x"], IDX["y"]]]                                  # stages 1..N-1 use prediction steps 0..N-2
    d = samples[:, :, :N - 1, :] - p[None, None]
    clear = (np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) - radius).min(axis=(0, 2))
    out = np.zeros(S, bool)
    out[np.argsort(clear, kind="stable")[:n_discard]] = True
    return out


def scenario_halfspaces(x0, samples, radius, n_rows=24, return_index=False, discard=None):
    """Per-stage polygon construction of SH-MPC (scenario_constraints.cpp:47,76-79 hand this to the external scenario_module, whose
    source is not in the reference tree; restated from the method the reference cites, README.md:22: every sampled obstacle
    position o of stage k gives the halfspace a = (o - p)/|o - p|, b = a.o - radius linearised around the previous plan's position
    p -- the linearisation LinearizedConstraints uses too, linearized_constraints.cpp:84-105 --, the free region of the stage is
    their intersection polygon, and only the halfspaces that form its boundary are constraints of the optimisation).  Exact here:
    `polygon_edges` keeps precisely the non-redundant halfspaces; if the polygon has more than n_rows edges (the solver's capacity)
    the n_rows closest to p are kept (lowest sample index on ties), unused slots stay dummies.  If the halfspaces contradict each
    other (the guess sits in the overlap of inflated discs on opposite sides: an EMPTY polygon) there is no edge; leaving the stage
    unconstrained would certify the most dangerous geometry as safe, so such a stage keeps the n_rows closest halfspaces of all samples
    (contradictory rows: the QP is infeasible or pays slack) and is reported in `empty` (advisor finding, round 2).
    x0 [N+1][nv]; samples [M][S_cen][N][2] (index k-1 for stage k).  Returns a1, a2, b [N][n_rows] with NaN = dummy; rows in order of
    increasing distance.  return_index: also the flat sample index m * S_cen + s behind each row ([N][n_rows], -1 = dummy) and
    empty [N] (bool: the stage's polygon was empty).  discard: bool [S_cen], scenarios left out (scenario_discard)."""
    N = x0.shape[0] - 1
    a1 = np.full((N, n_rows), np.nan); a2 = np.full((N, n_rows), np.nan); b = np.full((N, n_rows), np.nan)
    which = np.full((N, n_rows), -1, np.int32)
    empty = np.zeros(N, bool)
    keep = None
    if discard is not None:                                            # discarded scenarios (scenario_discard) do not exist for this trajectory
        keep = np.flatnonzero(~np.tile(np.asarray(discard, bool), samples.shape[0]))
    for k in range(1, N):
        p = x0[k, [IDX["x"], IDX["y"]]]
        o = samples[:, :, k - 1, :].reshape(-1, 2)
        if keep is not None:
            o = o[keep]
        diff = o - p
        dist = np.sqrt(diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1])
        ax = diff[:, 0] / dist; ay = diff[:, 1] / dist
        dm = dist - radius
        idx = np.nonzero(polygon_edges(ax, ay, dm))[0]
        if len(idx) == 0 and len(dm) > 0:                                  # empty polygon: the closest halfspaces of all samples
            idx = np.arange(len(dm)); empty[k] = True
        idx = idx[np.argsort(dm[idx], kind="stable")][:n_rows]             # closest first; stable: lowest sample index on ties
        m = len(idx)
        a1[k, :m] = ax[idx]; a2[k, :m] = ay[idx]
        b[k, :m] = ax[idx] * o[idx, 0] + ay[idx] * o[idx, 1] - radius
        which[k, :m] = idx if keep is None else keep[idx]
    return (a1, a2, b, which, empty) if return_index else (a1, a2, b)


def scenario_support(xtraj, params, pm, row_sample, n_scenarios, tol=1e-6, prefix="disc_0_scenario_constraint"):
    """Support of one trajectory's solution (host mirror of tmpc_scenario_support_kernel; ScenarioSolver::support,
    scenario_constraints.h:38-40, filled by the absent scenario_module -- restated from the definition of the method the reference
    cites, README.md:22): the scenarios with an active constraint  a.p_disc - (b + slack) >= -tol  at the solution, scenario of
    flat sample index i = i % n_scenarios (one scenario = one joint draw of all obstacles over the horizon).
    xtraj [N+1][nx(+1)], params [N][npar], row_sample [N][n_rows].  Returns (support, active_rows)."""
    N, n_rows = row_sample.shape
    off = params[:, pm.index("ego_disc_0_offset")]
    slack = xtraj[:N, 5] if xtraj.shape[1] > 5 else np.zeros(N)
    px = xtraj[:N, 0] + off * np.cos(xtraj[:N, 2]); py = xtraj[:N, 1] + off * np.sin(xtraj[:N, 2])
    active = set(); rows = 0
    for k in range(1, N):
        for r in range(n_rows):
            if row_sample[k, r] < 0:
                continue
            a1, a2, b = (params[k, pm.index(f"{prefix}_{r}_{f}")] for f in ("a1", "a2", "b"))
            if a1 * px[k] + a2 * py[k] - (b + slack[k]) >= -tol:
                active.add(int(row_sample[k, r]) % n_scenarios); rows += 1
    return len(active), rows


def scenario_risk(n_samples, support, confidence=1e-6, removed=0):
    """Bound on the collision probability of a plan certified by a scenario program with `n_samples` scenarios whose solution has
    `support` scenarios of support after `removed` scenarios were discarded (non-convex scenario optimisation, Campi-Garatti-Ramponi
    2018, Theorem 1, the bound SH-MPC builds on -- README.md:22; the discarded scenarios count into the compression set):
        eps(k) = 1 - (beta / (S * C(S, k)))^(1 / (S - k)),  k = support + removed,   eps(S) = 1,
    holds with probability >= 1 - beta (confidence = beta).  The reference's `probabilistic.risk` (settings.yaml) is the value this
    has to stay below."""
    from math import lgamma, log, exp
    S, k = int(n_samples), int(support) + int(removed)
    if k >= S:
        return 1.0
    log_binom = lgamma(S + 1) - lgamma(k + 1) - lgamma(S - k + 1)
    return 1.0 - exp((log(confidence) - log(S) - log_binom) / (S - k))


def scenario_sample_size(risk, confidence=1e-6, max_support=8, removed=0):
    """Smallest number of scenarios S for which a solution with at most `max_support` scenarios of support (after `removed`
    discarded ones) certifies  P(collision) <= risk  with confidence 1 - beta: the smallest S with scenario_risk(S, max_support)
    <= risk (eps decreases in S for fixed k)."""
    lo = max_support + removed + 1
    hi = lo
    while scenario_risk(hi, max_support, confidence, removed) > risk:
        hi *= 2
    while lo < hi:
        mid = (lo + hi) // 2
        if scenario_risk(mid, max_support, confidence, removed) <= risk:
            hi = mid
        else:
            lo = mid + 1
    return lo


def initialize_with_forward_propagation(state, N, dt, nv=NV):
    """Main-solver warm start: constant-velocity forward propagation of the current state (stand-in for
    the previous tick's solution used by initializeWarmstart, acados_solver_interface.cpp:344-376; same
    recursion as initializeWithBraking :303-342 with a = 0)."""
    x0 = np.zeros((N + 1, nv))
    x, y, psi, v, s = state[:5]
    for k in range(N + 1):
        x0[k, :NV] = [0.0, 0.0, x, y, psi, v, s]            # a slack state (column 7) is never initialised: 0
        x += v * dt * np.cos(psi); y += v * dt * np.sin(psi); s += v * dt
    return x0


def initialize_solver_with_guidance(x0, guidance_pos, guidance_vel):
    """GuidanceConstraints::initializeSolverWithGuidance (guidance_constraints.cpp:390-414):
    for k = 1..N-1 set x,y from the guidance spline at t = k*dt, psi = atan2(vy,vx), v = |vel|."""
    N = x0.shape[0] - 1
    for k in range(1, N):
        x0[k, IDX["x"]] = guidance_pos[k, 0]
        x0[k, IDX["y"]] = guidance_pos[k, 1]
        x0[k, IDX["psi"]] = np.arctan2(guidance_vel[k, 1], guidance_vel[k, 0])
        x0[k, IDX["v"]] = np.sqrt(guidance_vel[k, 0] ** 2 + guidance_vel[k, 1] ** 2)
    return x0


def initialize_warmstart(x0, state, xtraj_prev, utraj_prev, shift_previous_solution_forward=True):
    """Solver::initializeWarmstart (acados_solver_interface.cpp:344-376) on one solver's warm start x0 [N+1][nvar],
    in place, from its previous output (xtraj_prev [N+1][nx], utraj_prev [N][nu]).  shift = True:
    [state, out_2, ..., out_{N-1}, out_{N-1}, out_{N-1}]; the inputs of node 0 are written as 0 (the reference reads
    State::get(<input name>) there, an out-of-bounds index: state.cpp:21-24).  shift = False: x0[k] = out_k, k < N."""
    N = x0.shape[0] - 1
    nx = xtraj_prev.shape[1]
    if shift_previous_solution_forward:
        x0[0, :NU] = 0.0
        x0[0, NU:NU + nx] = state[:nx]
        for k in range(1, N + 1):
            ko = N - 1 if k >= N - 1 else k + 1
            x0[k, :NU] = utraj_prev[ko]
            x0[k, NU:NU + nx] = xtraj_prev[ko]
    else:
        for k in range(N):
            x0[k, :NU] = utraj_prev[k]
            x0[k, NU:NU + nx] = xtraj_prev[k]
    return x0


def initialize_with_braking(state, N, dt, deceleration, nv=NV):
    """Solver::initializeWithBraking (acados_solver_interface.cpp:303-342)."""
    x0 = np.zeros((N + 1, nv))
    x, y, psi, v, spline = state[:5]
    a = -abs(deceleration)
    for k in range(N + 1):
        if k >= 1:
            x += v * dt * np.cos(psi); y += v * dt * np.sin(psi); spline += v * dt
            v += a * dt; v = max(v, 0.0)
        x0[k, :NV] = [a, 0.0, x, y, psi, v, spline]
        x0[k, NV:] = state[5:]
    return x0


def map_guidance_trajectories_to_planners(planner_guidance_ids, topology_classes):
    """GuidanceConstraints::mapGuidanceTrajectoriesToPlanners (guidance_constraints.cpp:192-250), integer bookkeeping
    restated literally.  planner_guidance_ids[p] = result.guidance_ID of planner p's last solve; topology_classes[i] =
    class of guidance trajectory i.  Returns (mapping {i: p}, taken [P], existing_guidance [P]).  Note the reference's
    second loop has no `break`: the first unmatched trajectory claims every free planner (its mapping ends at the last
    one) and later unmatched trajectories get none."""
    P = len(planner_guidance_ids)
    taken = [False] * P; existing = [False] * P; mapping = {}; remaining = []
    for i, cls in enumerate(topology_classes):
        found = False
        for p in range(P):
            if planner_guidance_ids[p] == cls and not taken[p]:
                mapping[i] = p; taken[p] = True; existing[p] = True; found = True
                break
        if not found:
            remaining.append(i)
    for i in remaining:
        for p in range(P):
            if not taken[p]:
                mapping[i] = p; taken[p] = True; existing[p] = False
    return mapping, taken, existing


# ---- the guidance hand-off: host mirrors of tmpc_sample_guidance / tmpc_guidance_plan / tmpc_guidance_decide, bit for bit ------
GUIDANCE_MAX_NODES = 64
GUIDANCE_MAX_PATHS = 63


def sample_guidance(nodes, N, dt, n_nodes_max=GUIDANCE_MAX_NODES):
    """One guidance trajectory's nodes [n][3] = (t, x, y) to what initialize_solver_with_guidance reads: position and velocity [N + 1][2] at
    t = k dt (GetGuidanceTrajectory(id).spline.GetTrajectory(), guidance_constraints.cpp:390-414).  RosTools::Spline2D is not in the reference
    tree: restated as U18 -- x(t), y(t) the natural cubic splines of fit_cubic over the knots t_i; sample k on segment
    i = max{j <= n - 2 : t_j <= t}, 0 if there is none (so the first / last cubic continues outside the node span), tau = t - t_i, position
    ((a tau + b) tau + c) tau + d, velocity (3 a tau + 2 b) tau + c, no fused multiply-add.  Returns (pos, vel, status): status 1 and zero
    rows if n is outside [2, n_nodes_max] or a knot spacing is not positive and finite (path_knots_valid).  Host mirror of tmpc_sample_guidance."""
    nodes = np.asarray(nodes, float).reshape(-1, 3)
    n = len(nodes)
    pos, vel = np.zeros((N + 1, 2)), np.zeros((N + 1, 2))
    if n < 2 or n > n_nodes_max or not path_knots_valid(nodes[:, 0]):
        return pos, vel, 1
    t = nodes[:, 0]
    curves = [fit_cubic(t, nodes[:, 1]), fit_cubic(t, nodes[:, 2])]
    with np.errstate(all="ignore"):
        for k in range(N + 1):
            tk = float(k) * float(dt)
            i = 0
            for j in range(n - 1):
                if t[j] <= tk:
                    i = j
            tau = tk - float(t[i])
            for c, cur in enumerate(curves):
                a, b, cc, d = (float(x) for x in cur[i])
                pos[k, c] = ((a * tau + b) * tau + cc) * tau + d
                vel[k, c] = (3.0 * a * tau + 2.0 * b) * tau + cc
    return pos, vel, 0


def guidance_plan(traj_count, topology_class, planner_ids, selection, n_paths, use_tmpcpp=True, warmstart_with_mpc_solution=False,
                  shift_previous_solution_forward=True, selection_weight_consistency=1.0, previously_selected=None):
    """What every planner of every scene does this tick (host mirror of tmpc_guidance_plan): mapGuidanceTrajectoriesToPlanners and the
    per-planner branches of GuidanceConstraints::optimize (guidance_constraints.cpp:192-250, :283-317, :343-360) with the main solver's start
    (planner.cpp:78-86), `enable_constraints = true`.  Entry b = q P + p, P = n_paths + use_tmpcpp, the non-guided planner last; planner p
    follows trajectory p.  traj_count [Q], topology_class [Q][n_paths], previously_selected [Q][n_paths] or None; the cross-tick state
    planner_ids [Q][P] (each planner's last guidance ID, -1 at the start) and selection [Q][3] = (selected ID, selected was the non-guided
    planner, last best index; (-1, 0, -1) at the start) is read only.  Returns a dict of flat [Q P] arrays: mode / src for the warm start
    (main start: last best >= 0 ? (shift ? 1 : 2, q P + best) : (3, b); a guided, enabled planner with warmstart_with_mpc_solution and
    existing_guidance: its own solution), init_enabled (guidance initialisation), rows_dummy (non-guided or disabled), disabled,
    guidance_id (2 n_paths / class / -1), weight, and existing_guidance."""
    Q = len(traj_count)
    P = int(n_paths) + (1 if use_tmpcpp else 0)
    out = dict(mode=np.zeros(Q * P, np.int32), src=np.zeros(Q * P, np.int32), init_enabled=np.zeros(Q * P, np.uint8),
               rows_dummy=np.zeros(Q * P, np.uint8), disabled=np.zeros(Q * P, np.uint8), guidance_id=np.zeros(Q * P, np.int32),
               weight=np.ones(Q * P), existing_guidance=np.zeros(Q * P, np.uint8))
    warm_mode = 1 if shift_previous_solution_forward else 2
    for q in range(Q):
        n_traj = min(max(int(traj_count[q]), 0), int(n_paths))
        classes = [int(c) for c in topology_class[q][:n_traj]]
        _, _, existing = map_guidance_trajectories_to_planners([int(i) for i in planner_ids[q][:P]], classes)
        sel_id, sel_original, last_best = (int(v) for v in selection[q][:3])
        for p in range(P):
            b = q * P + p
            original = bool(use_tmpcpp) and p == P - 1
            disabled = p >= n_traj and not original                                   # (:286-293)
            mode, src = (warm_mode, q * P + last_best) if last_best >= 0 else (3, b)  # the copy of the main solver (planner.cpp:78-86)
            init = 0
            weight = 1.0
            if original:
                gid = 2 * int(n_paths)                                                # (:349)
            elif disabled:
                gid = -1                                                              # SolverResult::Reset
            else:
                if warmstart_with_mpc_solution and existing[p]:
                    mode, src = warm_mode, b                                          # (:310-311)
                else:
                    init = 1                                                          # (:312-313)
                gid = classes[p]
                if previously_selected is not None:
                    chosen = bool(previously_selected[q][p])
                else:
                    chosen = sel_id >= 0 and sel_original == 0 and gid == sel_id
                if chosen:
                    weight = float(selection_weight_consistency)                      # (:358-359)
            out["mode"][b], out["src"][b], out["init_enabled"][b] = mode, src, init
            out["rows_dummy"][b] = 1 if (original or disabled) else 0
            out["disabled"][b], out["guidance_id"][b], out["weight"][b] = (1 if disabled else 0), gid, weight
            out["existing_guidance"][b] = 1 if existing[p] else 0
    return out


def guidance_decide(pobj, exit_code, disabled, guidance_id, weight, state, xtraj, utraj, planner_ids, selection, n_paths, use_tmpcpp=True,
                    deceleration=3.0, control_dt=0.05, enable_output=True):
    """The decision after the solve (host mirror of tmpc_guidance_decide): FindBestPlanner (guidance_constraints.cpp:416-434) over each scene's
    P entries of the flat [Q P] arrays -- disabled skipped, success exit_code == 1, objective pobj x weight, initial value 1e10, strict '<' --,
    decide()'s exit code (:366-387: the winner's; without one planner 0's, -1 if that one is disabled), the command of
    ros1_jackalsimulator.cpp:181-201 from xtraj [Q P][N + 1][nx] / utraj [Q P][N][nu] and state [Q][nx], and the cross-tick state.
    Returns dict(best [Q], exit [Q], cmd [Q][2], planner_ids [Q][P], selection [Q][3]); the state arrays are new copies."""
    P = int(n_paths) + (1 if use_tmpcpp else 0)
    Q = len(state)
    ids = np.array(planner_ids, np.int32).reshape(Q, P).copy()
    sel = np.array(selection, np.int32).reshape(Q, 3).copy()
    best_out, exit_out, cmd = np.zeros(Q, np.int32), np.zeros(Q, np.int32), np.zeros((Q, 2))
    for q in range(Q):
        best_solution, best = 1e10, -1
        for p in range(P):
            b = q * P + p
            if disabled[b]:
                continue
            objective = float(pobj[b]) * float(weight[b])
            if int(exit_code[b]) == 1 and objective < best_solution:
                best_solution, best = objective, p
        best_out[q] = best
        if best >= 0:
            exit_out[q] = int(exit_code[q * P + best])
        else:
            exit_out[q] = -1 if disabled[q * P] else int(exit_code[q * P])
        if best >= 0 and enable_output:
            cmd[q] = (xtraj[q * P + best][1][3], utraj[q * P + best][0][1])
        else:
            w = float(state[q][3]) - float(deceleration) * float(control_dt)
            cmd[q] = (0.0 if w < 0.0 else w, 0.0)
        for p in range(P):
            ids[q, p] = int(guidance_id[q * P + p])
        if best >= 0:
            sel[q, 0] = int(guidance_id[q * P + best])
            sel[q, 1] = 1 if (use_tmpcpp and best == P - 1) else 0
        sel[q, 2] = best
    return dict(best=best_out, exit=exit_out, cmd=cmd, planner_ids=ids, selection=sel)


# ---- obstacle preparation: host mirror of mpc_planner/src/data_preparation.cpp and of tmpc_prepare_obstacles_kernel, bit for bit -----------
# An obstacle set is a dict of arrays over n obstacles: position [n][2] (the current position), pos [n][N][2], angle / major / minor [n][N]
# (mode 0 of the prediction), radius [n], gaussian [n] (bool: PredictionType::GAUSSIAN, else DETERMINISTIC).
OBSTACLE_NOISE = 0.3            # getConstantVelocityPrediction's `noise` in probabilistic mode (data_preparation.cpp:65)
OBSTACLE_KEYS = ("position", "pos", "angle", "major", "minor", "radius", "gaussian")


def define_robot_area(length, width, n_discs):
    """defineRobotArea (data_preparation.cpp:16-47): the discs that cover a length x width robot.  Returns (offsets [n_discs], radius):
    one disc sits at offset 0; otherwise the first at the back, the last at the front, the others spread evenly, every radius width / 2."""
    assert n_discs > 0, "Trying to create a collision region with less than a disc"          # (:23)
    center_offset = length / 2.0
    radius = width / 2.0
    if n_discs == 1:
        return np.array([0.0]), radius
    off = np.zeros(n_discs)
    for i in range(n_discs):
        if i == 0:
            off[i] = -center_offset + radius
        elif i == n_discs - 1:
            off[i] = -center_offset + length - radius
        else:
            off[i] = -center_offset + radius + float(i) * (length - 2.0 * radius) / (float(n_discs) - 1.0)
    return off, radius


def propagate_prediction_uncertainty(major, minor, dt):
    """propagatePredictionUncertainty (data_preparation.cpp:170-186) on one GAUSSIAN prediction: major_k = sqrt(major_{k-1}^2 + (sigma_k dt)^2)
    sequentially over k from 0, the same for minor; squares written x * x (what std::pow(x, 2.) evaluates to).  major, minor [N] -> new arrays."""
    major = np.array(major, float); minor = np.array(minor, float)
    a = 0.0; b = 0.0
    for k in range(len(major)):
        sa = major[k] * dt; sb = minor[k] * dt
        a = np.sqrt(a * a + sa * sa); b = np.sqrt(b * b + sb * sb)
        major[k] = a; minor[k] = b
    return major, minor


def constant_velocity_prediction(position, velocity, dt, steps, probabilistic=False, noise=OBSTACLE_NOISE, propagate=True):
    """getConstantVelocityPrediction (data_preparation.cpp:58-79): step i = position + (velocity dt) i, angle 0, major = minor = noise
    (0 unless probabilistic, :61-66); GAUSSIAN iff probabilistic, and then one propagatePredictionUncertainty pass (:75-76; propagate=False
    leaves it to the caller, as prepare_obstacles counts the passes itself).  Returns dict(pos [steps][2], angle, major, minor [steps], gaussian)."""
    position = np.asarray(position, float); velocity = np.asarray(velocity, float)
    i = np.arange(steps, dtype=float)[:, None]
    sigma = float(noise) if probabilistic else 0.0
    major = np.full(steps, sigma); minor = np.full(steps, sigma)
    if probabilistic and propagate:
        major, minor = propagate_prediction_uncertainty(major, minor, dt)
    return dict(pos=position[None, :] + (velocity[None, :] * dt) * i, angle=np.zeros(steps), major=major, minor=minor,
                gaussian=bool(probabilistic))


def _take_obstacles(obs, idx):
    return {k: np.asarray(obs[k])[idx] for k in OBSTACLE_KEYS}


def remove_distant_obstacles(obs, state, max_obstacle_distance):
    """removeDistantObstacles (data_preparation.cpp:81-93): keeps the obstacles whose CURRENT position is closer to the robot than
    max_obstacle_distance (strict '<'), in their order.  Returns (obstacle set, kept indices)."""
    dx = np.asarray(obs["position"], float)[:, 0] - state[0]; dy = np.asarray(obs["position"], float)[:, 1] - state[1]
    keep = np.flatnonzero(np.sqrt(dx * dx + dy * dy) < max_obstacle_distance)
    return _take_obstacles(obs, keep), keep


def obstacle_selection_distance(pred_pos, state):
    """The ranking key of ensureObstacleSize (data_preparation.cpp:113-131) for predictions pred_pos [n][N][2] and state (x, y, psi, v):
    min over k < N of ((k + 1) 0.6) |pred_k - (p + (v k) (cos psi, sin psi))|, starting from min_dist = 1e5.  `v k` carries no dt in the
    reference; kept."""
    pred_pos = np.asarray(pred_pos, float)
    n, N, _ = pred_pos.shape
    c, s = np.cos(state[2]), np.sin(state[2])
    out = np.full(n, 1e5)
    for k in range(N):
        vk = state[3] * float(k)
        dx = pred_pos[:, k, 0] - (state[0] + vk * c); dy = pred_pos[:, k, 1] - (state[1] + vk * s)
        dist = (float(k + 1) * 0.6) * np.sqrt(dx * dx + dy * dy)
        out = np.where(dist < out, dist, out)
    return out


def ensure_obstacle_size(obs, state, max_obstacles, dt, probabilistic=False, noise=OBSTACLE_NOISE):
    """ensureObstacleSize (data_preparation.cpp:95-168): exactly max_obstacles obstacles.  More: the max_obstacles with the smallest
    obstacle_selection_distance, in ascending order of it (:104-150) -- std::sort leaves ties unspecified, here the lower index wins
    (DESIGN.md U13).  Fewer: the obstacles in their order, then dummies (getDummyObstacle, :49-56: position (x + 100, y + 100), radius 0)
    with the constant-velocity prediction of zero velocity (:155-164; its uncertainty pass is left to the caller).
    Returns (obstacle set, selected [max_obstacles]: index into `obs`, -1 = dummy)."""
    n = len(obs["radius"]); M = int(max_obstacles)
    N = np.asarray(obs["pos"]).shape[1]
    if n > M:
        dist = obstacle_selection_distance(obs["pos"], state)
        sel = np.lexsort((np.arange(n), dist))[:M]                   # by distance, then index
        return _take_obstacles(obs, sel), sel.astype(np.int32)
    out = _take_obstacles(obs, np.arange(n))
    out = {k: np.array(v) for k, v in out.items()}
    for _ in range(M - n):
        p = np.array([state[0] + 100.0, state[1] + 100.0])
        cv = constant_velocity_prediction(p, np.zeros(2), dt, N, probabilistic, noise, propagate=False)
        out["position"] = np.concatenate([out["position"].reshape(-1, 2), p[None]])
        out["radius"] = np.concatenate([out["radius"], [0.0]])
        out["gaussian"] = np.concatenate([out["gaussian"].astype(bool), [cv["gaussian"]]])
        for key in ("pos", "angle", "major", "minor"):
            out[key] = np.concatenate([out[key].reshape((-1,) + cv[key].shape), cv[key][None]])
    return out, np.concatenate([np.arange(n), np.full(M - n, -1)]).astype(np.int32)


def prepare_obstacles(state, raw_pos, raw_radius, M, N, dt, raw_vel=None, raw_pred=None, probabilistic=False, noise=OBSTACLE_NOISE,
                      propagate_passes=0, max_obstacle_distance=0.0, risk=0.05):
    """What a wrapper's obstacle callback does before Planner::solveMPC, for one scene (host mirror of tmpc_prepare_obstacles, bit for bit):
    predictions -- constant velocity from raw_vel [n][2] (ros1_jackal.cpp:324-329) or given, raw_pred [n][N][5] = (x, y, angle, major,
    minor), GAUSSIAN iff probabilistic and the last step's major != 0 (ros1_jackalsimulator.cpp:331-334) --, the optional distance filter
    (removeDistantObstacles; no shipped wrapper calls it: off for max_obstacle_distance <= 0), ensureObstacleSize to exactly M, and
    propagate_passes propagatePredictionUncertainty passes over the GAUSSIAN predictions (dummies included).  Two passes is what
    ros1_jackal.cpp:324-332 does in probabilistic mode (one inside getConstantVelocityPrediction, one in the wrapper), one is
    ros1_jackalsimulator.cpp:345-346.  state = (x, y, psi, v).
    Returns the dict ellipsoid_set_parameters / gaussian_set_parameters take -- pos [M][N][2], angle, major, minor [M][N], radius [M],
    chi [M]; a DETERMINISTIC obstacle carries major = minor = 0, chi = 1 (ellipsoid_constraints.cpp:72-77), a GAUSSIAN one
    chi = -log(risk) / 0.5 (ExponentialQuantile(0.5, 1 - risk), :80) -- plus selected [M] (raw index, -1 = dummy), gaussian [M] and
    shape [M][N][3] = (angle, major, minor) as predicted, whatever the type (the device's d_obstacle_shape)."""
    assert (raw_vel is None) != (raw_pred is None), "exactly one of raw_vel / raw_pred"
    raw_pos = np.asarray(raw_pos, float).reshape(-1, 2); raw_radius = np.asarray(raw_radius, float).reshape(-1)
    n = len(raw_radius)
    obs = dict(position=raw_pos, pos=np.zeros((n, N, 2)), angle=np.zeros((n, N)), major=np.zeros((n, N)), minor=np.zeros((n, N)),
               radius=raw_radius, gaussian=np.zeros(n, bool))
    for j in range(n):
        if raw_vel is not None:
            cv = constant_velocity_prediction(raw_pos[j], np.asarray(raw_vel, float)[j], dt, N, probabilistic, noise, propagate=False)
            for key in ("pos", "angle", "major", "minor"):
                obs[key][j] = cv[key]
            obs["gaussian"][j] = cv["gaussian"]
        else:
            pr = np.asarray(raw_pred, float)[j]
            obs["pos"][j] = pr[:, 0:2]; obs["angle"][j] = pr[:, 2]; obs["major"][j] = pr[:, 3]; obs["minor"][j] = pr[:, 4]
            obs["gaussian"][j] = bool(probabilistic) and pr[N - 1, 3] != 0.0
    raw_index = np.arange(n)
    if max_obstacle_distance > 0.0:
        obs, raw_index = remove_distant_obstacles(obs, state, max_obstacle_distance)
    obs, sel = ensure_obstacle_size(obs, state, M, dt, probabilistic, noise)
    selected = np.where(sel >= 0, raw_index[np.maximum(sel, 0)] if len(raw_index) else -1, -1).astype(np.int32)
    major = np.array(obs["major"], float); minor = np.array(obs["minor"], float)
    gauss = np.asarray(obs["gaussian"], bool)
    for _ in range(int(propagate_passes)):
        for j in range(M):
            if gauss[j]:
                major[j], minor[j] = propagate_prediction_uncertainty(major[j], minor[j], dt)
    shape = np.stack([np.asarray(obs["angle"], float), major, minor], 2)
    live = gauss[:, None]
    return dict(pos=np.asarray(obs["pos"], float), angle=np.asarray(obs["angle"], float), radius=np.asarray(obs["radius"], float),
                major=np.where(live, major, 0.0), minor=np.where(live, minor, 0.0),
                chi=np.where(gauss, -np.log(risk) / 0.5, 1.0), selected=selected, gaussian=gauss, shape=shape)


# ---- Contouring::update on a whole reference path: closest point, segment window (contouring.cpp:28-48, :94-124) -------------------------
# RosTools::Spline2D is not in the reference tree: the search is restated, its assumptions are DESIGN.md U14.  Host mirrors of
# tmpc_track_path_kernel (csrc/tmpc_aux_kernels.hpp) and of mpc_planner_modules/reference_path.h, bit for bit: plain IEEE doubles, no
# fused multiply-add, the operation order below.

PATH_COARSE = 8          # coarse samples per segment: t_j = L (j / 8), j = 0 .. 8
PATH_BISECTIONS = 40     # fixed: no data-dependent exit, every lane of a wave does the same work


def _path_cubic(c, t):
    """Point and derivative of one 2-D cubic c = (ax bx cx dx ay by cy dy) at t, the Horner forms of _road_segment_eval."""
    px = ((c[0] * t + c[1]) * t + c[2]) * t + c[3]
    py = ((c[4] * t + c[5]) * t + c[6]) * t + c[7]
    dx = (3.0 * c[0] * t + 2.0 * c[1]) * t + c[2]
    dy = (3.0 * c[4] * t + 2.0 * c[5]) * t + c[6]
    return px, py, dx, dy


def _path_segment_length(path, length, i):
    """L_i = start_{i+1} - start_i; the last segment ends at `length`, the knot behind it."""
    return (float(path[i + 1][8]) if i + 1 < len(path) else float(length)) - float(path[i][8])


def closest_point_on_segment(c, L, px, py):
    """(D, t): the closest point of the cubic c on t in [0, L] to (px, py), D = |P(t) - p|^2, g(t) = (P(t) - p).P'(t).  Nine coarse samples
    t_j = L (j / 8); j* = argmin D(t_j), lowest j on ties; bracket [t_{max(j*-1, 0)}, t_{min(j*+1, 8)}]; g(lo) >= 0: t = lo, else g(hi) <= 0:
    t = hi, else exactly 40 bisections on the sign of g and the bracket's midpoint; the coarse sample wins if its D is strictly smaller."""
    c = [float(v) for v in c]; L = float(L); px = float(px); py = float(py)

    def D_g(t):
        x, y, dx, dy = _path_cubic(c, t)
        ex, ey = x - px, y - py
        return ex * ex + ey * ey, ex * dx + ey * dy

    tj = [L * (j / 8.0) for j in range(PATH_COARSE + 1)]
    js, Dj = 0, D_g(tj[0])[0]
    for j in range(1, PATH_COARSE + 1):
        Dc = D_g(tj[j])[0]
        if Dc < Dj:
            js, Dj = j, Dc
    lo, hi = tj[max(js - 1, 0)], tj[min(js + 1, PATH_COARSE)]
    if D_g(lo)[1] >= 0.0:
        tc = lo
    elif D_g(hi)[1] <= 0.0:
        tc = hi
    else:
        for _ in range(PATH_BISECTIONS):
            mid = 0.5 * (lo + hi)
            if D_g(mid)[1] > 0.0:
                hi = mid
            else:
                lo = mid
        tc = 0.5 * (lo + hi)
    Dc = D_g(tc)[0]
    if Dj < Dc:
        return Dj, tj[js]
    return Dc, tc


def find_closest_point(path, length, pos, segment=-1, search_range=2):
    """RosTools::Spline2D::findClosestPoint as Contouring::update uses it (contouring.cpp:37).  path [n][9] =
    (ax bx cx dx ay by cy dy start), `length` the knot behind the last segment.  segment < 0 (a new path, a reset): every segment is a
    candidate; otherwise [max(0, prev - R), min(n - 1, prev + R)] with prev = segment clamped into [0, n - 1] and R = search_range.  The
    comparison starts from the first candidate and replaces on strict `<`: the lowest segment index wins a tie (the convention of U13), and
    a NaN / inf position yields the first candidate, never an index out of range.  Returns (segment, s = start_segment + t)."""
    path = np.asarray(path, float)
    n = len(path)
    assert n > 0 and 0 <= int(search_range) <= 31
    if int(segment) < 0:
        first, last = 0, n - 1
    else:
        prev = min(max(int(segment), 0), n - 1)
        first, last = max(0, prev - int(search_range)), min(n - 1, prev + int(search_range))
    best_i, best_D, best_t = first, None, 0.0
    for i in range(first, last + 1):
        D, t = closest_point_on_segment(path[i, :8], _path_segment_length(path, length, i), pos[0], pos[1])
        if best_D is None or D < best_D:
            best_i, best_D, best_t = i, D, t
    return best_i, float(path[best_i, 8]) + best_t


def _path_end(coef, L_last):
    """Point and tangent at the end of a path: its last cubic at t = L_last."""
    return _path_cubic([float(v) for v in coef[-1][:8]], float(L_last))


def path_window(path, length, segment, S, left=None, right=None):
    """The S segments Contouring::setSplineParameters writes from `segment` on (contouring.cpp:94-124): slot w holds
    segment + w as given; a slot beyond the last segment continues the path STRAIGHT ALONG ITS END TANGENT -- (0, 0, x'(end), X(end), 0, 0,
    y'(end), Y(end)), start = length, from the last cubic at t = L_last -- so that |path'| never vanishes.  left, right [n][8]: the bound
    cubics on the same knots, windowed and padded the same way from their own last cubics.
    Returns window [S][9], or (window, left_window [S][8], right_window [S][8]) with bounds."""
    path = np.asarray(path, float)
    n = len(path)
    L_last = _path_segment_length(path, length, n - 1)

    def pad(coef):
        x, y, dx, dy = _path_end(coef, L_last)
        return [0.0, 0.0, dx, x, 0.0, 0.0, dy, y]

    window = np.zeros((S, 9))
    sides = [None if b is None else np.asarray(b, float) for b in (left, right)]
    side_windows = [None if b is None else np.zeros((S, 8)) for b in sides]
    for w in range(S):
        i = int(segment) + w
        if i < n:
            window[w] = path[i]
        else:
            window[w, :8] = pad(path); window[w, 8] = float(length)
        for b, bw in zip(sides, side_windows):
            if b is not None:
                bw[w] = b[i, :8] if i < n else pad(b)
    if left is None and right is None:
        return window
    return window, side_windows[0], side_windows[1]


def path_objective_reached(path, length, pos):
    """Contouring::isObjectiveReached (contouring.cpp:167-175): |p - P(length)| < 1.0."""
    path = np.asarray(path, float)
    x, y, _, _ = _path_end(path, _path_segment_length(path, length, len(path) - 1))
    ex, ey = x - float(pos[0]), y - float(pos[1])
    return bool(np.sqrt(ex * ex + ey * ey) < 1.0)


def track_path(path, length, pos, S, segment=-1, search_range=2, left=None, right=None):
    """One tick of Contouring::update on a whole path, for one scene (host mirror of tmpc_track_path): find_closest_point, path_window from
    the segment found, the objective-reached flag.  Returns dict(segment, s, window [S][9], reached, and left / right [S][8] with bounds)."""
    seg, s = find_closest_point(path, length, pos, segment, search_range)
    out = dict(segment=seg, s=s, reached=path_objective_reached(path, length, pos))
    if left is None and right is None:
        out["window"] = path_window(path, length, seg, S)
    else:
        out["window"], out["left"], out["right"] = path_window(path, length, seg, S, left, right)
    return out


# ---- Contouring::onDataReceived / PathReferenceVelocity::onDataReceived: waypoints -> cubic segments (contouring.cpp:126-157, ------------
# path_reference_velocity.cpp:28-40).  RosTools::Spline2D and tk::spline are not in the reference tree: the natural cubic spline is restated
# as DESIGN.md U15.  Host mirrors of tmpc_fit_path_kernel (csrc/tmpc_aux_kernels.hpp) and of ReferencePathSpline::fit
# (mpc_planner_modules/reference_path.h), bit for bit: plain IEEE doubles, no fused multiply-add, the operation order below.

PATH_FIT_MAX_POINTS = 1025


def path_knots(xy, s=None):
    """The knots t_0 .. t_{n-1} of n waypoints xy [n][2] (U15): the given s as supplied (not shifted), else the chord lengths accumulated
    strictly left to right, t_0 = 0, t_{i+1} = t_i + sqrt(dx dx + dy dy) -- a loop, not a scan: a parallel prefix sum rounds differently."""
    xy = np.asarray(xy, float).reshape(-1, 2)
    n = len(xy)
    if s is not None:
        return np.array(np.asarray(s, float).reshape(-1)[:n], float)
    t = np.zeros(n)
    with np.errstate(all="ignore"):
        d = xy[1:] - xy[:-1]
        chord = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
        for i in range(1, n):
            t[i] = t[i - 1] + chord[i - 1]
    return t


def path_knots_valid(knots):
    """U15: at least two knots, and every h_i = t_{i+1} - t_i satisfies h_i > 0 && h_i < inf (false for a duplicate waypoint, a
    non-increasing s, NaN and inf: tk::spline asserts there)."""
    t = np.asarray(knots, float)
    if len(t) < 2:
        return False
    with np.errstate(all="ignore"):
        h = t[1:] - t[:-1]
        return bool(np.all((h > 0.0) & (h < np.inf)))


def fit_cubic(knots, values):
    """The natural cubic spline through (t_i, y_i), second derivative zero at both ends, as [n-1][4] = (a, b, c, d) of
    ((a t + b) t + c) t + d on t = s - t_i (U15).  The tridiagonal system for the half second derivatives m_i (m_0 = m_{n-1} = 0) by the
    Thomas recurrence without pivoting -- rows (h_{i-1} / 3, 2 (h_{i-1} + h_i) / 3, h_i / 3), strictly diagonally dominant --, forward
    i = 1 .. n-2, back i = n-2 .. 1.  Two points: the straight line.  Raises ValueError on invalid knots (path_knots_valid)."""
    t = np.asarray(knots, float).reshape(-1)
    y = np.asarray(values, float).reshape(-1)
    n = len(t)
    if len(y) != n:
        raise ValueError("fit_cubic: one value per knot")
    if not path_knots_valid(t):
        raise ValueError("fit_cubic: fewer than two knots, or a knot spacing that is not positive and finite")
    with np.errstate(all="ignore"):
        h = t[1:] - t[:-1]
        up = h / 3.0                                                     # up_i; lo_i = up_{i-1}
        di = (2.0 * (h[:-1] + h[1:])) / 3.0                              # di_i at [i - 1]
        slope = (y[1:] - y[:-1]) / h
        r = slope[1:] - slope[:-1]                                       # r_i at [i - 1]
        cp, g, m = np.zeros(n), np.zeros(n), np.zeros(n)
        for i in range(1, n - 1):
            lo = up[i - 1]
            den = di[i - 1] - lo * cp[i - 1]
            cp[i] = up[i] / den
            g[i] = (r[i - 1] - lo * g[i - 1]) / den
        for i in range(n - 2, 0, -1):
            m[i] = g[i] - cp[i] * m[i + 1]
        out = np.zeros((n - 1, 4))
        out[:, 0] = (m[1:] - m[:-1]) / (3.0 * h)
        out[:, 1] = m[:-1]
        out[:, 2] = slope - ((2.0 * m[:-1] + m[1:]) * h) / 3.0
        out[:, 3] = y[:-1]
    return out


def fit_path(xy, s=None, left=None, right=None, v=None):
    """One scene of tmpc_fit_path (host mirror; Contouring::onDataReceived, contouring.cpp:126-157, and PathReferenceVelocity::onDataReceived,
    path_reference_velocity.cpp:28-40): the centreline through xy [n][2] on path_knots(xy, s); the bound curves through left / right [n][2]
    (both or neither) and the velocity curve through v [n] on the CENTRELINE's knots (getTVector(), set_points(s, v)), so they must have
    the centreline's point count; road_width = sqrt(ex ex + ey ey) between the bounds' first waypoints (:152).
    Returns dict(path [n-1][9] = (ax bx cx dx ay by cy dy start), count = n - 1, length = t_{n-1}, left, right [n-1][8] or None, velocity
    [n-1][4] or None, road_width or None, status).  An invalid scene (n < 2, or a knot spacing that is not positive and finite): count 0,
    status 1, arrays of zero rows, length / road_width None -- the device writes nothing else of such a scene."""
    xy = np.asarray(xy, float).reshape(-1, 2)
    n = len(xy)
    if (left is None) != (right is None):
        raise ValueError("fit_path: left and right go together (both or neither)")
    if n > PATH_FIT_MAX_POINTS:
        raise ValueError("fit_path: at most 1025 waypoints")
    sides = None if left is None else [np.asarray(b, float).reshape(-1, 2) for b in (left, right)]
    vel = None if v is None else np.asarray(v, float).reshape(-1)
    if (sides is not None and any(len(b) != n for b in sides)) or (vel is not None and len(vel) != n) or (s is not None and len(np.asarray(s).reshape(-1)) < n):
        raise ValueError("fit_path: bounds, velocity and s need the centreline's point count")
    t = path_knots(xy, s)
    if not path_knots_valid(t):
        return dict(path=np.zeros((0, 9)), count=0, length=None, left=None if sides is None else np.zeros((0, 8)),
                    right=None if sides is None else np.zeros((0, 8)), velocity=None if vel is None else np.zeros((0, 4)), road_width=None, status=1)
    path = np.concatenate([fit_cubic(t, xy[:, 0]), fit_cubic(t, xy[:, 1]), t[:-1, None]], 1)
    out = dict(path=path, count=n - 1, length=float(t[-1]), left=None, right=None, velocity=None, road_width=None, status=0)
    if sides is not None:
        out["left"], out["right"] = [np.concatenate([fit_cubic(t, b[:, 0]), fit_cubic(t, b[:, 1])], 1) for b in sides]
        with np.errstate(all="ignore"):
            ex, ey = sides[0][0, 0] - sides[1][0, 0], sides[0][0, 1] - sides[1][0, 1]
            out["road_width"] = float(np.sqrt(ex * ex + ey * ey))
    if vel is not None:
        out["velocity"] = fit_cubic(t, vel)
    return out


def path_velocity_window(velocity, count, segment, S, reference_velocity):
    """PathReferenceVelocity::setParameters (path_reference_velocity.cpp:59-95) for stacks that carry the spline_v{i}_{a..d} columns
    (codegen.stacks.contouring_path_velocity_ellipsoids): [S][4], slot w = velocity segment `segment + w` (velocity [count][4] as
    fit_path returns it); a slot beyond the last segment is (0, 0, 0, 0) -- "brake at the end"; without a profile (velocity None) every
    slot is (0, 0, 0, reference_velocity).  Host mirror of tmpc_path_velocity_window, which clamps the segment into [0, count - 1] first
    and also takes count <= 0 or a cleared flag for "no profile": pass a segment inside the path, and None for such a scene."""
    out = np.zeros((S, 4))
    if velocity is None:
        out[:, 3] = float(reference_velocity)
        return out
    velocity = np.asarray(velocity, float).reshape(-1, 4)
    for w in range(S):
        i = int(segment) + w
        if 0 <= i < int(count):
            out[w] = velocity[i]
    return out


def path_velocity_at(velocity, path, count, length, s, reference_velocity):
    """The velocity reference at path parameter s: what GuidanceConstraints::update hands to the guidance planner,
    path_velocity(state.spline) (guidance_constraints.cpp:91-94), else CONFIG reference_velocity.  tk::spline::operator() is not in the
    reference tree: restated as DESIGN.md U17.  velocity [count][4] and path [count][9] as fit_path returns them.  Segment
    i = max{j <= count - 1 : start_j <= s}, 0 if there is none (the lookup of U12); t = s - start_i; ((a t + b) t + c) t + d, no fused
    multiply-add.  At s >= length the last cubic continues (`length` is not read: tk::spline extrapolates there, and closest_s never
    exceeds it).  Without a profile (velocity None or count <= 0): reference_velocity.  Host mirror of tmpc_path_velocity_window's d_v_ref."""
    if velocity is None or int(count) <= 0:
        return float(reference_velocity)
    velocity = np.asarray(velocity, float).reshape(-1, 4)
    path = np.asarray(path, float).reshape(-1, 9)
    s = float(s)
    i = 0
    for j in range(int(count)):
        if path[j, 8] <= s:
            i = j
    a, b, c, d = (float(x) for x in velocity[i])
    with np.errstate(all="ignore"):
        t = s - float(path[i, 8])
        return ((a * t + b) * t + c) * t + d


def scatter_parameters(params, cols, values, scene_of, per_stage=False):
    """Caller-chosen columns of parameter rows, in place (host mirror of tmpc_scatter_parameters): params [B][N][npar]; cols distinct column
    numbers in [0, npar); values [n_scenes][n_cols] into every stage of every entry b with scene_of[b] inside [0, n_scenes), or with
    per_stage values [n_scenes][N][n_cols], stage k from row k.  Other entries and other columns are left alone."""
    cols = [int(c) for c in cols]
    B, N, npar = params.shape
    if not 1 <= len(cols) <= 128 or len(set(cols)) != len(cols) or min(cols) < 0 or max(cols) >= npar:
        raise ValueError("scatter_parameters: 1 .. 128 distinct columns inside [0, npar)")
    values = np.asarray(values, float)
    n_scenes = values.shape[0]
    values = values.reshape(n_scenes, N, len(cols)) if per_stage else values.reshape(n_scenes, 1, len(cols))
    for b in range(B):
        q = int(scene_of[b])
        if 0 <= q < n_scenes:
            for k in range(N):
                row = values[q, k if per_stage else 0]
                for c, col in enumerate(cols):
                    params[b, k, col] = row[c]


def path_velocity_set_parameters(pm, params, window):
    """The spline_v{i}_{a..d} columns of every stage from path_velocity_window's [S][4] (setSolverParameterSplineVA .. VD, :80-83)."""
    for i in range(len(window)):
        for w, k in enumerate("abcd"):
            params[:, pm.index(f"spline_v{i}_{k}")] = window[i, w]


# ---- DecompConstraints::update on a costmap: occupied cells, path polyline, one convex polygon per segment (decomp_constraints.cpp:52-148) ----
# DecompUtil is not in the reference tree: upstream DecompUtil's LineSegment algorithm restated in the frame of the segment, assumptions in
# DESIGN.md U16.  Host mirrors of tmpc_costmap_points_kernel / tmpc_decomp_halfspaces_kernel (csrc/tmpc_aux_kernels.hpp) and of
# mpc_planner_modules/free_space.h, bit for bit: plain IEEE doubles, no fused multiply-add, the operation order below (tmpc_arith's decomp_*).

DECOMP_EPS = 1e-10           # DecompUtil's epsilon_
DECOMP_TERMINATOR = 1e-3     # a row with a shorter normal (or NaN) ends the copy (decomp_constraints.cpp:98)
DECOMP_MAX_POINTS = 16384
COSTMAP_FREE_SPACE = 0       # costmap_2d::FREE_SPACE


def costmap_points(cost, origin, resolution, n_pts_max=None):
    """getOccupiedGridCells (decomp_constraints.cpp:122-148): cost u8 [size_y][size_x] (costmap_2d: index my * size_x + mx); every cell whose
    cost is not FREE_SPACE (0) becomes its centre (origin_x + (mx + 0.5) resolution, origin_y + (my + 0.5) resolution), mx outer, my inner.
    n_pts_max: keep the first n_pts_max.  Returns (points [count][2], count, overflow)."""
    cost = np.asarray(cost)
    mx, my = np.nonzero(cost.T != COSTMAP_FREE_SPACE)                    # row-major over [size_x][size_y]: mx outer, my inner
    total = len(mx)
    if n_pts_max is not None:
        mx, my = mx[:n_pts_max], my[:n_pts_max]
    pts = np.stack([float(origin[0]) + (mx.astype(float) + 0.5) * float(resolution),
                    float(origin[1]) + (my.astype(float) + 0.5) * float(resolution)], 1)
    return pts, len(pts), bool(total > len(pts))


def decomp_path_points(path, length, s0, v, dt):
    """The polyline of DecompConstraints::update (:68-82): P(s_k), k < len(v), s_0 = s0, s_{k+1} = s_k + v_k dt accumulated left to right, on
    a whole path [n][9] as fit_path returns it.  Segment i = max{j : start_j <= s} (0 below the first knot), the cubic at t = s - start_i;
    for s >= length the path continues straight along its end tangent, P(length) + (s - length) P'(length) from the last cubic at
    t = L_last (U14-3).  Returns (points [len(v)][2], s [len(v)])."""
    path = np.asarray(path, float)
    n = len(path)
    length = float(length)
    ex, ey, edx, edy = _path_end(path, _path_segment_length(path, length, n - 1))
    pts = np.zeros((len(v), 2)); ss = np.zeros(len(v))
    s = float(s0)
    with np.errstate(all="ignore"):
        for k in range(len(v)):
            ss[k] = s
            if s >= length:
                pts[k] = (ex + (s - length) * edx, ey + (s - length) * edy)
            else:
                i = 0
                for j in range(n):
                    if path[j, 8] <= s:
                        i = j
                x, y, _, _ = _path_cubic([float(c) for c in path[i, :8]], s - float(path[i, 8]))
                pts[k] = (x, y)
            s = s + float(v[k]) * float(dt)
    return pts, ss


def _decomp_argmin(key, members):
    """The argmin rule: the smallest key (NaN counts as +inf), the lowest point index among equal keys; members: ascending indices."""
    k = key[members]
    return int(members[int(np.argmin(np.where(k == k, k, np.inf)))])


def decomp_segment(p1, p2, points, R, n_rows, state_x=0.0):
    """One segment of EllipsoidDecomp2D::dilate + set_constraints as DecompConstraints::update copies it (:83-114): the rows
    A p <= b of the convex polygon around p1 -> p2 among `points` [m][2], at most n_rows obstacle rows followed by the four rows of the
    local box of half width R.  Returns (rows [n_rows][3], count, status): rows i < count as found, the rest the dummy (1, 0, state_x + 100);
    status 0 complete, 1 truncated (more rows found than n_rows), 2 degenerate (an invalid segment, or a row with |A_i| < 1e-3 or NaN ended
    the copy early)."""
    p1x, p1y, p2x, p2y = float(p1[0]), float(p1[1]), float(p2[0]), float(p2[1])
    o = np.asarray(points, float).reshape(-1, 2)
    R = float(R)
    out = np.zeros((n_rows, 3)); out[:] = (1.0, 0.0, float(state_x) + 100.0)
    with np.errstate(all="ignore"):
        dx, dy = p2x - p1x, p2y - p1y
        ln = float(np.sqrt(dx * dx + dy * dy))
        if not (ln > 0.0 and ln < np.inf):
            return out, 0, 2
        ex, ey = dx / ln, dy / ln
        cx, cy = (p1x + p2x) / 2.0, (p1y + p2y) / 2.0
        f = ln / 2.0
        rx, ry = o[:, 0] - cx, o[:, 1] - cy
        u = rx * ex + ry * ey
        w = rx * ey - ry * ex
        box = (np.abs(w) <= R + DECOMP_EPS) & (np.abs(u) <= f + R + DECOMP_EPS)
        a = b = f

        def d2():
            ua, wb = u / a, w / b
            return ua * ua + wb * wb

        inside = box & (np.sqrt(d2()) <= 1.0)
        while inside.any():
            j = _decomp_argmin(d2(), np.nonzero(inside)[0])
            if u[j] < a:
                ua = u[j] / a
                b = float(abs(w[j]) / np.sqrt(1.0 - ua * ua))
            inside &= (1.0 - np.sqrt(d2()) > DECOMP_EPS)
            inside[j] = False
        found = []
        left = box.copy()
        key = d2()
        while left.any() and len(found) < n_rows:
            j = _decomp_argmin(key, np.nonzero(left)[0])
            gu, gw = u[j] / (a * a), w[j] / (b * b)
            nrm = np.sqrt(gu * gu + gw * gw)
            nu, nw = gu / nrm, gw / nrm
            nx, ny = nu * ex + nw * ey, nu * ey - nw * ex
            beta = nx * o[j, 0] + ny * o[j, 1]
            left &= (nx * (o[:, 0] - o[j, 0]) + ny * (o[:, 1] - o[j, 1]) < 0.0)
            left[j] = False
            if nx * cx + ny * cy - beta > 0.0:
                nx, ny, beta = -nx, -ny, -beta
            found.append((nx, ny, beta))
        hx, hy = ey, -ex
        found.append((hx, hy, hx * (p1x + hx * R) + hy * (p1y + hy * R)))
        found.append((-hx, -hy, -(hx * (p1x - hx * R) + hy * (p1y - hy * R))))
        found.append((ex, ey, ex * (p2x + ex * R) + ey * (p2y + ey * R)))
        found.append((-ex, -ey, -(ex * (p1x - ex * R) + ey * (p1y - ey * R))))
        limit = min(len(found), n_rows)
        count = 0
        while count < limit:
            a1, a2, _ = found[count]
            if np.sqrt(a1 * a1 + a2 * a2) < DECOMP_TERMINATOR or a1 != a1:
                break
            out[count] = found[count]
            count += 1
    return out, count, (2 if count < limit else (1 if len(found) > n_rows else 0))


def decomp_halfspaces(path, length, s0, v, dt, points, R, n_rows, state_x=0.0):
    """DecompConstraints::update for one scene (host mirror of tmpc_decomp_halfspaces): the polyline decomp_path_points(path, length, s0,
    v[:N], dt) of N = len(v) points, segment k into stage k + 1 by decomp_segment, stage 0 all dummies with count 0 and status 0.
    Returns dict(rows [N][n_rows][3], count [N] i32, status [N] u8, and a1, a2, b [N][n_rows] with NaN where a row is a dummy -- what
    halfspace_rows_set_parameters takes)."""
    N = len(v)
    pts, _ = decomp_path_points(path, length, s0, v, dt)
    rows = np.zeros((N, n_rows, 3)); rows[:] = (1.0, 0.0, float(state_x) + 100.0)
    count = np.zeros(N, np.int32); status = np.zeros(N, np.uint8)
    for k in range(N - 1):
        rows[k + 1], count[k + 1], status[k + 1] = decomp_segment(pts[k], pts[k + 1], points, R, n_rows, state_x)
    live = np.arange(n_rows)[None, :] < count[:, None]
    nan = lambda x: np.where(live, x, np.nan)
    return dict(rows=rows, count=count, status=status, a1=nan(rows[:, :, 0]), a2=nan(rows[:, :, 1]), b=nan(rows[:, :, 2]))


# ---- the episode step: host mirror of tmpc_episode_step_kernel and of mpc_planner/episode.h, bit for bit ------------------
# The world of a closed loop for ONE scene: a velocity-commanded unicycle, obstacles that move at constant velocity and bounce inside a box,
# the intrusion measure, and the bookkeeping of JackalPlanner::loop / reset (ros1_jackalsimulator.cpp:146-226, :359-378), Planner::reset
# (planner.cpp:231-245) and ExperimentUtil::update / onTaskComplete (experiment_util.cpp:27-110).  Scalar by scalar on Python floats (IEEE
# doubles, no fused multiply-add, a correctly rounded sqrt) in the kernel's operation order.


def _small_angle(a):
    """(sin a, cos a, sin a / a) for |a| <= 1/16: fixed Horner polynomials in a^2 through a^9, a^10 and a^8; sin a = a (sin a / a)."""
    z = a * a
    sinc = (((z * (1.0 / 362880.0) + (-1.0 / 5040.0)) * z + (1.0 / 120.0)) * z + (-1.0 / 6.0)) * z + 1.0
    cs = ((((z * (-1.0 / 3628800.0) + (1.0 / 40320.0)) * z + (-1.0 / 720.0)) * z + (1.0 / 24.0)) * z + (-1.0 / 2.0)) * z + 1.0
    return a * sinc, cs, sinc


def plant_substep(p, cmd_v, cmd_w, h, max_acceleration, max_angular_velocity):
    """One substep h of the plant p = (x, y, psi, v, c, s) -> the new six floats: w clipped by two comparisons (a NaN passes), dv clipped to
    +-max_acceleration h when the limit is positive, the exact arc of the mean velocity through the half angle a = (w h) / 2, (c, s) rotated
    twice by a and renormalised, psi += w h."""
    import math
    x, y, psi, v, c, s = (float(t) for t in p)
    w = float(cmd_w)
    if w > max_angular_velocity:
        w = max_angular_velocity
    if w < -max_angular_velocity:
        w = -max_angular_velocity
    dv = float(cmd_v) - v
    if max_acceleration > 0.0:
        lim = max_acceleration * h
        if dv > lim:
            dv = lim
        if dv < -lim:
            dv = -lim
    v1 = v + dv
    vm = (v + v1) / 2.0
    a = (w * h) / 2.0
    sn, cs, sinc = _small_angle(a)
    cm = c * cs - s * sn
    sm = s * cs + c * sn
    d = (vm * h) * sinc
    x = x + d * cm
    y = y + d * sm
    c2 = cm * cs - sm * sn
    s2 = sm * cs + cm * sn
    nn = c2 * c2 + s2 * s2
    n = math.sqrt(nn) if nn >= 0.0 else float("nan")
    return [x, y, psi + w * h, v1, c2 / n, s2 / n]


def episode_step(cmd, plant, plant0, count, raw_pos, raw_vel, raw_radius, raw_pos0, raw_vel0, episode, episode_f, log, substeps, timeout_ticks,
                 control_dt, max_acceleration, max_angular_velocity, robot_radius, goal_x=float("inf"), box=None, goal=None, state_nx=None,
                 state_batch=None, planner_ids=None, selection=None, segment=None):
    """One control period of one scene (host mirror of tmpc_episode_step; include/tmpc_hip_episode.h states the seven steps).  IN PLACE on the
    scene's rows of the device arrays, as numpy arrays (views): plant [6], raw_pos / raw_vel [n_slots][2], episode [4] i32, episode_f [2],
    log [max_episodes][4], and -- each may be None -- state_nx [nx], state_batch [P][nx], planner_ids [P], selection [3], segment [1].
    cmd [2], plant0 [6], raw_radius [n_slots], raw_pos0 / raw_vel0, box [4] or None and goal [3] or None are read.  Slots at or beyond the
    clipped count are neither read nor written.  Returns (was_reset, state4)."""
    import math
    control_dt = float(control_dt); max_acceleration = float(max_acceleration); max_angular_velocity = float(max_angular_velocity)
    robot_radius = float(robot_radius); goal_x = float(goal_x)
    n_slots, max_episodes = len(raw_radius), len(log)
    cnt = min(max(int(count), 0), n_slots)
    # 1. the plant
    p = [float(t) for t in plant]
    h = control_dt / float(substeps)
    for _ in range(int(substeps)):
        p = plant_substep(p, cmd[0], cmd[1], h, max_acceleration, max_angular_velocity)
    # 2. the obstacles, 3. the intrusion
    intrusion = 0.0
    for i in range(cnt):
        for axis in range(2):
            pos = float(raw_pos[i][axis]) + float(raw_vel[i][axis]) * control_dt
            raw_pos[i][axis] = pos
            if box is not None and (pos < float(box[2 * axis]) or pos > float(box[2 * axis + 1])):
                raw_vel[i][axis] = -float(raw_vel[i][axis])
        dx = float(raw_pos[i][0]) - p[0]
        dy = float(raw_pos[i][1]) - p[1]
        dd = dx * dx + dy * dy
        cand = (robot_radius + float(raw_radius[i])) - (math.sqrt(dd) if dd >= 0.0 else float("nan"))
        if cand > intrusion:
            intrusion = cand
    # 4. the counters, 5. the verdict
    ticks = int(episode[0]) + 1
    collisions = int(episode[1]) + (1 if intrusion > 0.0 else 0)
    finished = int(episode[2])
    max_intrusion = float(episode_f[0])
    if intrusion > max_intrusion:
        max_intrusion = intrusion
    completed = p[0] > goal_x
    if goal is not None:
        dx = p[0] - float(goal[0])
        dy = p[1] - float(goal[1])
        dd = dx * dx + dy * dy
        completed = completed or ((math.sqrt(dd) if dd >= 0.0 else float("nan")) < float(goal[2]))
    reset = bool(completed or (timeout_ticks > 0 and ticks >= timeout_ticks))
    # 6. the log and the restart
    if reset:
        if 0 <= finished < max_episodes:
            log[finished] = (float(ticks) * control_dt, 1.0 if completed else 0.0, float(collisions), max_intrusion)
        finished += 1
        p = [float(t) for t in plant0]
        for i in range(cnt):
            raw_pos[i] = raw_pos0[i]
            raw_vel[i] = raw_vel0[i]
        ticks, collisions, max_intrusion = 0, 0, 0.0
        if planner_ids is not None:
            planner_ids[:] = -1
        if selection is not None:
            selection[:] = (-1, 0, -1)
        if segment is not None:
            segment[:] = -1
    episode[:] = (ticks, collisions, finished, 0)
    episode_f[:] = (max_intrusion, intrusion)
    plant[:] = p
    # 7. the planner's states
    for out in ([] if state_nx is None else [state_nx]) + ([] if state_batch is None else list(state_batch)):
        out[0:4] = p[0:4]
        if reset:
            out[4:] = 0.0
    return reset, np.array(p[0:4])


# ---- the guidance search: host mirror of tmpc_guidance_search, bit for bit --------------------------------------------------
GS_GUARDS, GS_CONNECTORS, GS_KEPT = 32, 128, 16
_GS_MASK = (1 << 64) - 1


def _gs_mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _GS_MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _GS_MASK
    return z ^ (z >> 31)


def gs_sample_bits(seed, scene, i):
    """The three 64-bit draws of sample i of a scene: splitmix64 of (seed, scene, i, component), the generator of sample_scenarios."""
    key = _gs_mix((int(seed) & _GS_MASK) ^ _gs_mix((int(scene) + 0x51ED270B1) & _GS_MASK))
    return [_gs_mix((key + (3 * i + c + 1) * 0x9E3779B97F4A7C15) & _GS_MASK) for c in range(3)]


def winding_number(poly):
    """Winding number about the origin of the closed polygon poly [n][2] by the crossing rule: comparisons and the cross product
    u_x w_y - u_y w_x only, an integer."""
    u = np.asarray(poly, np.float64)
    w = np.roll(u, -1, axis=0)
    with np.errstate(invalid="ignore", over="ignore"):
        c = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
        up = (u[:, 1] <= 0.0) & (w[:, 1] > 0.0) & (c > 0.0)
        down = (u[:, 1] > 0.0) & (w[:, 1] <= 0.0) & (c < 0.0)
    return int(up.sum()) - int(down.sum())


def _gs_line(ka, pa, kb, pb, ks):
    """The connection a -> b at the stages ks: p_a + (p_b - p_a) ((k - k_a) / (k_b - k_a)), the endpoints as they are."""
    ks = np.asarray(ks)
    with np.errstate(invalid="ignore", over="ignore"):
        f = (ks - ka).astype(np.float64) / float(kb - ka)
        p = pa[None, :] + (pb - pa)[None, :] * f[:, None]
    p[ks == ka] = pa
    p[ks == kb] = pb
    return p


def _gs_polyline(nodes, S):
    """The polyline through nodes [(k, x, y), ...] of increasing stage at every stage it spans, as an array indexed by stage [S][2]."""
    out = np.full((S, 2), np.nan)
    for (ka, xa, ya), (kb, xb, yb) in zip(nodes[:-1], nodes[1:]):
        ks = np.arange(ka, kb + 1)
        out[ks] = _gs_line(ka, np.array([xa, ya]), kb, np.array([xb, yb]), ks)
    return out


def gs_equivalent(A, B, ka, kb, opos):
    """Are the polylines A, B (indexed by stage) equivalent over [ka, kb]: for every obstacle (opos [n][S][2], by stage) the polygon
    A(k) - o(k) ascending, B(k) - o(k) descending does not wind about the origin."""
    for o in opos:
        with np.errstate(invalid="ignore", over="ignore"):
            poly = np.concatenate([A[ka:kb + 1] - o[ka:kb + 1], (B[ka:kb + 1] - o[ka:kb + 1])[::-1]])
        if winding_number(poly) != 0:
            return False
    return True


def gs_connection_valid(ka, pa, kb, pb, opos, rr2, max_velocity, dt):
    """Is the connection valid: k_a < k_b, |p_b - p_a|^2 <= (max_velocity (k_b - k_a) dt)^2, and at every stage k >= 1 of [k_a, k_b]
    |p(k) - o_j(k)|^2 >= (r_j + robot_radius)^2 for every obstacle.  A NaN anywhere: invalid."""
    if not ka < kb:
        return False
    pa, pb = np.asarray(pa, np.float64), np.asarray(pb, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = pb - pa
        lim = (max_velocity * float(kb - ka)) * dt
        if not d[0] * d[0] + d[1] * d[1] <= lim * lim:
            return False
        if len(opos) == 0:
            return True
        ks = np.arange(max(ka, 1), kb + 1)
        e = _gs_line(ka, pa, kb, pb, ks)[None, :, :] - opos[:, ks, :]
        return bool(np.all(e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] >= rr2[:, None]))


def guidance_search(start, goals, obstacle_pos, obstacle_radius, selected, N, dt, scene, n_paths, n_samples, seed, n_nodes_max, max_expansions,
                    robot_radius, max_velocity, margin, weight_length, prev_traj, prev_class, prev_count, next_class, nodes, node_count,
                    topology_class, was_reset=False):
    """The guidance search of one scene (host mirror of tmpc_guidance_search; include/tmpc_hip_guidance_search.h states the algorithm, U20).
    start [>= 2], goals [n_goals][3] = (x, y, cost), obstacle_pos [M][N][2], obstacle_radius [M] and selected [M] as prepare_obstacles
    leaves them; `scene` is the scene's index (it enters the samples' counter).  IN PLACE on the scene's rows of the device arrays (views):
    the carried prev_traj [n_paths][N + 1][2], prev_class [n_paths], prev_count [1], next_class [1] and the outputs nodes [n_paths][R][3],
    node_count [n_paths], topology_class [n_paths].  Returns (traj_count, status)."""
    import math
    N, S, R, P = int(N), int(N) + 1, int(n_nodes_max), int(n_paths)
    dt, max_velocity, weight_length, margin = float(dt), float(max_velocity), float(weight_length), float(margin)
    real = [j for j in range(len(selected)) if int(selected[j]) >= 0]
    stage_step = np.maximum(np.arange(S) - 1, 0)
    opos = np.asarray(obstacle_pos, np.float64)[real][:, stage_step, :] if real else np.zeros((0, S, 2))
    rr = np.asarray(obstacle_radius, np.float64)[real] + float(robot_radius)
    rr2 = rr * rr
    valid = lambda a, b: gs_connection_valid(a[0], a[1:], b[0], b[1:], opos, rr2, max_velocity, dt)
    length = lambda a, b: math.sqrt((b[1] - a[1]) * (b[1] - a[1]) + (b[2] - a[2]) * (b[2] - a[2]))
    status = 0
    # guards: (k, x, y), the goal index and cost beside them
    sx, sy = float(start[0]), float(start[1])
    guards, goal_of, goal_cost = [(0, sx, sy)], [-1], [0.0]
    for i, g in enumerate(np.asarray(goals, np.float64)):
        if np.isfinite(g[0]) and np.isfinite(g[1]):
            guards.append((N, float(g[0]), float(g[1]))); goal_of.append(i); goal_cost.append(float(g[2]))
    xs, ys = [g[1] for g in guards], [g[2] for g in guards]
    lox, hix, loy, hiy = min(xs) - margin, max(xs) + margin, min(ys) - margin, max(ys) + margin
    # the visibility-PRM
    connectors = []                                                    # [g1, g2, (k, x, y), length]
    for i in range(int(n_samples) if N >= 2 else 0):
        u = gs_sample_bits(seed, scene, i)
        s = (1 + u[0] % (N - 1), lox + (hix - lox) * (float(u[1] >> 11) * 2.0 ** -53), loy + (hiy - loy) * (float(u[2] >> 11) * 2.0 ** -53))
        visible = [g for g, gd in enumerate(guards) if gd[0] != s[0] and (valid(gd, s) if gd[0] < s[0] else valid(s, gd))]
        if not visible:
            if len(guards) < GS_GUARDS:
                guards.append(s); goal_of.append(-1); goal_cost.append(0.0)
            else:
                status |= 1
            continue
        d2 = lambda g: (s[1] - guards[g][1]) * (s[1] - guards[g][1]) + (s[2] - guards[g][2]) * (s[2] - guards[g][2])
        before = [g for g in visible if guards[g][0] < s[0]]
        after = [g for g in visible if guards[g][0] > s[0]]
        if not before or not after:
            continue
        g1, g2 = min(before, key=lambda g: (d2(g), g)), min(after, key=lambda g: (d2(g), g))
        cand_len = length(guards[g1], s) + length(s, guards[g2])
        A = _gs_polyline([guards[g1], s, guards[g2]], S)
        for c in connectors:
            if c[0] == g1 and c[1] == g2 and gs_equivalent(A, _gs_polyline([guards[g1], c[2], guards[g2]], S), guards[g1][0], guards[g2][0], opos):
                if cand_len < c[3]:
                    c[2], c[3] = s, cand_len
                break
        else:
            if len(connectors) < GS_CONNECTORS:
                connectors.append([g1, g2, s, cand_len])
            else:
                status |= 2
    # the paths
    kept = []                                                          # [cost, node list, polyline]

    def consider(path, goal_guard):
        nonlocal status
        if len(path) > R:
            status |= 8
            return
        acc = 0.0
        for a, b in zip(path[:-1], path[1:]):
            acc = acc + length(a, b)
        cost = weight_length * acc + goal_cost[goal_guard]
        line = _gs_polyline(path, S)
        for kp in kept:
            if gs_equivalent(line, kp[2], 0, N, opos):
                if cost < kp[0]:
                    kp[:] = [cost, path, line]
                return
        if len(kept) < GS_KEPT:
            kept.append([cost, path, line])
            return
        worst = 0
        for p in range(1, len(kept)):
            if kept[p][0] >= kept[worst][0]:
                worst = p
        if cost < kept[worst][0]:
            kept[worst] = [cost, path, line]

    for g in range(1, len(guards)):
        if goal_of[g] >= 0 and valid(guards[0], guards[g]):
            consider([guards[0], guards[g]], g)
    visits = 0

    class _Stop(Exception):
        pass

    def descend(g, path):
        nonlocal visits, status
        for c in connectors:
            if c[0] != g:
                continue
            if visits >= max_expansions:
                status |= 4
                raise _Stop()
            visits += 1
            longer = path + [c[2], guards[c[1]]]
            if goal_of[c[1]] >= 0:
                consider(longer, c[1])
            else:
                descend(c[1], longer)

    try:
        descend(0, [guards[0]])
    except _Stop:
        pass
    # insertion by ascending cost, stable (a cost that is not a number stays where it is met)
    order = []
    for i in range(len(kept)):
        j = len(order)
        while j > 0 and kept[order[j - 1]][0] > kept[i][0]:
            j -= 1
        order.insert(j, i)
    count = min(len(kept), P)
    # class identity
    n_prev, nxt = int(prev_count[0]), int(next_class[0])
    if was_reset:
        n_prev, nxt = 0, 0
    n_prev = min(max(n_prev, 0), P)
    shifted = []
    for r in range(n_prev):
        line = np.asarray(prev_traj[r], np.float64)[np.minimum(np.arange(S) + 1, N)].copy()
        line[0] = (sx, sy)
        shifted.append(line)
    claimed, classes = set(), []
    for i in range(count):
        line = kept[order[i]][2]
        for r in range(n_prev):
            if r not in claimed and gs_equivalent(line, shifted[r], 0, N, opos):
                classes.append(int(prev_class[r])); claimed.add(r)
                break
        else:
            classes.append(nxt); nxt += 1
    for i in range(P):
        if i >= count:
            node_count[i] = 0; topology_class[i] = -1; prev_class[i] = -1
            continue
        path = kept[order[i]][1]
        for e, (k, x, y) in enumerate(path):
            nodes[i][e] = (float(k) * dt, x, y)
        node_count[i] = len(path); topology_class[i] = classes[i]; prev_class[i] = classes[i]
        prev_traj[i] = kept[order[i]][2]
    prev_count[0] = count; next_class[0] = nxt
    return count, status
