/* mpc_planner_types/prep_arithmetic.h -- the double-precision arithmetic of data preparation (road rows, obstacle preparation, path tracking,
 * path fitting, free-space decomposition, the guidance hand-off, the episode step, the guidance search), written ONCE for the device kernels (csrc/tmpc_aux_kernels.hpp) and the Solver-free C++ headers
 * (reference_path.h, free_space.h, guidance_handoff.h, data_preparation.h, episode.h, guidance_search.h, Contouring in modules_hip.h): both compile these functions, so they cannot drift apart.  The independent statement the
 * tests compare both against is the numpy mirror, mpc_planner_amd/modules.py; every function keeps the mirror's operation order, and nothing is
 * fused into multiply-adds (the pragma under clang; build host code with -ffp-contract=off).  Plain functions on doubles: no containers, no
 * planner types.  A cubic is its eight coefficients c = (ax bx cx dx ay by cy dy): x(t) = ((ax t + bx) t + cx) t + dx, the same for y. */
#ifndef MPC_PREP_ARITHMETIC_HIP_H
#define MPC_PREP_ARITHMETIC_HIP_H

#include <math.h>

#ifdef __HIPCC__
#define TMPC_ARITH_FN __host__ __device__ inline
#else
#define TMPC_ARITH_FN inline
#endif
#ifdef __clang__
#define TMPC_ARITH_NO_FMA _Pragma("clang fp contract(off)")
#else
#define TMPC_ARITH_NO_FMA
#endif

namespace tmpc_arith
{
    /* ---- cubic: point and derivative at t, Horner form ---- */
    TMPC_ARITH_FN void cubic(const double c[8], double t, double &x, double &y, double &dx, double &dy)
    {
        TMPC_ARITH_NO_FMA
        x = ((c[0] * t + c[1]) * t + c[2]) * t + c[3];
        y = ((c[4] * t + c[5]) * t + c[6]) * t + c[7];
        dx = (3.0 * c[0] * t + 2.0 * c[1]) * t + c[2];
        dy = (3.0 * c[4] * t + 2.0 * c[5]) * t + c[6];
    }

    /* ---- scalar cubic c = (a b c d): its value at t, Horner form (the velocity profile v(s) on t = s - start) ---- */
    TMPC_ARITH_FN double cubic_value(const double c[4], double t) { TMPC_ARITH_NO_FMA return ((c[0] * t + c[1]) * t + c[2]) * t + c[3]; }

    /* ---- closest point of the cubic on t in [0, L] to (px, py) (RosTools::Spline2D::findClosestPoint restated): D = |P(t) - p|^2,
     * g = (P(t) - p).P'(t).  Nine coarse samples t_j = L (j / 8), the bracket around the best (lowest j on ties), an end of the bracket if g does
     * not change sign inside it, else exactly 40 bisections (no data-dependent exit) and the bracket's midpoint; the coarse sample wins if its D
     * is strictly smaller. ---- */
    constexpr int COARSE = 8, BISECTIONS = 40;
    TMPC_ARITH_FN void closest_on_segment(const double cg[8], double L, double px, double py, double &D_out, double &t_out)
    {
        TMPC_ARITH_NO_FMA
        double c[8];
        for (int i = 0; i < 8; i++) c[i] = cg[i];
        auto eval = [&](double t, double &g) {
            TMPC_ARITH_NO_FMA
            double x, y, dx, dy;
            cubic(c, t, x, y, dx, dy);
            const double ex = x - px, ey = y - py;
            g = ex * dx + ey * dy;
            return ex * ex + ey * ey;
        };
        double g;
        int js = 0;
        double Dj = eval(L * (0.0 / 8.0), g);
        for (int j = 1; j <= COARSE; j++) {
            const double Dc = eval(L * ((double)j / 8.0), g);
            if (Dc < Dj) { js = j; Dj = Dc; }
        }
        double lo = L * ((double)(js > 0 ? js - 1 : 0) / 8.0), hi = L * ((double)(js < COARSE ? js + 1 : COARSE) / 8.0);
        double tc;
        eval(lo, g);
        if (g >= 0.0) tc = lo;
        else {
            eval(hi, g);
            if (g <= 0.0) tc = hi;
            else {
                for (int it = 0; it < BISECTIONS; it++) {
                    const double mid = 0.5 * (lo + hi);
                    eval(mid, g);
                    if (g > 0.0) hi = mid; else lo = mid;
                }
                tc = 0.5 * (lo + hi);
            }
        }
        const double Dc = eval(tc, g);
        if (Dj < Dc) { D_out = Dj; t_out = L * ((double)js / 8.0); }
        else { D_out = Dc; t_out = tc; }
    }

    /* ---- road rows (Contouring::constructRoadConstraints, contouring.cpp:181-262).  RosTools::Spline2D is not in the reference tree; ASSUMED
     * (DESIGN.md U12): getOrthogonal(s) = (y'(s), -x'(s)) / |.| (to the right of travel: the only sign for which bounds mode is a corridor between
     * the bounds), and P, x', y' are the plain piecewise cubics, no sigmoid glue.  The lookup of the segment that holds s, i = max{j : start_j <= s},
     * rounds nothing and stays with each caller's storage. ---- */
    /* point P and right-hand unit normal A of a cubic at t */
    TMPC_ARITH_FN void road_frame(const double c[8], double t, double &px, double &py, double &ax, double &ay)
    {
        TMPC_ARITH_NO_FMA
        double dx, dy;
        cubic(c, t, px, py, dx, dy);
        const double n = sqrt(dx * dx + dy * dy);
        ax = dy / n; ay = -dx / n;
    }
    /* A.(P + A off) and A.(P - A off) */
    TMPC_ARITH_FN double road_offset_plus(double px, double py, double ax, double ay, double off) { TMPC_ARITH_NO_FMA return ax * (px + ax * off) + ay * (py + ay * off); }
    TMPC_ARITH_FN double road_offset_minus(double px, double py, double ax, double ay, double off) { TMPC_ARITH_NO_FMA return ax * (px - ax * off) + ay * (py - ay * off); }
    /* centreline form (:191-235): rows (A, A.(P + A off_first)) and (-A, -A.(P - A off_second)) of the path's cubic c; row = (a1 a2 b) twice */
    TMPC_ARITH_FN void road_rows_centreline(const double c[8], double t, double off_first, double off_second, double *row)
    {
        double px, py, ax, ay;
        road_frame(c, t, px, py, ax, ay);
        const double b0 = road_offset_plus(px, py, ax, ay, off_first);
        const double b1 = road_offset_minus(px, py, ax, ay, off_second);
        row[0] = ax; row[1] = ay; row[2] = b0;
        row[3] = -ax; row[4] = -ay; row[5] = -b1;
    }
    /* bounds form (:237-262): row (-A_l, -A_l.(P_l + A_l off)) of the left bound's cubic, row (A_r, A_r.(P_r - A_r off)) of the right bound's */
    TMPC_ARITH_FN void road_row_left_bound(const double c[8], double t, double off, double *row)
    {
        double px, py, ax, ay;
        road_frame(c, t, px, py, ax, ay);
        const double vl = road_offset_plus(px, py, ax, ay, off);
        row[0] = -ax; row[1] = -ay; row[2] = -vl;
    }
    TMPC_ARITH_FN void road_row_right_bound(const double c[8], double t, double off, double *row)
    {
        double px, py, ax, ay;
        road_frame(c, t, px, py, ax, ay);
        const double vr = road_offset_minus(px, py, ax, ay, off);
        row[0] = ax; row[1] = ay; row[2] = vr;
    }

    /* ---- window padding: column col of the row (0, 0, x'(end), X(end), 0, 0, y'(end), Y(end)), start = length, that continues a
     * path straight along its end tangent; x, y, dx, dy = cubic() of the last segment at t = L_last ---- */
    TMPC_ARITH_FN double padding_entry(int col, double x, double y, double dx, double dy, double length) { return col == 2 ? dx : col == 3 ? x : col == 6 ? dy : col == 7 ? y : col == 8 ? length : 0.0; }
    /* the same for a bound cubic: eight columns, no start (written out: composed from the other, the kernel's column switch compiles differently) */
    TMPC_ARITH_FN double padding_entry(int col, double x, double y, double dx, double dy) { return col == 2 ? dx : col == 3 ? x : col == 6 ? dy : col == 7 ? y : 0.0; }

    /* ---- natural cubic spline through (t_i, y_i): Thomas recurrence on the half second derivatives m_i, m_0 = m_{n-1} = 0, no
     * pivoting (strictly diagonally dominant).  Row i of the system: lo_i = spline_off(h_{i-1}), di_i, up_i = spline_off(h_i), r_i ---- */
    TMPC_ARITH_FN bool spacing_valid(double h) { TMPC_ARITH_NO_FMA return h > 0.0 && h < __builtin_huge_val(); }
    TMPC_ARITH_FN double spline_off(double h) { TMPC_ARITH_NO_FMA return h / 3.0; }
    TMPC_ARITH_FN double spline_diag(double hm, double h) { TMPC_ARITH_NO_FMA return (2.0 * (hm + h)) / 3.0; }
    TMPC_ARITH_FN double spline_rhs(double ym, double y0, double yp, double hm, double h) { TMPC_ARITH_NO_FMA return (yp - y0) / h - (y0 - ym) / hm; }
    /* forward sweep, row i: (cp, g) of row i - 1 become those of row i */
    TMPC_ARITH_FN void thomas_forward(double lo, double di, double up, double r, double &cp, double &g)
    {
        TMPC_ARITH_NO_FMA
        const double den = di - lo * cp;
        cp = up / den;
        g = (r - lo * g) / den;
    }
    /* back substitution: m_i from m_{i+1} */
    TMPC_ARITH_FN double thomas_backward(double g, double cp, double m_next) { TMPC_ARITH_NO_FMA return g - cp * m_next; }
    /* a, c, d of ((a u + b) u + c) u + d on u = s - t_i; b = m0 */
    TMPC_ARITH_FN void spline_row(double m0, double m1, double h, double y0, double y1, double &a, double &c, double &d)
    {
        TMPC_ARITH_NO_FMA
        a = (m1 - m0) / (3.0 * h);
        c = (y1 - y0) / h - ((2.0 * m0 + m1) * h) / 3.0;
        d = y0;
    }

    /* ---- obstacle preparation (mpc_planner/src/data_preparation.cpp) ---- */
    /* step k of the constant-velocity prediction, one coordinate (:58-79) */
    TMPC_ARITH_FN double cv_step(double p, double v, double dt, int k) { TMPC_ARITH_NO_FMA return p + (v * dt) * (double)k; }
    /* |(px, py) - (x, y)| < max_dist: removeDistantObstacles keeps the obstacle (:81-93); Contouring::isObjectiveReached with max_dist 1 */
    TMPC_ARITH_FN bool within_distance(double px, double py, double x, double y, double max_dist)
    {
        TMPC_ARITH_NO_FMA
        const double dx = px - x, dy = py - y;
        return sqrt(dx * dx + dy * dy) < max_dist;
    }
    /* the selection key (:113-131) is the minimum over k < N, from SELECTION_KEY_START, of ((k + 1) 0.6) |o_k - (p + (v k) (cos psi, sin psi))|
     * (`v k` has no dt: kept); c, s = cos psi, sin psi */
    constexpr double SELECTION_KEY_START = 1e5;
    TMPC_ARITH_FN double selection_key_term(int k, double ox, double oy, double x, double y, double v, double c, double s)
    {
        TMPC_ARITH_NO_FMA
        const double vk = v * (double)k;
        const double dx = ox - (x + vk * c), dy = oy - (y + vk * s);
        return ((double)(k + 1) * 0.6) * sqrt(dx * dx + dy * dy);
    }
    /* propagatePredictionUncertainty (:170-186), one step of one axis: sqrt(acc^2 + (sigma dt)^2), squares written x * x */
    TMPC_ARITH_FN double propagate_step(double acc, double sigma, double dt)
    {
        TMPC_ARITH_NO_FMA
        const double s = sigma * dt;
        return sqrt(acc * acc + s * s);
    }
    /* getDummyObstacle (:49-56): one coordinate of the dummy's position from the robot's */
    TMPC_ARITH_FN double dummy_coordinate(double x) { TMPC_ARITH_NO_FMA return x + 100.0; }

    /* ---- free-space decomposition (DecompConstraints::update, decomp_constraints.cpp:52-148).  DecompUtil is not in the reference tree: upstream
     * DecompUtil's LineSegment algorithm restated in the frame of the segment.  e = unit direction p1 -> p2, h = (e_y, -e_x),
     * c = midpoint, f = half length; a point o has the local coordinates u = (o - c).e along the segment and w = (o - c).h across it; the
     * ellipse has the semi-axes a (along, = f) and b (across). ---- */
    constexpr double DECOMP_EPS = 1e-10;            /* DecompUtil's epsilon_ */
    constexpr double DECOMP_TERMINATOR = 1e-3;      /* a row with a shorter normal (or NaN) ends the copy (decomp_constraints.cpp:98) */
    /* centre of costmap cell m along one axis (costmap_2d::Costmap2D::mapToWorld) */
    TMPC_ARITH_FN double cell_centre(double origin, int m, double resolution) { TMPC_ARITH_NO_FMA return origin + ((double)m + 0.5) * resolution; }
    /* s_{k+1} = s_k + v_k dt (:81) */
    TMPC_ARITH_FN double advance(double s, double v, double dt) { TMPC_ARITH_NO_FMA return s + v * dt; }
    /* one coordinate of the path beyond its end: straight along the end tangent (U14-3) */
    TMPC_ARITH_FN double continue_straight(double x_end, double dx_end, double s, double length) { TMPC_ARITH_NO_FMA return x_end + (s - length) * dx_end; }
    /* frame of the segment p1 -> p2; false: the segment is degenerate (length zero, NaN or inf) and the outputs mean nothing */
    TMPC_ARITH_FN bool decomp_frame(double p1x, double p1y, double p2x, double p2y, double &ex, double &ey, double &cx, double &cy, double &f)
    {
        TMPC_ARITH_NO_FMA
        const double dx = p2x - p1x, dy = p2y - p1y;
        const double len = sqrt(dx * dx + dy * dy);
        ex = dx / len; ey = dy / len;
        cx = (p1x + p2x) / 2.0; cy = (p1y + p2y) / 2.0;
        f = len / 2.0;
        return len > 0.0 && len < __builtin_huge_val();
    }
    TMPC_ARITH_FN void decomp_local(double ox, double oy, double cx, double cy, double ex, double ey, double &u, double &w)
    {
        TMPC_ARITH_NO_FMA
        const double rx = ox - cx, ry = oy - cy;
        u = rx * ex + ry * ey;
        w = rx * ey - ry * ex;
    }
    /* add_local_bbox + points_inside: the box of half width R across and f + R along */
    TMPC_ARITH_FN bool decomp_in_box(double u, double w, double f, double R) { TMPC_ARITH_NO_FMA return fabs(w) <= R + DECOMP_EPS && fabs(u) <= f + R + DECOMP_EPS; }
    /* squared ellipse distance, and the key of the argmin rule: d2, a NaN counts as +inf */
    TMPC_ARITH_FN double decomp_d2(double u, double w, double a, double b) { TMPC_ARITH_NO_FMA const double ua = u / a, wb = w / b; return ua * ua + wb * wb; }
    TMPC_ARITH_FN double decomp_key(double d2) { return d2 == d2 ? d2 : __builtin_huge_val(); }
    TMPC_ARITH_FN bool decomp_inside_first(double d2) { TMPC_ARITH_NO_FMA return sqrt(d2) <= 1.0; }
    TMPC_ARITH_FN bool decomp_inside(double d2) { TMPC_ARITH_NO_FMA return 1.0 - sqrt(d2) > DECOMP_EPS; }
    /* the ellipse shrunk through the point (u, w): the new b (unchanged unless u < a) */
    TMPC_ARITH_FN double decomp_shrink(double u, double w, double a, double b)
    {
        TMPC_ARITH_NO_FMA
        if (!(u < a)) return b;
        const double ua = u / a;
        return fabs(w) / sqrt(1.0 - ua * ua);
    }
    /* tangent row of the ellipse through the point o = (ox, oy) with local (u, w): unit normal n, beta = n.o; not yet flipped */
    TMPC_ARITH_FN void decomp_row(double u, double w, double a, double b, double ex, double ey, double ox, double oy, double &nx, double &ny, double &beta)
    {
        TMPC_ARITH_NO_FMA
        const double gu = u / (a * a), gw = w / (b * b);
        const double nrm = sqrt(gu * gu + gw * gw);
        const double nu = gu / nrm, nw = gw / nrm;
        nx = nu * ex + nw * ey; ny = nu * ey - nw * ex;
        beta = nx * ox + ny * oy;
    }
    /* n.(o - o*): a point stays in the remaining set iff this is < 0 */
    TMPC_ARITH_FN double decomp_side(double nx, double ny, double ox, double oy, double sx, double sy) { TMPC_ARITH_NO_FMA return nx * (ox - sx) + ny * (oy - sy); }
    /* LinearConstraint's flip: the centre of the segment has to satisfy the row */
    TMPC_ARITH_FN void decomp_flip(double cx, double cy, double &nx, double &ny, double &beta)
    {
        TMPC_ARITH_NO_FMA
        if (nx * cx + ny * cy - beta > 0.0) { nx = -nx; ny = -ny; beta = -beta; }
    }
    /* the four rows of the local box, in DecompUtil's order: (h, h.(p1 + R h)), (-h, -h.(p1 - R h)), (e, e.(p2 + R e)), (-e, -e.(p1 - R e)); row [4][3] */
    TMPC_ARITH_FN void decomp_box_rows(double p1x, double p1y, double p2x, double p2y, double ex, double ey, double R, double *row)
    {
        const double hx = ey, hy = -ex;
        row[0] = hx; row[1] = hy; row[2] = road_offset_plus(p1x, p1y, hx, hy, R);
        row[3] = -hx; row[4] = -hy; row[5] = -road_offset_minus(p1x, p1y, hx, hy, R);
        row[6] = ex; row[7] = ey; row[8] = road_offset_plus(p2x, p2y, ex, ey, R);
        row[9] = -ex; row[10] = -ey; row[11] = -road_offset_minus(p1x, p1y, ex, ey, R);
    }
    /* does row (a1, a2, .) end the copy (:98)? */
    TMPC_ARITH_FN bool decomp_terminator(double a1, double a2) { TMPC_ARITH_NO_FMA return sqrt(a1 * a1 + a2 * a2) < DECOMP_TERMINATOR || a1 != a1; }

    /* ---- guidance hand-off: the time spline through a guidance trajectory's nodes, and GuidanceConstraints' bookkeeping around
     * the solve (guidance_constraints.cpp:192-250, :283-387, :416-434).  + - x / and comparisons only ---- */
    /* the sample time of node k, and the velocity of a scalar cubic c = (a b c d) at tau (its position is cubic_value) */
    TMPC_ARITH_FN double sample_time(int k, double dt) { TMPC_ARITH_NO_FMA return (double)k * dt; }
    TMPC_ARITH_FN double cubic_slope(const double c[4], double tau) { TMPC_ARITH_NO_FMA return (3.0 * c[0] * tau + 2.0 * c[1]) * tau + c[2]; }
    /* the braking command's velocity, std::max(v - deceleration dt, 0.) (ros1_jackalsimulator.cpp:191-199) */
    TMPC_ARITH_FN double braking_velocity(double v, double deceleration, double dt)
    {
        TMPC_ARITH_NO_FMA
        const double w = v - deceleration * dt;
        return w < 0.0 ? 0.0 : w;
    }

    /* mapGuidanceTrajectoriesToPlanners (:192-250) over P <= 64 planners with last tick's IDs and n_traj <= 63 trajectories' classes, literally,
     * the second loop without its `break` included: bit p of the result is planners_[p].existing_guidance.  The sets are 64-bit masks. */
    TMPC_ARITH_FN unsigned long long guidance_existing(const int *ids, int P, const int *cls, int n_traj)
    {
        unsigned long long taken = 0, existing = 0, remaining = 0;
        for (int i = 0; i < n_traj; i++) {
            bool found = false;
            for (int p = 0; p < P; p++)
                if (ids[p] == cls[i] && !((taken >> p) & 1ull)) {
                    taken |= 1ull << p; existing |= 1ull << p; found = true;
                    break;
                }
            if (!found) remaining |= 1ull << i;
        }
        for (int i = 0; i < n_traj; i++) {
            if (!((remaining >> i) & 1ull)) continue;
            for (int p = 0; p < P; p++)
                if (!((taken >> p) & 1ull)) { taken |= 1ull << p; existing &= ~(1ull << p); }
        }
        return existing;
    }

    /* One scene of tmpc_guidance_plan; `first` = q P is the scene's first batch entry and every output points at that entry.  cls / prev
     * [n_paths] (prev may be null), ids [P] and sel [3] the cross-tick state (read only).  Steps 1-7 of the header's description. */
    TMPC_ARITH_FN void guidance_plan_scene(int first, int n_paths, int use_tmpcpp, int warmstart_with_mpc_solution, int shift, double weight_consistency,
                                           int traj_count, const int *cls, const unsigned char *prev, const int *ids, const int *sel, int *mode,
                                           int *src, unsigned char *init_enabled, unsigned char *rows_dummy, unsigned char *disabled, int *guidance_id,
                                           double *weight)
    {
        const int P = n_paths + (use_tmpcpp ? 1 : 0);
        const int n_traj = traj_count < 0 ? 0 : (traj_count > n_paths ? n_paths : traj_count);
        const unsigned long long existing = guidance_existing(ids, P, cls, n_traj);
        const int warm_mode = shift ? 1 : 2;
        const bool was_feasible = sel[2] >= 0;
        for (int p = 0; p < P; p++) {
            const bool original = use_tmpcpp && p == P - 1;
            const bool off = p >= n_traj && !original;
            const bool guided = !original && !off;
            int m = was_feasible ? warm_mode : 3, s = was_feasible ? first + sel[2] : first + p;
            unsigned char init = 0;
            if (guided) {
                if (warmstart_with_mpc_solution && ((existing >> p) & 1ull)) { m = warm_mode; s = first + p; }
                else init = 1;
            }
            bool selected = false;
            if (guided) selected = prev ? prev[p] != 0 : (sel[0] >= 0 && sel[1] == 0 && cls[p] == sel[0]);
            mode[p] = m; src[p] = s; init_enabled[p] = init;
            rows_dummy[p] = (original || off) ? 1 : 0;
            disabled[p] = off ? 1 : 0;
            guidance_id[p] = original ? 2 * n_paths : (off ? -1 : cls[p]);
            weight[p] = selected ? weight_consistency : 1.0;
        }
    }

    /* FindBestPlanner (:416-434) over one scene's P planners: index of the winner or -1 */
    TMPC_ARITH_FN int guidance_best(int P, const double *pobj, const int *exit_code, const unsigned char *disabled, const double *weight)
    {
        TMPC_ARITH_NO_FMA
        double best_solution = 1e10;
        int best = -1;
        for (int p = 0; p < P; p++) {
            if (disabled[p]) continue;
            const double objective = pobj[p] * weight[p];
            if (exit_code[p] == 1 && objective < best_solution) { best_solution = objective; best = p; }
        }
        return best;
    }

    /* One scene of tmpc_guidance_decide: every pointer at the scene's first entry (xtraj / utraj: its first trajectory, x_entry / u_entry doubles
     * per trajectory, nx doubles per node, nu per input node; v is state 3, w input 1).  Steps 1-5 of the header's description. */
    TMPC_ARITH_FN void guidance_decide_scene(int P, int use_tmpcpp, const double *pobj, const int *exit_code, const unsigned char *disabled,
                                             const int *guidance_id, const double *weight, const double *xtraj, int x_entry, int nx, const double *utraj,
                                             int u_entry, double v_state, double deceleration, double control_dt, int enable_output, int *best_out,
                                             int *exit_out, double *cmd, int *ids, int *sel)
    {
        const int best = guidance_best(P, pobj, exit_code, disabled, weight);
        *best_out = best;
        *exit_out = best >= 0 ? exit_code[best] : (disabled[0] ? -1 : exit_code[0]);
        if (best >= 0 && enable_output) {
            cmd[0] = xtraj[(long long)best * x_entry + nx + 3];
            cmd[1] = utraj[(long long)best * u_entry + 1];
        } else {
            cmd[0] = braking_velocity(v_state, deceleration, control_dt);
            cmd[1] = 0.0;
        }
        for (int p = 0; p < P; p++) ids[p] = guidance_id[p];
        if (best >= 0) { sel[0] = guidance_id[best]; sel[1] = (use_tmpcpp && best == P - 1) ? 1 : 0; }
        sel[2] = best;
    }

    /* ---- the episode step: the velocity-commanded unicycle plant, the obstacles' motion and the intrusion measure.
     * + - x /, sqrt and comparisons only: no libm trigonometry ---- */
    /* sin a, cos a and sin a / a for |a| <= 1/16 as fixed Horner polynomials in a^2: terms through a^9, a^10 and a^8 (the first omitted
     * terms, a^11 / 11! and a^12 / 12!, stay below 2e-21 there).  sin a = a (sin a / a): the same polynomial, one evaluation */
    TMPC_ARITH_FN void small_angle(double a, double &sn, double &cs, double &sinc)
    {
        TMPC_ARITH_NO_FMA
        const double z = a * a;
        sinc = (((z * (1.0 / 362880.0) + (-1.0 / 5040.0)) * z + (1.0 / 120.0)) * z + (-1.0 / 6.0)) * z + 1.0;
        cs = ((((z * (-1.0 / 3628800.0) + (1.0 / 40320.0)) * z + (-1.0 / 720.0)) * z + (1.0 / 24.0)) * z + (-1.0 / 2.0)) * z + 1.0;
        sn = a * sinc;
    }
    /* one substep h of the plant p = (x, y, psi, v, c, s), (c, s) the heading as a unit vector: w clipped to +-max_w by two comparisons (a NaN
     * passes), dv = cmd_v - v clipped to +-max_acc h when max_acc > 0, the exact arc of the mean velocity at constant w through the half angle
     * a = (w h) / 2 -- chord (vm h) (sin a / a) along the mid heading --, (c, s) rotated twice by a and renormalised, psi += w h */
    TMPC_ARITH_FN void plant_substep(double cmd_v, double cmd_w, double h, double max_acc, double max_w, double *p)
    {
        TMPC_ARITH_NO_FMA
        double w = cmd_w;
        if (w > max_w) w = max_w;
        if (w < -max_w) w = -max_w;
        double dv = cmd_v - p[3];
        if (max_acc > 0.0) {
            const double lim = max_acc * h;
            if (dv > lim) dv = lim;
            if (dv < -lim) dv = -lim;
        }
        const double v1 = p[3] + dv, vm = (p[3] + v1) / 2.0;
        const double a = (w * h) / 2.0;
        double sn, cs, sinc;
        small_angle(a, sn, cs, sinc);
        const double cm = p[4] * cs - p[5] * sn, sm = p[5] * cs + p[4] * sn;
        const double d = (vm * h) * sinc;
        p[0] = p[0] + d * cm;
        p[1] = p[1] + d * sm;
        const double c2 = cm * cs - sm * sn, s2 = sm * cs + cm * sn;
        const double n = sqrt(c2 * c2 + s2 * s2);
        p[4] = c2 / n; p[5] = s2 / n;
        p[2] = p[2] + w * h;
        p[3] = v1;
    }
    /* one coordinate of an obstacle over a control period: pos += vel dt; with a box, a position now outside [lo, hi] flips the velocity's
     * sign and stays where it is */
    TMPC_ARITH_FN void obstacle_step(double &pos, double &vel, double dt, bool boxed, double lo, double hi)
    {
        TMPC_ARITH_NO_FMA
        pos = pos + vel * dt;
        if (boxed && (pos < lo || pos > hi)) vel = -vel;
    }
    /* how far the robot's disc at (x, y) and the obstacle's at (ox, oy) overlap: negative when apart, 0 when they touch */
    TMPC_ARITH_FN double intrusion_candidate(double robot_radius, double radius, double ox, double oy, double x, double y)
    {
        TMPC_ARITH_NO_FMA
        const double dx = ox - x, dy = oy - y;
        return (robot_radius + radius) - sqrt(dx * dx + dy * dy);
    }

    /* ---- the guidance search: a visibility-PRM on the stage grid, a homotopy filter by winding numbers and the selection of
     * the cheapest topology classes.  Decisions (integers), copies and fixed-order + - x / sqrt expressions only.  The search of one scene is
     * written once, gs_scene below, over a lane policy W: the device kernel runs it with the 64 lanes of a wave (lane-strided loops, votes,
     * integer sums, a minimum with an index tie-break: no reduction whose result depends on the lane order), the host twin
     * (mpc_planner_modules/guidance_search.h) with GsOneLane.  Everything outside the lane-strided loops is wave-uniform: every lane holds
     * the same value, takes the same branch and stores the same value to a table entry ---- */
    constexpr int GS_MAX_OBSTACLES = 32, GS_MAX_GOALS = 16, GS_GUARDS = 32, GS_CONNECTORS = 128, GS_KEPT = 16, GS_MAX_NODES = 64, GS_MAX_STAGES = 64,
                  GS_MAX_CHAIN = 31, GS_MAX_SAMPLES = 256, GS_MAX_EXPANSIONS = 65536;
    enum { GS_GUARDS_FULL = 1, GS_CONNECTORS_FULL = 2, GS_EXPANSIONS_STOPPED = 4, GS_PATH_TOO_LONG = 8 };

    /* the fields of tmpc_guidance_search_options behind `size` */
    struct GsOptions { int n_paths, n_samples, n_nodes_max, max_expansions; unsigned long long seed; double robot_radius, max_velocity, margin, weight_length; };

    /* what tmpc_guidance_search refuses (N + 1 stages have to fit the tables: every handle's N does) */
    TMPC_ARITH_FN bool gs_valid(const GsOptions &o, int n_scenes, int n_goals, int max_obstacles, int N)
    {
        TMPC_ARITH_NO_FMA
        const double inf = __builtin_huge_val();
        return n_scenes > 0 && n_goals >= 1 && n_goals <= GS_MAX_GOALS && max_obstacles >= 1 && max_obstacles <= GS_MAX_OBSTACLES && N >= 1 &&
               N < GS_MAX_STAGES && o.n_paths >= 1 && o.n_paths <= GS_KEPT && o.n_samples >= 0 && o.n_samples <= GS_MAX_SAMPLES &&
               o.n_nodes_max >= 2 && o.n_nodes_max <= GS_MAX_NODES && o.max_expansions >= 1 && o.max_expansions <= GS_MAX_EXPANSIONS &&
               o.robot_radius >= 0.0 && o.max_velocity > 0.0 && o.max_velocity < inf && o.weight_length > 0.0 && o.weight_length < inf &&
               o.margin >= 0.0 && o.margin < inf;
    }

    /* the tables of one scene: LDS on the device (about 42 KB), an object on the host */
    struct GsWork {
        double opos[GS_MAX_OBSTACLES][GS_MAX_STAGES][2];     /* the real obstacles by STAGE: stage k sees prepared step max(k - 1, 0) */
        double orr2[GS_MAX_OBSTACLES];                       /* (r_j + robot_radius)^2 */
        double gxy[GS_GUARDS][2], gcost[GS_GUARDS];          /* guards: position, the goal's cost */
        int gk[GS_GUARDS], ggoal[GS_GUARDS];                 /* stage; goal index, -1 for the start and for sample guards */
        double cxy[GS_CONNECTORS][2], clen[GS_CONNECTORS];   /* connectors (g1, s, g2): the sample, the two legs' length */
        int cg1[GS_CONNECTORS], cg2[GS_CONNECTORS], ck[GS_CONNECTORS];
        double a[GS_MAX_STAGES][2], b[GS_MAX_STAGES][2];     /* the two polylines of a homotopy test, by stage */
        double kcost[GS_KEPT];                               /* kept paths: cost, connectors, the connector chain, the goal's guard */
        int knc[GS_KEPT], kgoal[GS_KEPT], kchain[GS_KEPT][GS_MAX_CHAIN];
        int chain[GS_MAX_CHAIN], it[GS_MAX_CHAIN + 1];       /* the enumeration's stack: the candidate path */
        int order[GS_KEPT], cls[GS_KEPT];
    };

    /* the host's lane policy: one lane */
    struct GsOneLane {
        static constexpr int width = 1;
        int lane() const { return 0; }
        bool any(bool b) const { return b; }
        int sum(int v) const { return v; }
        void argmin(double &, int &) const {}
        void sync() const {}
    };

    /* splitmix64, counter-based, as tmpc_sample_scenarios draws its bits: the scene's key, then the bits of counter ctr */
    TMPC_ARITH_FN unsigned long long gs_mix(unsigned long long z)
    {
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    TMPC_ARITH_FN unsigned long long gs_key(unsigned long long seed, int q) { return gs_mix(seed ^ gs_mix((unsigned long long)q + 0x51ED270B1ull)); }
    TMPC_ARITH_FN unsigned long long gs_bits(unsigned long long key, unsigned long long ctr) { return gs_mix(key + (ctr + 1ull) * 0x9E3779B97F4A7C15ull); }
    TMPC_ARITH_FN double gs_unit(unsigned long long bits) { TMPC_ARITH_NO_FMA return (double)(bits >> 11) * (1.0 / 9007199254740992.0); }
    TMPC_ARITH_FN double gs_sample_coordinate(double lo, double hi, unsigned long long bits) { TMPC_ARITH_NO_FMA return lo + (hi - lo) * gs_unit(bits); }
    TMPC_ARITH_FN bool gs_finite(double x) { return x == x && fabs(x) < __builtin_huge_val(); }
    /* one coordinate of the connection a -> b at stage k: the endpoints as they are */
    TMPC_ARITH_FN double gs_lerp(double a, double b, int k, int ka, int kb)
    {
        TMPC_ARITH_NO_FMA
        return k == ka ? a : k == kb ? b : a + (b - a) * ((double)(k - ka) / (double)(kb - ka));
    }
    TMPC_ARITH_FN double gs_dist2(double ax, double ay, double bx, double by) { TMPC_ARITH_NO_FMA const double dx = bx - ax, dy = by - ay; return dx * dx + dy * dy; }
    TMPC_ARITH_FN double gs_length(double ax, double ay, double bx, double by) { TMPC_ARITH_NO_FMA return sqrt(gs_dist2(ax, ay, bx, by)); }
    TMPC_ARITH_FN bool gs_reachable(double d2, double max_velocity, int dk, double dt) { TMPC_ARITH_NO_FMA const double lim = (max_velocity * (double)dk) * dt; return d2 <= lim * lim; }
    /* one polygon edge u -> w of a winding number about the origin, by the crossing rule: +1 for an upward crossing with the origin on the
     * left, -1 for a downward one with the origin on the right */
    TMPC_ARITH_FN int gs_crossing(double ux, double uy, double wx, double wy)
    {
        TMPC_ARITH_NO_FMA
        const double c = ux * wy - uy * wx;
        if (uy <= 0.0) return (wy > 0.0 && c > 0.0) ? 1 : 0;
        return (wy <= 0.0 && c < 0.0) ? -1 : 0;
    }
    /* the winding number of the closed polygon v [n][2] about the origin (the statement the tests hold against atan2) */
    TMPC_ARITH_FN int gs_winding(const double *v, int n)
    {
        int wn = 0;
        for (int e = 0; e < n; e++) { const int f = e + 1 == n ? 0 : e + 1; wn += gs_crossing(v[e * 2], v[e * 2 + 1], v[f * 2], v[f * 2 + 1]); }
        return wn;
    }

    /* is the connection (ka, xa, ya) -> (kb, xb, yb) valid: ka < kb, reachable at max_velocity, clear of every real obstacle at every stage
     * >= 1 of [ka, kb].  The stages x obstacles over the lanes, one vote */
    template <class W> TMPC_ARITH_FN bool gs_connection_valid(const W &w, const GsWork &t, int n_real, const GsOptions &o, double dt, int ka, double xa,
                                                              double ya, int kb, double xb, double yb)
    {
        TMPC_ARITH_NO_FMA
        if (!(ka < kb)) return false;
        bool bad = !gs_reachable(gs_dist2(xa, ya, xb, yb), o.max_velocity, kb - ka, dt);
        const int items = (kb - ka + 1) * n_real;
        for (int e = w.lane(); e < items; e += W::width) {
            const int k = ka + e / n_real, j = e % n_real;
            if (k >= 1 && !(gs_dist2(gs_lerp(xa, xb, k, ka, kb), gs_lerp(ya, yb, k, ka, kb), t.opos[j][k][0], t.opos[j][k][1]) >= t.orr2[j])) bad = true;
        }
        return !w.any(bad);
    }
    /* the two-leg polyline (k0, p0) -> (k1, p1) -> (k2, p2) at every stage of [k0, k2] */
    template <class W> TMPC_ARITH_FN void gs_expand_legs(const W &w, double (*buf)[2], int k0, double x0, double y0, int k1, double x1, double y1, int k2,
                                                         double x2, double y2)
    {
        w.sync();
        for (int k = k0 + w.lane(); k <= k2; k += W::width) {
            buf[k][0] = k <= k1 ? gs_lerp(x0, x1, k, k0, k1) : gs_lerp(x1, x2, k, k1, k2);
            buf[k][1] = k <= k1 ? gs_lerp(y0, y1, k, k0, k1) : gs_lerp(y1, y2, k, k1, k2);
        }
        w.sync();
    }
    /* node i of the path (nc connectors `chain`, then the goal's guard): start, c, g, c', g', ..., goal; a direct path has nc = 0 */
    TMPC_ARITH_FN int gs_path_nodes(int nc) { return nc > 0 ? 1 + 2 * nc : 2; }
    TMPC_ARITH_FN void gs_path_node(const GsWork &t, int nc, const int *chain, int goal, int i, int &k, double &x, double &y)
    {
        if (i & 1) {
            if (nc == 0) { k = t.gk[goal]; x = t.gxy[goal][0]; y = t.gxy[goal][1]; }
            else { const int c = chain[(i - 1) / 2]; k = t.ck[c]; x = t.cxy[c][0]; y = t.cxy[c][1]; }
        } else {
            const int g = i == 0 ? 0 : t.cg2[chain[i / 2 - 1]];
            k = t.gk[g]; x = t.gxy[g][0]; y = t.gxy[g][1];
        }
    }
    /* a path at every stage 0 .. N: stage k lies on the first leg that ends at or after it */
    template <class W> TMPC_ARITH_FN void gs_expand_path(const W &w, const GsWork &t, double (*buf)[2], int N, int nc, const int *chain, int goal)
    {
        w.sync();
        const int n = gs_path_nodes(nc);
        for (int k = w.lane(); k <= N; k += W::width) {
            int ka, kb; double xa, ya, xb, yb;
            gs_path_node(t, nc, chain, goal, 0, ka, xa, ya);
            gs_path_node(t, nc, chain, goal, 1, kb, xb, yb);
            for (int i = 2; i < n && kb < k; i++) { ka = kb; xa = xb; ya = yb; gs_path_node(t, nc, chain, goal, i, kb, xb, yb); }
            buf[k][0] = gs_lerp(xa, xb, k, ka, kb); buf[k][1] = gs_lerp(ya, yb, k, ka, kb);
        }
        w.sync();
    }
    /* are the polylines t.a and t.b, given at every stage of [ka, kb], equivalent: for every real obstacle the winding number about the origin
     * of the closed polygon a(k) - o(k), k ascending, then b(k) - o(k), k descending, is 0.  The polygon's edges over the lanes, one integer
     * sum per obstacle */
    template <class W> TMPC_ARITH_FN bool gs_equivalent(const W &w, const GsWork &t, int n_real, int ka, int kb)
    {
        TMPC_ARITH_NO_FMA
        const int m = kb - ka + 1, n = 2 * m;
        for (int j = 0; j < n_real; j++) {
            int local = 0;
            for (int e = w.lane(); e < n; e += W::width) {
                const int f = e + 1 == n ? 0 : e + 1;
                const int ke = e < m ? ka + e : kb - (e - m), kf = f < m ? ka + f : kb - (f - m);
                const double(*pe)[2] = e < m ? t.a : t.b, (*pf)[2] = f < m ? t.a : t.b;
                local += gs_crossing(pe[ke][0] - t.opos[j][ke][0], pe[ke][1] - t.opos[j][ke][1], pf[kf][0] - t.opos[j][kf][0], pf[kf][1] - t.opos[j][kf][1]);
            }
            if (w.sum(local) != 0) return false;
        }
        return true;
    }
    /* a candidate path (the enumeration's stack t.chain, nc connectors, the goal's guard) against the kept list: one path per class */
    template <class W> TMPC_ARITH_FN void gs_consider(const W &w, GsWork &t, int n_real, const GsOptions &o, int N, int nc, int goal, int &n_kept, int &status)
    {
        TMPC_ARITH_NO_FMA
        const int n = gs_path_nodes(nc);
        if (n > o.n_nodes_max) { status |= GS_PATH_TOO_LONG; return; }
        double acc = 0.0;
        {
            int ka, kb; double xa, ya, xb, yb;
            gs_path_node(t, nc, t.chain, goal, 0, ka, xa, ya);
            for (int i = 1; i < n; i++) { gs_path_node(t, nc, t.chain, goal, i, kb, xb, yb); acc = acc + gs_length(xa, ya, xb, yb); xa = xb; ya = yb; }
        }
        const double cost = o.weight_length * acc + t.gcost[goal];
        gs_expand_path(w, t, t.a, N, nc, t.chain, goal);
        int slot = -1;
        for (int p = 0; p < n_kept && slot < 0; p++) {
            gs_expand_path(w, t, t.b, N, t.knc[p], t.kchain[p], t.kgoal[p]);
            if (gs_equivalent(w, t, n_real, 0, N)) {
                if (!(cost < t.kcost[p])) return;
                slot = p;
            }
        }
        if (slot < 0) {
            if (n_kept < GS_KEPT) slot = n_kept++;
            else {
                int worst = 0;
                for (int p = 1; p < n_kept; p++) if (t.kcost[p] >= t.kcost[worst]) worst = p;
                if (!(cost < t.kcost[worst])) return;
                slot = worst;
            }
        }
        w.sync();
        t.kcost[slot] = cost; t.knc[slot] = nc; t.kgoal[slot] = goal;
        for (int i = 0; i < nc; i++) t.kchain[slot][i] = t.chain[i];
        w.sync();
    }

    /* The guidance search of scene q (include/tmpc_hip_guidance_search.h states the arrays and the algorithm).  Every pointer is the whole
     * array; was_reset may be null. */
    template <class W> TMPC_ARITH_FN void gs_scene(const W &w, GsWork &t, int q, int N, double dt, int n_goals, int M, const GsOptions &o, const double *state4,
                                                   const double *goals, const double *obstacle_pos, const double *obstacle_radius, const int *selected,
                                                   const unsigned char *was_reset, double *prev_traj, int *prev_class, int *prev_count, int *next_class,
                                                   double *nodes, int *node_count, int *traj_count, int *topology_class, int *status_out)
    {
        TMPC_ARITH_NO_FMA
        const int lane = w.lane(), S = N + 1, R = o.n_nodes_max, P = o.n_paths;
        int status = 0;
        /* the real obstacles, by stage */
        int n_real = 0;
        for (int s = 0; s < M; s++) {
            if (selected[(size_t)q * M + s] < 0) continue;
            const double rr = obstacle_radius[(size_t)q * M + s] + o.robot_radius;
            t.orr2[n_real] = rr * rr;
            for (int e = lane; e < S * 2; e += W::width) {
                const int k = e >> 1, step = k >= 1 ? k - 1 : 0;
                t.opos[n_real][k][e & 1] = obstacle_pos[(((size_t)q * M + s) * N + step) * 2 + (e & 1)];
            }
            n_real++;
        }
        /* the guards: the start, then the present goals; the sampling box */
        const double sx = state4[(size_t)q * 4], sy = state4[(size_t)q * 4 + 1];
        int n_guards = 1;
        t.gk[0] = 0; t.ggoal[0] = -1; t.gxy[0][0] = sx; t.gxy[0][1] = sy; t.gcost[0] = 0.0;
        double lox = sx, hix = sx, loy = sy, hiy = sy;
        for (int i = 0; i < n_goals; i++) {
            const double *g = goals + ((size_t)q * n_goals + i) * 3;
            if (!gs_finite(g[0]) || !gs_finite(g[1])) continue;
            t.gk[n_guards] = N; t.ggoal[n_guards] = i; t.gxy[n_guards][0] = g[0]; t.gxy[n_guards][1] = g[1]; t.gcost[n_guards] = g[2];
            n_guards++;
            if (g[0] < lox) lox = g[0];
            if (g[0] > hix) hix = g[0];
            if (g[1] < loy) loy = g[1];
            if (g[1] > hiy) hiy = g[1];
        }
        lox = lox - o.margin; hix = hix + o.margin; loy = loy - o.margin; hiy = hiy + o.margin;
        w.sync();
        /* the visibility-PRM: the samples in order */
        int n_conn = 0;
        const unsigned long long key = gs_key(o.seed, q);
        for (int i = 0; i < o.n_samples && N >= 2; i++) {
            const int k = 1 + (int)(gs_bits(key, 3ull * (unsigned long long)i) % (unsigned long long)(N - 1));
            const double x = gs_sample_coordinate(lox, hix, gs_bits(key, 3ull * (unsigned long long)i + 1ull));
            const double y = gs_sample_coordinate(loy, hiy, gs_bits(key, 3ull * (unsigned long long)i + 2ull));
            unsigned visible = 0u;
            for (int g = 0; g < n_guards; g++) {
                const int kg = t.gk[g];
                if (kg == k) continue;
                const bool ok = kg < k ? gs_connection_valid(w, t, n_real, o, dt, kg, t.gxy[g][0], t.gxy[g][1], k, x, y)
                                       : gs_connection_valid(w, t, n_real, o, dt, k, x, y, kg, t.gxy[g][0], t.gxy[g][1]);
                if (ok) visible |= 1u << g;
            }
            if (visible == 0u) {
                if (n_guards < GS_GUARDS) {
                    t.gk[n_guards] = k; t.ggoal[n_guards] = -1; t.gxy[n_guards][0] = x; t.gxy[n_guards][1] = y; t.gcost[n_guards] = 0.0;
                    n_guards++;
                    w.sync();
                } else status |= GS_GUARDS_FULL;
                continue;
            }
            /* the nearest visible guard either side in time: the guards over the lanes, a minimum with the lowest index on ties */
            int g1 = -1, g2 = -1;
            double d1 = 0.0, d2 = 0.0;
            for (int g = lane; g < n_guards; g += W::width) {
                if (!((visible >> g) & 1u)) continue;
                const double d = gs_dist2(t.gxy[g][0], t.gxy[g][1], x, y);
                if (t.gk[g] < k) { if (g1 < 0 || d < d1) { g1 = g; d1 = d; } }
                else if (g2 < 0 || d < d2) { g2 = g; d2 = d; }
            }
            w.argmin(d1, g1);
            w.argmin(d2, g2);
            if (g1 < 0 || g2 < 0) continue;
            const int k1 = t.gk[g1], k2 = t.gk[g2];
            const double x1 = t.gxy[g1][0], y1 = t.gxy[g1][1], x2 = t.gxy[g2][0], y2 = t.gxy[g2][1];
            const double len = gs_length(x1, y1, x, y) + gs_length(x, y, x2, y2);
            gs_expand_legs(w, t.a, k1, x1, y1, k, x, y, k2, x2, y2);
            int slot = -1;
            bool dropped = false;
            for (int c = 0; c < n_conn && slot < 0 && !dropped; c++) {
                if (t.cg1[c] != g1 || t.cg2[c] != g2) continue;
                gs_expand_legs(w, t.b, k1, x1, y1, t.ck[c], t.cxy[c][0], t.cxy[c][1], k2, x2, y2);
                if (gs_equivalent(w, t, n_real, k1, k2)) {
                    if (len < t.clen[c]) slot = c;
                    else dropped = true;
                }
            }
            if (dropped) continue;
            if (slot < 0) {
                if (n_conn >= GS_CONNECTORS) { status |= GS_CONNECTORS_FULL; continue; }
                slot = n_conn++;
            }
            w.sync();
            t.cg1[slot] = g1; t.cg2[slot] = g2; t.ck[slot] = k; t.cxy[slot][0] = x; t.cxy[slot][1] = y; t.clen[slot] = len;
            w.sync();
        }
        /* the paths: the direct connections in goal order, then the chains, depth first with the connectors in table order */
        int n_kept = 0;
        for (int g = 1; g < n_guards; g++)
            if (t.ggoal[g] >= 0 && gs_connection_valid(w, t, n_real, o, dt, 0, sx, sy, t.gk[g], t.gxy[g][0], t.gxy[g][1]))
                gs_consider(w, t, n_real, o, N, 0, g, n_kept, status);
        int depth = 0, visits = 0;
        t.it[0] = 0;
        w.sync();
        while (depth >= 0) {
            const int g = depth == 0 ? 0 : t.cg2[t.chain[depth - 1]];
            int c = t.it[depth];
            while (c < n_conn && t.cg1[c] != g) c++;
            if (c >= n_conn) { depth--; continue; }
            if (visits >= o.max_expansions) { status |= GS_EXPANSIONS_STOPPED; break; }
            visits++;
            w.sync();
            t.it[depth] = c + 1; t.chain[depth] = c;
            w.sync();
            const int g2 = t.cg2[c];
            if (t.ggoal[g2] >= 0) gs_consider(w, t, n_real, o, N, depth + 1, g2, n_kept, status);
            else if (depth + 1 < GS_MAX_CHAIN) { depth++; w.sync(); t.it[depth] = 0; w.sync(); }
        }
        /* the kept paths, stably by ascending cost */
        w.sync();
        for (int i = 0; i < n_kept; i++) {
            int j = i;
            while (j > 0 && t.kcost[t.order[j - 1]] > t.kcost[i]) { t.order[j] = t.order[j - 1]; j--; }
            t.order[j] = i;
        }
        w.sync();
        const int count = n_kept < P ? n_kept : P;
        /* class identity across ticks: previous trajectories name classes, against this tick's obstacles */
        int n_prev = prev_count[q], next = next_class[q];
        if (was_reset && was_reset[q]) { n_prev = 0; next = 0; }
        n_prev = n_prev < 0 ? 0 : (n_prev > P ? P : n_prev);
        unsigned claimed = 0u;
        for (int i = 0; i < count; i++) {
            const int p = t.order[i];
            gs_expand_path(w, t, t.a, N, t.knc[p], t.kchain[p], t.kgoal[p]);
            int cls = -1;
            for (int r = 0; r < n_prev && cls < 0; r++) {
                if ((claimed >> r) & 1u) continue;
                w.sync();
                for (int k = lane; k <= N; k += W::width) {
                    const double *pt = prev_traj + (((size_t)q * P + r) * S + (k + 1 < N ? k + 1 : N)) * 2;
                    t.b[k][0] = k == 0 ? sx : pt[0]; t.b[k][1] = k == 0 ? sy : pt[1];
                }
                w.sync();
                if (gs_equivalent(w, t, n_real, 0, N)) { cls = prev_class[(size_t)q * P + r]; claimed |= 1u << r; }
            }
            if (cls < 0) cls = next++;
            t.cls[i] = cls;
        }
        w.sync();
        /* the outputs and the carried arrays */
        for (int i = 0; i < P; i++) {
            const size_t f = (size_t)q * P + i;
            if (i >= count) {
                if (lane == 0) { node_count[f] = 0; topology_class[f] = -1; prev_class[f] = -1; }
                continue;
            }
            const int p = t.order[i], nc = t.knc[p], n = gs_path_nodes(nc);
            gs_expand_path(w, t, t.a, N, nc, t.kchain[p], t.kgoal[p]);
            for (int e = lane; e < n; e += W::width) {
                int k; double x, y;
                gs_path_node(t, nc, t.kchain[p], t.kgoal[p], e, k, x, y);
                double *nd = nodes + (f * R + e) * 3;
                nd[0] = (double)k * dt; nd[1] = x; nd[2] = y;
            }
            for (int e = lane; e < S * 2; e += W::width) prev_traj[f * S * 2 + e] = t.a[e >> 1][e & 1];
            if (lane == 0) { node_count[f] = n; topology_class[f] = t.cls[i]; prev_class[f] = t.cls[i]; }
        }
        if (lane == 0) { traj_count[q] = count; prev_count[q] = count; next_class[q] = next; status_out[q] = status; }
    }
}
#endif
