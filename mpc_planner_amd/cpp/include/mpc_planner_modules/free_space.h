/*
 * mpc_planner_modules/free_space.h -- what DecompConstraints::update computes (decomp_constraints.cpp:52-148): the occupied cells of the
 * costmap, the polyline on the reference path, and one convex polygon per segment of it.  Needs no Solver and no generated header.
 * DecompUtil is not in the reference tree: upstream DecompUtil's LineSegment algorithm is restated in the frame of the segment (DESIGN.md
 * U16; the reference uses a modified copy nobody here has read, so parity with it is not pinned).  The arithmetic is that of
 * mpc_planner_types/prep_arithmetic.h, the one source tmpc_costmap_points_kernel and tmpc_decomp_halfspaces_kernel compile too; the
 * independent statement both are tested against, bit for bit, is mpc_planner_amd/modules.py (costmap_points, decomp_path_points,
 * decomp_segment) -- where the compiler does not fuse multiply-adds (build with -ffp-contract=off on a target that has them).
 */
#ifndef MPC_FREE_SPACE_HIP_H
#define MPC_FREE_SPACE_HIP_H

#include <vector>

#include <mpc_planner_modules/reference_path.h>
#include <mpc_planner_types/prep_arithmetic.h>

namespace MPCPlanner
{
    namespace FreeSpace
    {
        enum Status { COMPLETE = 0, TRUNCATED = 1, DEGENERATE = 2 };

        /* getOccupiedGridCells (:122-148): the centre of every cell whose cost is not FREE_SPACE (0), mx outer and my inner, as (x, y) pairs;
         * at most max_points of them (0: all); returns true iff there were more.  Costmap: costmap_2d::Costmap2D or anything with its members. */
        template <class Costmap>
        bool occupiedCells(const Costmap &costmap, std::vector<double> &xy, size_t max_points = 0)
        {
            xy.clear();
            double x, y;
            for (unsigned int i = 0; i < costmap.getSizeInCellsX(); i++)
                for (unsigned int j = 0; j < costmap.getSizeInCellsY(); j++) {
                    if (costmap.getCost(i, j) == 0) continue;
                    if (max_points && xy.size() >= 2 * max_points) return true;
                    costmap.mapToWorld(i, j, x, y);
                    xy.push_back(x); xy.push_back(y);
                }
            return false;
        }

        /* P(s) on a whole path: the cubic of segment i = max{j : start_j <= s} (0 below the first knot) at t = s - start_i; from `length` on
         * straight along the end tangent (U14-3).  The path must not be empty. */
        inline void pathPoint(const ReferencePathSpline &path, double s, double &x, double &y)
        {
            const int n = path.numSegments();
            double dx, dy;
            if (s >= path.length) {
                double ex, ey;
                ReferencePathSpline::cubic(path.segments[n - 1], path.segmentLength(n - 1), ex, ey, dx, dy);
                x = tmpc_arith::continue_straight(ex, dx, s, path.length); y = tmpc_arith::continue_straight(ey, dy, s, path.length);
                return;
            }
            int i = 0;
            for (int j = 0; j < n; j++) if (path.segments[j].start <= s) i = j;
            ReferencePathSpline::cubic(path.segments[i], s - path.segments[i].start, x, y, dx, dy);
        }

        /* the polyline (:68-82): P(s_k), k < v.size(), s_0 = s0, s_{k+1} = s_k + v_k dt accumulated left to right; (x, y) pairs */
        inline void pathPoints(const ReferencePathSpline &path, double s0, const std::vector<double> &v, double dt, std::vector<double> &xy)
        {
            xy.assign(2 * v.size(), 0.);
            double s = s0;
            for (size_t k = 0; k < v.size(); k++) {
                pathPoint(path, s, xy[2 * k], xy[2 * k + 1]);
                s = tmpc_arith::advance(s, v[k], dt);
            }
        }

        /* One segment p1 -> p2 among `count` points (x, y pairs): rows [n_rows][3] = (a1, a2, b) of A p <= b, the first `written` as found --
         * at most n_rows obstacle rows, then the four rows of the local box of half width R --, the rest the dummy (1, 0, state_x + 100).
         * Returns the status: COMPLETE, TRUNCATED (more rows found than n_rows) or DEGENERATE (a segment whose length is not positive and
         * finite, or a row with |A_i| < 1e-3 or NaN ended the copy early, as the reference's loop does, :96-101). */
        inline int decompose(double p1x, double p1y, double p2x, double p2y, const double *pts, int count, double R, int n_rows, double state_x,
                             double *rows, int &written)
        {
            using namespace tmpc_arith;
            const double dummy_b = dummy_coordinate(state_x);
            for (int r = 0; r < n_rows; r++) { rows[3 * r] = 1.0; rows[3 * r + 1] = 0.0; rows[3 * r + 2] = dummy_b; }
            written = 0;
            double ex, ey, cx, cy, f;
            if (!decomp_frame(p1x, p1y, p2x, p2y, ex, ey, cx, cy, f)) return DEGENERATE;
            double a = f, b = f;
            std::vector<char> box(count, 0), set(count, 0);
            auto local = [&](int i, double &u, double &w) { decomp_local(pts[2 * i], pts[2 * i + 1], cx, cy, ex, ey, u, w); };
            /* the smallest key among the set, the lowest index among equals; -1: the set is empty */
            auto argmin = [&]() {
                int best = -1;
                double best_key = 0.;
                for (int i = 0; i < count; i++) {
                    if (!set[i]) continue;
                    double u, w;
                    local(i, u, w);
                    const double key = decomp_key(decomp_d2(u, w, a, b));
                    if (best < 0 || key < best_key) { best = i; best_key = key; }
                }
                return best;
            };
            for (int i = 0; i < count; i++) {
                double u, w;
                local(i, u, w);
                box[i] = decomp_in_box(u, w, f, R);
                set[i] = box[i] && decomp_inside_first(decomp_d2(u, w, a, b));
            }
            for (int pass = 0; pass < count; pass++) {
                const int j = argmin();
                if (j < 0) break;
                double u, w;
                local(j, u, w);
                b = decomp_shrink(u, w, a, b);
                for (int i = 0; i < count; i++) {
                    if (!set[i]) continue;
                    local(i, u, w);
                    set[i] = i != j && decomp_inside(decomp_d2(u, w, a, b));
                }
            }
            std::vector<double> found;
            set = box;
            while ((int)found.size() < 3 * n_rows) {
                const int j = argmin();
                if (j < 0) break;
                double u, w, nx, ny, beta;
                local(j, u, w);
                decomp_row(u, w, a, b, ex, ey, pts[2 * j], pts[2 * j + 1], nx, ny, beta);
                for (int i = 0; i < count; i++)
                    if (set[i]) set[i] = i != j && decomp_side(nx, ny, pts[2 * i], pts[2 * i + 1], pts[2 * j], pts[2 * j + 1]) < 0.0;
                decomp_flip(cx, cy, nx, ny, beta);
                found.push_back(nx); found.push_back(ny); found.push_back(beta);
            }
            const size_t n_obstacle = found.size();
            found.resize(n_obstacle + 12);
            decomp_box_rows(p1x, p1y, p2x, p2y, ex, ey, R, found.data() + n_obstacle);
            const int n_found = (int)(found.size() / 3), limit = n_found < n_rows ? n_found : n_rows;
            while (written < limit && !decomp_terminator(found[3 * written], found[3 * written + 1])) {
                for (int c = 0; c < 3; c++) rows[3 * written + c] = found[3 * written + c];
                written++;
            }
            return written < limit ? DEGENERATE : (n_found > n_rows ? TRUNCATED : COMPLETE);
        }

        /* DecompConstraints::update for one scene: N = v.size() stages; segment k of the polyline into stage k + 1, stage 0 all dummies.
         * rows [N][n_rows][3], written [N], status [N]. */
        inline void decomposePath(const ReferencePathSpline &path, double s0, const std::vector<double> &v, double dt, const std::vector<double> &points,
                                  double R, int n_rows, double state_x, std::vector<double> &rows, std::vector<int> &written, std::vector<int> &status)
        {
            const int N = (int)v.size();
            std::vector<double> poly;
            pathPoints(path, s0, v, dt, poly);
            rows.assign((size_t)N * n_rows * 3, 0.); written.assign(N, 0); status.assign(N, COMPLETE);
            const double dummy_b = tmpc_arith::dummy_coordinate(state_x);
            for (int r = 0; r < n_rows && N > 0; r++) { rows[3 * r] = 1.0; rows[3 * r + 1] = 0.0; rows[3 * r + 2] = dummy_b; }
            for (int k = 0; k + 1 < N; k++)
                status[k + 1] = decompose(poly[2 * k], poly[2 * k + 1], poly[2 * k + 2], poly[2 * k + 3], points.data(), (int)(points.size() / 2), R, n_rows,
                                          state_x, rows.data() + (size_t)(k + 1) * n_rows * 3, written[k + 1]);
        }
    }
}
#endif
