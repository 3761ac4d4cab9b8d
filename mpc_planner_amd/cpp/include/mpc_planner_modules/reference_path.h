/*
 * mpc_planner_modules/reference_path.h -- a whole reference path as Contouring::update needs it every tick (contouring.cpp:28-48): the closest
 * point, the segment window setSplineParameters writes (:94-124), the objective-reached test (:167-175).  Needs no Solver and no generated
 * header.  RosTools::Spline2D is not in the reference tree: the search is restated, its assumptions are DESIGN.md U14.  The arithmetic and its
 * order are those of mpc_planner_amd/modules.py (closest_point_on_segment, find_closest_point, path_window) and of tmpc_track_path_kernel: the
 * three agree bit for bit where the compiler does not fuse multiply-adds (build with -ffp-contract=off on a target that has them).
 */
#ifndef MPC_REFERENCE_PATH_HIP_H
#define MPC_REFERENCE_PATH_HIP_H

#include <cmath>
#include <vector>

#include <mpc_planner_types/path_segment.h>

namespace MPCPlanner
{
    struct ReferencePathSpline
    {
        std::vector<PathSegment> segments;                      /* the whole path */
        double length{0.};                                      /* the knot behind the last segment: L_i = start_{i+1} - start_i, L_last = length - start_last */
        std::vector<PathSegment> left_bound, right_bound;       /* optional: bound cubics on the same knots (their `start` is not read) */

        static constexpr int COARSE = 8, BISECTIONS = 40;

        bool empty() const { return segments.empty(); }
        int numSegments() const { return (int)segments.size(); }
        double segmentLength(int i) const { return (i + 1 < numSegments() ? segments[i + 1].start : length) - segments[i].start; }

        /* point and derivative of one cubic at t, Horner form (the forms of Contouring::evaluateSegments) */
        static void cubic(const PathSegment &c, double t, double &x, double &y, double &dx, double &dy)
        {
            x = ((c.ax * t + c.bx) * t + c.cx) * t + c.dx;
            y = ((c.ay * t + c.by) * t + c.cy) * t + c.dy;
            dx = (3.0 * c.ax * t + 2.0 * c.bx) * t + c.cx;
            dy = (3.0 * c.ay * t + 2.0 * c.by) * t + c.cy;
        }

        /* closest point of the cubic on t in [0, L] to (px, py): D = |P(t) - p|^2, g = (P(t) - p).P'(t).  Nine coarse samples t_j = L (j / 8); the
         * bracket around the best (lowest j on ties); an end of the bracket if g does not change sign inside it, else exactly 40 bisections and
         * the bracket's midpoint; the coarse sample wins if its D is strictly smaller. */
        static void closestOnSegment(const PathSegment &c, double L, double px, double py, double &D_out, double &t_out)
        {
            auto eval = [&](double t, double &g) {
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

        /* RosTools::Spline2D::findClosestPoint as Contouring::update uses it (:37; U14-1).  segment < 0 (a new path, a reset): every segment is a
         * candidate; otherwise [max(0, prev - range), min(n - 1, prev + range)], prev clamped into [0, n - 1].  The comparison starts from the
         * first candidate and replaces on strict `<`: the lowest segment wins a tie, a NaN / inf position yields the first candidate.
         * Vec2: anything with operator()(int), e.g. MPCPlanner::Vector2d.  An empty path leaves segment and s alone. */
        template <class Vec2>
        void findClosestPoint(const Vec2 &p, int &segment, double &s, int range = 2) const
        {
            const int n = numSegments();
            if (n <= 0) return;
            int first = 0, last = n - 1;
            if (segment >= 0) {
                const int prev = segment > n - 1 ? n - 1 : segment;
                first = prev - range > 0 ? prev - range : 0;
                last = prev + range < n - 1 ? prev + range : n - 1;
            }
            int best = first;
            double best_D = 0., best_t = 0.;
            for (int i = first; i <= last; i++) {
                double D, t;
                closestOnSegment(segments[i], segmentLength(i), p(0), p(1), D, t);
                if (i == first || D < best_D) { best = i; best_D = D; best_t = t; }
            }
            segment = best;
            s = segments[best].start + best_t;
        }

        /* The S segments from `segment` on (U14-2); beyond the last one the path continues STRAIGHT ALONG ITS END TANGENT (U14-3): (0, 0, x'(end),
         * X(end), 0, 0, y'(end), Y(end)), start = length, from the last cubic at t = L_last -- a constant point would give |path'| = 0, which the
         * NLP and the road normals divide by.  left / right: the bound cubics of the same slots, padded the same way from their own last cubics
         * (start = the path's knots). */
        void window(int segment, int S, std::vector<PathSegment> &out, std::vector<PathSegment> *left = nullptr, std::vector<PathSegment> *right = nullptr) const
        {
            const int n = numSegments();
            out.clear();
            if (left) left->clear();
            if (right) right->clear();
            if (n <= 0) return;
            const double L_last = segmentLength(n - 1);
            auto pad = [&](const PathSegment &last) {
                double x, y, dx, dy;
                cubic(last, L_last, x, y, dx, dy);
                return PathSegment{0., 0., dx, x, 0., 0., dy, y, length};
            };
            for (int w = 0; w < S; w++) {
                const int i = segment + w;
                out.push_back(i < n ? segments[i] : pad(segments[n - 1]));
                if (left && !left_bound.empty()) { PathSegment b = i < n ? left_bound[i] : pad(left_bound[n - 1]); b.start = out.back().start; left->push_back(b); }
                if (right && !right_bound.empty()) { PathSegment b = i < n ? right_bound[i] : pad(right_bound[n - 1]); b.start = out.back().start; right->push_back(b); }
            }
        }

        /* Contouring::isObjectiveReached (:167-175): |p - P(length)| < 1.0 */
        template <class Vec2>
        bool reached(const Vec2 &p) const
        {
            const int n = numSegments();
            if (n <= 0) return false;
            double x, y, dx, dy;
            cubic(segments[n - 1], segmentLength(n - 1), x, y, dx, dy);
            const double ex = x - p(0), ey = y - p(1);
            return std::sqrt(ex * ex + ey * ey) < 1.0;
        }
    };
}
#endif
