/* mpc_planner_types/path_segment.h -- one cubic segment of the contouring reference and the waypoint container it is fitted from, on their
 * own so that Solver-free headers
 * (mpc_planner_modules/reference_path.h) can use it without the generated solver dimensions. */
#ifndef MPC_PATH_SEGMENT_HIP_H
#define MPC_PATH_SEGMENT_HIP_H

#include <vector>

namespace MPCPlanner
{
    /* One cubic segment of the contouring reference (contouring.cpp:94-124 reads these numbers out of RosTools::Spline2D, which
     * is not in the reference tree): x(t) = ax t^3 + bx t^2 + cx t + dx, same for y, t = s - start. */
    struct PathSegment { double ax, bx, cx, dx, ay, by, cy, dy, start; };
    /* its eight coefficients as the array mpc_planner_types/prep_arithmetic.h and the device buffers take: (ax bx cx dx ay by cy dy) */
    inline void coefficients(const PathSegment &c, double o[8]) { o[0] = c.ax; o[1] = c.bx; o[2] = c.cx; o[3] = c.dx; o[4] = c.ay; o[5] = c.by; o[6] = c.cy; o[7] = c.dy; }

    /* Waypoints as they arrive (the reference's ReferencePath, mpc_planner_types/data_types.h:93-111): x, y, and optionally the heading psi
     * (not used by the fit), the velocity v at each waypoint and the path parameter s of each waypoint (empty: chord lengths). */
    struct ReferencePath
    {
        std::vector<double> x, y, psi, v, s;
        void clear() { x.clear(); y.clear(); psi.clear(); v.clear(); s.clear(); }
        bool empty() const { return x.empty(); }
        bool hasVelocity() const { return !v.empty(); }
        bool hasDistance() const { return !s.empty(); }
    };
    typedef ReferencePath Boundary;

    /* One space-time node of a guidance trajectory as the guidance search delivers it: the time spline through the nodes is
     * mpc_planner_modules/guidance_handoff.h's GuidanceSpline. */
    struct GuidanceNode { double t, x, y; };
}
#endif
