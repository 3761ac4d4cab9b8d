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
}
#endif
