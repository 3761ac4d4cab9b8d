/* mpc_planner_types/path_segment.h -- one cubic segment of the contouring reference, on its own so that Solver-free headers
 * (mpc_planner_modules/reference_path.h) can use it without the generated solver dimensions. */
#ifndef MPC_PATH_SEGMENT_HIP_H
#define MPC_PATH_SEGMENT_HIP_H

namespace MPCPlanner
{
    /* One cubic segment of the contouring reference (contouring.cpp:94-124 reads these numbers out of RosTools::Spline2D, which
     * is not in the reference tree): x(t) = ax t^3 + bx t^2 + cx t + dx, same for y, t = s - start. */
    struct PathSegment { double ax, bx, cx, dx, ay, by, cy, dy, start; };
}
#endif
