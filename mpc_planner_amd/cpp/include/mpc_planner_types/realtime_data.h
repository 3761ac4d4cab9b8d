/*
 * mpc_planner_types/realtime_data.h (HIP flavour) -- what the accelerated path reads of the per-tick sensor data; written
 * after mpc_planner_types/include/mpc_planner_types/realtime_data.h:16-51 (member names and reset() semantics kept so that module
 * code compiles unchanged; the past trajectory is not on this path and stays with the reference's own header in a full tree).  The costmap is
 * on it since DecompConstraints reads it (decomp_constraints.cpp:122-148): a pointer, null by default, to a costmap_2d::Costmap2D
 * (mpc_planner_types/costmap.h holds the members that are read; a full tree passes its own).
 * The reference path is on it since Contouring::update tracks it (contouring.cpp:28-48): the reference keeps waypoints and fits a
 * RosTools::Spline2D (absent); here `reference_path` holds the fitted cubics of the whole path, empty = the caller supplies the window in
 * ModuleData::path; waypoints go into `reference_path_points` (and `left_bound_points` / `right_bound_points`), from which
 * Contouring::onDataReceived fits the cubics (mpc_planner_modules/reference_path.h).  The road bounds ARE on the path (Contouring::constructRoadConstraintsFromBounds, contouring.cpp:237-262): the
 * reference keeps them as point lists and fits RosTools::Spline2D objects on the centreline's knot vector (:142-149); ros_tools is absent, so
 * here they are the fitted cubics themselves, one PathSegment per segment of ModuleData::path (same window, same knots).
 */
#ifndef MPC_REALTIME_DATA_HIP_H
#define MPC_REALTIME_DATA_HIP_H

#include <chrono>
#include <utility>
#include <vector>

#include <mpc_planner_types/costmap.h>
#include <mpc_planner_types/data_types.h>

namespace MPCPlanner
{
    struct RealTimeData
    {
        // consumers on the path:
        std::vector<DynamicObstacle> dynamic_obstacles;                       // Ellipsoid-/LinearizedConstraints::setParameters, update
        std::vector<Disc> robot_area;                                         // ego_disc_<d>_offset parameters
        std::chrono::system_clock::time_point planning_start_time;           // solver_timeout bookkeeping of the optimize() loops
        Vector2d goal;                                                        // GoalModule (generated solvers)
        bool goal_received{false};
        double intrusion{0.};                                                 // feedback value published by the ROS wrappers
        std::vector<PathSegment> left_bound, right_bound;                     // Contouring's road constraints; aligned with ModuleData::path, empty = not supplied
        std::vector<PathSegment> reference_path;                              // the WHOLE path (fitted cubics); non-empty: Contouring::update finds the closest point and
        double reference_path_length{0.};                                     // the window itself, and the bounds above are aligned with THIS vector; the knot behind the last segment
        ReferencePath reference_path_points;                                  // waypoints as they arrive (the reference's RealTimeData::reference_path); non-empty:
        Boundary left_bound_points, right_bound_points;                       // Contouring::onDataReceived("reference_path") fits reference_path / left_bound / right_bound from them
        costmap_2d::Costmap2D *costmap{nullptr};                              // DecompConstraints::getOccupiedGridCells; not owned (reference :24)

        // Everything but the robot's disc model is per-tick data (reference :37-47).
        void reset()
        {
            RealTimeData fresh;
            fresh.robot_area = std::move(robot_area);
            *this = std::move(fresh);
        }
    };
}
#endif
