/*
 * mpc_planner/data_preparation.h (HIP flavour) -- the reference's obstacle preparation (mpc_planner/include/mpc_planner/data_preparation.h,
 * mpc_planner/src/data_preparation.cpp) with its six functions, their names and signatures, on the Eigen-free types of
 * mpc_planner_types/data_types.h.  The reference reads the global CONFIG; these read a ModuleConfig passed as the last argument (N,
 * integrator_step, max_obstacles, max_obstacle_distance, probabilistic_enable).  The arithmetic is that of
 * mpc_planner_types/prep_arithmetic.h, the one source tmpc_prepare_obstacles_kernel compiles too; the independent statement both are tested
 * against is mpc_planner_amd/modules.py (prepare_obstacles and its parts): values agree bit for bit, and so does the
 * selection wherever the ranking keys differ (ties: the lower index, DESIGN.md U13 -- the reference's std::sort leaves them unspecified).
 * The batched device twin is mpc_planner/data_preparation_batch.h.
 */
#ifndef MPC_DATA_PREPARATION_HIP_H
#define MPC_DATA_PREPARATION_HIP_H

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include <mpc_planner_modules/modules_hip.h>
#include <mpc_planner_types/prep_arithmetic.h>

namespace MPCPlanner
{
    /* data_preparation.cpp:16-47 */
    inline std::vector<Disc> defineRobotArea(double length, double width, int n_discs)
    {
        const double center_offset = length / 2.;                      // where the centre is w.r.t. the back of the vehicle
        const double radius = width / 2.;
        std::vector<Disc> robot_area;
        if (n_discs <= 0) { std::fprintf(stderr, "Trying to create a collision region with less than a disc\n"); std::abort(); }     // ROSTOOLS_ASSERT (:23)
        if (n_discs == 1) {
            robot_area.emplace_back(0., radius);
        } else {
            for (int i = 0; i < n_discs; i++) {
                if (i == 0) robot_area.emplace_back(-center_offset + radius, radius);                                  // first disc at the back
                else if (i == n_discs - 1) robot_area.emplace_back(-center_offset + length - radius, radius);         // last disc at the front
                else robot_area.emplace_back(-center_offset + radius + (double)i * (length - 2. * radius) / ((double)(n_discs - 1.)), radius);
            }
        }
        return robot_area;
    }

    /* :49-56 */
    inline DynamicObstacle getDummyObstacle(const State &state)
    {
        return DynamicObstacle(-1, Vector2d(tmpc_arith::dummy_coordinate(state.get("x")), tmpc_arith::dummy_coordinate(state.get("y"))), 0., 0.);
    }

    /* :170-186 */
    inline void propagatePredictionUncertainty(Prediction &prediction, const ModuleConfig &cfg)
    {
        if (prediction.type != PredictionType::GAUSSIAN) return;
        const double dt = cfg.integrator_step;
        double major = 0., minor = 0.;
        for (int k = 0; k < cfg.N; k++) {
            major = tmpc_arith::propagate_step(major, prediction.modes[0][k].major_radius, dt);
            minor = tmpc_arith::propagate_step(minor, prediction.modes[0][k].minor_radius, dt);
            prediction.modes[0][k].major_radius = major;
            prediction.modes[0][k].minor_radius = minor;
        }
    }
    /* :188-192 */
    inline void propagatePredictionUncertainty(std::vector<DynamicObstacle> &obstacles, const ModuleConfig &cfg)
    {
        for (auto &obstacle : obstacles) propagatePredictionUncertainty(obstacle.prediction, cfg);
    }

    /* :58-79 */
    inline Prediction getConstantVelocityPrediction(const Vector2d &position, const Vector2d &velocity, double dt, int steps, const ModuleConfig &cfg)
    {
        Prediction prediction;
        double noise = 0.;
        if (cfg.probabilistic_enable) { prediction = Prediction(PredictionType::GAUSSIAN); noise = 0.3; }
        else prediction = Prediction(PredictionType::DETERMINISTIC);
        for (int i = 0; i < steps; i++)
            prediction.modes[0].push_back(PredictionStep(Vector2d(tmpc_arith::cv_step(position(0), velocity(0), dt, i), tmpc_arith::cv_step(position(1), velocity(1), dt, i)),
                                                         0., noise, noise));
        if (cfg.probabilistic_enable) propagatePredictionUncertainty(prediction, cfg);
        return prediction;
    }

    /* :81-93 */
    inline void removeDistantObstacles(std::vector<DynamicObstacle> &obstacles, const State &state, const ModuleConfig &cfg)
    {
        std::vector<DynamicObstacle> nearby_obstacles;
        const Vector2d pos = state.getPos();
        for (auto &obstacle : obstacles)
            if (tmpc_arith::within_distance(obstacle.position(0), obstacle.position(1), pos(0), pos(1), cfg.max_obstacle_distance)) nearby_obstacles.push_back(obstacle);
        obstacles = nearby_obstacles;
    }

    /* the ranking key of :113-131: the minimum over k < N of tmpc_arith::selection_key_term */
    inline double obstacleSelectionDistance(const DynamicObstacle &obstacle, const State &state, const ModuleConfig &cfg)
    {
        double min_dist = tmpc_arith::SELECTION_KEY_START;
        const double c = std::cos(state.get("psi")), s = std::sin(state.get("psi"));
        const Vector2d pos = state.getPos();
        const double v = state.get("v");
        for (int k = 0; k < cfg.N; k++) {
            const Vector2d &o = obstacle.prediction.modes[0][k].position;
            const double dist = tmpc_arith::selection_key_term(k, o(0), o(1), pos(0), pos(1), v, c, s);
            if (dist < min_dist) min_dist = dist;
        }
        return min_dist;
    }

    /* :95-168.  `selected` (optional): for every obstacle of the result its index in the list that came in, -1 for a dummy. */
    inline void ensureObstacleSize(std::vector<DynamicObstacle> &obstacles, const State &state, const ModuleConfig &cfg, std::vector<int> *selected = nullptr)
    {
        const size_t max_obstacles = (size_t)cfg.max_obstacles;
        std::vector<int> indices(obstacles.size());
        std::iota(indices.begin(), indices.end(), 0);
        if (obstacles.size() > max_obstacles) {                         // more: sort and keep the closest
            std::vector<double> distances;
            for (auto &obstacle : obstacles) distances.push_back(obstacleSelectionDistance(obstacle, state, cfg));
            std::sort(indices.begin(), indices.end(), [&](const int a, const int b) { return distances[a] < distances[b] || (distances[a] == distances[b] && a < b); });
            std::vector<DynamicObstacle> processed_obstacles;
            for (size_t v = 0; v < max_obstacles; v++) processed_obstacles.push_back(obstacles[indices[v]]);
            for (size_t i = 0; i < processed_obstacles.size(); i++) processed_obstacles[i].index = (int)i;           // sequential IDs
            obstacles = processed_obstacles;
            indices.resize(max_obstacles);
        } else if (obstacles.size() < max_obstacles) {                  // fewer: dummies
            for (size_t cur_size = obstacles.size(); cur_size < max_obstacles; cur_size++) {
                obstacles.push_back(getDummyObstacle(state));
                auto &obstacle = obstacles.back();
                obstacle.prediction = getConstantVelocityPrediction(obstacle.position, Vector2d(0., 0.), cfg.integrator_step, cfg.N, cfg);
                indices.push_back(-1);
            }
        }
        if (selected) *selected = indices;
    }
}
#endif
