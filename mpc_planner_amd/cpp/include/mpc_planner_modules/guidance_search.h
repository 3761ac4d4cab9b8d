/*
 * mpc_planner_modules/guidance_search.h (HIP flavour) -- the guidance search on the host: MPCPlanner::guidanceSearch is
 * tmpc_guidance_search (include/tmpc_hip_guidance_search.h) for callers of the C++ mirror, on host arrays in the device's layouts, and the CPU
 * check of the kernel's indexing.  Header-only, Solver-free, no GPU.  The reference's search is the external guidance_planner, whose source is
 * not in the reference tree: the method is this project's own restatement -- a visibility-PRM on the stage grid, winding numbers
 * as the homotopy test, one path per class, the n_paths cheapest.  The search of a scene is tmpc_arith::gs_scene of
 * mpc_planner_types/prep_arithmetic.h, the one source tmpc_guidance_search_kernel compiles too, here with one lane; the independent statement
 * both are tested against, bit for bit, is mpc_planner_amd/modules.py guidance_search.  Build with -ffp-contract=off.
 */
#ifndef MPC_GUIDANCE_SEARCH_HIP_H
#define MPC_GUIDANCE_SEARCH_HIP_H

#include <cstddef>
#include <cstdint>
#include <memory>

#include <mpc_planner_types/prep_arithmetic.h>

namespace MPCPlanner
{
    /* the fields of tmpc_guidance_search_options behind `size` */
    using GuidanceSearchOptions = tmpc_arith::GsOptions;

    /* the configuration the reference ships (guidance_planner.yaml: n_paths 4, n_samples 30) */
    inline GuidanceSearchOptions guidanceSearchDefaults()
    {
        return GuidanceSearchOptions{4, 30, 64, 4096, 0ull, 0.325, 3.0, 0.5, 1.0};
    }

    /* One tick of n_scenes scenes: every array as tmpc_guidance_search documents it (was_reset may be null), N and dt the solver's.
     * The scenes in order.  false: refused, nothing written. */
    inline bool guidanceSearch(int n_scenes, int n_goals, int max_obstacles, int N, double dt, const GuidanceSearchOptions &o, const double *state4,
                               const double *goals, const double *obstacle_pos, const double *obstacle_radius, const int32_t *selected,
                               const uint8_t *was_reset, double *prev_traj, int32_t *prev_class, int32_t *prev_count, int32_t *next_class,
                               double *nodes, int32_t *node_count, int32_t *traj_count, int32_t *topology_class, int32_t *status)
    {
        if (!tmpc_arith::gs_valid(o, n_scenes, n_goals, max_obstacles, N)) return false;
        if (!state4 || !goals || !obstacle_pos || !obstacle_radius || !selected || !prev_traj || !prev_class || !prev_count || !next_class || !nodes ||
            !node_count || !traj_count || !topology_class || !status)
            return false;
        std::unique_ptr<tmpc_arith::GsWork> work(new tmpc_arith::GsWork());
        const tmpc_arith::GsOneLane one;
        for (int q = 0; q < n_scenes; q++)
            tmpc_arith::gs_scene(one, *work, q, N, dt, n_goals, max_obstacles, o, state4, goals, obstacle_pos, obstacle_radius, selected, was_reset,
                                 prev_traj, prev_class, prev_count, next_class, nodes, node_count, traj_count, topology_class, status);
        return true;
    }
}
#endif
