// mpc_planner_amd/csrc/tmpc_guidance_search_entry.hpp -- the entry point of include/tmpc_hip_guidance_search.h: the checks, then one launch of
// tmpc_guidance_search_kernel (tmpc_guidance_search.hpp), one wave per scene, on the handle's stream.  It touches no parameter row and needs no
// batch (the handle's N, dt and stream only), so it is the same in a generated solver.  Part of the C-ABI translation unit: tmpc_capi.hip
// includes this file once, behind its handle, TMPC_HIP_CHECK and read_options, so that the one-translation-unit builds of the generated
// libraries carry it too.
#pragma once
#include "../../include/tmpc_hip_guidance_search.h"
#include "tmpc_guidance_search.hpp"

// every horizon a handle can have fits the search's tables: N + 1 stages per table row
static_assert(tmpc::STAGE_MAX + 1 <= tmpc_arith::GS_MAX_STAGES, "the stage tables of tmpc_arith::GsWork are too short for STAGE_MAX");

extern "C" int tmpc_guidance_search(tmpc_handle *h, int32_t n_scenes, int32_t n_goals, int32_t max_obstacles, const tmpc_guidance_search_options *opt,
                                    const void *d_state4, const void *d_goals, const void *d_obstacle_pos, const void *d_obstacle_radius,
                                    const void *d_selected, const void *d_was_reset, void *d_prev_traj, void *d_prev_class, void *d_prev_count,
                                    void *d_next_class, void *d_nodes, void *d_node_count, void *d_traj_count, void *d_topology_class, void *d_status)
{
    if (!h) return TMPC_ERR_INVALID;
    const std::string who = "tmpc_guidance_search: ";
    if (!opt) { h->err = who + "NULL options"; return TMPC_ERR_INVALID; }
    tmpc_guidance_search_options o{};
    if (!read_options(h, "tmpc_guidance_search", "tmpc_guidance_search_options", opt, o)) return TMPC_ERR_INVALID;
    const double inf = __builtin_huge_val();
    if (o.reserved != 0) { h->err = who + "options->reserved must be 0"; return TMPC_ERR_INVALID; }
    if (n_scenes <= 0) { h->err = who + "n_scenes must be positive"; return TMPC_ERR_INVALID; }
    if (n_goals < 1 || n_goals > tmpc_arith::GS_MAX_GOALS) { h->err = who + "1 <= n_goals <= 16"; return TMPC_ERR_INVALID; }
    if (max_obstacles < 1 || max_obstacles > tmpc_arith::GS_MAX_OBSTACLES) { h->err = who + "1 <= max_obstacles <= 32"; return TMPC_ERR_INVALID; }
    if (o.n_paths < 1 || o.n_paths > tmpc_arith::GS_KEPT) { h->err = who + "1 <= n_paths <= 16"; return TMPC_ERR_INVALID; }
    if (o.n_samples < 0 || o.n_samples > tmpc_arith::GS_MAX_SAMPLES) { h->err = who + "0 <= n_samples <= 256"; return TMPC_ERR_INVALID; }
    if (o.n_nodes_max < 2 || o.n_nodes_max > tmpc_arith::GS_MAX_NODES) { h->err = who + "2 <= n_nodes_max <= 64"; return TMPC_ERR_INVALID; }
    if (o.max_expansions < 1 || o.max_expansions > tmpc_arith::GS_MAX_EXPANSIONS) { h->err = who + "1 <= max_expansions <= 65536"; return TMPC_ERR_INVALID; }
    if (!(o.robot_radius >= 0.0)) { h->err = who + "robot_radius must not be negative"; return TMPC_ERR_INVALID; }
    if (!(o.max_velocity > 0.0) || !(o.max_velocity < inf)) { h->err = who + "max_velocity must be positive and finite"; return TMPC_ERR_INVALID; }
    if (!(o.weight_length > 0.0) || !(o.weight_length < inf)) { h->err = who + "weight_length must be positive and finite"; return TMPC_ERR_INVALID; }
    if (!(o.margin >= 0.0) || !(o.margin < inf)) { h->err = who + "margin must be finite and not negative"; return TMPC_ERR_INVALID; }
    if (!d_state4 || !d_goals || !d_obstacle_pos || !d_obstacle_radius || !d_selected) {
        h->err = who + "NULL input (d_state4, d_goals, d_obstacle_pos, d_obstacle_radius, d_selected)"; return TMPC_ERR_INVALID;
    }
    if (!d_prev_traj || !d_prev_class || !d_prev_count || !d_next_class) {
        h->err = who + "NULL carried array (d_prev_traj, d_prev_class, d_prev_count, d_next_class)"; return TMPC_ERR_INVALID;
    }
    if (!d_nodes || !d_node_count || !d_traj_count || !d_topology_class || !d_status) {
        h->err = who + "NULL output (d_nodes, d_node_count, d_traj_count, d_topology_class, d_status)"; return TMPC_ERR_INVALID;
    }
    const tmpc_arith::GsOptions k{o.n_paths, o.n_samples, o.n_nodes_max, o.max_expansions, (unsigned long long)o.seed, o.robot_radius, o.max_velocity,
                                  o.margin, o.weight_length};
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(tmpc::tmpc_guidance_search_kernel, dim3((unsigned)n_scenes), dim3(64), 0, h->stream, h->d.N, h->d.dt, n_goals, max_obstacles, k,
                       (const double *)d_state4, (const double *)d_goals, (const double *)d_obstacle_pos, (const double *)d_obstacle_radius,
                       (const int *)d_selected, (const uint8_t *)d_was_reset, (double *)d_prev_traj, (int *)d_prev_class, (int *)d_prev_count,
                       (int *)d_next_class, (double *)d_nodes, (int *)d_node_count, (int *)d_traj_count, (int *)d_topology_class, (int *)d_status);
    TMPC_HIP_CHECK(h, hipGetLastError());
    return TMPC_OK;
}
