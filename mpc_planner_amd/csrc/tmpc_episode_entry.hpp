// mpc_planner_amd/csrc/tmpc_episode_entry.hpp -- the entry point of include/tmpc_hip_episode.h: the checks, then one launch of
// tmpc_episode_step_kernel (tmpc_aux_kernels.hpp), one wave per scene, on the handle's stream.  It touches no parameter row and needs no batch
// (the handle's nx and stream only), so it is the same in a generated solver.  Part of the C-ABI translation unit: tmpc_capi.hip includes this
// file once, behind its handle, TMPC_HIP_CHECK and read_options, so that the one-translation-unit builds of the generated libraries carry it too.
#pragma once
#include "../../include/tmpc_hip_episode.h"

extern "C" int tmpc_episode_step(tmpc_handle *h, int32_t n_scenes, int32_t n_slots, int32_t P, const tmpc_episode_options *opt, const void *d_cmd,
                                 void *d_plant, const void *d_plant0, const void *d_count, void *d_raw_pos, void *d_raw_vel, const void *d_raw_radius,
                                 const void *d_raw_pos0, const void *d_raw_vel0, const void *d_box, const void *d_goal, void *d_episode,
                                 void *d_episode_f, void *d_log, void *d_was_reset, void *d_state4, void *d_state_nx, void *d_state_batch,
                                 void *d_planner_ids, void *d_selection, void *d_segment)
{
    if (!h) return TMPC_ERR_INVALID;
    const std::string who = "tmpc_episode_step: ";
    if (!opt) { h->err = who + "NULL options"; return TMPC_ERR_INVALID; }
    tmpc_episode_options o{};
    if (!read_options(h, "tmpc_episode_step", "tmpc_episode_options", opt, o)) return TMPC_ERR_INVALID;
    if (n_scenes <= 0) { h->err = who + "n_scenes must be positive"; return TMPC_ERR_INVALID; }
    if (n_slots < 0 || n_slots > tmpc::EPISODE_MAX_SLOTS) { h->err = who + "0 <= n_slots <= 1024"; return TMPC_ERR_INVALID; }
    if (P < 1) { h->err = who + "P must be at least 1"; return TMPC_ERR_INVALID; }
    if (o.substeps < 1 || o.substeps > tmpc::EPISODE_MAX_SUBSTEPS) { h->err = who + "1 <= substeps <= 16"; return TMPC_ERR_INVALID; }
    if (!(o.control_dt > 0.0) || !(o.control_dt < __builtin_huge_val())) { h->err = who + "control_dt must be positive and finite"; return TMPC_ERR_INVALID; }
    if (!(o.max_angular_velocity > 0.0)) { h->err = who + "max_angular_velocity must be positive"; return TMPC_ERR_INVALID; }
    if (!(o.max_angular_velocity * o.control_dt / (double)o.substeps <= 0.125)) {
        h->err = who + "max_angular_velocity control_dt / substeps must be at most 0.125 (the plant's polynomials are stated for a half angle up to 1/16)";
        return TMPC_ERR_INVALID;
    }
    if (o.max_episodes < 1 || o.max_episodes > tmpc::EPISODE_MAX_LOG) { h->err = who + "1 <= max_episodes <= 4096"; return TMPC_ERR_INVALID; }
    if (o.timeout_ticks < 0) { h->err = who + "timeout_ticks must not be negative"; return TMPC_ERR_INVALID; }
    if (!(o.robot_radius >= 0.0)) { h->err = who + "robot_radius must not be negative"; return TMPC_ERR_INVALID; }
    if (!d_cmd || !d_plant0 || !d_count || !d_raw_radius || !d_raw_pos0 || !d_raw_vel0) {
        h->err = who + "NULL input (d_cmd, d_plant0, d_count, d_raw_radius, d_raw_pos0, d_raw_vel0)"; return TMPC_ERR_INVALID;
    }
    if (!d_plant || !d_raw_pos || !d_raw_vel || !d_episode || !d_episode_f) {
        h->err = who + "NULL carried array (d_plant, d_raw_pos, d_raw_vel, d_episode, d_episode_f)"; return TMPC_ERR_INVALID;
    }
    if (!d_log || !d_was_reset || !d_state4) { h->err = who + "NULL output (d_log, d_was_reset, d_state4)"; return TMPC_ERR_INVALID; }
    const tmpc::EpisodeOptions k{o.substeps, o.timeout_ticks, o.max_episodes, o.control_dt, o.max_acceleration, o.max_angular_velocity, o.robot_radius,
                                 o.goal_x};
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(tmpc::tmpc_episode_step_kernel, dim3((unsigned)n_scenes), dim3(64), 0, h->stream, n_slots, P, tmpc::ext_nx(h->d), k,
                       (const double *)d_cmd, (double *)d_plant, (const double *)d_plant0, (const int *)d_count, (double *)d_raw_pos, (double *)d_raw_vel,
                       (const double *)d_raw_radius, (const double *)d_raw_pos0, (const double *)d_raw_vel0, (const double *)d_box, (const double *)d_goal,
                       (int *)d_episode, (double *)d_episode_f, (double *)d_log, (uint8_t *)d_was_reset, (double *)d_state4, (double *)d_state_nx,
                       (double *)d_state_batch, (int *)d_planner_ids, (int *)d_selection, (int *)d_segment);
    TMPC_HIP_CHECK(h, hipGetLastError());
    return TMPC_OK;
}
