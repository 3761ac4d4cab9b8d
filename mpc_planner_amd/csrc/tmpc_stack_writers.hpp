// mpc_planner_amd/csrc/tmpc_stack_writers.hpp -- the entry points of include/tmpc_hip_stack.h: the obstacle and topology rows of a generated
// solver's module stack, written into columns the caller names.  Part of the C-ABI translation unit: tmpc_capi.hip includes this file once, behind
// its handle, TMPC_HIP_CHECK and read_options, so that the one-translation-unit builds of the generated libraries carry the entry points too.  The
// kernels are the templates of tmpc_aux_kernels.hpp (LayoutRows / ColumnRows): the arithmetic of the hand-written layout's writers, one source.
#pragma once
#include "../../include/tmpc_hip_stack.h"

// tmpc_prepare_obstacles and tmpc_stack_prepare_obstacles: the checks and the launch (fn: the entry point's name, for the messages).  Uses N, dt
// and the stream of the handle only.
static int prepare_obstacles_checked(tmpc_handle *h, const char *fn, int32_t n_scenes, int32_t n_slots, int32_t max_obstacles, const void *d_count,
                                     const void *d_state, const void *d_raw_pos, const void *d_raw_radius, const void *d_raw_vel, const void *d_raw_pred,
                                     const tmpc_obstacle_options *options, void *d_obstacle_pos, void *d_obstacle_shape, void *d_obstacle_radius,
                                     void *d_obstacle_gaussian, void *d_selected)
{
    if (!h) return TMPC_ERR_INVALID;
    const std::string who = std::string(fn) + ": ";
    tmpc_obstacle_options o{};                                        // NULL: the defaults (deterministic, no passes, no distance filter)
    o.size = sizeof(o); o.noise = 0.3;
    if (!read_options(h, fn, "tmpc_obstacle_options", options, o)) return TMPC_ERR_INVALID;
    if (n_scenes <= 0) { h->err = who + "n_scenes must be positive"; return TMPC_ERR_INVALID; }
    if (n_slots < 0 || n_slots > tmpc::PREP_MAX_SLOTS) { h->err = who + "0 <= n_slots <= 1024"; return TMPC_ERR_INVALID; }
    if (max_obstacles <= 0 || max_obstacles > 4096) { h->err = who + "1 <= max_obstacles <= 4096"; return TMPC_ERR_INVALID; }
    if (!d_count || !d_state || !d_raw_pos || !d_raw_radius) { h->err = who + "NULL input (d_count, d_state, d_raw_pos, d_raw_radius)"; return TMPC_ERR_INVALID; }
    if ((d_raw_vel == nullptr) == (d_raw_pred == nullptr)) { h->err = who + "exactly one of d_raw_vel and d_raw_pred"; return TMPC_ERR_INVALID; }
    if (!d_obstacle_pos || !d_obstacle_shape || !d_obstacle_radius || !d_obstacle_gaussian || !d_selected) {
        h->err = who + "NULL output buffer"; return TMPC_ERR_INVALID;
    }
    if (o.propagate_passes < 0 || o.propagate_passes > 2) { h->err = who + "propagate_passes is 0, 1 or 2"; return TMPC_ERR_INVALID; }
    if ((o.probabilistic != 0 && o.probabilistic != 1) || !(o.noise >= 0.0)) { h->err = who + "probabilistic is 0 or 1, noise >= 0"; return TMPC_ERR_INVALID; }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(tmpc::tmpc_prepare_obstacles_kernel, dim3((unsigned)n_scenes), dim3(tmpc::PREP_THREADS), (size_t)max_obstacles * sizeof(int), h->stream,
                       h->d.N, h->d.dt, n_slots, max_obstacles, (const int *)d_count, (const double *)d_state, (const double *)d_raw_pos,
                       (const double *)d_raw_radius, (const double *)d_raw_vel, (const double *)d_raw_pred, o.probabilistic, o.noise, o.propagate_passes,
                       o.max_obstacle_distance, (double *)d_obstacle_pos, (double *)d_obstacle_shape, (double *)d_obstacle_radius,
                       (uint8_t *)d_obstacle_gaussian, (int *)d_selected);
    TMPC_HIP_CHECK(h, hipGetLastError());
    return TMPC_OK;
}

// The caller's column table into the kernel argument: every entry inside [0, npar), all distinct (two threads never write one address), as in
// tmpc_scatter_parameters.  n_cols is already known to be in [1, 128].
static bool read_stack_columns(tmpc_handle *h, const std::string &who, const int32_t *cols, int n_cols, tmpc::ScatterCols &list)
{
    list.n = n_cols;
    for (int i = 0; i < n_cols; i++) {
        if (cols[i] < 0 || cols[i] >= h->d.npar) { h->err = who + "cols holds a column outside [0, npar)"; return false; }
        for (int j = 0; j < i; j++)
            if (cols[j] == cols[i]) { h->err = who + "cols holds a duplicate column (the value written would depend on thread order)"; return false; }
        list.col[i] = cols[i];
    }
    return true;
}

extern "C" {

int tmpc_stack_prepare_obstacles(tmpc_handle *h, int32_t n_scenes, int32_t n_slots, int32_t max_obstacles, const void *d_count, const void *d_state,
                                 const void *d_raw_pos, const void *d_raw_radius, const void *d_raw_vel, const void *d_raw_pred,
                                 const tmpc_obstacle_options *options, void *d_obstacle_pos, void *d_obstacle_shape, void *d_obstacle_radius,
                                 void *d_obstacle_gaussian, void *d_selected)
{
    return prepare_obstacles_checked(h, "tmpc_stack_prepare_obstacles", n_scenes, n_slots, max_obstacles, d_count, d_state, d_raw_pos, d_raw_radius, d_raw_vel,
                                     d_raw_pred, options, d_obstacle_pos, d_obstacle_shape, d_obstacle_radius, d_obstacle_gaussian, d_selected);
}

int tmpc_stack_set_obstacle_columns(tmpc_handle *h, const int32_t *cols, int32_t n_cols, int32_t row_model, int32_t max_obstacles,
                                    const void *d_obstacle_pos, const void *d_obstacle_shape, const void *d_obstacle_radius, const void *d_obstacle_gaussian,
                                    const void *d_scene_of, const void *d_state, double robot_radius, double disc_offset, double risk, double chi, double obstacle_radius)
{
    if (!h) return TMPC_ERR_INVALID;
    const std::string who = "tmpc_stack_set_obstacle_columns: ";
    if (h->B <= 0 || !h->params) { h->err = who + "no batch (call tmpc_set_batch* first)"; return TMPC_ERR_INVALID; }
    if (row_model != 0 && row_model != 1) { h->err = who + "row_model is 0 (ellipsoids) or 1 (Gaussian rows)"; return TMPC_ERR_INVALID; }
    if (max_obstacles < 1) { h->err = who + "max_obstacles must be at least 1"; return TMPC_ERR_INVALID; }
    if (!cols || !d_obstacle_pos || !d_obstacle_shape || !d_obstacle_radius || !d_obstacle_gaussian || !d_scene_of || !d_state) {
        h->err = who + "NULL argument (cols, d_obstacle_pos, d_obstacle_shape, d_obstacle_radius, d_obstacle_gaussian, d_scene_of, d_state)"; return TMPC_ERR_INVALID;
    }
    const int64_t want = 2 + (int64_t)(row_model == 1 ? 6 : 7) * max_obstacles;
    if (n_cols != want || n_cols > tmpc::SCATTER_MAX_COLS) {
        h->err = who + "n_cols must be 2 + 7 max_obstacles (row_model 0) or 2 + 6 max_obstacles (row_model 1), at most 128"; return TMPC_ERR_INVALID;
    }
    tmpc::ColumnRows where{};
    where.count = max_obstacles; where.model = row_model;
    if (!read_stack_columns(h, who, cols, n_cols, where.t)) return TMPC_ERR_INVALID;
    const int64_t n = (int64_t)h->B * h->d.N * max_obstacles;
    if (n > 0x7fffffff) { h->err = who + "B x N x max_obstacles too large"; return TMPC_ERR_INVALID; }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(tmpc::tmpc_set_obstacle_columns_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->d, h->B,
                       const_cast<double *>(h->params), (const double *)d_obstacle_pos, (const double *)d_obstacle_shape,
                       (const double *)d_obstacle_radius, (const uint8_t *)d_obstacle_gaussian, (const int *)d_scene_of, (const double *)d_state,
                       robot_radius, disc_offset, chi, risk, obstacle_radius, where);
    TMPC_HIP_CHECK(h, hipGetLastError());
    return TMPC_OK;
}

int tmpc_stack_linearize_topology_columns(tmpc_handle *h, const int32_t *cols, int32_t n_rows, const void *d_obstacle_pos, int32_t n_obstacles,
                                          const void *d_obstacle_radius, const void *d_static_halfspaces, int32_t n_static, const void *d_scene_of, const void *d_state_x,
                                          double robot_radius, const void *d_is_original)
{
    if (!h) return TMPC_ERR_INVALID;
    const std::string who = "tmpc_stack_linearize_topology_columns: ";
    if (h->B <= 0 || !h->params || !h->x0) { h->err = who + "no batch (call tmpc_set_batch* first)"; return TMPC_ERR_INVALID; }
    if (n_rows < 1 || 3 * (int64_t)n_rows > tmpc::SCATTER_MAX_COLS) { h->err = who + "n_rows must be at least 1 and 3 n_rows at most 128"; return TMPC_ERR_INVALID; }
    if (!cols || !d_scene_of || !d_state_x) { h->err = who + "NULL argument (cols, d_scene_of, d_state_x)"; return TMPC_ERR_INVALID; }
    if (n_obstacles < 0 || n_static < 0 || (int64_t)n_obstacles + n_static > n_rows) {
        h->err = who + "more obstacle + static rows than n_rows (n_obstacles, n_static >= 0, n_obstacles + n_static <= n_rows)"; return TMPC_ERR_INVALID;
    }
    if (n_obstacles > 0 && !d_obstacle_pos) { h->err = who + "NULL d_obstacle_pos with n_obstacles > 0"; return TMPC_ERR_INVALID; }
    if (n_static > 0 && !d_static_halfspaces) { h->err = who + "NULL d_static_halfspaces with n_static > 0"; return TMPC_ERR_INVALID; }
    tmpc::ColumnRows where{};
    where.count = n_rows; where.model = 0;
    if (!read_stack_columns(h, who, cols, 3 * n_rows, where.t)) return TMPC_ERR_INVALID;
    const int64_t n = (int64_t)h->B * h->d.N;
    if (n > 0x7fffffff) { h->err = who + "B x N too large"; return TMPC_ERR_INVALID; }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(tmpc::tmpc_linearize_topology_columns_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->d, h->B,
                       h->x0, const_cast<double *>(h->params), (const double *)d_obstacle_pos, (const int *)d_scene_of,
                       (const double *)d_state_x, robot_radius, (const uint8_t *)d_is_original, n_obstacles, (const double *)d_obstacle_radius,
                       (const double *)d_static_halfspaces, n_static, where);
    TMPC_HIP_CHECK(h, hipGetLastError());
    return TMPC_OK;
}

}  // extern "C"
