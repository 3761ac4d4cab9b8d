// mpc_planner_amd/csrc/tmpc_row_entries.hpp -- the entry points of the device row writers, by writer.  Every writer has two destinations: the
// hand-written kernels' parameter layout (include/tmpc_hip.h) and the columns of a generated solver's module stack that the caller names
// (include/tmpc_hip_stack.h, tmpc_hip_stack_env.h, tmpc_hip_stack_scenario.h).  The rule: ONE BODY PER WRITER, TWO THIN ENTRY POINTS.  The static
// `*_checked` body holds what does not depend on the destination -- batch present, the pointer arguments, n_scenes, the 64-bit size of the flat
// index, the launch -- and takes the entry point's name (fn, for the messages), the kernel and the kernel's trailing `where` (the column table),
// if any.  The layout entry keeps TMPC_NOT_IN_GENERATED_SOLVER, the count out of the handle's dims and first_row; the column entry keeps cols, the
// count's range, the table read and the spline-state refusal.  Part of the C-ABI translation unit: tmpc_capi.hip includes this file once, behind
// its handle, TMPC_HIP_CHECK, TMPC_NOT_IN_GENERATED_SOLVER, read_options and grow_scratch, so that the one-translation-unit builds of the
// generated libraries carry every entry point too.  The kernels are the templates of tmpc_aux_kernels.hpp on Layout*Rows / Column*Rows.
#pragma once
#include <type_traits>
#include "../../include/tmpc_hip_stack.h"
#include "../../include/tmpc_hip_stack_env.h"
#include "../../include/tmpc_hip_stack_scenario.h"

// no batch yet (tmpc_set_batch* sets B, x0 and the parameter rows together)
static bool no_batch(tmpc_handle *h, const std::string &who)
{
    if (h->B > 0 && h->params && h->x0) return false;
    h->err = who + "no batch (call tmpc_set_batch* first)";
    return true;
}

// One thread per flat index e < n, 256 to a workgroup, on the handle's stream; `extent` names n's factors for the refusal of an n beyond int.
template <class Kernel, class... Args>
static int launch_flat(tmpc_handle *h, const std::string &who, const char *extent, int64_t n, Kernel kernel, Args... args)
{
    if (n > 0x7fffffff) { h->err = who + extent + " too large"; return TMPC_ERR_INVALID; }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, args...);
    TMPC_HIP_CHECK(h, hipGetLastError());
    return TMPC_OK;
}

// The caller's column table into the kernel argument: every entry inside [0, npar), all distinct (two threads never write one address).  The
// callers (the column entries below, tmpc_scatter_parameters) have checked that cols is not NULL and n_cols in [1, 128].
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

// the path columns of a call (path window, road rows): n_segments in range, then the table
static bool read_path_columns(tmpc_handle *h, const std::string &who, const int32_t *cols, int32_t n_segments, tmpc::ColumnEnvRows &where)
{
    if (n_segments < 1 || 9 * (int64_t)n_segments > tmpc::SCATTER_MAX_COLS) { h->err = who + "n_segments must be at least 1 and 9 n_segments at most 128"; return false; }
    where.count = n_segments;
    return read_stack_columns(h, who, cols, 9 * n_segments, where.t);
}

// a generated library whose model has no spline state (SecondOrderUnicycleModel: the fifth state slot is inert) has no s to read or write
static bool stack_has_spline_state()
{
#ifdef TMPC_GENERATED_STAGE
    return tmpc_gen::MODEL != 1;
#else
    return true;
#endif
}

// ---- obstacles: the preparation (it writes no parameter row: one kernel; uses N, dt and the stream of the handle only), then the collision rows ---
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

extern "C" int tmpc_prepare_obstacles(tmpc_handle *h, int32_t n_scenes, int32_t n_slots, int32_t max_obstacles, const void *d_count, const void *d_state,
                                      const void *d_raw_pos, const void *d_raw_radius, const void *d_raw_vel, const void *d_raw_pred,
                                      const tmpc_obstacle_options *options, void *d_obstacle_pos, void *d_obstacle_shape, void *d_obstacle_radius,
                                      void *d_obstacle_gaussian, void *d_selected)
{
    TMPC_NOT_IN_GENERATED_SOLVER(h, "tmpc_prepare_obstacles");
    return prepare_obstacles_checked(h, "tmpc_prepare_obstacles", n_scenes, n_slots, max_obstacles, d_count, d_state, d_raw_pos, d_raw_radius, d_raw_vel,
                                     d_raw_pred, options, d_obstacle_pos, d_obstacle_shape, d_obstacle_radius, d_obstacle_gaussian, d_selected);
}

extern "C" int tmpc_stack_prepare_obstacles(tmpc_handle *h, int32_t n_scenes, int32_t n_slots, int32_t max_obstacles, const void *d_count,
                                            const void *d_state, const void *d_raw_pos, const void *d_raw_radius, const void *d_raw_vel,
                                            const void *d_raw_pred, const tmpc_obstacle_options *options, void *d_obstacle_pos, void *d_obstacle_shape,
                                            void *d_obstacle_radius, void *d_obstacle_gaussian, void *d_selected)
{
    return prepare_obstacles_checked(h, "tmpc_stack_prepare_obstacles", n_scenes, n_slots, max_obstacles, d_count, d_state, d_raw_pos, d_raw_radius, d_raw_vel,
                                     d_raw_pred, options, d_obstacle_pos, d_obstacle_shape, d_obstacle_radius, d_obstacle_gaussian, d_selected);
}

// max_obstacles: the obstacles per scene of the destination (the layout's M, the column call's own)
template <class Kernel, class... Where>
static int set_obstacle_rows_checked(tmpc_handle *h, const char *fn, Kernel kernel, int32_t max_obstacles, const void *d_obstacle_pos,
                                     const void *d_obstacle_shape, const void *d_obstacle_radius, const void *d_obstacle_gaussian, const void *d_scene_of,
                                     const void *d_state, double robot_radius, double disc_offset, double risk, double chi, double obstacle_radius,
                                     Where... where)
{
    const std::string who = std::string(fn) + ": ";
    if (no_batch(h, who)) return TMPC_ERR_INVALID;
    if (!d_obstacle_pos || !d_obstacle_shape || !d_obstacle_radius || !d_obstacle_gaussian || !d_scene_of || !d_state) {
        h->err = who + "NULL argument (d_obstacle_pos, d_obstacle_shape, d_obstacle_radius, d_obstacle_gaussian, d_scene_of, d_state)"; return TMPC_ERR_INVALID;
    }
    return launch_flat(h, who, "B x N x max_obstacles", (int64_t)h->B * h->d.N * max_obstacles, kernel, h->d, h->B, const_cast<double *>(h->params),
                       (const double *)d_obstacle_pos, (const double *)d_obstacle_shape, (const double *)d_obstacle_radius,
                       (const uint8_t *)d_obstacle_gaussian, (const int *)d_scene_of, (const double *)d_state, robot_radius, disc_offset, chi, risk,
                       obstacle_radius, where...);
}

extern "C" int tmpc_set_obstacle_parameters(tmpc_handle *h, const void *d_obstacle_pos, const void *d_obstacle_shape, const void *d_obstacle_radius,
                                            const void *d_obstacle_gaussian, const void *d_scene_of, const void *d_state, double robot_radius,
                                            double disc_offset, double risk, double chi, double obstacle_radius)
{
    TMPC_NOT_IN_GENERATED_SOLVER(h, "tmpc_set_obstacle_parameters");
    if (!h) return TMPC_ERR_INVALID;
    if (h->d.M <= 0) { h->err = "tmpc_set_obstacle_parameters: the problem has no obstacle rows (M = 0)"; return TMPC_ERR_INVALID; }
    return set_obstacle_rows_checked(h, "tmpc_set_obstacle_parameters", tmpc::tmpc_set_obstacle_parameters_kernel, h->d.M, d_obstacle_pos, d_obstacle_shape,
                                     d_obstacle_radius, d_obstacle_gaussian, d_scene_of, d_state, robot_radius, disc_offset, risk, chi, obstacle_radius);
}

extern "C" int tmpc_stack_set_obstacle_columns(tmpc_handle *h, const int32_t *cols, int32_t n_cols, int32_t row_model, int32_t max_obstacles,
                                               const void *d_obstacle_pos, const void *d_obstacle_shape, const void *d_obstacle_radius,
                                               const void *d_obstacle_gaussian, const void *d_scene_of, const void *d_state, double robot_radius,
                                               double disc_offset, double risk, double chi, double obstacle_radius)
{
    if (!h) return TMPC_ERR_INVALID;
    const std::string who = "tmpc_stack_set_obstacle_columns: ";
    if (!cols) { h->err = who + "NULL argument (cols)"; return TMPC_ERR_INVALID; }
    if (row_model != 0 && row_model != 1) { h->err = who + "row_model is 0 (ellipsoids) or 1 (Gaussian rows)"; return TMPC_ERR_INVALID; }
    if (max_obstacles < 1) { h->err = who + "max_obstacles must be at least 1"; return TMPC_ERR_INVALID; }
    const int64_t want = 2 + (int64_t)(row_model == 1 ? 6 : 7) * max_obstacles;
    if (n_cols != want || n_cols > tmpc::SCATTER_MAX_COLS) {
        h->err = who + "n_cols must be 2 + 7 max_obstacles (row_model 0) or 2 + 6 max_obstacles (row_model 1), at most 128"; return TMPC_ERR_INVALID;
    }
    tmpc::ColumnRows where{};
    where.count = max_obstacles; where.model = row_model;
    if (!read_stack_columns(h, who, cols, n_cols, where.t)) return TMPC_ERR_INVALID;
    return set_obstacle_rows_checked(h, "tmpc_stack_set_obstacle_columns", tmpc::tmpc_set_obstacle_columns_kernel, max_obstacles, d_obstacle_pos,
                                     d_obstacle_shape, d_obstacle_radius, d_obstacle_gaussian, d_scene_of, d_state, robot_radius, disc_offset, risk, chi,
                                     obstacle_radius, where);
}

// ---- topology rows.  n_rows: the topology rows of the destination (the layout's n_lin, the column call's own) ------------------------------------
template <class Kernel, class... Where>
static int linearize_topology_checked(tmpc_handle *h, const char *fn, Kernel kernel, int32_t n_rows, const void *d_obstacle_pos, int32_t n_obstacles,
                                      const void *d_obstacle_radius, const void *d_static_halfspaces, int32_t n_static, const void *d_scene_of,
                                      const void *d_state_x, double robot_radius, const void *d_is_original, Where... where)
{
    const std::string who = std::string(fn) + ": ";
    if (no_batch(h, who)) return TMPC_ERR_INVALID;
    if (!d_scene_of || !d_state_x) { h->err = who + "NULL argument (d_scene_of, d_state_x)"; return TMPC_ERR_INVALID; }
    if (n_obstacles < 0 || n_static < 0 || (int64_t)n_obstacles + n_static > n_rows) {
        h->err = who + "more obstacle + static rows than topology rows (n_obstacles, n_static >= 0, n_obstacles + n_static <= the rows of the destination)";
        return TMPC_ERR_INVALID;
    }
    if (n_obstacles > 0 && !d_obstacle_pos) { h->err = who + "NULL d_obstacle_pos with n_obstacles > 0"; return TMPC_ERR_INVALID; }
    if (n_static > 0 && !d_static_halfspaces) { h->err = who + "NULL d_static_halfspaces with n_static > 0"; return TMPC_ERR_INVALID; }
    return launch_flat(h, who, "B x N", (int64_t)h->B * h->d.N, kernel, h->d, h->B, h->x0, const_cast<double *>(h->params), (const double *)d_obstacle_pos,
                       (const int *)d_scene_of, (const double *)d_state_x, robot_radius, (const uint8_t *)d_is_original, n_obstacles,
                       (const double *)d_obstacle_radius, (const double *)d_static_halfspaces, n_static, where...);
}

extern "C" int tmpc_linearize_topology_ex(tmpc_handle *h, const void *d_obstacle_pos, int32_t n_obstacles, const void *d_obstacle_radius,
                                          const void *d_static_halfspaces, int32_t n_static, const void *d_scene_of, const void *d_state_x,
                                          double robot_radius, const void *d_is_original)
{
    TMPC_NOT_IN_GENERATED_SOLVER(h, "tmpc_linearize_topology");
    if (!h) return TMPC_ERR_INVALID;
    if (h->d.n_lin <= 0) { h->err = "tmpc_linearize_topology: the problem has no topology rows (n_lin = 0)"; return TMPC_ERR_INVALID; }
    return linearize_topology_checked(h, "tmpc_linearize_topology", tmpc::tmpc_linearize_topology_kernel, h->d.n_lin, d_obstacle_pos, n_obstacles,
                                      d_obstacle_radius, d_static_halfspaces, n_static, d_scene_of, d_state_x, robot_radius, d_is_original);
}

extern "C" int tmpc_linearize_topology(tmpc_handle *h, const void *d_obstacle_pos, const void *d_scene_of, const void *d_state_x, double robot_radius,
                                       const void *d_is_original)
{
    if (!h || !d_obstacle_pos) { if (h) h->err = "tmpc_linearize_topology: bad argument"; return TMPC_ERR_INVALID; }
    return tmpc_linearize_topology_ex(h, d_obstacle_pos, h->d.n_lin, nullptr, nullptr, 0, d_scene_of, d_state_x, robot_radius, d_is_original);
}

extern "C" int tmpc_stack_linearize_topology_columns(tmpc_handle *h, const int32_t *cols, int32_t n_rows, const void *d_obstacle_pos, int32_t n_obstacles,
                                                     const void *d_obstacle_radius, const void *d_static_halfspaces, int32_t n_static,
                                                     const void *d_scene_of, const void *d_state_x, double robot_radius, const void *d_is_original)
{
    if (!h) return TMPC_ERR_INVALID;
    const std::string who = "tmpc_stack_linearize_topology_columns: ";
    if (n_rows < 1 || 3 * (int64_t)n_rows > tmpc::SCATTER_MAX_COLS) { h->err = who + "n_rows must be at least 1 and 3 n_rows at most 128"; return TMPC_ERR_INVALID; }
    if (!cols) { h->err = who + "NULL argument (cols)"; return TMPC_ERR_INVALID; }
    tmpc::ColumnRows where{};
    where.count = n_rows; where.model = 0;
    if (!read_stack_columns(h, who, cols, 3 * n_rows, where.t)) return TMPC_ERR_INVALID;
    return linearize_topology_checked(h, "tmpc_stack_linearize_topology_columns", tmpc::tmpc_linearize_topology_columns_kernel, n_rows, d_obstacle_pos,
                                      n_obstacles, d_obstacle_radius, d_static_halfspaces, n_static, d_scene_of, d_state_x, robot_radius, d_is_original, where);
}

// ---- path window.  n_segments: the window's segments in the destination (the layout's S, the column call's own) ----------------------------------
template <class Kernel, class... Where>
static int set_path_rows_checked(tmpc_handle *h, const char *fn, Kernel kernel, int32_t n_segments, const void *d_window, const void *d_scene_of,
                                 int32_t n_scenes, const void *d_closest_s, void *d_state, Where... where)
{
    const std::string who = std::string(fn) + ": ";
    if (no_batch(h, who)) return TMPC_ERR_INVALID;
    if (!d_window || !d_scene_of) { h->err = who + "bad argument: NULL argument (d_window, d_scene_of)"; return TMPC_ERR_INVALID; }
    if (n_scenes <= 0) { h->err = who + "bad argument: n_scenes must be positive"; return TMPC_ERR_INVALID; }
    if ((d_closest_s == nullptr) != (d_state == nullptr)) { h->err = who + "d_closest_s and d_state go together (both or neither)"; return TMPC_ERR_INVALID; }
    return launch_flat(h, who, "B x N x n_segments", (int64_t)h->B * h->d.N * n_segments, kernel, h->d, h->B, const_cast<double *>(h->params),
                       (const double *)d_window, (const int *)d_scene_of, n_scenes, (const double *)d_closest_s, (double *)d_state, where...);
}

extern "C" int tmpc_set_path_parameters(tmpc_handle *h, const void *d_window, const void *d_scene_of, int32_t n_scenes, const void *d_closest_s, void *d_state)
{
    TMPC_NOT_IN_GENERATED_SOLVER(h, "tmpc_set_path_parameters");
    if (!h) return TMPC_ERR_INVALID;
    if (h->d.S <= 0) { h->err = "tmpc_set_path_parameters: the problem has no path segments (S = 0)"; return TMPC_ERR_INVALID; }
    return set_path_rows_checked(h, "tmpc_set_path_parameters", tmpc::tmpc_set_path_parameters_kernel, h->d.S, d_window, d_scene_of, n_scenes, d_closest_s,
                                 d_state);
}

extern "C" int tmpc_stack_set_path_columns(tmpc_handle *h, const int32_t *cols, int32_t n_segments, const void *d_window, const void *d_scene_of,
                                           int32_t n_scenes, const void *d_closest_s, void *d_state)
{
    if (!h) return TMPC_ERR_INVALID;
    const std::string who = "tmpc_stack_set_path_columns: ";
    if (!cols) { h->err = who + "NULL argument (cols)"; return TMPC_ERR_INVALID; }
    if (d_closest_s && !stack_has_spline_state()) { h->err = who + "d_closest_s: this generated solver's model has no spline state"; return TMPC_ERR_INVALID; }
    tmpc::ColumnEnvRows where{};
    if (!read_path_columns(h, who, cols, n_segments, where)) return TMPC_ERR_INVALID;
    return set_path_rows_checked(h, "tmpc_stack_set_path_columns", tmpc::tmpc_set_path_columns_kernel, n_segments, d_window, d_scene_of, n_scenes,
                                 d_closest_s, d_state, where);
}

// ---- road rows (they read the path window; written to the caller's d_static_halfspaces, rows first_row and first_row + 1 of n_static) -------------
template <class Kernel, class... Where>
static int road_halfspaces_checked(tmpc_handle *h, const char *fn, Kernel kernel, const void *d_main_of, int32_t n_scenes, const void *d_bound_segments,
                                   double offset_first, double offset_second, void *d_static_halfspaces, int32_t n_static, int32_t first_row, Where... where)
{
    const std::string who = std::string(fn) + ": ";
    if (no_batch(h, who)) return TMPC_ERR_INVALID;
    if (!d_main_of || !d_static_halfspaces) { h->err = who + "bad argument: NULL argument (d_main_of, d_static_halfspaces)"; return TMPC_ERR_INVALID; }
    if (n_scenes <= 0) { h->err = who + "bad argument: n_scenes must be positive"; return TMPC_ERR_INVALID; }
    if (first_row < 0 || n_static < (int64_t)first_row + 2) { h->err = who + "the two road rows do not fit (first_row < 0 or n_static < first_row + 2)"; return TMPC_ERR_INVALID; }
    return launch_flat(h, who, "n_scenes x N", (int64_t)n_scenes * h->d.N, kernel, h->d, h->B, n_scenes, h->x0, h->params, (const int *)d_main_of,
                       (const double *)d_bound_segments, offset_first, offset_second, (double *)d_static_halfspaces, n_static, first_row, where...);
}

extern "C" int tmpc_road_halfspaces(tmpc_handle *h, const void *d_main_of, int32_t n_scenes, const void *d_bound_segments, double offset_first,
                                    double offset_second, void *d_static_halfspaces, int32_t n_static, int32_t first_row)
{
    TMPC_NOT_IN_GENERATED_SOLVER(h, "tmpc_road_halfspaces");
    if (!h) return TMPC_ERR_INVALID;
    if (h->d.S <= 0) { h->err = "tmpc_road_halfspaces: the problem has no path segments (S = 0)"; return TMPC_ERR_INVALID; }
    return road_halfspaces_checked(h, "tmpc_road_halfspaces", tmpc::tmpc_road_halfspaces_kernel, d_main_of, n_scenes, d_bound_segments, offset_first,
                                   offset_second, d_static_halfspaces, n_static, first_row);
}

extern "C" int tmpc_stack_road_halfspaces(tmpc_handle *h, const int32_t *cols, int32_t n_segments, const void *d_main_of, int32_t n_scenes,
                                          const void *d_bound_segments, double offset_first, double offset_second, void *d_static_halfspaces,
                                          int32_t n_static, int32_t first_row)
{
    if (!h) return TMPC_ERR_INVALID;
    const std::string who = "tmpc_stack_road_halfspaces: ";
    if (!stack_has_spline_state()) { h->err = who + "this generated solver's model has no spline state"; return TMPC_ERR_INVALID; }
    if (!cols) { h->err = who + "NULL argument (cols)"; return TMPC_ERR_INVALID; }
    tmpc::ColumnEnvRows where{};
    if (!read_path_columns(h, who, cols, n_segments, where)) return TMPC_ERR_INVALID;
    return road_halfspaces_checked(h, "tmpc_stack_road_halfspaces", tmpc::tmpc_road_halfspaces_columns_kernel, d_main_of, n_scenes, d_bound_segments,
                                   offset_first, offset_second, d_static_halfspaces, n_static, first_row, where);
}

// ---- decomposition (it writes no parameter row: one kernel; uses N, dt, the warm start and the stream of the handle only), then the halfspace rows
static int decomp_halfspaces_checked(tmpc_handle *h, const char *fn, const void *d_main_of, int32_t n_scenes, int32_t n_seg_max, const void *d_path,
                                     const void *d_path_count, const void *d_path_length, const void *d_s0, const void *d_state_x, const void *d_points,
                                     const void *d_count, int32_t n_pts_max, double range, int32_t n_rows, void *d_rows, void *d_row_count, void *d_status)
{
    if (!h) return TMPC_ERR_INVALID;
    const std::string who = std::string(fn) + ": ";
    if (no_batch(h, who)) return TMPC_ERR_INVALID;
    if (n_scenes <= 0) { h->err = who + "n_scenes must be positive"; return TMPC_ERR_INVALID; }
    if (n_seg_max < 1 || n_seg_max > tmpc::PATH_MAX_SEGMENTS) { h->err = who + "1 <= n_seg_max <= 1024"; return TMPC_ERR_INVALID; }
    if (n_pts_max < 1 || n_pts_max > tmpc::DECOMP_MAX_POINTS) { h->err = who + "1 <= n_pts_max <= 16384"; return TMPC_ERR_INVALID; }
    if (n_rows < 1 || n_rows > tmpc::DECOMP_MAX_ROWS) { h->err = who + "1 <= n_rows <= 64"; return TMPC_ERR_INVALID; }
    if (!(range >= 0.0) || !(range < __builtin_huge_val())) { h->err = who + "range must be finite and not negative"; return TMPC_ERR_INVALID; }
    if (!d_main_of || !d_path || !d_path_count || !d_path_length || !d_s0 || !d_state_x || !d_points || !d_count) {
        h->err = who + "NULL input (d_main_of, d_path, d_path_count, d_path_length, d_s0, d_state_x, d_points, d_count)"; return TMPC_ERR_INVALID;
    }
    if (!d_rows || !d_row_count || !d_status) { h->err = who + "NULL output (d_rows, d_row_count, d_status)"; return TMPC_ERR_INVALID; }
    const int64_t n = (int64_t)n_scenes * h->d.N;
    if (n > 0x7fffffff) { h->err = who + "n_scenes x N too large"; return TMPC_ERR_INVALID; }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(tmpc::tmpc_decomp_halfspaces_kernel, dim3((unsigned)n), dim3(tmpc::DECOMP_THREADS), 0, h->stream, h->d, h->B, n_scenes, h->x0,
                       (const int *)d_main_of, n_seg_max, (const double *)d_path, (const int *)d_path_count, (const double *)d_path_length,
                       (const double *)d_s0, (const double *)d_state_x, (const double *)d_points, (const int *)d_count, n_pts_max, range, n_rows,
                       (double *)d_rows, (int *)d_row_count, (uint8_t *)d_status);
    TMPC_HIP_CHECK(h, hipGetLastError());
    return TMPC_OK;
}

extern "C" int tmpc_decomp_halfspaces(tmpc_handle *h, const void *d_main_of, int32_t n_scenes, int32_t n_seg_max, const void *d_path, const void *d_path_count,
                                      const void *d_path_length, const void *d_s0, const void *d_state_x, const void *d_points, const void *d_count,
                                      int32_t n_pts_max, double range, int32_t n_rows, void *d_rows, void *d_row_count, void *d_status)
{
    TMPC_NOT_IN_GENERATED_SOLVER(h, "tmpc_decomp_halfspaces");
    return decomp_halfspaces_checked(h, "tmpc_decomp_halfspaces", d_main_of, n_scenes, n_seg_max, d_path, d_path_count, d_path_length, d_s0, d_state_x,
                                     d_points, d_count, n_pts_max, range, n_rows, d_rows, d_row_count, d_status);
}

extern "C" int tmpc_stack_decomp_halfspaces(tmpc_handle *h, const void *d_main_of, int32_t n_scenes, int32_t n_seg_max, const void *d_path,
                                            const void *d_path_count, const void *d_path_length, const void *d_s0, const void *d_state_x,
                                            const void *d_points, const void *d_count, int32_t n_pts_max, double range, int32_t n_rows, void *d_rows,
                                            void *d_row_count, void *d_status)
{
    return decomp_halfspaces_checked(h, "tmpc_stack_decomp_halfspaces", d_main_of, n_scenes, n_seg_max, d_path, d_path_count, d_path_length, d_s0, d_state_x,
                                     d_points, d_count, n_pts_max, range, n_rows, d_rows, d_row_count, d_status);
}

// where: the layout's first_row (an int, in front of scene_of in its kernel's arguments) or the column table (the last argument of its kernel)
template <class Kernel, class Where>
static int set_halfspace_rows_checked(tmpc_handle *h, const char *fn, Kernel kernel, int32_t n_rows, const void *d_rows, const void *d_scene_of,
                                      int32_t n_scenes, double disc_offset, Where where)
{
    const std::string who = std::string(fn) + ": ";
    if (no_batch(h, who)) return TMPC_ERR_INVALID;
    if (!d_rows || !d_scene_of) { h->err = who + "bad argument: NULL argument (d_rows, d_scene_of)"; return TMPC_ERR_INVALID; }
    if (n_scenes <= 0) { h->err = who + "bad argument: n_scenes must be positive"; return TMPC_ERR_INVALID; }
    const int64_t n = (int64_t)h->B * h->d.N * n_rows;
    double *params = const_cast<double *>(h->params);
    if constexpr (std::is_same<Where, int32_t>::value)
        return launch_flat(h, who, "B x N x n_rows", n, kernel, h->d, h->B, params, (const double *)d_rows, n_rows, where, (const int *)d_scene_of, n_scenes, disc_offset);
    else
        return launch_flat(h, who, "B x N x n_rows", n, kernel, h->d, h->B, params, (const double *)d_rows, n_rows, (const int *)d_scene_of, n_scenes, disc_offset, where);
}

extern "C" int tmpc_set_halfspace_rows(tmpc_handle *h, const void *d_rows, int32_t n_rows, int32_t first_row, const void *d_scene_of, int32_t n_scenes,
                                       double disc_offset)
{
    TMPC_NOT_IN_GENERATED_SOLVER(h, "tmpc_set_halfspace_rows");
    if (!h) return TMPC_ERR_INVALID;
    if (n_rows < 1 || first_row < 0 || (int64_t)first_row + n_rows > h->d.n_slk) {
        h->err = "tmpc_set_halfspace_rows: the rows do not fit (n_rows >= 1, first_row >= 0, first_row + n_rows <= the problem's slack rows)"; return TMPC_ERR_INVALID;
    }
    return set_halfspace_rows_checked(h, "tmpc_set_halfspace_rows", tmpc::tmpc_set_halfspace_rows_kernel, n_rows, d_rows, d_scene_of, n_scenes, disc_offset,
                                      first_row);
}

extern "C" int tmpc_stack_set_halfspace_columns(tmpc_handle *h, const int32_t *cols, int32_t n_rows, const void *d_rows, const void *d_scene_of,
                                                int32_t n_scenes, double disc_offset)
{
    if (!h) return TMPC_ERR_INVALID;
    const std::string who = "tmpc_stack_set_halfspace_columns: ";
    if (!cols) { h->err = who + "NULL argument (cols)"; return TMPC_ERR_INVALID; }
    if (n_rows < 1 || 1 + 3 * (int64_t)n_rows > tmpc::SCATTER_MAX_COLS) { h->err = who + "n_rows must be at least 1 and 1 + 3 n_rows at most 128"; return TMPC_ERR_INVALID; }
    tmpc::ColumnEnvRows where{};
    where.count = n_rows;
    if (!read_stack_columns(h, who, cols, 1 + 3 * n_rows, where.t)) return TMPC_ERR_INVALID;
    return set_halfspace_rows_checked(h, "tmpc_stack_set_halfspace_columns", tmpc::tmpc_set_halfspace_columns_kernel, n_rows, d_rows, d_scene_of, n_scenes,
                                      disc_offset, where);
}

// ---- scenario rows (SH-MPC polygons) and the support of the solution ------------------------------------------------------------------------------
// The checks both entries share, the bookkeeping buffer (scn_sample), the discard marks and the two passes (the callers have checked n_rows).
// `kernel` is the instantiation that is launched: its own static LDS counts in the 160 KiB refusal and its own dynamic-LDS attribute is raised
// when the list exceeds 48 KiB -- the attribute belongs to the function, so the sibling's does not help.
template <class Kernel, class... Where>
static int scenario_halfspaces_checked(tmpc_handle *h, const char *fn, Kernel kernel, bool by_column, const void *d_samples, int32_t n_pts, int32_t n_rows,
                                       const void *d_scene_of, const void *d_state_x, double radius, double disc_offset, Where... where)
{
    const std::string who = std::string(fn) + ": ";
    if (no_batch(h, who)) return TMPC_ERR_INVALID;
    if (!d_samples || !d_scene_of || !d_state_x) { h->err = who + "NULL argument (d_samples, d_scene_of, d_state_x)"; return TMPC_ERR_INVALID; }
    if (n_pts <= 0) { h->err = who + "n_pts must be positive"; return TMPC_ERR_INVALID; }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    const void *symbol = reinterpret_cast<const void *>(kernel);
    const size_t per_entry = 3 * sizeof(double) + sizeof(int);                        // a candidate: normal, margin, index word
    hipFuncAttributes fa;
    TMPC_HIP_CHECK(h, hipFuncGetAttributes(&fa, symbol));
    if ((size_t)n_pts * per_entry + fa.sharedSizeBytes > 160 * 1024) {      // the second pass's list (room for every sample) + the kernel's static tables
        h->err = who + "n_pts: that many samples per stage do not fit a workgroup's LDS (160 KiB minus the kernel's static tables: about 5480)";
        return TMPC_ERR_INVALID;
    }
    const size_t units = (size_t)h->B * h->d.N;
    const size_t need = units * n_rows + 1 + units + (size_t)h->B;  // rows' samples, the first pass's overflow list (count, units), empty-polygon stages per trajectory
    if (int rc = grow_scratch(h, &h->scn_sample, &h->scn_cap, need)) return rc;
    h->scn_rows = n_rows; h->scn_B = h->B; h->scn_by_column = by_column;
    // scenarios discarded for this batch (tmpc_scenario_discard after the batch was set) are left out of the polygons
    const bool use_discard = h->scn_discard && h->scn_discard_B == h->B && h->scn_discard_S > 0 && n_pts % h->scn_discard_S == 0;
    // first pass with a short candidate list (more workgroups per CU); second pass, with room for every sample, only for the
    // units the first pass recorded as not fitting
    int *overflow = h->scn_sample + units * n_rows;
    int *empty_stages = overflow + 1 + units;
    TMPC_HIP_CHECK(h, hipMemsetAsync(overflow, 0, sizeof(int), h->stream));
    TMPC_HIP_CHECK(h, hipMemsetAsync(empty_stages, 0, sizeof(int) * (size_t)h->B, h->stream));
    int list_cap = tmpc::POLY_LIST_CAP;
    if (const char *e = lab_env("TMPC_POLY_LIST_CAP")) { const int v = atoi(e); if (v >= 64 && v <= 4096) list_cap = v; }   // experiments
    const int cap1 = n_pts < list_cap ? n_pts : list_cap;
    for (int pass = 0; pass < (cap1 < n_pts ? 2 : 1); pass++) {
        const int cap = pass == 0 ? cap1 : n_pts;
        const size_t lds = (size_t)cap * per_entry;
        if (lds > 48 * 1024)
            TMPC_HIP_CHECK(h, hipFuncSetAttribute(symbol, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kernel, dim3(pass == 0 ? units : (units < 512 ? units : 512)), dim3(256), lds, h->stream, h->d, h->B, h->x0,
                           const_cast<double *>(h->params), (const double *)d_samples, n_pts, n_rows, (const int *)d_scene_of,
                           (const double *)d_state_x, radius, disc_offset, h->scn_sample, cap, overflow, pass, empty_stages,
                           use_discard ? h->scn_discard : nullptr, use_discard ? h->scn_discard_S : 1, where...);
    }
    TMPC_HIP_CHECK(h, hipGetLastError());
    return TMPC_OK;
}

// the scenario columns of a call: n_rows in range, then the table
static bool read_scenario_columns(tmpc_handle *h, const std::string &who, const int32_t *cols, int32_t n_rows, tmpc::ColumnEnvRows &where)
{
    if (n_rows < 1 || 1 + 3 * (int64_t)n_rows > tmpc::SCATTER_MAX_COLS) { h->err = who + "n_rows must be at least 1 and at most 42 (1 + 3 n_rows columns, at most 128)"; return false; }
    where.count = n_rows;
    return read_stack_columns(h, who, cols, 1 + 3 * n_rows, where.t);
}

extern "C" int tmpc_scenario_halfspaces(tmpc_handle *h, const void *d_samples, int32_t n_pts, int32_t n_rows, const void *d_scene_of,
                                        const void *d_state_x, double radius, double disc_offset)
{
    TMPC_NOT_IN_GENERATED_SOLVER(h, "tmpc_scenario_halfspaces");
    if (!h) return TMPC_ERR_INVALID;
    if (n_rows <= 0 || n_rows > 64 || n_rows > h->d.n_slk) {
        h->err = "tmpc_scenario_halfspaces: n_rows must be at least 1, at most 64 and at most the problem's slack rows";
        return TMPC_ERR_INVALID;
    }
    return scenario_halfspaces_checked(h, "tmpc_scenario_halfspaces", tmpc::tmpc_scenario_halfspaces_kernel, false, d_samples, n_pts, n_rows, d_scene_of,
                                       d_state_x, radius, disc_offset);
}

extern "C" int tmpc_stack_scenario_halfspaces(tmpc_handle *h, const int32_t *cols, int32_t n_rows, const void *d_samples, int32_t n_pts,
                                              const void *d_scene_of, const void *d_state_x, double radius, double disc_offset)
{
    if (!h) return TMPC_ERR_INVALID;
    const std::string who = "tmpc_stack_scenario_halfspaces: ";
    if (!cols) { h->err = who + "NULL argument (cols)"; return TMPC_ERR_INVALID; }
    tmpc::ColumnEnvRows where{};
    if (!read_scenario_columns(h, who, cols, n_rows, where)) return TMPC_ERR_INVALID;
    return scenario_halfspaces_checked(h, "tmpc_stack_scenario_halfspaces", tmpc::tmpc_scenario_halfspaces_columns_kernel, true, d_samples, n_pts, n_rows,
                                       d_scene_of, d_state_x, radius, disc_offset, where);
}

// The support reads the rows its own destination's scenario_halfspaces built for the current batch (by_column; n_rows: the rows of the call).
template <class Kernel, class... Where>
static int scenario_support_checked(tmpc_handle *h, const char *fn, Kernel kernel, bool by_column, int32_t n_rows, int32_t n_scenarios, double tol,
                                    void *d_support, void *d_active_rows, Where... where)
{
    const std::string who = std::string(fn) + ": ";
    if (!d_support) { h->err = who + "bad argument: NULL argument (d_support)"; return TMPC_ERR_INVALID; }
    if (n_scenarios <= 0 || n_scenarios > 8192) { h->err = who + "bad argument: 1 <= n_scenarios <= 8192"; return TMPC_ERR_INVALID; }
    if (!(tol >= 0.0)) { h->err = who + "bad argument: tol must not be negative"; return TMPC_ERR_INVALID; }
    if (!h->scn_sample || h->scn_B != h->B || h->B <= 0 || !h->params || h->scn_by_column != by_column) {
        h->err = who + "the scenario rows of the current batch were not built by " + (by_column ? "tmpc_stack_scenario_halfspaces" : "tmpc_scenario_halfspaces") +
                 " (call it after tmpc_set_batch)";
        return TMPC_ERR_INVALID;
    }
    if (h->scn_rows != n_rows) { h->err = who + "n_rows: the scenario rows of the current batch were built with another n_rows"; return TMPC_ERR_INVALID; }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(kernel, dim3(h->B), dim3(64), 0, h->stream, h->d, h->B, h->params, h->xtraj, h->scn_sample, h->scn_rows, n_scenarios, tol,
                       (int *)d_support, (int *)d_active_rows, where...);
    TMPC_HIP_CHECK(h, hipGetLastError());
    return TMPC_OK;
}

extern "C" int tmpc_scenario_support(tmpc_handle *h, int32_t n_scenarios, double tol, void *d_support, void *d_active_rows)
{
    TMPC_NOT_IN_GENERATED_SOLVER(h, "tmpc_scenario_support");     // (its rows can only be tmpc_stack_scenario_halfspaces': read them with tmpc_stack_scenario_support)
    if (!h) return TMPC_ERR_INVALID;
    return scenario_support_checked(h, "tmpc_scenario_support", tmpc::tmpc_scenario_support_kernel, false, h->scn_rows, n_scenarios, tol, d_support,
                                    d_active_rows);
}

extern "C" int tmpc_stack_scenario_support(tmpc_handle *h, const int32_t *cols, int32_t n_rows, int32_t n_scenarios, double tol, void *d_support,
                                           void *d_active_rows)
{
    if (!h) return TMPC_ERR_INVALID;
    const std::string who = "tmpc_stack_scenario_support: ";
    if (!cols) { h->err = who + "NULL argument (cols)"; return TMPC_ERR_INVALID; }
    tmpc::ColumnEnvRows where{};
    if (!read_scenario_columns(h, who, cols, n_rows, where)) return TMPC_ERR_INVALID;
    return scenario_support_checked(h, "tmpc_stack_scenario_support", tmpc::tmpc_scenario_support_columns_kernel, true, n_rows, n_scenarios, tol, d_support,
                                    d_active_rows, where);
}
