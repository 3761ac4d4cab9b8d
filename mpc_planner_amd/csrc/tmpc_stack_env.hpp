// mpc_planner_amd/csrc/tmpc_stack_env.hpp -- the entry points of include/tmpc_hip_stack_env.h: the path window, the road rows and the free-space
// (decomp) rows of a generated solver's module stack, in columns the caller names.  Part of the C-ABI translation unit: tmpc_capi.hip includes this
// file once, behind tmpc_stack_writers.hpp (read_stack_columns), so that the one-translation-unit builds of the generated libraries carry the
// entry points too.  The kernels are the templates of tmpc_aux_kernels.hpp (LayoutEnvRows / ColumnEnvRows): the arithmetic of the hand-written
// layout's writers, one source.
#pragma once
#include "../../include/tmpc_hip_stack_env.h"

// tmpc_decomp_halfspaces and tmpc_stack_decomp_halfspaces: the checks and the launch (fn: the entry point's name, for the messages).  Uses N, dt,
// the warm start and the stream of the handle only.
static int decomp_halfspaces_checked(tmpc_handle *h, const char *fn, const void *d_main_of, int32_t n_scenes, int32_t n_seg_max, const void *d_path,
                                     const void *d_path_count, const void *d_path_length, const void *d_s0, const void *d_state_x, const void *d_points,
                                     const void *d_count, int32_t n_pts_max, double range, int32_t n_rows, void *d_rows, void *d_row_count, void *d_status)
{
    if (!h) return TMPC_ERR_INVALID;
    const std::string who = std::string(fn) + ": ";
    if (h->B <= 0 || !h->x0) { h->err = who + "no batch (call tmpc_set_batch* first)"; return TMPC_ERR_INVALID; }
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

// the path columns of a call: n_segments in range, then the table
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

extern "C" {

int tmpc_stack_set_path_columns(tmpc_handle *h, const int32_t *cols, int32_t n_segments, const void *d_window, const void *d_scene_of, int32_t n_scenes,
                                const void *d_closest_s, void *d_state)
{
    if (!h) return TMPC_ERR_INVALID;
    const std::string who = "tmpc_stack_set_path_columns: ";
    if (h->B <= 0 || !h->params) { h->err = who + "no batch (call tmpc_set_batch* first)"; return TMPC_ERR_INVALID; }
    if (!cols || !d_window || !d_scene_of) { h->err = who + "NULL argument (cols, d_window, d_scene_of)"; return TMPC_ERR_INVALID; }
    if (n_scenes <= 0) { h->err = who + "n_scenes must be positive"; return TMPC_ERR_INVALID; }
    if ((d_closest_s == nullptr) != (d_state == nullptr)) { h->err = who + "d_closest_s and d_state go together (both or neither)"; return TMPC_ERR_INVALID; }
    if (d_closest_s && !stack_has_spline_state()) { h->err = who + "d_closest_s: this generated solver's model has no spline state"; return TMPC_ERR_INVALID; }
    tmpc::ColumnEnvRows where{};
    if (!read_path_columns(h, who, cols, n_segments, where)) return TMPC_ERR_INVALID;
    const int64_t n = (int64_t)h->B * h->d.N * n_segments;
    if (n > 0x7fffffff) { h->err = who + "B x N x n_segments too large"; return TMPC_ERR_INVALID; }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(tmpc::tmpc_set_path_columns_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->d, h->B,
                       const_cast<double *>(h->params), (const double *)d_window, (const int *)d_scene_of, n_scenes, (const double *)d_closest_s,
                       (double *)d_state, where);
    TMPC_HIP_CHECK(h, hipGetLastError());
    return TMPC_OK;
}

int tmpc_stack_road_halfspaces(tmpc_handle *h, const int32_t *cols, int32_t n_segments, const void *d_main_of, int32_t n_scenes,
                               const void *d_bound_segments, double offset_first, double offset_second, void *d_static_halfspaces, int32_t n_static,
                               int32_t first_row)
{
    if (!h) return TMPC_ERR_INVALID;
    const std::string who = "tmpc_stack_road_halfspaces: ";
    if (!stack_has_spline_state()) { h->err = who + "this generated solver's model has no spline state"; return TMPC_ERR_INVALID; }
    if (h->B <= 0 || !h->x0 || !h->params) { h->err = who + "no batch (call tmpc_set_batch* first)"; return TMPC_ERR_INVALID; }
    if (!cols || !d_main_of || !d_static_halfspaces) { h->err = who + "NULL argument (cols, d_main_of, d_static_halfspaces)"; return TMPC_ERR_INVALID; }
    if (n_scenes <= 0) { h->err = who + "n_scenes must be positive"; return TMPC_ERR_INVALID; }
    if (first_row < 0 || n_static < (int64_t)first_row + 2) { h->err = who + "the two road rows do not fit (first_row >= 0, n_static >= first_row + 2)"; return TMPC_ERR_INVALID; }
    tmpc::ColumnEnvRows where{};
    if (!read_path_columns(h, who, cols, n_segments, where)) return TMPC_ERR_INVALID;
    const int64_t n = (int64_t)n_scenes * h->d.N;
    if (n > 0x7fffffff) { h->err = who + "n_scenes x N too large"; return TMPC_ERR_INVALID; }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(tmpc::tmpc_road_halfspaces_columns_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->d, h->B, n_scenes, h->x0,
                       h->params, (const int *)d_main_of, (const double *)d_bound_segments, offset_first, offset_second,
                       (double *)d_static_halfspaces, n_static, first_row, where);
    TMPC_HIP_CHECK(h, hipGetLastError());
    return TMPC_OK;
}

int tmpc_stack_decomp_halfspaces(tmpc_handle *h, const void *d_main_of, int32_t n_scenes, int32_t n_seg_max, const void *d_path, const void *d_path_count,
                                 const void *d_path_length, const void *d_s0, const void *d_state_x, const void *d_points, const void *d_count,
                                 int32_t n_pts_max, double range, int32_t n_rows, void *d_rows, void *d_row_count, void *d_status)
{
    return decomp_halfspaces_checked(h, "tmpc_stack_decomp_halfspaces", d_main_of, n_scenes, n_seg_max, d_path, d_path_count, d_path_length, d_s0, d_state_x,
                                     d_points, d_count, n_pts_max, range, n_rows, d_rows, d_row_count, d_status);
}

int tmpc_stack_set_halfspace_columns(tmpc_handle *h, const int32_t *cols, int32_t n_rows, const void *d_rows, const void *d_scene_of, int32_t n_scenes,
                                     double disc_offset)
{
    if (!h) return TMPC_ERR_INVALID;
    const std::string who = "tmpc_stack_set_halfspace_columns: ";
    if (h->B <= 0 || !h->params) { h->err = who + "no batch (call tmpc_set_batch* first)"; return TMPC_ERR_INVALID; }
    if (!cols || !d_rows || !d_scene_of) { h->err = who + "NULL argument (cols, d_rows, d_scene_of)"; return TMPC_ERR_INVALID; }
    if (n_scenes <= 0) { h->err = who + "n_scenes must be positive"; return TMPC_ERR_INVALID; }
    if (n_rows < 1 || 1 + 3 * (int64_t)n_rows > tmpc::SCATTER_MAX_COLS) { h->err = who + "n_rows must be at least 1 and 1 + 3 n_rows at most 128"; return TMPC_ERR_INVALID; }
    tmpc::ColumnEnvRows where{};
    where.count = n_rows;
    if (!read_stack_columns(h, who, cols, 1 + 3 * n_rows, where.t)) return TMPC_ERR_INVALID;
    const int64_t n = (int64_t)h->B * h->d.N * n_rows;
    if (n > 0x7fffffff) { h->err = who + "B x N x n_rows too large"; return TMPC_ERR_INVALID; }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(tmpc::tmpc_set_halfspace_columns_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->d, h->B,
                       const_cast<double *>(h->params), (const double *)d_rows, n_rows, (const int *)d_scene_of, n_scenes, disc_offset, where);
    TMPC_HIP_CHECK(h, hipGetLastError());
    return TMPC_OK;
}

}  // extern "C"
