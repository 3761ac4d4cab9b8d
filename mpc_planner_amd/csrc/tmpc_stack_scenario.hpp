// mpc_planner_amd/csrc/tmpc_stack_scenario.hpp -- the entry points of include/tmpc_hip_stack_scenario.h: the scenario rows (SH-MPC polygons) of a
// generated solver's module stack and the support of its solution, in columns the caller names.  Part of the C-ABI translation unit:
// tmpc_capi.hip includes this file once, behind tmpc_stack_env.hpp, so that the one-translation-unit builds of the generated libraries carry the
// entry points too.  The kernels are the templates of tmpc_aux_kernels.hpp (poly_stage and scenario_support_rows on LayoutEnvRows /
// ColumnEnvRows): the arithmetic of the hand-written layout's kernels, one source.
#pragma once
#include "../../include/tmpc_hip_stack_scenario.h"

// tmpc_scenario_halfspaces and tmpc_stack_scenario_halfspaces: the checks both share, the bookkeeping buffer (scn_sample), the discard marks and
// the two passes (fn: the entry point's name, for the messages; the callers have checked n_rows).  `kernel` is the instantiation that is
// launched: its own static LDS counts in the 160 KiB refusal and its own dynamic-LDS attribute is raised when the list exceeds 48 KiB -- the
// attribute belongs to the function, so the sibling's does not help.  where...: the kernel's trailing argument (the column table), if any.
template <class Kernel, class... Where>
static int scenario_halfspaces_checked(tmpc_handle *h, const char *fn, Kernel kernel, bool by_column, const void *d_samples, int32_t n_pts, int32_t n_rows,
                                       const void *d_scene_of, const void *d_state_x, double radius, double disc_offset, Where... where)
{
    const std::string who = std::string(fn) + ": ";
    if (h->B <= 0 || !h->params || !h->x0) { h->err = who + "no batch (call tmpc_set_batch* first)"; return TMPC_ERR_INVALID; }
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

extern "C" {

int tmpc_stack_scenario_halfspaces(tmpc_handle *h, const int32_t *cols, int32_t n_rows, const void *d_samples, int32_t n_pts, const void *d_scene_of,
                                   const void *d_state_x, double radius, double disc_offset)
{
    if (!h) return TMPC_ERR_INVALID;
    const std::string who = "tmpc_stack_scenario_halfspaces: ";
    if (!cols) { h->err = who + "NULL argument (cols)"; return TMPC_ERR_INVALID; }
    tmpc::ColumnEnvRows where{};
    if (!read_scenario_columns(h, who, cols, n_rows, where)) return TMPC_ERR_INVALID;
    return scenario_halfspaces_checked(h, "tmpc_stack_scenario_halfspaces", tmpc::tmpc_scenario_halfspaces_columns_kernel, true, d_samples, n_pts, n_rows,
                                       d_scene_of, d_state_x, radius, disc_offset, where);
}

int tmpc_stack_scenario_support(tmpc_handle *h, const int32_t *cols, int32_t n_rows, int32_t n_scenarios, double tol, void *d_support, void *d_active_rows)
{
    if (!h) return TMPC_ERR_INVALID;
    const std::string who = "tmpc_stack_scenario_support: ";
    if (!cols || !d_support) { h->err = who + "NULL argument (cols, d_support)"; return TMPC_ERR_INVALID; }
    if (n_scenarios <= 0 || n_scenarios > 8192) { h->err = who + "1 <= n_scenarios <= 8192"; return TMPC_ERR_INVALID; }
    if (!(tol >= 0.0)) { h->err = who + "tol must not be negative"; return TMPC_ERR_INVALID; }
    tmpc::ColumnEnvRows where{};
    if (!read_scenario_columns(h, who, cols, n_rows, where)) return TMPC_ERR_INVALID;
    if (!h->scn_sample || h->scn_B != h->B || h->B <= 0 || !h->params || !h->scn_by_column) {
        h->err = who + "the scenario rows of the current batch were not built by tmpc_stack_scenario_halfspaces (call it after tmpc_set_batch)";
        return TMPC_ERR_INVALID;
    }
    if (h->scn_rows != n_rows) { h->err = who + "n_rows: the scenario rows of the current batch were built with another n_rows"; return TMPC_ERR_INVALID; }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(tmpc::tmpc_scenario_support_columns_kernel, dim3(h->B), dim3(64), 0, h->stream, h->d, h->B, h->params, h->xtraj,
                       h->scn_sample, h->scn_rows, n_scenarios, tol, (int *)d_support, (int *)d_active_rows, where);
    TMPC_HIP_CHECK(h, hipGetLastError());
    return TMPC_OK;
}

}  // extern "C"
