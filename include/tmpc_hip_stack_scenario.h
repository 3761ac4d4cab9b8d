/*
 * tmpc_hip_stack_scenario.h -- the scenario rows (SH-MPC) of a GENERATED solver's module stack on device, by column: the per-stage polygon
 * of the sampled scenarios and the support of the solution.
 *
 * The fourth header, next to tmpc_hip.h, tmpc_hip_stack.h (obstacle and topology rows) and tmpc_hip_stack_env.h (path window, road and
 * free-space rows).  A generated library's parameter row layout belongs to its stack, so tmpc_scenario_halfspaces of tmpc_hip.h refuses in it,
 * and tmpc_scenario_support with it -- and both keep refusing.  The two entry points below are the same device code with the columns named by
 * the CALLER: the column numbers of the stack's parameter map (<name>_meta.json "parameter_map"), as tmpc_scatter_parameters takes them.  Every
 * build of the library (libtmpc_hip.so, the lab twin, every generated library) exports them, so the same calls work on a hand-written shape
 * with the columns of its own map.
 *
 * Both are stream-ordered on the handle's stream and do not synchronise; the first grows the handle's bookkeeping buffer when the batch or
 * the row count grew, as tmpc_scenario_halfspaces does.  `cols` is a HOST array, copied before the call returns; every entry in [0, npar), all
 * distinct.  A refused call (TMPC_ERR_INVALID, the message in tmpc_last_error names the argument) launches nothing.
 *
 * These entries of tmpc_hip.h touch no parameter column and work on any handle: tmpc_sample_scenarios, tmpc_scenario_discard,
 * tmpc_scenario_discarded, tmpc_scenario_empty_stages.  One tick of a generated Safe-Horizon stack without a host round trip:
 *   tmpc_warmstart -> tmpc_sample_scenarios -> tmpc_scenario_discard -> tmpc_stack_scenario_halfspaces -> tmpc_solve_iterations
 *   -> tmpc_stack_scenario_support -> tmpc_scenario_empty_stages
 */
#ifndef TMPC_HIP_STACK_SCENARIO_H
#define TMPC_HIP_STACK_SCENARIO_H

#include "tmpc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What tmpc_scenario_halfspaces documents -- for every stage k >= 1 of every entry b of the CURRENT batch the polygon of the samples
 * d_samples f64 [n_scenes][N][n_pts][2] of scene d_scene_of[b] (i32 [B]) around the warm start, its n_rows closest edges by margin, dummies
 * (1, 0, d_state_x[scene] + 100) behind them and at stage 0; the scenarios tmpc_scenario_discard marked for this batch left out; the
 * bookkeeping tmpc_stack_scenario_support and tmpc_scenario_empty_stages read -- written into the caller's columns of the parameter rows:
 *   cols[0] = ego_disc_0_offset (set to disc_offset at every stage),  cols[1 + 3 r + w] = disc_0_scenario_constraint_{r}_{a1, a2, b};
 *   1 <= n_rows <= 42 (the table holds at most 128 columns; the layout entry's own limit is 64).
 * The same kernel source as tmpc_scenario_halfspaces: on a library whose map is the hand-written one the rows are equal bit for bit, and to
 * mpc_planner_amd.modules.scenario_halfspaces + halfspace_rows_set_parameters.
 * TMPC_ERR_INVALID: no batch, NULL cols / d_samples / d_scene_of / d_state_x, n_pts <= 0, n_rows out of range, a column outside [0, npar), a
 * duplicate column, n_pts beyond what a workgroup's LDS holds (160 KiB minus the kernel's static tables: about 5480). */
int tmpc_stack_scenario_halfspaces(tmpc_handle *h, const int32_t *cols, int32_t n_rows, const void *d_samples, int32_t n_pts, const void *d_scene_of,
                                   const void *d_state_x, double radius, double disc_offset);

/* What tmpc_scenario_support documents -- d_support i32 [B]: the distinct scenarios (sample index % n_scenarios) with an active row
 * a . p_disc - (b + slack) >= -tol at the solution the handle holds, d_active_rows i32 [B] (may be NULL): the active rows -- with the rows READ
 * from the caller's columns: cols and n_rows as given to the tmpc_stack_scenario_halfspaces that built the rows of the current batch.
 * TMPC_ERR_INVALID: NULL cols / d_support, n_scenarios outside [1, 8192], tol < 0, n_rows out of range, a column outside [0, npar), a duplicate
 * column, the scenario rows of the current batch not built by tmpc_stack_scenario_halfspaces, or built with another n_rows. */
int tmpc_stack_scenario_support(tmpc_handle *h, const int32_t *cols, int32_t n_rows, int32_t n_scenarios, double tol, void *d_support,
                                void *d_active_rows);

#ifdef __cplusplus
}
#endif
#endif
