/*
 * tmpc_hip_stack_env.h -- the static environment of a GENERATED solver's module stack on device, by column: the path window, the road rows and
 * the free-space (decomp) rows.
 *
 * The third header, next to tmpc_hip.h and tmpc_hip_stack.h (obstacle and topology rows).  A generated library's parameter row layout belongs
 * to its stack, so tmpc_set_path_parameters, tmpc_road_halfspaces, tmpc_decomp_halfspaces and tmpc_set_halfspace_rows of tmpc_hip.h refuse in
 * it -- and keep refusing.  The entry points below are the same device code with the columns named by the CALLER: the column numbers of the
 * stack's parameter map (<name>_meta.json "parameter_map"), as tmpc_scatter_parameters takes them.  Every build of the library (libtmpc_hip.so,
 * the lab twin, every generated library) exports them, so the same calls work on a hand-written shape with the columns of its own map.
 *
 * All four are stream-ordered on the handle's stream: no allocation, no synchronisation.  `cols` is a HOST array, copied before the call
 * returns; every entry in [0, npar), all distinct, at most 128 (the table travels in the kernel arguments).  A refused call (TMPC_ERR_INVALID,
 * the message in tmpc_last_error names the argument) launches nothing.
 *
 * One tick of a generated contouring stack with guidance, road and decomp rows without a host round trip:
 *   tmpc_warmstart -> tmpc_track_path (window_segments) -> tmpc_stack_set_path_columns -> tmpc_stack_prepare_obstacles
 *   -> tmpc_stack_set_obstacle_columns -> tmpc_stack_road_halfspaces -> tmpc_stack_linearize_topology_columns -> tmpc_costmap_points
 *   -> tmpc_stack_decomp_halfspaces -> tmpc_stack_set_halfspace_columns -> tmpc_solve
 * The scenario rows of such stacks (tmpc_scenario_halfspaces, tmpc_scenario_support): the fourth header, tmpc_hip_stack_scenario.h.
 */
#ifndef TMPC_HIP_STACK_ENV_H
#define TMPC_HIP_STACK_ENV_H

#include "tmpc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What tmpc_set_path_parameters documents (Contouring::setParameters / setSplineParameters, mpc_planner_modules/src/contouring.cpp:94-124;
 * state.set("spline", closest_s), :42) for a stack with n_segments path segments: d_window f64 [n_scenes][n_segments][9] as tmpc_track_path
 * with window_segments = n_segments wrote it, into the caller's columns of the CURRENT batch's parameter rows:
 *   cols [n_segments][9] = spline_x{i}_{a,b,c,d}, spline_y{i}_{a,b,c,d}, spline{i}_start of segment i;  1 <= n_segments, 9 n_segments <= 128.
 * Every stage k < N of every entry b with d_scene_of[b] (i32 [B]) inside [0, n_scenes), and nothing else.  Optional d_closest_s (f64 [n_scenes])
 * with d_state (f64 [B][nx]; both or neither): the `spline` entry of each named entry's state becomes its scene's closest_s; the ORDER note of
 * tmpc_set_path_parameters holds.  The same copy as tmpc_set_path_parameters: on a library whose map is the hand-written one the rows are equal.
 * TMPC_ERR_INVALID: no batch, NULL cols / d_window / d_scene_of, n_scenes <= 0, n_segments out of range, a column outside [0, npar), a duplicate
 * column, one of d_closest_s / d_state without the other, B x N x n_segments beyond 2^31 - 1, d_closest_s in a generated solver whose model
 * has no spline state. */
int tmpc_stack_set_path_columns(tmpc_handle *h, const int32_t *cols, int32_t n_segments, const void *d_window, const void *d_scene_of, int32_t n_scenes,
                                const void *d_closest_s, void *d_state);

/* What tmpc_road_halfspaces documents (Contouring::constructRoadConstraints, mpc_planner_modules/src/contouring.cpp:181-262; s_k =
 * `_solver->getEgoPrediction(k, "spline")`, :208, :250; centreline mode :191-235, bounds mode :237-262 on the centreline's knots, :142-149; the
 * assumptions of DESIGN.md U12) -- both modes, rows first_row and first_row + 1 of d_static_halfspaces f64 [n_scenes][N][n_static][3] for
 * k >= 1, stage 0 and everything else untouched -- with the path window READ from the caller's columns of the parameter row of stage k of entry
 * d_main_of[q]: cols [n_segments][9] as for tmpc_stack_set_path_columns.  A generated handle has no S, so n_segments is the call's;
 * d_bound_segments f64 [n_scenes][2][n_segments][8].  The same arithmetic as tmpc_road_halfspaces: equal bit for bit on the same map, and to
 * mpc_planner_amd.modules.road_halfspaces / road_halfspaces_from_bounds.
 * TMPC_ERR_INVALID: no batch, NULL cols / d_main_of / d_static_halfspaces, n_scenes <= 0, n_segments out of range, a column outside [0, npar),
 * a duplicate column, first_row < 0, n_static < first_row + 2, n_scenes x N beyond 2^31 - 1, a generated solver whose model has no spline
 * state. */
int tmpc_stack_road_halfspaces(tmpc_handle *h, const int32_t *cols, int32_t n_segments, const void *d_main_of, int32_t n_scenes,
                               const void *d_bound_segments, double offset_first, double offset_second, void *d_static_halfspaces, int32_t n_static,
                               int32_t first_row);

/* tmpc_decomp_halfspaces (tmpc_hip.h: DecompConstraints::update, mpc_planner_modules/src/decomp_constraints.cpp:52-118; the polyline :68-82,
 * the copy :90-114; the same kernel, arguments, checks and outputs) without the generated-solver refusal: it reads N, dt and the warm start's v
 * at the model's own stride, and no parameter column. */
int tmpc_stack_decomp_halfspaces(tmpc_handle *h, const void *d_main_of, int32_t n_scenes, int32_t n_seg_max, const void *d_path, const void *d_path_count,
                                 const void *d_path_length, const void *d_s0, const void *d_state_x, const void *d_points, const void *d_count,
                                 int32_t n_pts_max, double range, int32_t n_rows, void *d_rows, void *d_row_count, void *d_status);

/* What tmpc_set_halfspace_rows documents (DecompConstraints::setParameters, decomp_constraints.cpp:150-189): the rows d_rows f64
 * [n_scenes][N][n_rows][3] of EVERY stage, stage 0 included, and ego_disc_0_offset = disc_offset, into the caller's columns of every entry b of
 * the CURRENT batch with d_scene_of[b] (i32 [B]) inside [0, n_scenes):
 *   cols[0] = ego_disc_0_offset,  cols[1 + 3 r + w] = disc_0_decomp_{r}_{a1, a2, b};  1 <= n_rows, 1 + 3 n_rows <= 128.
 * There is no first_row: the columns name the rows.  Nothing else is touched, an entry whose scene is outside that range not at all.
 * ego_disc_0_offset is the column tmpc_stack_set_obstacle_columns writes as its cols[1]: the later call overwrites the earlier one's value, so a stack
 * with both modules passes the same disc_offset to both.
 * TMPC_ERR_INVALID: no batch, NULL cols / d_rows / d_scene_of, n_scenes <= 0, n_rows out of range, a column outside [0, npar), a duplicate
 * column, B x N x n_rows beyond 2^31 - 1. */
int tmpc_stack_set_halfspace_columns(tmpc_handle *h, const int32_t *cols, int32_t n_rows, const void *d_rows, const void *d_scene_of, int32_t n_scenes,
                                     double disc_offset);

#ifdef __cplusplus
}
#endif
#endif
