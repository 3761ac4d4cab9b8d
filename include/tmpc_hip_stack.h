/*
 * tmpc_hip_stack.h -- the module-stack writers: the obstacle and topology rows of a GENERATED solver on device.
 *
 * "stack" = the module stack of a generated solver (mpc_planner_amd/codegen, libtmpc_hip_<name>.so).  Such a library's parameter row layout
 * belongs to its stack, so the writers of tmpc_hip.h that know the hand-written layout (tmpc_prepare_obstacles, tmpc_set_obstacle_parameters,
 * tmpc_linearize_topology(_ex), ...) refuse in it -- and keep refusing.  The entry points below are the same device code with the destination
 * named by the CALLER: the column numbers of the stack's parameter map (<name>_meta.json "parameter_map"; for a C++ caller the
 * parameter_map.yaml generate_solver writes), as tmpc_scatter_parameters takes them.  They live apart from tmpc_hip.h the way the reference keeps
 * mpc_planner_modules apart from mpc_planner_solver; every build of the library (libtmpc_hip.so, the lab twin, every generated library) exports
 * them, so the same calls work on a hand-written shape with the columns of its own map.
 *
 * All three are stream-ordered on the handle's stream: no allocation, no synchronisation.  `cols` is a HOST array, copied before the call
 * returns; every entry in [0, npar), all distinct, at most 128 (the table travels in the kernel arguments).  A refused call (TMPC_ERR_INVALID,
 * the message in tmpc_last_error names the argument) launches nothing.
 *
 * One tick of a generated T-MPC stack without a host round trip:
 *   tmpc_guidance_plan -> tmpc_warmstart -> tmpc_sample_guidance -> tmpc_init_with_guidance -> tmpc_stack_prepare_obstacles
 *   -> tmpc_stack_set_obstacle_columns -> tmpc_stack_linearize_topology_columns -> tmpc_solve -> tmpc_guidance_decide
 * (the path side: tmpc_track_path with window_segments, tmpc_path_velocity_window, tmpc_scatter_parameters).
 * The path window, the road rows and the decomp rows of such stacks: include/tmpc_hip_stack_env.h; their scenario rows: include/tmpc_hip_stack_scenario.h.
 */
#ifndef TMPC_HIP_STACK_H
#define TMPC_HIP_STACK_H

#include "tmpc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tmpc_prepare_obstacles (tmpc_hip.h: the same kernel, arguments, checks and outputs) without the generated-solver refusal: it uses N, dt and
 * the stream of the handle only and needs no batch. */
int tmpc_stack_prepare_obstacles(tmpc_handle *h, int32_t n_scenes, int32_t n_slots, int32_t max_obstacles, const void *d_count, const void *d_state,
                                 const void *d_raw_pos, const void *d_raw_radius, const void *d_raw_vel, const void *d_raw_pred,
                                 const tmpc_obstacle_options *options, void *d_obstacle_pos, void *d_obstacle_shape, void *d_obstacle_radius,
                                 void *d_obstacle_gaussian, void *d_selected);

/* What tmpc_set_obstacle_parameters documents for row_model 0 (EllipsoidConstraints) and 1 (GaussianConstraints) -- stage 0 the dummies, stage
 * k >= 1 prediction step k - 1, the DETERMINISTIC / GAUSSIAN rule, ego_disc_radius = robot_radius and ego_disc_0_offset = disc_offset at every
 * stage -- from the four buffers of tmpc_(stack_)prepare_obstacles with max_obstacles obstacles per scene (d_scene_of i32 [B], d_state f64
 * [n_scenes][4]), into the caller's columns of the CURRENT batch's parameter rows; nothing else is touched.  The order of cols is fixed:
 *   cols[0] ego_disc_radius, cols[1] ego_disc_0_offset, then per obstacle j < max_obstacles the module's fields in the reference's order,
 *   row_model 0: ellipsoid_obst_j_{x, y, psi, major, minor, chi, r}   (cols[2 + 7 j + w])
 *   row_model 1: gaussian_obst_j_{x, y, major, minor, risk, r}       (cols[2 + 6 j + w])
 * so n_cols = 2 + 7 max_obstacles or 2 + 6 max_obstacles.  row_model and max_obstacles are the CALL's, not the handle's (a generated handle has
 * neither).  The same arithmetic as tmpc_set_obstacle_parameters: on a library whose map is the hand-written one the rows are equal bit for bit.
 * TMPC_ERR_INVALID: no batch, a NULL pointer, row_model outside 0 / 1, max_obstacles < 1, n_cols not 2 + F max_obstacles (or above 128), a
 * column outside [0, npar), a duplicate column, B x N x max_obstacles beyond 2^31 - 1. */
int tmpc_stack_set_obstacle_columns(tmpc_handle *h, const int32_t *cols, int32_t n_cols, int32_t row_model, int32_t max_obstacles,
                                    const void *d_obstacle_pos, const void *d_obstacle_shape, const void *d_obstacle_radius, const void *d_obstacle_gaussian,
                                    const void *d_scene_of, const void *d_state, double robot_radius, double disc_offset, double risk, double chi, double obstacle_radius);

/* What tmpc_linearize_topology_ex documents -- the projection to safety of the warm start in the handle's x0, guidance mode or per-obstacle
 * radii (d_obstacle_radius), the static halfspaces copied as given, dummy rows and stage 0 (1, 0, state_x + 100), a non-guided planner's rows
 * after d_is_original -- for a stack with n_rows topology rows, into the caller's columns of the CURRENT batch's parameter rows:
 *   cols [n_rows][3] = lin_constraint_j_{a1, a2, b} of row j;  n_obstacles + n_static <= n_rows,  3 n_rows <= 128.
 * Nothing else is touched.  The same arithmetic as tmpc_linearize_topology_ex: equal bit for bit on the same map, and to the host mirror
 * mpc_planner_amd.modules.linearized_update as closely as that entry point is.
 * TMPC_ERR_INVALID: no batch, NULL cols / d_scene_of / d_state_x, NULL d_obstacle_pos with n_obstacles > 0, NULL d_static_halfspaces with
 * n_static > 0, n_rows < 1 or 3 n_rows > 128, n_obstacles or n_static negative or more of them than n_rows, a column outside [0, npar), a
 * duplicate column, B x N beyond 2^31 - 1. */
int tmpc_stack_linearize_topology_columns(tmpc_handle *h, const int32_t *cols, int32_t n_rows, const void *d_obstacle_pos, int32_t n_obstacles,
                                          const void *d_obstacle_radius, const void *d_static_halfspaces, int32_t n_static, const void *d_scene_of, const void *d_state_x,
                                          double robot_radius, const void *d_is_original);

#ifdef __cplusplus
}
#endif
#endif
