/*
 * tmpc_hip_episode.h -- the world of a closed loop on device: the plant step, the obstacles' motion and the episode log.
 *
 * The fifth header, next to tmpc_hip.h and the three stack headers.  Every per-tick piece of the planner has a device producer; the one entry
 * point below turns the command tmpc_guidance_decide wrote into the NEXT tick's inputs, measures the episode and restarts it, so that a closed
 * loop over thousands of scenes runs stream-ordered without a host round trip.  It reads no parameter column and needs no batch: every build of
 * the library (libtmpc_hip.so, the lab twin, every generated library) exports it, like the guidance entries.  One tick of the T-MPC pipeline:
 *   tmpc_episode_step -> tmpc_prepare_obstacles -> tmpc_guidance_plan -> tmpc_warmstart -> tmpc_sample_guidance -> tmpc_init_with_guidance
 *   -> tmpc_set_obstacle_parameters -> tmpc_linearize_topology_ex -> tmpc_solve -> tmpc_guidance_decide
 *
 * The simulators of the reference's experiments are external; the world model is this project's own.  The bookkeeping around
 * it restates JackalPlanner::loop / reset / objectiveReached (ros1_jackalsimulator.cpp:146-226, :359-378), Planner::reset (planner.cpp:231-245)
 * and ExperimentUtil::update / onTaskComplete (experiment_util.cpp:27-110).
 *
 * Carried multipliers are out of scope: tmpc_solve never reads persistent solver state.  A caller of tmpc_solve_iterations reads d_was_reset
 * and clears the slots of the scenes that were reset itself (tmpc_clear_slot).
 */
#ifndef TMPC_HIP_EPISODE_H
#define TMPC_HIP_EPISODE_H

#include "tmpc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tmpc_episode_options {
    uint32_t size;                 /* sizeof(tmpc_episode_options): the rule of tmpc_create_v2 / tmpc_obstacle_options */
    int32_t substeps;              /* plant substeps per control period, 1 .. 16 */
    int32_t timeout_ticks;         /* > 0: reset(false) when the ticks since the last reset reach it; 0: never */
    int32_t max_episodes;          /* rows of the log per scene, 1 .. 4096 */
    double control_dt;             /* 1 / control_frequency */
    double max_acceleration;       /* plant limit on |dv/dt|; <= 0: v takes the commanded value at once */
    double max_angular_velocity;   /* > 0: the commanded w is clipped to +- it */
    double robot_radius;
    double goal_x;                 /* objective reached when x > goal_x (ros1_jackalsimulator.cpp:146-151); +inf: off */
} tmpc_episode_options;

/* Advance n_scenes worlds by one control period, one wave per scene; stream-ordered on the handle's stream, no allocation, no synchronisation,
 * no batch needed (the handle's nx and stream only).  Device arrays:
 *   d_cmd          f64 [n_scenes][2]            (v, w) as tmpc_guidance_decide wrote it
 *   d_plant        f64 [n_scenes][6]  in/out    (x, y, psi, v, c, s); (c, s) is the heading as a unit vector, carried so that no libm
 *   d_plant0       f64 [n_scenes][6]            trigonometry is on the path: the caller evaluates cos / sin of the start heading once
 *   d_count        i32 [n_scenes]               raw obstacles of the scene, clipped to [0, n_slots]; this and the next three in the layouts
 *   d_raw_pos, d_raw_vel  f64 [n_scenes][n_slots][2]  in/out    tmpc_prepare_obstacles reads; slots at or beyond the count are neither read nor
 *   d_raw_radius   f64 [n_scenes][n_slots]      written
 *   d_raw_pos0, d_raw_vel0                      as d_raw_pos / d_raw_vel: what a reset restores
 *   d_box          f64 [n_scenes][4] or NULL    (xmin, xmax, ymin, ymax)
 *   d_goal         f64 [n_scenes][3] or NULL    (gx, gy, radius): objective reached when |p - g| < radius (contouring.cpp:175)
 *   d_episode      i32 [n_scenes][4]  in/out    (ticks since reset, collision ticks of this episode, episodes finished, 0); start from zeros
 *   d_episode_f    f64 [n_scenes][2]  in/out    (max intrusion of this episode, intrusion of this tick); start from zeros
 *   d_log          f64 [n_scenes][max_episodes][4]   one row per finished episode (step 6)
 *   d_was_reset    u8  [n_scenes]               every entry written on every call
 *   d_state4       f64 [n_scenes][4]            (x, y, psi, v) for tmpc_prepare_obstacles
 *   d_state_nx     f64 [n_scenes][nx] or NULL   for tmpc_guidance_decide / tmpc_track_path: entries 0 .. 3 are written; entries >= 4 are left
 *                                               alone unless the scene was reset, then they become 0 (state = State(), planner.cpp:241)
 *   d_state_batch  f64 [n_scenes P][nx] or NULL the same, once per planner, for tmpc_warmstart
 *   d_planner_ids  i32 [n_scenes][P] or NULL,  d_selection i32 [n_scenes][3] or NULL,  d_segment i32 [n_scenes] or NULL: written only on a reset
 * Per scene, in this order:
 *   1. plant: a velocity-commanded unicycle, `substeps` times with h = control_dt / substeps: w = cmd_w clipped to +-max_angular_velocity by two
 *      comparisons (a NaN passes through); dv = cmd_v - v, clipped to +-max_acceleration h if the limit is positive, v' = v + dv,
 *      vm = (v + v') / 2; a = (w h) / 2, with sin a, cos a and sin a / a as fixed polynomials in a^2 (through a^9, a^10, a^8); (c, s) rotated by
 *      a to the mid heading (cm, sm); x += ((vm h) (sin a / a)) cm, y likewise with sm; rotated by a again; renormalised by sqrt(c^2 + s^2);
 *      psi += w h
 *   2. obstacles: every slot below the count pos += vel control_dt; with a box, a coordinate now outside its interval flips the sign of that
 *      velocity component (the position is not mirrored)
 *   3. intrusion: the maximum over the slots of (robot_radius + radius_j) - sqrt(dx^2 + dy^2) at the advanced positions, from 0.0, replaced on
 *      strict `>` (a NaN never enters); intrusion > 0 counts one collision tick (experiment_util.cpp:65-66)
 *   4. ticks since reset += 1
 *   5. termination on the advanced state (ros1_jackalsimulator.cpp:161-168): completed if x > goal_x or the goal disc is reached; otherwise
 *      timed out if timeout_ticks > 0 and the ticks since reset >= timeout_ticks
 *   6. on either (reset, Planner::reset, onTaskComplete): with fewer than max_episodes episodes finished the log row (ticks control_dt,
 *      completed 1.0 / 0.0, collision ticks, max intrusion) -- beyond the cap nothing is written --; the finished episode counted in either
 *      case; plant and the obstacles' positions and velocities restored from the start arrays; ticks, collision ticks and max intrusion
 *      zeroed (the intrusion of this tick stays this tick's); d_planner_ids[q][.] = -1, d_selection[q] = (-1, 0, -1), d_segment[q] = -1: the
 *      freshly constructed planner (tmpc_guidance_plan then chooses the braking start, tmpc_track_path the global search)
 *   7. the three state outputs from the plant as it now stands
 * Equal bit for bit to mpc_planner_amd.modules.episode_step and to MPCPlanner::episodeStep (mpc_planner/episode.h).
 * TMPC_ERR_INVALID, before any launch, the message in tmpc_last_error names the entry: NULL handle, NULL options, a NULL pointer that is not
 * marked "or NULL"; n_scenes <= 0, n_slots outside [0, 1024], P < 1; substeps outside [1, 16]; control_dt not positive and finite;
 * max_angular_velocity <= 0 or max_angular_velocity control_dt / substeps > 0.125 (the polynomials are stated for |a| <= 1/16); max_episodes
 * outside [1, 4096]; timeout_ticks < 0; robot_radius < 0; an options->size the library cannot honour. */
int tmpc_episode_step(tmpc_handle *h, int32_t n_scenes, int32_t n_slots, int32_t P, const tmpc_episode_options *opt,
                      const void *d_cmd, void *d_plant, const void *d_plant0,
                      const void *d_count, void *d_raw_pos, void *d_raw_vel, const void *d_raw_radius,
                      const void *d_raw_pos0, const void *d_raw_vel0, const void *d_box, const void *d_goal,
                      void *d_episode, void *d_episode_f, void *d_log, void *d_was_reset,
                      void *d_state4, void *d_state_nx, void *d_state_batch,
                      void *d_planner_ids, void *d_selection, void *d_segment);

#ifdef __cplusplus
}
#endif
#endif
