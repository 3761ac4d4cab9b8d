/*
 * tmpc_hip_guidance_search.h -- the guidance search on device: topology-distinct trajectories per scene.
 *
 * The sixth header, next to tmpc_hip.h, the three stack headers and tmpc_hip_episode.h.  tmpc_sample_guidance and tmpc_guidance_plan read nodes,
 * counts and topology classes "the caller delivers"; the one entry point below produces them on the device from the obstacles
 * tmpc_prepare_obstacles just wrote, so that the closed loop tmpc_episode_step advances also plans through topologies that look at those
 * obstacles.  It reads no parameter column and needs no batch, only the handle's N, dt and stream: every build of the library (libtmpc_hip.so,
 * the lab twin, every generated library) exports it.  One tick of the T-MPC pipeline:
 *   tmpc_episode_step -> tmpc_prepare_obstacles -> tmpc_guidance_search -> tmpc_guidance_plan -> tmpc_warmstart -> tmpc_sample_guidance
 *   -> tmpc_init_with_guidance -> tmpc_set_obstacle_parameters -> tmpc_linearize_topology_ex -> tmpc_solve -> tmpc_guidance_decide
 *
 * The reference's search is the external guidance_planner (a visibility-PRM in (x, y, t), a homotopy filter, the n_paths cheapest classes); its
 * source is not in the reference tree, only its configuration is.  What is built here is this project's own restatement of the method, stated
 * completely below.  No parity with a real guidance_planner is claimed.
 */
#ifndef TMPC_HIP_GUIDANCE_SEARCH_H
#define TMPC_HIP_GUIDANCE_SEARCH_H

#include "tmpc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tmpc_guidance_search_options {
    uint32_t size;                 /* sizeof(tmpc_guidance_search_options): the rule of tmpc_create_v2 / tmpc_obstacle_options */
    int32_t n_paths;               /* trajectories per scene at most, 1 .. 16 (guidance_planner.yaml n_paths) */
    int32_t n_samples;             /* samples of the visibility-PRM, 0 .. 256 (n_samples) */
    int32_t reserved;              /* 0: any other value is refused */
    uint64_t seed;                 /* of the counter-based samples */
    int32_t n_nodes_max;           /* R: nodes per trajectory at most, 2 .. 64; the n_nodes_max of tmpc_sample_guidance */
    int32_t max_expansions;        /* connector visits of the path enumeration at most, 1 .. 65536 */
    double robot_radius;           /* >= 0 */
    double max_velocity;           /* a connection may not be faster; positive and finite */
    double margin;                 /* the sampling box is the bounding box of the start and the goals grown by it; >= 0 and finite */
    double weight_length;          /* path cost = weight_length length + goal cost; positive and finite */
} tmpc_guidance_search_options;

/* Search n_scenes scenes, one wave per scene; stream-ordered on the handle's stream, no allocation, no synchronisation, no batch needed (the
 * handle's N, dt and stream only).  Device arrays, P = n_paths, R = n_nodes_max:
 *   d_state4          f64 [n_scenes][4]                     the start (x, y); psi and v are not read
 *   d_goals           f64 [n_scenes][n_goals][3]            (x, y, cost), 1 <= n_goals <= 16; a goal with a non-finite coordinate is absent
 *   d_obstacle_pos    f64 [n_scenes][max_obstacles][N][2]   as tmpc_prepare_obstacles writes them, max_obstacles <= 32 here; a slot with
 *   d_obstacle_radius f64 [n_scenes][max_obstacles]         d_selected < 0 is a dummy and does not exist for the search.  At STAGE k an obstacle is
 *   d_selected        i32 [n_scenes][max_obstacles]         where the solver's collision row of stage k sees it: prepared step max(k - 1, 0)
 *   d_was_reset       u8  [n_scenes] or NULL                as tmpc_episode_step writes it
 *   d_prev_traj       f64 [n_scenes][P][N + 1][2]  in/out   carried state, caller-owned, zero-initialised: last tick's trajectories at every stage,
 *   d_prev_class      i32 [n_scenes][P]            in/out   their classes (-1 beyond the count),
 *   d_prev_count      i32 [n_scenes]               in/out   their number,
 *   d_next_class      i32 [n_scenes]               in/out   the next unused class id
 *   d_nodes           f64 [n_scenes P][R][3]                (t, x, y) per node and d_node_count i32 [n_scenes P]: what tmpc_sample_guidance takes with
 *   d_node_count                                            n_traj = n_scenes P.  Unused trajectories get count 0; unused nodes are left alone
 *   d_traj_count      i32 [n_scenes]                        what tmpc_guidance_plan takes; d_topology_class i32 [n_scenes][P], -1 beyond the count
 *   d_status          i32 [n_scenes]                        flags: 1 the guard table was full, 2 the connector table was full, 4 the enumeration
 *                                                           stopped at max_expansions, 8 a path was skipped because it has more than R nodes
 * Per scene, in this order (U20):
 *   stage grid   a node is (k, x, y), 0 <= k <= N, t = k dt.  A CONNECTION a -> b needs k_a < k_b and is the straight line at the stages,
 *                p(k) = p_a + (p_b - p_a) ((k - k_a) / (k_b - k_a)), the endpoints as they are.  It is VALID if |p_b - p_a|^2 <=
 *                ((max_velocity (k_b - k_a)) dt)^2 and for every stage 1 <= k in [k_a, k_b] and every real obstacle j |p(k) - o_j(k)|^2 >=
 *                (r_j + robot_radius)^2; stage 0 is never tested; a NaN anywhere makes it invalid
 *   homotopy     two polylines A, B given at every stage of a common span [k_a, k_b] are EQUIVALENT iff for every real obstacle j the closed
 *                polygon A(k) - o_j(k), k ascending, then B(k) - o_j(k), k descending, has winding number 0 about the origin by the crossing
 *                rule: an edge u -> w counts +1 if u_y <= 0 < w_y and u_x w_y - u_y w_x > 0, -1 if w_y <= 0 < u_y and u_x w_y - u_y w_x < 0.
 *                Comparisons and that cross product only: an integer, no libm.  With no real obstacle everything is equivalent.  (The
 *                `Winding` comparison of the planner's configuration made exact, in place of the H-signature default.)
 *   PRM          guards: the start (k = 0), then the present goals in index order (k = N); the table holds 32.  The sampling box is the bounding
 *                box of the start and the present goals, grown by margin.  Sample i < n_samples (none with N < 2), in order: u_c = splitmix64
 *                bits of (seed, scene, 3 i + c) as tmpc_sample_scenarios draws them; k = 1 + (u_0 mod (N - 1)), x = lo + (hi - lo) ((u_1 >> 11)
 *                2^-53), y likewise from u_2.  The sample is VISIBLE from a guard of another stage when the connection between them, earlier
 *                stage first, is valid.  No guard visible: the sample becomes a guard (flag 1 if the table is full).  Otherwise g1 = the visible
 *                guard of an earlier stage with the smallest squared planar distance, the lowest index on ties, g2 the same among the later
 *                ones; either missing: dropped.  The candidate connector (g1, s, g2) has length |s - g1| + |g2 - s|; it is compared, in table
 *                order, with every connector of the same pair (g1, g2) by the homotopy test on the two-leg polylines: the first equivalent one
 *                is replaced if the candidate is strictly shorter, else the candidate is dropped; with none it is appended (the table holds
 *                128; flag 2 if it is full)
 *   paths        candidates: the direct connections start -> goal in goal order where valid, then all chains start, c, g, c', g', ..., goal
 *                depth first with the connectors in table order; a connector visit is a connector found to leave the current guard, at most
 *                max_expansions of them (flag 4 at the next).  A path with more than R nodes is skipped (flag 8).  cost = weight_length (sum of
 *                the legs' planar lengths, in path order, from 0.0) + goal cost.  The kept list (16) holds one path per class: a candidate
 *                equivalent (both at all N + 1 stages) to a kept one, in list order, replaces it if strictly cheaper, else is dropped; not
 *                equivalent to any: appended, or with the list full it replaces the most expensive kept path (the highest index on ties) if
 *                strictly cheaper.  The kept paths are ordered stably by ascending cost; the first min(kept, P) are the scene's trajectories,
 *                their nodes the graph nodes with t = k dt
 *   identity     d_was_reset[q] != 0: prev_count and next_class become 0 first.  The shifted previous trajectory p is the current start at
 *                stage 0 and prev[p][min(k + 1, N)] at stage k >= 1.  Trajectory i, in output order, takes the class of the first previous
 *                trajectory that no earlier trajectory of this tick has claimed and that is equivalent to it against THIS tick's obstacles,
 *                otherwise next_class, which then grows by one.  Then the carried arrays take this tick's trajectories (at every stage),
 *                classes and count.  Previous trajectories name classes only: they are not re-entered as candidates
 * Equal bit for bit to mpc_planner_amd.modules.guidance_search and to MPCPlanner::guidanceSearch (mpc_planner_modules/guidance_search.h).
 * TMPC_ERR_INVALID, before any launch, the message in tmpc_last_error names the entry: NULL handle, NULL options, a NULL pointer other than
 * d_was_reset; n_scenes <= 0; n_goals outside [1, 16]; max_obstacles outside [1, 32]; n_paths outside [1, 16]; n_samples outside [0, 256];
 * n_nodes_max outside [2, 64]; max_expansions outside [1, 65536]; robot_radius < 0; max_velocity or weight_length not positive and finite;
 * margin negative or not finite; options->reserved != 0; an options->size the library cannot honour. */
int tmpc_guidance_search(tmpc_handle *h, int32_t n_scenes, int32_t n_goals, int32_t max_obstacles, const tmpc_guidance_search_options *opt,
                         const void *d_state4, const void *d_goals, const void *d_obstacle_pos, const void *d_obstacle_radius,
                         const void *d_selected, const void *d_was_reset, void *d_prev_traj, void *d_prev_class, void *d_prev_count,
                         void *d_next_class, void *d_nodes, void *d_node_count, void *d_traj_count, void *d_topology_class, void *d_status);

#ifdef __cplusplus
}
#endif
#endif
