/*
 * mpc_planner/episode.h (HIP flavour) -- the world of a closed loop on the host: MPCPlanner::episodeStep is tmpc_episode_step
 * (include/tmpc_hip_episode.h) for callers of the C++ mirror, on host arrays in the device's layouts, and the CPU check of the kernel's
 * indexing.  Header-only, Solver-free, no GPU.  The bookkeeping restates JackalPlanner::loop / reset / objectiveReached
 * (ros1_jackalsimulator.cpp:146-226, :359-378), Planner::reset (planner.cpp:231-245) and ExperimentUtil::update / onTaskComplete
 * (experiment_util.cpp:27-110); the world model is this project's own.  The arithmetic is that of
 * mpc_planner_types/prep_arithmetic.h, the one source tmpc_episode_step_kernel compiles too; the independent statement both are tested against,
 * bit for bit, is mpc_planner_amd/modules.py episode_step.  Build with -ffp-contract=off.
 */
#ifndef MPC_EPISODE_HIP_H
#define MPC_EPISODE_HIP_H

#include <cstddef>
#include <cstdint>

#include <mpc_planner_types/prep_arithmetic.h>

namespace MPCPlanner
{
    /* the fields of tmpc_episode_options behind `size` */
    struct EpisodeOptions {
        int substeps = 1, timeout_ticks = 0, max_episodes = 1;
        double control_dt = 0.05, max_acceleration = 0., max_angular_velocity = 2., robot_radius = 0., goal_x = __builtin_huge_val();
    };

    /* what tmpc_episode_step refuses */
    inline bool episodeOptionsValid(const EpisodeOptions &o, int n_scenes, int n_slots, int P)
    {
        return n_scenes > 0 && n_slots >= 0 && n_slots <= 1024 && P >= 1 && o.substeps >= 1 && o.substeps <= 16 && o.control_dt > 0. &&
               o.control_dt < __builtin_huge_val() && o.max_angular_velocity > 0. && o.max_angular_velocity * o.control_dt / (double)o.substeps <= 0.125 &&
               o.max_episodes >= 1 && o.max_episodes <= 4096 && o.timeout_ticks >= 0 && o.robot_radius >= 0.;
    }

    /* One control period of n_scenes scenes: every array as tmpc_episode_step documents it (box, goal, state_nx, state_batch, planner_ids,
     * selection and segment may be null), nx doubles per planner state.  The scenes in order, the slots of a scene in order: the running
     * maximum of the intrusion replaces on strict `>` from 0.0, so the order does not matter.  false: refused, nothing written. */
    inline bool episodeStep(int n_scenes, int n_slots, int P, int nx, const EpisodeOptions &o, const double *cmd, double *plant, const double *plant0,
                            const int32_t *count, double *raw_pos, double *raw_vel, const double *raw_radius, const double *raw_pos0,
                            const double *raw_vel0, const double *box, const double *goal, int32_t *episode, double *episode_f, double *log,
                            uint8_t *was_reset, double *state4, double *state_nx, double *state_batch, int32_t *planner_ids, int32_t *selection,
                            int32_t *segment)
    {
        if (!episodeOptionsValid(o, n_scenes, n_slots, P)) return false;
        const size_t R = (size_t)n_slots;
        for (size_t q = 0; q < (size_t)n_scenes; q++) {
            int cnt = count[q];
            cnt = cnt < 0 ? 0 : (cnt > n_slots ? n_slots : cnt);
            double p[6];
            for (int i = 0; i < 6; i++) p[i] = plant[q * 6 + i];
            const double h = o.control_dt / (double)o.substeps;
            for (int it = 0; it < o.substeps; it++)
                tmpc_arith::plant_substep(cmd[q * 2], cmd[q * 2 + 1], h, o.max_acceleration, o.max_angular_velocity, p);
            const bool boxed = box != nullptr;
            double xlo = 0., xhi = 0., ylo = 0., yhi = 0.;
            if (boxed) { xlo = box[q * 4]; xhi = box[q * 4 + 1]; ylo = box[q * 4 + 2]; yhi = box[q * 4 + 3]; }
            double *rp = raw_pos + q * R * 2, *rv = raw_vel + q * R * 2;
            double intrusion = 0.;
            for (int i = 0; i < cnt; i++) {
                tmpc_arith::obstacle_step(rp[i * 2], rv[i * 2], o.control_dt, boxed, xlo, xhi);
                tmpc_arith::obstacle_step(rp[i * 2 + 1], rv[i * 2 + 1], o.control_dt, boxed, ylo, yhi);
                const double cand = tmpc_arith::intrusion_candidate(o.robot_radius, raw_radius[q * R + i], rp[i * 2], rp[i * 2 + 1], p[0], p[1]);
                if (cand > intrusion) intrusion = cand;
            }
            int ticks = episode[q * 4] + 1, collisions = episode[q * 4 + 1] + (intrusion > 0. ? 1 : 0), finished = episode[q * 4 + 2];
            double max_intrusion = episode_f[q * 2];
            if (intrusion > max_intrusion) max_intrusion = intrusion;
            bool completed = p[0] > o.goal_x;
            if (goal) completed = completed || tmpc_arith::within_distance(p[0], p[1], goal[q * 3], goal[q * 3 + 1], goal[q * 3 + 2]);
            const bool reset = completed || (o.timeout_ticks > 0 && ticks >= o.timeout_ticks);
            if (reset) {
                if (finished >= 0 && finished < o.max_episodes) {
                    double *row = log + (q * (size_t)o.max_episodes + (size_t)finished) * 4;
                    row[0] = (double)ticks * o.control_dt; row[1] = completed ? 1. : 0.; row[2] = (double)collisions; row[3] = max_intrusion;
                }
                finished += 1;
                for (int i = 0; i < 6; i++) p[i] = plant0[q * 6 + i];
                for (int i = 0; i < cnt * 2; i++) { rp[i] = raw_pos0[q * R * 2 + i]; rv[i] = raw_vel0[q * R * 2 + i]; }
                ticks = 0; collisions = 0; max_intrusion = 0.;
                if (planner_ids) for (int e = 0; e < P; e++) planner_ids[q * (size_t)P + e] = -1;
                if (selection) { selection[q * 3] = -1; selection[q * 3 + 1] = 0; selection[q * 3 + 2] = -1; }
                if (segment) segment[q] = -1;
            }
            episode[q * 4] = ticks; episode[q * 4 + 1] = collisions; episode[q * 4 + 2] = finished; episode[q * 4 + 3] = 0;
            episode_f[q * 2] = max_intrusion; episode_f[q * 2 + 1] = intrusion;
            was_reset[q] = reset ? 1 : 0;
            for (int i = 0; i < 6; i++) plant[q * 6 + i] = p[i];
            for (int i = 0; i < 4; i++) state4[q * 4 + i] = p[i];
            auto write_state = [&](double *s) {
                for (int e = 0; e < nx; e++) {
                    if (e < 4) s[e] = p[e];
                    else if (reset) s[e] = 0.;
                }
            };
            if (state_nx) write_state(state_nx + q * (size_t)nx);
            if (state_batch) for (int e = 0; e < P; e++) write_state(state_batch + (q * (size_t)P + e) * (size_t)nx);
        }
        return true;
    }
}
#endif
