/*
 * mpc_planner_modules/guidance_handoff.h -- the hand-off either side of the guidance search, on the host.  GuidanceSpline: the
 * space-time nodes a guidance search delivers per trajectory -> the time splines x(t), y(t) -> the samples at t = k dt that
 * GuidanceConstraints::initializeSolverWithGuidance reads (guidance_constraints.cpp:390-414; RosTools::Spline2D and the guidance planner's
 * trajectory type are not in the reference tree: a real guidance_planner may parametrise or extrapolate differently).  guidancePlan /
 * guidanceDecide: GuidanceConstraints' bookkeeping around the solve for many scenes at once (:192-250, :283-317, :343-387, :416-434;
 * planner.cpp:78-86; ros1_jackalsimulator.cpp:181-201), entry b = q P + p.  Needs no Solver and no generated header.  The arithmetic and the
 * bookkeeping are those of mpc_planner_types/prep_arithmetic.h, the one source tmpc_sample_guidance_kernel, tmpc_guidance_plan_kernel and
 * tmpc_guidance_decide_kernel compile too; the independent statement both are tested against, bit for bit, is mpc_planner_amd/modules.py
 * (sample_guidance, guidance_plan, guidance_decide) -- where the compiler does not fuse multiply-adds (build with -ffp-contract=off).
 */
#ifndef MPC_GUIDANCE_HANDOFF_HIP_H
#define MPC_GUIDANCE_HANDOFF_HIP_H

#include <cstdint>
#include <vector>

#include <mpc_planner_modules/reference_path.h>

namespace MPCPlanner
{
    struct GuidanceSpline
    {
        static constexpr int MAX_NODES = 64;                    /* tmpc_sample_guidance's limit */
        std::vector<double> t;                                  /* the knots; empty: no valid spline */
        std::vector<double> cx[4], cy[4];                       /* (a b c d) of x and y per segment, on tau = t - t_i */

        bool valid() const { return !t.empty(); }
        int numSegments() const { return valid() ? (int)t.size() - 1 : 0; }

        /* The natural cubic splines of U15 through the nodes (ReferencePathSpline::fitCubic; two nodes: the straight line).  False -- and no
         * spline -- if the count is outside [2, n_nodes_max] or a knot spacing is not positive and finite. */
        bool fit(const std::vector<GuidanceNode> &nodes, int n_nodes_max = MAX_NODES)
        {
            t.clear();
            const size_t n = nodes.size();
            if (n < 2 || n > (size_t)n_nodes_max) return false;
            std::vector<double> knots(n), x(n), y(n);
            for (size_t i = 0; i < n; i++) { knots[i] = nodes[i].t; x[i] = nodes[i].x; y[i] = nodes[i].y; }
            if (!ReferencePathSpline::fitCubic(knots, x, cx[0], cx[1], cx[2], cx[3]) || !ReferencePathSpline::fitCubic(knots, y, cy[0], cy[1], cy[2], cy[3])) return false;
            t = knots;
            return true;
        }
        /* the segment of time s: max{j <= n - 2 : t_j <= s}, 0 if there is none -- outside the node span the first / last cubic continues */
        int segment(double s) const
        {
            int i = 0;
            for (int j = 0; j + 1 < (int)t.size(); j++) if (t[j] <= s) i = j;
            return i;
        }
        /* position and velocity at t = k dt, k = 0 .. N, as [N + 1][2] each; zeros without a valid spline.  Returns the status of
         * tmpc_sample_guidance: 0 ok, 1 invalid. */
        int sample(int N, double dt, std::vector<double> &pos, std::vector<double> &vel) const
        {
            pos.assign((size_t)(N + 1) * 2, 0.); vel.assign((size_t)(N + 1) * 2, 0.);
            if (!valid()) return 1;
            for (int k = 0; k <= N; k++) {
                const double s = tmpc_arith::sample_time(k, dt);
                const int i = segment(s);
                const double tau = s - t[i];
                const double kx[4] = {cx[0][i], cx[1][i], cx[2][i], cx[3][i]}, ky[4] = {cy[0][i], cy[1][i], cy[2][i], cy[3][i]};
                pos[(size_t)k * 2] = tmpc_arith::cubic_value(kx, tau); pos[(size_t)k * 2 + 1] = tmpc_arith::cubic_value(ky, tau);
                vel[(size_t)k * 2] = tmpc_arith::cubic_slope(kx, tau); vel[(size_t)k * 2 + 1] = tmpc_arith::cubic_slope(ky, tau);
            }
            return 0;
        }
    };

    /* one trajectory of the guidance search as the hand-off needs it: what GuidanceTrajectory (mpc_planner_types/data_types.h) carries, without
     * the Solver's types */
    struct GuidanceCandidate
    {
        std::vector<GuidanceNode> nodes;
        int topology_class{0};
        bool previously_selected{false};
    };

    /* the settings both calls share (tmpc_guidance_options) */
    struct GuidanceHandoffConfig
    {
        int n_paths{1};
        bool use_tmpcpp{true}, warmstart_with_mpc_solution{false}, shift_previous_solution_forward{true};
        double selection_weight_consistency{1.};
        int P() const { return n_paths + (use_tmpcpp ? 1 : 0); }
    };
    /* the cross-tick state of n_scenes scenes: planner_ids [n_scenes][P], selection [n_scenes][3], as tmpc_guidance_plan reads them */
    struct GuidanceHandoffState
    {
        std::vector<int32_t> planner_ids, selection;
        void reset(int n_scenes, int P)
        {
            planner_ids.assign((size_t)n_scenes * P, -1); selection.assign((size_t)n_scenes * 3, -1);
            for (int q = 0; q < n_scenes; q++) selection[(size_t)q * 3 + 1] = 0;
        }
    };
    /* what every planner does this tick, [n_scenes P] each (tmpc_guidance_plan's outputs) */
    struct GuidancePlan
    {
        std::vector<int32_t> mode, src, guidance_id;
        std::vector<uint8_t> init_enabled, rows_dummy, disabled;
        std::vector<double> weight;
    };
    /* traj_count [n_scenes], topology_class [n_scenes][n_paths], previously_selected [n_scenes][n_paths] or nullptr */
    inline void guidancePlan(const GuidanceHandoffConfig &cfg, int n_scenes, const int32_t *traj_count, const int32_t *topology_class, const uint8_t *previously_selected,
                             const GuidanceHandoffState &state, GuidancePlan &plan)
    {
        const size_t P = (size_t)cfg.P(), B = (size_t)n_scenes * P;
        plan.mode.assign(B, 0); plan.src.assign(B, 0); plan.guidance_id.assign(B, 0); plan.init_enabled.assign(B, 0); plan.rows_dummy.assign(B, 0);
        plan.disabled.assign(B, 0); plan.weight.assign(B, 1.);
        for (size_t q = 0; q < (size_t)n_scenes; q++) {
            const size_t f = q * P;
            tmpc_arith::guidance_plan_scene((int)f, cfg.n_paths, cfg.use_tmpcpp, cfg.warmstart_with_mpc_solution, cfg.shift_previous_solution_forward,
                                            cfg.selection_weight_consistency, traj_count[q], topology_class + q * cfg.n_paths,
                                            previously_selected ? previously_selected + q * cfg.n_paths : nullptr, &state.planner_ids[f], &state.selection[q * 3],
                                            &plan.mode[f], &plan.src[f], &plan.init_enabled[f], &plan.rows_dummy[f], &plan.disabled[f], &plan.guidance_id[f],
                                            &plan.weight[f]);
        }
    }
    /* the decision of every scene (tmpc_guidance_decide's outputs): best, exit [n_scenes], cmd [n_scenes][2] */
    struct GuidanceDecision
    {
        std::vector<int32_t> best, exit_code;
        std::vector<double> cmd;
    };
    /* pobj, exit_code [n_scenes P]; xtraj [n_scenes P][N + 1][nx], utraj [n_scenes P][N][nu], state [n_scenes][nx] (v = entry 3, w = input 1);
     * `state_io` is committed for the next tick's guidancePlan */
    inline void guidanceDecide(const GuidanceHandoffConfig &cfg, int n_scenes, const double *pobj, const int32_t *exit_code, const GuidancePlan &plan, const double *state,
                               const double *xtraj, const double *utraj, int N, int nx, int nu, double deceleration, double control_dt, bool enable_output,
                               GuidanceHandoffState &state_io, GuidanceDecision &out)
    {
        const size_t P = (size_t)cfg.P();
        out.best.assign((size_t)n_scenes, -1); out.exit_code.assign((size_t)n_scenes, -1); out.cmd.assign((size_t)n_scenes * 2, 0.);
        const int x_entry = (N + 1) * nx, u_entry = N * nu;
        for (size_t q = 0; q < (size_t)n_scenes; q++) {
            const size_t f = q * P;
            tmpc_arith::guidance_decide_scene((int)P, cfg.use_tmpcpp, pobj + f, exit_code + f, &plan.disabled[f], &plan.guidance_id[f], &plan.weight[f], xtraj + f * x_entry,
                                              x_entry, nx, utraj + f * u_entry, u_entry, state[q * nx + 3], deceleration, control_dt, enable_output, &out.best[q],
                                              &out.exit_code[q], &out.cmd[q * 2], &state_io.planner_ids[f], &state_io.selection[q * 3]);
        }
    }
}
#endif
