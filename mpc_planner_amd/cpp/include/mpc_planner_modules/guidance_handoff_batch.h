/*
 * mpc_planner_modules/guidance_handoff_batch.h -- the batched device twin of mpc_planner_modules/guidance_handoff.h, next to
 * mpc_planner_modules/reference_path_batch.h: the guidance search's output for several scenes -- per scene the trajectories found, each with
 * its nodes, its topology class and its selection flag -- is uploaded ONCE per tick with setGuidance() (one staging block: nodes, node counts,
 * trajectory counts, classes, flags); sample() enqueues tmpc_sample_guidance, plan() tmpc_guidance_plan and, after the solve, decide()
 * tmpc_guidance_decide.  The twin owns the cross-tick state arrays (each planner's last guidance ID, the selection) and every output buffer,
 * laid out as the existing calls read them: mode() / src() for tmpc_warmstart, positions() / velocities() / initEnabled() for
 * tmpc_init_with_guidance, rowsDummy() for tmpc_linearize_topology_ex (d_is_original), best() for tmpc_gather_best.  The batch layout is the
 * C-ABI's: entry b = q P + p, the non-guided planner last (include/tmpc_hip.h).  Bit for bit what GuidanceSpline, guidancePlan and
 * guidanceDecide give on the host.  For callers of the C-ABI that keep a launch of many scenes on the device; needs the HIP
 * runtime header (compile with -D__HIP_PLATFORM_AMD__ and the ROCm include directory).  Everything is enqueued on the handle's stream;
 * setGuidance() and reset() wait for their own uploads (the staging memory is their own), not for the kernels.
 */
#ifndef MPC_GUIDANCE_HANDOFF_BATCH_HIP_H
#define MPC_GUIDANCE_HANDOFF_BATCH_HIP_H

#include <cstring>

#include <mpc_planner_modules/guidance_handoff.h>
#include <mpc_planner_solver/device_plumbing.h>

namespace MPCPlanner
{
    class BatchedGuidanceHandoff : private DevicePlumbing
    {
    public:
        /* n_scenes scenes of P = cfg.P() planners; up to n_nodes_max (2 .. 64) nodes per trajectory; N = the solver's horizon (tmpc_dims::N) */
        BatchedGuidanceHandoff(tmpc_handle *handle, int n_scenes, const GuidanceHandoffConfig &cfg, int n_nodes_max, int N)
            : DevicePlumbing(handle, "BatchedGuidanceHandoff"), _Q(n_scenes), _P(cfg.P()), _R(n_nodes_max), _N(N), _cfg(cfg)
        {
            const size_t Q = (size_t)_Q, B = Q * _P, K = (size_t)_N + 1;
            alloc(_d_stage, stageBytes());
            alloc(_d_ids, B * sizeof(int)); alloc(_d_selection, Q * 3 * sizeof(int));
            alloc(_d_mode, B * sizeof(int)); alloc(_d_src, B * sizeof(int)); alloc(_d_guidance_id, B * sizeof(int));
            alloc(_d_init, B); alloc(_d_dummy, B); alloc(_d_disabled, B); alloc(_d_weight, B * 8);
            alloc(_d_gpos, B * K * 2 * 8); alloc(_d_gvel, B * K * 2 * 8); alloc(_d_status, B * sizeof(int));
            alloc(_d_best, Q * sizeof(int)); alloc(_d_exit, Q * sizeof(int)); alloc(_d_cmd, Q * 2 * 8);
            _opt.size = sizeof(_opt); _opt.n_paths = cfg.n_paths; _opt.use_tmpcpp = cfg.use_tmpcpp; _opt.warmstart_with_mpc_solution = cfg.warmstart_with_mpc_solution;
            _opt.shift_previous_solution_forward = cfg.shift_previous_solution_forward; _opt.reserved = 0;
            _opt.selection_weight_consistency = cfg.selection_weight_consistency;
            reset();
        }
        ~BatchedGuidanceHandoff()
        {
            for (void *p : {_d_stage, _d_ids, _d_selection, _d_mode, _d_src, _d_guidance_id, _d_init, _d_dummy, _d_disabled, _d_weight, _d_gpos, _d_gvel, _d_status, _d_best,
                            _d_exit, _d_cmd}) if (p) (void)hipFree(p);
        }
        BatchedGuidanceHandoff(const BatchedGuidanceHandoff &) = delete;
        BatchedGuidanceHandoff &operator=(const BatchedGuidanceHandoff &) = delete;

        /* the state of a fresh GuidanceConstraints: every planner's guidance ID -1 (SolverResult::Reset), nothing selected, no previous solution */
        void reset()
        {
            GuidanceHandoffState s;
            s.reset(_Q, _P);
            void *stream = this->stream();
            copy(_d_ids, s.planner_ids.data(), s.planner_ids.size() * sizeof(int), stream);
            copy(_d_selection, s.selection.data(), s.selection.size() * sizeof(int), stream);
            sync(stream);
        }

        /* This tick's output of the guidance search: guidance[q] = the trajectories of scene q, trajectory i for planner i (those beyond n_paths
         * are not seen); of each its nodes (those beyond n_nodes_max make it invalid), topology_class and -- with use_previously_selected --
         * previously_selected; without, the flags come from the twin's selection state (tmpc_guidance_plan with d_previously_selected = NULL).
         * One upload. */
        void setGuidance(const std::vector<std::vector<GuidanceCandidate>> &guidance, bool use_previously_selected)
        {
            const size_t Q = (size_t)_Q, R = (size_t)_R, n_paths = (size_t)_cfg.n_paths;
            if (guidance.size() != Q) fail("setGuidance: one list of trajectories per scene");
            std::vector<double> stage((stageBytes() + 7) / 8, 0.);
            char *base = reinterpret_cast<char *>(stage.data());
            double *nodes = stage.data();
            int *node_count = reinterpret_cast<int *>(base + oNodeCount()), *traj_count = reinterpret_cast<int *>(base + oTrajCount());
            int *classes = reinterpret_cast<int *>(base + oClasses());
            unsigned char *prev = reinterpret_cast<unsigned char *>(base + oPrev());
            for (size_t q = 0; q < Q; q++) {
                const size_t n = guidance[q].size() < n_paths ? guidance[q].size() : n_paths;
                traj_count[q] = (int)n;
                for (size_t i = 0; i < n; i++) {
                    const GuidanceCandidate &g = guidance[q][i];
                    const size_t b = q * _P + i;
                    node_count[b] = (int)g.nodes.size();
                    for (size_t j = 0; j < g.nodes.size() && j < R; j++) { double *o = nodes + (b * R + j) * 3; o[0] = g.nodes[j].t; o[1] = g.nodes[j].x; o[2] = g.nodes[j].y; }
                    classes[q * n_paths + i] = g.topology_class;
                    prev[q * n_paths + i] = g.previously_selected ? 1 : 0;
                }
            }
            _use_prev = use_previously_selected;
            void *stream = this->stream();
            copy(_d_stage, stage.data(), stageBytes(), stream);
            sync(stream);                                                     // the staging vector ends with this call
        }
        /* tmpc_sample_guidance for every entry: positions() / velocities() [B][N + 1][2] and status() i32 [B]; an entry without a trajectory
         * (the non-guided planner, a planner beyond the scene's count) has no nodes: status 1, zeros -- its initEnabled() is 0 */
        void sample()
        {
            char *base = static_cast<char *>(_d_stage);
            if (tmpc_sample_guidance(_h, _Q * _P, _R, base, base + oNodeCount(), _d_gpos, _d_gvel, _d_status)) fail(tmpc_last_error(_h));
        }
        /* tmpc_guidance_plan from the uploaded counts and classes and the twin's state; pure, the state is not touched */
        void plan()
        {
            char *base = static_cast<char *>(_d_stage);
            if (tmpc_guidance_plan(_h, _Q, &_opt, base + oTrajCount(), base + oClasses(), _use_prev ? base + oPrev() : nullptr, _d_ids, _d_selection, _d_mode, _d_src,
                                   _d_init, _d_dummy, _d_disabled, _d_guidance_id, _d_weight)) fail(tmpc_last_error(_h));
        }
        /* After tmpc_solve on the handle's batch of n_scenes P entries: tmpc_guidance_decide on the handle's own results.  d_state f64
         * [n_scenes][nx] on the device.  Commits the state for the next tick's plan(). */
        void decide(const void *d_state, double deceleration, double control_dt, bool enable_output = true)
        {
            void *d_pobj = nullptr, *d_code = nullptr;
            if (tmpc_result_device_ptrs(_h, &d_pobj, &d_code)) fail(tmpc_last_error(_h));
            if (tmpc_guidance_decide(_h, _Q, &_opt, d_pobj, d_code, _d_disabled, _d_guidance_id, _d_weight, d_state, deceleration, control_dt, enable_output ? 1 : 0,
                                     _d_best, _d_exit, _d_cmd, _d_ids, _d_selection)) fail(tmpc_last_error(_h));
        }

        /* device buffers.  After plan(), [B]: i32 mode / src / guidanceId, u8 initEnabled / rowsDummy / disabled, f64 weight */
        const void *mode() const { return _d_mode; }
        const void *src() const { return _d_src; }
        const void *guidanceId() const { return _d_guidance_id; }
        const void *initEnabled() const { return _d_init; }
        const void *rowsDummy() const { return _d_dummy; }
        const void *disabled() const { return _d_disabled; }
        const void *weight() const { return _d_weight; }
        /* after sample() */
        const void *positions() const { return _d_gpos; }
        const void *velocities() const { return _d_gvel; }
        const void *status() const { return _d_status; }
        /* after decide(): i32 best / exitCode [n_scenes], f64 cmd [n_scenes][2]; the state: i32 plannerIds [n_scenes][P], selection [n_scenes][3] */
        const void *best() const { return _d_best; }
        const void *exitCode() const { return _d_exit; }
        const void *cmd() const { return _d_cmd; }
        const void *plannerIds() const { return _d_ids; }
        const void *selection() const { return _d_selection; }

    private:
        /* the staging block: nodes f64 [B][R][3], node_count i32 [B], traj_count i32 [Q], classes i32 [Q][n_paths], previously_selected u8 [Q][n_paths] */
        size_t oNodeCount() const { return (size_t)_Q * _P * _R * 3 * 8; }
        size_t oTrajCount() const { return oNodeCount() + (size_t)_Q * _P * sizeof(int); }
        size_t oClasses() const { return oTrajCount() + (size_t)_Q * sizeof(int); }
        size_t oPrev() const { return oClasses() + (size_t)_Q * _cfg.n_paths * sizeof(int); }
        size_t stageBytes() const { return oPrev() + (size_t)_Q * _cfg.n_paths; }

        int _Q, _P, _R, _N;
        GuidanceHandoffConfig _cfg;
        tmpc_guidance_options _opt{};
        bool _use_prev{false};
        void *_d_stage{nullptr}, *_d_ids{nullptr}, *_d_selection{nullptr};
        void *_d_mode{nullptr}, *_d_src{nullptr}, *_d_guidance_id{nullptr}, *_d_init{nullptr}, *_d_dummy{nullptr}, *_d_disabled{nullptr}, *_d_weight{nullptr};
        void *_d_gpos{nullptr}, *_d_gvel{nullptr}, *_d_status{nullptr}, *_d_best{nullptr}, *_d_exit{nullptr}, *_d_cmd{nullptr};
    };
}
#endif
