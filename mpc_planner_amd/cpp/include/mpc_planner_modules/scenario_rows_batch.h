/*
 * mpc_planner_modules/scenario_rows_batch.h -- the scenario rows of SH-MPC for a whole launch, kept on the device, next to
 * mpc_planner_modules/free_space_batch.h: per tick update() enqueues tmpc_sample_scenarios (every parallel solver draws its own scenarios from
 * the obstacles' mixture predictions, scenario_constraints.cpp:121-131), tmpc_scenario_discard (when n_discard > 0) and
 * tmpc_scenario_halfspaces -- the polygon of each stage around the warm start, written into the scenario rows and ego_disc_0_offset of the
 * handle's current batch; after the solve support() enqueues tmpc_scenario_support and tmpc_scenario_empty_stages (ScenarioSolver::support,
 * scenario_constraints.h:38-40).  Column mode (setColumns): for a handle of a GENERATED library, where tmpc_scenario_halfspaces and
 * tmpc_scenario_support refuse -- the same steps through include/tmpc_hip_stack_scenario.h (tmpc_stack_scenario_halfspaces,
 * tmpc_stack_scenario_support), the rows written into the columns of the stack's parameter map; without setColumns() nothing changes.  It does
 * not replace ScenarioConstraints of mpc_planner_modules/modules_hip.h, which builds its rows on the host.  For callers of the C-ABI that keep a
 * launch on the device; needs the HIP runtime header (compile with -D__HIP_PLATFORM_AMD__ and the ROCm include directory).  Everything is
 * enqueued on the handle's stream; update() waits for its own uploads (the staging memory is the caller's), not for the kernels.
 */
#ifndef MPC_SCENARIO_ROWS_BATCH_HIP_H
#define MPC_SCENARIO_ROWS_BATCH_HIP_H

#include <cstdint>

#include <mpc_planner_solver/device_plumbing.h>

#include "tmpc_hip_stack_scenario.h"

namespace MPCPlanner
{
    class BatchedScenarioRows : private DevicePlumbing
    {
    public:
        /* n_solvers parallel solvers (the scenes of the samples: batch entry b reads the scenarios of solver scene_of[b]), n_obstacles obstacles
         * with n_modes prediction modes each, n_scenarios joint draws per solver, of which n_discard (>= 0) are removed; N = the solver's horizon
         * (tmpc_dims::N); n_rows scenario rows per stage (<= 64; <= 42 in column mode); B_max: the largest batch support() is asked about */
        BatchedScenarioRows(tmpc_handle *handle, int n_solvers, int n_obstacles, int n_modes, int n_scenarios, int n_discard, int N, int n_rows, int B_max)
            : DevicePlumbing(handle, "BatchedScenarioRows"), _Q(n_solvers), _M(n_obstacles), _modes(n_modes), _S(n_scenarios), _n_discard(n_discard), _N(N),
              _n_rows(n_rows), _B_max(B_max)
        {
            const size_t Q = (size_t)_Q;
            alloc(_d_pred, Q * _M * _modes * _N * 6 * 8); alloc(_d_prob, Q * _M * _modes * 8); alloc(_d_samples, Q * _N * (size_t)_M * _S * 2 * 8);
            alloc(_d_state_x, Q * 8); alloc(_d_support, (size_t)_B_max * sizeof(int)); alloc(_d_active, (size_t)_B_max * sizeof(int));
            alloc(_d_empty, (size_t)_B_max * sizeof(int));
        }
        ~BatchedScenarioRows()
        {
            for (void *p : {_d_pred, _d_prob, _d_samples, _d_state_x, _d_support, _d_active, _d_empty}) if (p) (void)hipFree(p);
        }
        BatchedScenarioRows(const BatchedScenarioRows &) = delete;
        BatchedScenarioRows &operator=(const BatchedScenarioRows &) = delete;

        /* Column mode, for a handle of a GENERATED library: scenario_cols = ego_disc_0_offset, then disc_0_scenario_constraint_{r}_{a1, a2, b} for
         * r = 0 .. n_rows - 1, the columns of the stack's parameter map (parameter_map.yaml).  From then on update() and support() use
         * tmpc_stack_scenario_halfspaces and tmpc_stack_scenario_support. */
        void setColumns(const std::vector<int32_t> &scenario_cols, int n_rows)
        {
            if (n_rows != _n_rows || (int)scenario_cols.size() != 1 + 3 * _n_rows) fail("setColumns: 1 + 3 n_rows columns");
            _columns = true; _cols = scenario_cols;
        }

        /* One tick for the handle's CURRENT batch (tmpc_set_batch* or tmpc_warmstart first: the polygons are built around its warm start).  pred
         * f64 [n_solvers][n_obstacles][n_modes][N][6] and prob f64 [n_solvers][n_obstacles][n_modes] as tmpc_sample_scenarios takes them,
         * state_x f64 [n_solvers] (the dummy rows lie at state_x + 100), scene_of[b] = solver of batch entry b: host memory.  sample -> discard ->
         * halfspaces, enqueued; nothing is read back. */
        void update(const std::vector<double> &pred, const std::vector<double> &prob, const std::vector<double> &state_x, const std::vector<int> &scene_of,
                    uint64_t seed, double radius, double disc_offset = 0.)
        {
            const size_t Q = (size_t)_Q;
            if (pred.size() != Q * _M * _modes * _N * 6 || prob.size() != Q * _M * _modes || state_x.size() != Q) fail("update: pred, prob or state_x of the wrong size");
            void *stream = this->stream();
            copy(_d_pred, pred.data(), pred.size() * 8, stream); copy(_d_prob, prob.data(), prob.size() * 8, stream);
            copy(_d_state_x, state_x.data(), state_x.size() * 8, stream);
            sync(stream);
            const void *d_scene_of = uploadSceneOf(scene_of);
            const int n_pts = _M * _S;
            if (tmpc_sample_scenarios(_h, _d_pred, _d_prob, _Q, _M, _modes, _S, seed, _d_samples)) fail(tmpc_last_error(_h));
            if (_n_discard > 0 && tmpc_scenario_discard(_h, _d_samples, n_pts, _S, _n_discard, d_scene_of, radius)) fail(tmpc_last_error(_h));
            const int rc = _columns ? tmpc_stack_scenario_halfspaces(_h, _cols.data(), _n_rows, _d_samples, n_pts, d_scene_of, _d_state_x, radius, disc_offset)
                                    : tmpc_scenario_halfspaces(_h, _d_samples, n_pts, _n_rows, d_scene_of, _d_state_x, radius, disc_offset);
            if (rc) fail(tmpc_last_error(_h));
        }

        /* After the solve: support and active rows of every entry's solution (tol: a row is active when it is violated or closer than tol) and the
         * stages whose polygon was empty.  Enqueued; read supports() / activeRows() / emptyStages() after a synchronisation of the handle. */
        void support(double tol)
        {
            const int rc = _columns ? tmpc_stack_scenario_support(_h, _cols.data(), _n_rows, _S, tol, _d_support, _d_active)
                                    : tmpc_scenario_support(_h, _S, tol, _d_support, _d_active);
            if (rc) fail(tmpc_last_error(_h));
            if (tmpc_scenario_empty_stages(_h, _d_empty)) fail(tmpc_last_error(_h));
        }

        /* device buffers: samples f64 [n_solvers][N][n_obstacles * n_scenarios][2] (valid after update()); i32 [B] each, valid after support() */
        const void *samples() const { return _d_samples; }
        const void *supports() const { return _d_support; }
        const void *activeRows() const { return _d_active; }
        const void *emptyStages() const { return _d_empty; }

    private:
        int _Q, _M, _modes, _S, _n_discard, _N, _n_rows, _B_max;
        bool _columns{false};
        std::vector<int32_t> _cols;
        void *_d_pred{nullptr}, *_d_prob{nullptr}, *_d_samples{nullptr}, *_d_state_x{nullptr};
        void *_d_support{nullptr}, *_d_active{nullptr}, *_d_empty{nullptr};
    };
}
#endif
