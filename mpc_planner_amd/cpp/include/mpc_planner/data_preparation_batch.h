/*
 * mpc_planner/data_preparation_batch.h -- the batched device twin of mpc_planner/data_preparation.h, next to the batched optimize() path:
 * the raw obstacle lists of several scenes are uploaded ONCE, tmpc_prepare_obstacles turns each into exactly cfg.max_obstacles prepared
 * obstacles (distance filter, closest-M selection or dummies, uncertainty passes) and tmpc_set_obstacle_parameters writes the collision
 * columns of the handle's current batch -- what ensureObstacleSize / propagatePredictionUncertainty and EllipsoidConstraints::setParameters
 * (or GaussianConstraints') do per scene on the host, bit for bit.  obstaclePositions() / obstacleRadii() are then ready for
 * tmpc_linearize_topology_ex (d_obstacle_pos, d_obstacle_radius).  For callers of the C-ABI (include/tmpc_hip.h) that keep a launch of many
 * scenes on the device; needs the HIP runtime header (compile with -D__HIP_PLATFORM_AMD__ and the ROCm include directory).
 * Column mode (setColumns): for a handle of a GENERATED library, whose parameter layout is its module stack's and where the entries above
 * refuse -- the same steps through include/tmpc_hip_stack.h (tmpc_stack_prepare_obstacles, tmpc_stack_set_obstacle_columns), the collision
 * columns named by the caller from the stack's parameter map; linearizeTopology() then writes the topology rows too.
 * Everything is enqueued on the handle's stream; prepare() waits for its own uploads (the staging memory is its own), not for the kernels.
 */
#ifndef MPC_DATA_PREPARATION_BATCH_HIP_H
#define MPC_DATA_PREPARATION_BATCH_HIP_H

#include <mpc_planner/data_preparation.h>
#include <mpc_planner_solver/device_plumbing.h>

#include "tmpc_hip_stack.h"

namespace MPCPlanner
{
    class BatchedObstaclePreparation : private DevicePlumbing
    {
    public:
        /* n_scenes scenes of up to n_slots (<= 1024) raw obstacles each; cfg.max_obstacles prepared obstacles and cfg.N steps per scene */
        BatchedObstaclePreparation(tmpc_handle *handle, int n_scenes, int n_slots, const ModuleConfig &cfg)
            : DevicePlumbing(handle, "BatchedObstaclePreparation"), _Q(n_scenes), _R(n_slots), _M(cfg.max_obstacles), _N(cfg.N), _cfg(cfg)
        {
            const size_t Q = (size_t)_Q, R = (size_t)_R, M = (size_t)_M, N = (size_t)_N;
            alloc(_d_count, Q * sizeof(int)); alloc(_d_state, Q * 4 * 8); alloc(_d_state_x, Q * 8); alloc(_d_pos, Q * R * 2 * 8); alloc(_d_radius, Q * R * 8);
            alloc(_d_vel, Q * R * 2 * 8); alloc(_d_pred, Q * R * N * 5 * 8);
            alloc(_o_pos, Q * M * N * 2 * 8); alloc(_o_shape, Q * M * N * 3 * 8); alloc(_o_radius, Q * M * 8); alloc(_o_gauss, Q * M); alloc(_o_sel, Q * M * sizeof(int));
        }
        ~BatchedObstaclePreparation()
        {
            for (void *p : {_d_count, _d_state, _d_state_x, _d_pos, _d_radius, _d_vel, _d_pred, _o_pos, _o_shape, _o_radius, _o_gauss, _o_sel}) if (p) (void)hipFree(p);
        }
        BatchedObstaclePreparation(const BatchedObstaclePreparation &) = delete;
        BatchedObstaclePreparation &operator=(const BatchedObstaclePreparation &) = delete;

        /* Column mode: the handle is a generated library's.  row_model 0 / 1 = the stack's EllipsoidConstraints / GaussianConstraints module;
         * obstacle_cols = ego_disc_radius, ego_disc_0_offset, then per obstacle j < cfg.max_obstacles ellipsoid_obst_j_{x, y, psi, major, minor,
         * chi, r} or gaussian_obst_j_{x, y, major, minor, risk, r}; topology_cols = lin_constraint_j_{a1, a2, b} per topology row (may be
         * empty: a stack without LinearizedConstraints) -- the column numbers of the stack's parameter map.  From here on prepare(),
         * setParameters() and linearizeTopology() go through include/tmpc_hip_stack.h; the library checks the tables. */
        void setColumns(int row_model, const std::vector<int32_t> &obstacle_cols, const std::vector<int32_t> &topology_cols)
        {
            if (topology_cols.size() % 3) fail("setColumns: topology_cols holds (a1, a2, b) per row");
            _columns = true; _row_model = row_model; _obstacle_cols = obstacle_cols; _topology_cols = topology_cols;
        }

        /* The raw lists of every scene (position, radius; obstacles beyond n_slots are not seen) and the robots' states.
         * velocities != nullptr: constant-velocity mode (ros1_jackal.cpp:324-329), one velocity per obstacle; otherwise the obstacles'
         * own predictions are taken as given (ros1_jackalsimulator.cpp:312-334; an obstacle without one: its position, zero radii).
         * propagate_passes: propagatePredictionUncertainty passes over the GAUSSIAN predictions -- 2 is what getConstantVelocityPrediction
         * plus the wrapper's own call do in probabilistic mode (ros1_jackal.cpp:324-332), 1 the simulator wrapper with cfg.propagate_uncertainty. */
        void prepare(const std::vector<std::vector<DynamicObstacle>> &raw, const std::vector<State> &states,
                     const std::vector<std::vector<Vector2d>> *velocities, int propagate_passes)
        {
            const size_t Q = (size_t)_Q, R = (size_t)_R, N = (size_t)_N;
            if (raw.size() != Q || states.size() != Q || (velocities && velocities->size() != Q)) fail("prepare: one obstacle list, state (and velocity list) per scene");
            std::vector<int> count(Q);
            std::vector<double> state(Q * 4), state_x(Q), pos(Q * R * 2, 0.), radius(Q * R, 0.), aux(velocities ? Q * R * 2 : Q * R * N * 5, 0.);
            for (size_t q = 0; q < Q; q++) {
                count[q] = (int)std::min(raw[q].size(), R);
                state[q * 4] = states[q].get("x"); state[q * 4 + 1] = states[q].get("y"); state[q * 4 + 2] = states[q].get("psi"); state[q * 4 + 3] = states[q].get("v");
                state_x[q] = state[q * 4];
                for (size_t i = 0; i < (size_t)count[q]; i++) {
                    const DynamicObstacle &ob = raw[q][i];
                    pos[(q * R + i) * 2] = ob.position(0); pos[(q * R + i) * 2 + 1] = ob.position(1); radius[q * R + i] = ob.radius;
                    if (velocities) { aux[(q * R + i) * 2] = (*velocities)[q][i](0); aux[(q * R + i) * 2 + 1] = (*velocities)[q][i](1); continue; }
                    for (size_t k = 0; k < N; k++) {
                        double *e = &aux[((q * R + i) * N + k) * 5];
                        if (ob.prediction.empty() || ob.prediction.modes[0].size() <= k) { e[0] = ob.position(0); e[1] = ob.position(1); continue; }
                        const PredictionStep &st = ob.prediction.modes[0][k];
                        e[0] = st.position(0); e[1] = st.position(1); e[2] = st.angle; e[3] = st.major_radius; e[4] = st.minor_radius;
                    }
                }
            }
            void *stream = this->stream();
            copy(_d_count, count.data(), Q * sizeof(int), stream); copy(_d_state, state.data(), Q * 4 * 8, stream); copy(_d_state_x, state_x.data(), Q * 8, stream);
            copy(_d_pos, pos.data(), pos.size() * 8, stream); copy(_d_radius, radius.data(), radius.size() * 8, stream);
            copy(velocities ? _d_vel : _d_pred, aux.data(), aux.size() * 8, stream);
            sync(stream);                                                     // the staging vectors end with this call
            tmpc_obstacle_options opt{};
            opt.size = sizeof(opt); opt.probabilistic = _cfg.probabilistic_enable ? 1 : 0; opt.propagate_passes = propagate_passes; opt.noise = 0.3;
            opt.max_obstacle_distance = _cfg.max_obstacle_distance;
            if ((_columns ? tmpc_stack_prepare_obstacles : tmpc_prepare_obstacles)(_h, _Q, _R, _M, _d_count, _d_state, _d_pos, _d_radius, velocities ? _d_vel : nullptr, velocities ? nullptr : _d_pred, &opt,
                                                                                   _o_pos, _o_shape, _o_radius, _o_gauss, _o_sel)) fail(tmpc_last_error(_h));
        }

        /* The collision columns of the handle's CURRENT batch (tmpc_set_batch* first): scene_of[b] = scene of batch entry b.
         * EllipsoidConstraints / GaussianConstraints::setParameters for every entry, stage and obstacle in one launch. */
        void setParameters(const std::vector<int> &scene_of, double disc_offset = 0.)
        {
            const void *d_scene_of = uploadSceneOf(scene_of);
            const double chi = ExponentialQuantile(0.5, 1.0 - _cfg.risk);                                  // on the host: no device logarithm enters
            if (_columns) {
                if (tmpc_stack_set_obstacle_columns(_h, _obstacle_cols.data(), (int32_t)_obstacle_cols.size(), _row_model, _M, _o_pos, _o_shape, _o_radius, _o_gauss,
                                                    d_scene_of, _d_state, _cfg.robot_radius, disc_offset, _cfg.risk, chi, _cfg.obstacle_radius)) fail(tmpc_last_error(_h));
                return;
            }
            if (tmpc_set_obstacle_parameters(_h, _o_pos, _o_shape, _o_radius, _o_gauss, d_scene_of, _d_state, _cfg.robot_radius, disc_offset, _cfg.risk, chi,
                                             _cfg.obstacle_radius)) fail(tmpc_last_error(_h));
        }

        /* The topology rows of the handle's CURRENT batch from the prepared obstacles (LinearizedConstraints::update + setParameters for every
         * entry and stage in one launch; the warm start is the handle's): every prepared obstacle is a row, guidance mode (radius 1e-3 +
         * robot_radius) or, with use_guidance = false, each obstacle's own radius; d_is_original u8 [B] (device) or nullptr marks the non-guided
         * planners.  Column mode: into topology_cols (tmpc_stack_linearize_topology_columns); otherwise tmpc_linearize_topology_ex. */
        void linearizeTopology(const std::vector<int> &scene_of, const void *d_is_original = nullptr, bool use_guidance = true)
        {
            const void *d_scene_of = uploadSceneOf(scene_of);
            const void *radii = use_guidance ? nullptr : _o_radius;
            const int rc = _columns ? tmpc_stack_linearize_topology_columns(_h, _topology_cols.data(), (int32_t)(_topology_cols.size() / 3), _o_pos, _M, radii, nullptr, 0,
                                                                            d_scene_of, _d_state_x, _cfg.robot_radius, d_is_original)
                                    : tmpc_linearize_topology_ex(_h, _o_pos, _M, radii, nullptr, 0, d_scene_of, _d_state_x, _cfg.robot_radius, d_is_original);
            if (rc) fail(tmpc_last_error(_h));
        }

        /* device buffers, valid after prepare(): what tmpc_linearize_topology_ex reads (d_obstacle_pos [n_scenes][M][N][2], d_obstacle_radius
         * [n_scenes][M]), the rest of the prepared obstacles, and the states (x, y, psi, v) per scene */
        const void *obstaclePositions() const { return _o_pos; }
        const void *obstacleRadii() const { return _o_radius; }
        const void *obstacleShapes() const { return _o_shape; }
        const void *obstacleGaussian() const { return _o_gauss; }
        const void *states() const { return _d_state; }
        /* raw index of every prepared obstacle (-1: dummy), [n_scenes][max_obstacles]; synchronises the handle's stream */
        std::vector<int> selected() const
        {
            std::vector<int> out((size_t)_Q * _M);
            if (tmpc_synchronize(_h)) fail(tmpc_last_error(_h));
            if (hipMemcpy(out.data(), _o_sel, out.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) fail("hipMemcpy");
            return out;
        }

    private:
        int _Q, _R, _M, _N;
        ModuleConfig _cfg;
        bool _columns{false};
        int _row_model{0};
        std::vector<int32_t> _obstacle_cols, _topology_cols;
        void *_d_state_x{nullptr};
        void *_d_count{nullptr}, *_d_state{nullptr}, *_d_pos{nullptr}, *_d_radius{nullptr}, *_d_vel{nullptr}, *_d_pred{nullptr};
        void *_o_pos{nullptr}, *_o_shape{nullptr}, *_o_radius{nullptr}, *_o_gauss{nullptr}, *_o_sel{nullptr};
    };
}
#endif
