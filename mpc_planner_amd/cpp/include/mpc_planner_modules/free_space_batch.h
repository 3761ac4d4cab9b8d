/*
 * mpc_planner_modules/free_space_batch.h -- the batched device twin of mpc_planner_modules/free_space.h, next to
 * mpc_planner_modules/reference_path_batch.h: the costmaps of several scenes (one size, one resolution) are uploaded with setCostmaps(); per
 * tick update() enqueues tmpc_costmap_points when a map has changed since the last tick, then tmpc_decomp_halfspaces -- the polyline on the
 * whole paths along the warm start of each scene's main solver, one polygon per segment -- and setParameters() enqueues
 * tmpc_set_halfspace_rows, which writes the decomp rows and ego_disc_0_offset of the handle's current batch: what DecompConstraints::update /
 * setParameters do per scene on the host (decomp_constraints.cpp:52-189), bit for bit.  The paths are device buffers in
 * tmpc_fit_path's layout, e.g. BatchedPathTracking::paths() / pathCounts() / pathLengths(), and s0 its closestS().  Column mode (setColumns):
 * for a handle of a GENERATED library, where those two entries refuse -- the same steps through include/tmpc_hip_stack_env.h
 * (tmpc_stack_decomp_halfspaces, tmpc_stack_set_halfspace_columns), the rows written into the columns of the stack's parameter map; without
 * setColumns() nothing changes.  For callers of the C-ABI
 * (include/tmpc_hip.h) that keep a launch of many scenes on the device; needs the HIP runtime header (compile with -D__HIP_PLATFORM_AMD__
 * and the ROCm include directory).  Everything is enqueued on the handle's stream; setCostmaps() and setParameters() wait for their own
 * uploads (the staging memory is their own), not for the kernels.
 */
#ifndef MPC_FREE_SPACE_BATCH_HIP_H
#define MPC_FREE_SPACE_BATCH_HIP_H

#include <mpc_planner_modules/free_space.h>
#include <mpc_planner_solver/device_plumbing.h>
#include <mpc_planner_types/costmap.h>

#include "tmpc_hip_stack_env.h"

namespace MPCPlanner
{
    class BatchedFreeSpace : private DevicePlumbing
    {
    public:
        /* n_scenes maps of size_x x size_y cells (at most 2^20); up to n_pts_max (<= 16384) occupied cells per scene are kept; N = the solver's
         * horizon (tmpc_dims::N); range = decomp/range, n_rows = decomp/max_constraints (<= 64) */
        BatchedFreeSpace(tmpc_handle *handle, int n_scenes, int size_x, int size_y, int n_pts_max, int N, double range, int n_rows)
            : DevicePlumbing(handle, "BatchedFreeSpace"), _Q(n_scenes), _size_x(size_x), _size_y(size_y), _P(n_pts_max), _N(N), _n_rows(n_rows), _range(range)
        {
            const size_t Q = (size_t)_Q;
            alloc(_d_cost, Q * size_x * size_y); alloc(_d_origin, Q * 2 * 8); alloc(_d_points, Q * (size_t)_P * 2 * 8); alloc(_d_count, Q * sizeof(int));
            alloc(_d_overflow, Q); alloc(_d_rows, Q * (size_t)_N * _n_rows * 3 * 8); alloc(_d_row_count, Q * (size_t)_N * sizeof(int)); alloc(_d_status, Q * (size_t)_N);
        }
        ~BatchedFreeSpace()
        {
            for (void *p : {_d_cost, _d_origin, _d_points, _d_count, _d_overflow, _d_rows, _d_row_count, _d_status}) if (p) (void)hipFree(p);
        }
        BatchedFreeSpace(const BatchedFreeSpace &) = delete;
        BatchedFreeSpace &operator=(const BatchedFreeSpace &) = delete;

        /* New maps for every scene: one upload; the next update() extracts the occupied cells again.  Every map has the twin's size; they
         * share one resolution (the first map's). */
        void setCostmaps(const std::vector<const costmap_2d::Costmap2D *> &maps)
        {
            const size_t Q = (size_t)_Q, cells = (size_t)_size_x * _size_y;
            if (maps.size() != Q) fail("setCostmaps: one costmap per scene");
            std::vector<unsigned char> cost(Q * cells);
            std::vector<double> origin(Q * 2);
            for (size_t q = 0; q < Q; q++) {
                const costmap_2d::Costmap2D &m = *maps[q];
                if ((int)m.getSizeInCellsX() != _size_x || (int)m.getSizeInCellsY() != _size_y || m.getResolution() != maps[0]->getResolution()) fail("setCostmaps: one size and one resolution");
                for (int my = 0; my < _size_y; my++) for (int mx = 0; mx < _size_x; mx++) cost[q * cells + (size_t)my * _size_x + mx] = m.getCost(mx, my);
                origin[q * 2] = m.getOriginX(); origin[q * 2 + 1] = m.getOriginY();
            }
            _resolution = maps[0]->getResolution();
            void *stream = this->stream();
            copy(_d_cost, cost.data(), cost.size(), stream); copy(_d_origin, origin.data(), origin.size() * 8, stream);
            sync(stream);                                                     // the staging vectors end with this call
            _map_changed = true;
        }

        /* Column mode, for a handle of a GENERATED library: decomp_cols = ego_disc_0_offset, then disc_0_decomp_{r}_{a1, a2, b} for r = 0 .. n_rows - 1,
         * the columns of the stack's parameter map (parameter_map.yaml).  From then on update() and setParameters() use
         * tmpc_stack_decomp_halfspaces and tmpc_stack_set_halfspace_columns. */
        void setColumns(const std::vector<int32_t> &decomp_cols)
        {
            if ((int)decomp_cols.size() != 1 + 3 * _n_rows) fail("setColumns: 1 + 3 n_rows columns");
            _columns = true; _decomp_cols = decomp_cols;
        }

        /* One tick of DecompConstraints::update for every scene of the handle's CURRENT batch (tmpc_set_batch* first: the speeds are read from
         * its warm start).  d_main_of i32 [n_scenes]: the batch entry of each scene's main solver; d_path / d_path_count / d_path_length: the
         * whole paths, rows n_seg_max apart; d_s0, d_state_x f64 [n_scenes].  All device pointers.  Enqueued; nothing is read back. */
        void update(const void *d_main_of, int n_seg_max, const void *d_path, const void *d_path_count, const void *d_path_length, const void *d_s0,
                    const void *d_state_x)
        {
            if (_map_changed) {
                if (tmpc_costmap_points(_h, _Q, _size_x, _size_y, _d_cost, _d_origin, _resolution, _P, _d_points, _d_count, _d_overflow)) fail(tmpc_last_error(_h));
                _map_changed = false;
            }
            if ((_columns ? tmpc_stack_decomp_halfspaces : tmpc_decomp_halfspaces)(_h, d_main_of, _Q, n_seg_max, d_path, d_path_count, d_path_length, d_s0, d_state_x, _d_points,
                                                                                   _d_count, _P, _range, _n_rows, _d_rows, _d_row_count, _d_status)) fail(tmpc_last_error(_h));
        }

        /* The decomp rows (slack rows first_row .. first_row + n_rows - 1) and ego_disc_0_offset of the handle's current batch: scene_of[b] =
         * scene of batch entry b, outside [0, n_scenes): the entry is left alone.  Column mode: into decomp_cols, which name the rows (first_row is
         * not used and must be 0). */
        void setParameters(const std::vector<int> &scene_of, double disc_offset = 0., int first_row = 0)
        {
            if (_columns && first_row != 0) fail("setParameters: the columns name the rows (first_row = 0)");
            const void *d_scene_of = uploadSceneOf(scene_of);
            const int rc = _columns ? tmpc_stack_set_halfspace_columns(_h, _decomp_cols.data(), _n_rows, _d_rows, d_scene_of, _Q, disc_offset)
                                    : tmpc_set_halfspace_rows(_h, _d_rows, _n_rows, first_row, d_scene_of, _Q, disc_offset);
            if (rc) fail(tmpc_last_error(_h));
        }

        /* device buffers, valid after update(): points [n_scenes][n_pts_max][2], their count (i32) and overflow flag (u8) per scene, the rows
         * [n_scenes][N][n_rows][3], rows that are not dummies (i32) and FreeSpace::Status (u8) [n_scenes][N] */
        const void *points() const { return _d_points; }
        const void *pointCounts() const { return _d_count; }
        const void *overflow() const { return _d_overflow; }
        const void *rows() const { return _d_rows; }
        const void *rowCounts() const { return _d_row_count; }
        const void *status() const { return _d_status; }

    private:
        int _Q, _size_x, _size_y, _P, _N, _n_rows;
        double _range, _resolution{0.};
        bool _map_changed{false};
        bool _columns{false};
        std::vector<int32_t> _decomp_cols;
        void *_d_cost{nullptr}, *_d_origin{nullptr}, *_d_points{nullptr}, *_d_count{nullptr}, *_d_overflow{nullptr};
        void *_d_rows{nullptr}, *_d_row_count{nullptr}, *_d_status{nullptr};
    };
}
#endif
