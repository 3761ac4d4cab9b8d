// mpc_planner_amd/csrc/tmpc_guidance_search.hpp -- the guidance search on device (include/tmpc_hip_guidance_search.h): a
// visibility-PRM on the stage grid, winding numbers as the homotopy test, one path per class, the n_paths cheapest.  One wave per scene.
//
// The sample loop and the path enumeration are sequential by definition; the width is inside each step, and that is where the 64 lanes go:
//   - the stages x obstacles of a validity test (lane-strided, one __any vote),
//   - the guards of a nearest-visible-guard pass (one guard per lane, a __shfl_xor minimum with the lower index on ties),
//   - the polygon edges of a winding number (lane-strided, a __shfl_xor integer sum per obstacle),
//   - the stages of a polyline expansion and the copies in and out.
// Every reduction is a boolean, an integer sum or a minimum with an index tie-break: the lane order cannot change a bit.  Everything else is
// wave-uniform -- each lane holds the same counters, takes the same branch and stores the same value to the same table entry -- so nothing is
// broadcast.  The scene's obstacle positions by stage, the guard and connector tables, the kept paths, the enumeration's stack and the two
// polylines of a homotopy test live in LDS (tmpc_arith::GsWork, about 42 KB: one scene per CU's worth of LDS is not the bound at one wave per
// block, the 64 KB static limit is); no per-lane array exists, so nothing can go to scratch.  A path is kept as its chain of connector
// indices (at most 31) and its goal's guard, not as nodes: that is what makes the tables fit.
//
// The search itself is tmpc_arith::gs_scene (mpc_planner_types/prep_arithmetic.h), the source the host twin
// mpc_planner_modules/guidance_search.h compiles with one lane; this file is the lane policy and the launch shape.  Bit-equal to the
// independent modules.py::guidance_search.
#pragma once
#include "../cpp/include/mpc_planner_types/prep_arithmetic.h"

namespace tmpc {

// the 64 lanes of a wave as the lane policy of tmpc_arith::gs_scene
struct GsWave64 {
    static constexpr int width = 64;
    __device__ int lane() const { return (int)threadIdx.x; }
    __device__ bool any(bool b) const { return __any(b ? 1 : 0) != 0; }
    __device__ int sum(int v) const
    {
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
        return v;
    }
    // the smallest key among the lanes whose idx >= 0, the lower idx on equal keys; every lane leaves with the winner (idx < 0: none)
    __device__ void argmin(double &key, int &idx) const
    {
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const double ok = __shfl_xor(key, s, 64);
            const int oi = __shfl_xor(idx, s, 64);
            if (oi >= 0 && (idx < 0 || ok < key || (ok == key && oi < idx))) { key = ok; idx = oi; }
        }
    }
    // one wave per block: the barrier orders the lanes' LDS and global accesses either side of it
    __device__ void sync() const { __syncthreads(); }
};

__global__ __launch_bounds__(64) void tmpc_guidance_search_kernel(int N, double dt, int n_goals, int M, tmpc_arith::GsOptions o, const double *state4,
                                                                  const double *goals, const double *obstacle_pos, const double *obstacle_radius,
                                                                  const int *selected, const uint8_t *was_reset, double *prev_traj, int *prev_class,
                                                                  int *prev_count, int *next_class, double *nodes, int *node_count, int *traj_count,
                                                                  int *topology_class, int *status)
{
#pragma clang fp contract(off)
    __shared__ tmpc_arith::GsWork work;
    const GsWave64 wave;
    tmpc_arith::gs_scene(wave, work, (int)blockIdx.x, N, dt, n_goals, M, o, state4, goals, obstacle_pos, obstacle_radius, selected, was_reset, prev_traj,
                         prev_class, prev_count, next_class, nodes, node_count, traj_count, topology_class, status);
}

}   // namespace tmpc
