// mpc_planner_amd/csrc/tmpc_handle_layout.hpp -- where the inputs and outputs of a solve live inside a handle (csrc/tmpc_capi.hip).  Plain C++, no HIP:
// tests/cpp/test_handle_layout.cpp compiles it on the host alone.
// Every handle holds ONE device allocation for its owned inputs (+ the slot map) and ONE for its outputs; each array of B_max trajectories is a region at a
// 256-byte-aligned offset, in the order of the enums below.  A TICK-SIZE handle (both allocations at most IO_TICK_MAX bytes: a control tick's handle)
// mirrors both in pinned host memory with the same layout.  This table is the only place that knows an array's bytes per trajectory.
#pragma once
#include <cstddef>

namespace tmpc {
enum IoIn { IN_XINIT, IN_X0, IN_PARAMS, IN_SLOT, IN_COUNT };           // IN_XINIT .. IN_PARAMS: the batch (tmpc_set_batch); IN_SLOT: tmpc_set_slots
enum IoOut { OUT_XTRAJ, OUT_UTRAJ, OUT_POBJ, OUT_RES_EQ, OUT_EXIT_CODE, OUT_QP_STATUS, OUT_SQP_ITER, OUT_QP_ITER, OUT_COUNT };
constexpr size_t IO_BATCH_ARRAYS = IN_SLOT;        // the input regions one tmpc_set_batch writes
constexpr size_t IO_NU = 2;                        // controls per stage (tmpc::NU)
constexpr size_t IO_TICK_MAX = 2u << 20;

struct IoRegion {
    size_t per_traj = 0;        // bytes of one trajectory
    size_t offset = 0;          // of the region of B_max trajectories inside its allocation: a multiple of 256
    size_t bytes(size_t B) const { return B * per_traj; }
    size_t doubles() const { return per_traj / sizeof(double); }      // of one trajectory, for the f64 arrays (the kernels' strides)
};
struct IoLayout {
    IoRegion in[IN_COUNT], out[OUT_COUNT];
    size_t in_total = 0, out_total = 0;     // bytes of the two allocations
    bool tick = false;                      // tick-size: pinned mirrors exist
    // bytes of the batch arrays' first B trajectories (what one tmpc_set_batch moves)
    size_t batch_bytes(size_t B) const { size_t n = 0; for (size_t i = 0; i < IO_BATCH_ARRAYS; i++) n += in[i].bytes(B); return n; }
};

inline IoLayout io_layout(size_t N, size_t ext_nx, size_t ext_nv, size_t npar, size_t B_max)
{
    IoLayout l;
    const size_t in_per[IN_COUNT] = {ext_nx * 8, (N + 1) * ext_nv * 8, N * npar * 8, 4};
    const size_t out_per[OUT_COUNT] = {(N + 1) * ext_nx * 8, N * IO_NU * 8, 8, 8, 4, 4, 4, 4};
    auto place = [B_max](IoRegion *r, const size_t *per, int n) {
        size_t off = 0;
        for (int i = 0; i < n; i++) { r[i].per_traj = per[i]; r[i].offset = off; off += (r[i].bytes(B_max) + 255) & ~(size_t)255; }
        return off;
    };
    l.in_total = place(l.in, in_per, IN_COUNT);
    l.out_total = place(l.out, out_per, OUT_COUNT);
    l.tick = l.in_total <= IO_TICK_MAX && l.out_total <= IO_TICK_MAX;
    return l;
}
}  // namespace tmpc
