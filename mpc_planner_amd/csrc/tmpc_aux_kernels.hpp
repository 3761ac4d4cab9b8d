// Kernels either side of the solve: FindBestPlanner and the multi-GPU records, the "next" rows f-1 (topology
// linearisation), f-2 (cross-tick warm start), f-3 (scenario -> halfspace reduction) and the stage-function debug kernel.
// Included by tmpc_solve.hip after the stage functions (tmpc_stage.hpp).
#pragma once
#include "../cpp/include/mpc_planner_types/prep_arithmetic.h"      // the data-preparation arithmetic, shared with the C++ headers

namespace tmpc {

// ---- FindBestPlanner on device (guidance_constraints.cpp:416-434) ---------------------------------
__global__ void tmpc_select_best_kernel(int first, int count, const double *pobj, const int *exit_code,
                                        const double *weight, const uint8_t *disabled, int *best_out)
{
    __shared__ double s_val[256];
    __shared__ int s_idx[256];
    double best = 1e10; int idx = -1;
    for (int i = threadIdx.x; i < count; i += blockDim.x) {
        const int g = first + i;
        if (disabled && disabled[i]) continue;
        if (exit_code[g] != 1) continue;
        const double o = weight ? pobj[g] * weight[i] : pobj[g];
        if (o < best) { best = o; idx = i; }       // ascending i per thread: strict '<' keeps the lowest index
    }
    s_val[threadIdx.x] = best; s_idx[threadIdx.x] = idx;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const double ov = s_val[threadIdx.x + s]; const int oi = s_idx[threadIdx.x + s];
            const double mv = s_val[threadIdx.x]; const int mi = s_idx[threadIdx.x];
            const bool take = (oi >= 0) && (mi < 0 || ov < mv || (ov == mv && oi < mi));
            if (take) { s_val[threadIdx.x] = ov; s_idx[threadIdx.x] = oi; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *best_out = s_idx[0];
}

// ---- multi-GPU records ------------------------------------------------------------
__global__ void tmpc_pack_records_kernel(int B, const double *pobj, const int *exit_code, const int *gid,
                                         const double *weight, tmpc_record *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    tmpc_record r;
    r.objective = weight ? pobj[i] * weight[i] : pobj[i];
    r.exit_code = exit_code[i];
    r.guidance_id = gid ? gid[i] : i;
    out[i] = r;
}

// one workgroup (64 lanes) per scene; records [n_ranks][n_scenes][per_rank]
__global__ void tmpc_select_best_records_kernel(const tmpc_record *rec, int n_ranks, int n_scenes, int per_rank, int *best_out)
{
    const int s = blockIdx.x;
    double best = 1e10; int idx = -1;
    const int total = n_ranks * per_rank;
    for (int g = threadIdx.x; g < total; g += 64) {           // ascending global index per lane
        const int rk = g / per_rank, t = g - rk * per_rank;
        const tmpc_record r = rec[((size_t)rk * n_scenes + s) * per_rank + t];
        if (r.exit_code == 1 && r.objective < best) { best = r.objective; idx = g; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double ov = __shfl_xor(best, o, 64); const int oi = __shfl_xor(idx, o, 64);
        const bool take = (oi >= 0) && (idx < 0 || ov < best || (ov == best && oi < idx));
        if (take) { best = ov; idx = oi; }
    }
    if (threadIdx.x == 0) best_out[s] = idx;
}

// the winners' trajectories, one workgroup per set (guidance_constraints.cpp:382-384 for every set of the launch)
__global__ void tmpc_gather_best_kernel(const int *best, int set_size, int index_offset, int nx_doubles, int nu_doubles, const double *xtraj,
                                        const double *utraj, double *out_x, double *out_u)
{
    const int s = blockIdx.x;
    const int g = best[s], loc = g - index_offset;
    if (g >= 0 && (loc < 0 || loc >= set_size)) return;                 // another rank's winner
    const size_t b = (size_t)s * set_size + (g >= 0 ? loc : 0);
    const double nan = __builtin_nan("");
    for (int e = threadIdx.x; e < nx_doubles; e += blockDim.x) out_x[(size_t)s * nx_doubles + e] = g >= 0 ? xtraj[b * nx_doubles + e] : nan;
    for (int e = threadIdx.x; e < nu_doubles; e += blockDim.x) out_u[(size_t)s * nu_doubles + e] = g >= 0 ? utraj[b * nu_doubles + e] : nan;
}

// ---- where a row writer puts its values.  The topology and the collision writers below are templates on it: the arithmetic is one source, the
// destination is either the hand-written parameter layout (the problem's own counts, the ip_* offsets of tmpc_stage.hpp) or a column table the
// caller read from a generated stack's parameter map (include/tmpc_hip_stack.h).  The table travels by value in the kernel arguments, like
// tmpc_scatter_parameters' (at most 128 entries: 516 bytes).
constexpr int SCATTER_MAX_COLS = 128;
struct ScatterCols { int n; int col[SCATTER_MAX_COLS]; };

struct LayoutRows {
    __device__ __forceinline__ int n_lin(const Dims &d) const { return d.n_lin; }
    __device__ __forceinline__ int n_obstacles(const Dims &d) const { return d.M; }
    __device__ __forceinline__ int row_model(const Dims &d) const { return d.row_model; }
    __device__ __forceinline__ int lin(const Dims &d, int j, int w) const { return ip_lin(d, j, w); }
    __device__ __forceinline__ int disc_radius(const Dims &d) const { return ip_disc_radius(d); }
    __device__ __forceinline__ int disc_offset(const Dims &d) const { return ip_disc_offset(d); }
    __device__ __forceinline__ int ellipsoid(const Dims &d, int j, int w) const { return ip_ellipsoid(d, j, w); }
    __device__ __forceinline__ int gauss(const Dims &d, int j, int w) const { return ip_gauss(d, j, w); }
};
// topology: col[3 j + w] = (a1, a2, b) of row j < count.  Collision: col[0] = ego_disc_radius, col[1] = ego_disc_0_offset, then per obstacle
// j < count the module's fields, 7 (model 0: x, y, psi, major, minor, chi, r) or 6 (model 1: x, y, major, minor, risk, r) apart.
struct ColumnRows {
    ScatterCols t;
    int count, model;
    __device__ __forceinline__ int n_lin(const Dims &) const { return count; }
    __device__ __forceinline__ int n_obstacles(const Dims &) const { return count; }
    __device__ __forceinline__ int row_model(const Dims &) const { return model; }
    __device__ __forceinline__ int lin(const Dims &, int j, int w) const { return t.col[3 * j + w]; }
    __device__ __forceinline__ int disc_radius(const Dims &) const { return t.col[0]; }
    __device__ __forceinline__ int disc_offset(const Dims &) const { return t.col[1]; }
    __device__ __forceinline__ int ellipsoid(const Dims &, int j, int w) const { return t.col[2 + 7 * j + w]; }
    __device__ __forceinline__ int gauss(const Dims &, int j, int w) const { return t.col[2 + 6 * j + w]; }
};

// The sibling pair for the static environment (include/tmpc_hip_stack_env.h): the path window and the slack (decomp) rows.  The layout side
// carries the first slack row of the call; the column side names every row, so it has none.
struct LayoutEnvRows {
    int first_row;
    __device__ __forceinline__ int n_segments(const Dims &d) const { return d.S; }
    __device__ __forceinline__ int spline(const Dims &d, int i, int c) const { return ip_spline(d, i, c); }
    __device__ __forceinline__ int slk(const Dims &d, int r, int c) const { return ip_slk(d, first_row + r, c); }
    __device__ __forceinline__ int disc_offset(const Dims &d) const { return ip_disc_offset(d); }
    // the centreline rows of segment i: its eight coefficients (ax bx cx dx ay by cy dy) are contiguous in the layout
    __device__ __forceinline__ void centreline_rows(const Dims &d, const double *p, int i, double t, double off_first, double off_second, double *row) const
    {
        tmpc_arith::road_rows_centreline(p + ip_spline(d, i, 0), t, off_first, off_second, row);
    }
};
// path: col[9 i + c] = spline_x{i}_{a,b,c,d}, spline_y{i}_{a,b,c,d}, spline{i}_start of segment i < count.  Halfspace rows: col[0] =
// ego_disc_0_offset, col[1 + 3 r + c] = (a1, a2, b) of row r < count.
struct ColumnEnvRows {
    ScatterCols t;
    int count;
    __device__ __forceinline__ int n_segments(const Dims &) const { return count; }
    __device__ __forceinline__ int spline(const Dims &, int i, int c) const { return t.col[9 * i + c]; }
    __device__ __forceinline__ int slk(const Dims &, int r, int c) const { return t.col[1 + 3 * r + c]; }
    __device__ __forceinline__ int disc_offset(const Dims &) const { return t.col[0]; }
    // the columns need not be contiguous: gathered into a local array in the layout's order, then the same call
    __device__ __forceinline__ void centreline_rows(const Dims &, const double *p, int i, double s, double off_first, double off_second, double *row) const
    {
        double local[8];
#pragma unroll
        for (int c = 0; c < 8; c++) local[c] = p[t.col[9 * i + c]];
        tmpc_arith::road_rows_centreline(local, s, off_first, off_second, row);
    }
};

// ---- f-1: LinearizedConstraints::update + setParameters on device (linearized_constraints.cpp:49-189) ----------
// one thread per (trajectory, stage)
// n_obs dynamic obstacles (rows 0 .. n_obs-1), then n_static static halfspaces per stage copied as they are (linearized_constraints.cpp:
// 107-123, `add_halfspaces`), then dummies up to n_lin.  obst_radius == nullptr: guidance mode, every disc has radius 1e-3 + robot_radius
// (:99, :140); otherwise the `_use_guidance == false` branch (:63-73): obstacle j's own radius + robot_radius, in the projection and in b.
template <class Where>
__device__ __forceinline__ void linearize_topology_rows(const Where &where, const Dims &d, int B, const double *x0, double *params, const double *obst,
                                                        const int *scene_of, const double *state_x, double robot_radius,
                                                        const uint8_t *is_original, int n_obs, const double *obst_radius, const double *stat, int n_static)
{
#pragma clang fp contract(off)                                          // the rows too are the mirror's (modules.py::linearized_update) bit for bit: a batch whose rows
                                                                        // were built here solves exactly like the same batch built on the host (tests/test_gpu_obstacles.py)
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = d.N;
    if (e >= B * N) return;
    const int b = e / N, k = e - b * N;
    const int sc = scene_of[b];
    double *p = params + ((size_t)b * N + k) * d.npar;
    const double dummy_b = state_x[sc] + 100.0;                         // _dummy_b (:54)
    const bool dummy = k == 0;
    // the non-guided T-MPC++ planner is updated with empty_data_ (guidance_constraints.cpp:301-305): ZERO obstacles, so its static halfspaces
    // sit in rows 0 .. n_static-1 (:113-124, :173-179) and everything behind them is a dummy; without static halfspaces: dummies only
    if (is_original && is_original[b]) n_obs = 0;
    auto radius_of = [&](int j) { return (obst_radius ? obst_radius[(size_t)sc * n_obs + j] : 1e-3) + robot_radius; };   // (:99, :140)
    double px = x0[((size_t)b * (N + 1) + k) * ext_nv(d) + ZX], py = x0[((size_t)b * (N + 1) + k) * ext_nv(d) + ZY];
    const double *ob = obst + (size_t)sc * n_obs * N * 2;
    if (!dummy && n_obs > 0) {
        // projectToSafety (:130-148): at most 3 sweeps over the obstacles of ros_tools' Douglas-Rachford step with obstacle 0 as the
        // anchor.  ros_tools is not in the reference tree; restated from the published operator p <- (p + R_delta R_anchor p) / 2,
        // R = 2 P - I, P = nearest point outside the disc of radius r, applied when p is inside the obstacle's disc (same arithmetic
        // as modules.py::project_to_safety and the C++ DouglasRachford).  No FMA contraction: bit-equal to the host mirrors.
        const double ax0 = ob[(size_t)(k - 1) * 2], ay0 = ob[(size_t)(k - 1) * 2 + 1];          // anchor = obstacle 0 at step k-1
        auto outside = [&](double qx, double qy, double cx, double cy, double r, double &ox_, double &oy_) {
            const double dx = qx - cx, dy = qy - cy;
            const double dist = sqrt(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
            if (dist >= r) { ox_ = qx; oy_ = qy; }
            else if (dist > 1e-12) { const double s = r / dist; ox_ = __dadd_rn(cx, __dmul_rn(dx, s)); oy_ = __dadd_rn(cy, __dmul_rn(dy, s)); }
            else { ox_ = cx; oy_ = cy + r; }
        };
        for (int sweep = 0; sweep < 3; sweep++)
            for (int j = 0; j < n_obs; j++) {
                const double ox = ob[((size_t)j * N + (k - 1)) * 2], oy = ob[((size_t)j * N + (k - 1)) * 2 + 1];
                const double dx = px - ox, dy = py - oy;
                const double r = radius_of(j);
                if (sqrt(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy))) < r) {
                    double qx, qy, bx, by;
                    outside(px, py, ax0, ay0, r, qx, qy);
                    const double rx = __dmul_rn(2.0, qx) - px, ry = __dmul_rn(2.0, qy) - py;
                    outside(rx, ry, ox, oy, r, bx, by);
                    const double sx = __dmul_rn(2.0, bx) - rx, sy = __dmul_rn(2.0, by) - ry;
                    px = (px + sx) / 2.0; py = (py + sy) / 2.0;
                }
            }
    }
    const int n_rows = where.n_lin(d);
    for (int j = 0; j < n_rows; j++) {
        double a1 = 1.0, a2 = 0.0, bb = dummy_b;                        // _dummy_a1, _dummy_a2
        if (!dummy && j < n_obs) {
            const double ox = ob[((size_t)j * N + (k - 1)) * 2], oy = ob[((size_t)j * N + (k - 1)) * 2 + 1];
            const double dx = ox - px, dy = oy - py;
            const double dist = sqrt(dx * dx + dy * dy);
            a1 = dx / dist; a2 = dy / dist;
            bb = a1 * ox + a2 * oy - radius_of(j);
        } else if (!dummy && stat && j < n_obs + n_static) {            // static halfspaces of the stage, as given (:107-123)
            const double *hs = stat + (((size_t)sc * N + k) * n_static + (j - n_obs)) * 3;
            a1 = hs[0]; a2 = hs[1]; bb = hs[2];
        }
        p[where.lin(d, j, 0)] = a1; p[where.lin(d, j, 1)] = a2; p[where.lin(d, j, 2)] = bb;
    }
}
__global__ void tmpc_linearize_topology_kernel(Dims d, int B, const double *x0, double *params, const double *obst,
                                               const int *scene_of, const double *state_x, double robot_radius,
                                               const uint8_t *is_original, int n_obs, const double *obst_radius, const double *stat, int n_static)
{
    linearize_topology_rows(LayoutRows{}, d, B, x0, params, obst, scene_of, state_x, robot_radius, is_original, n_obs, obst_radius, stat, n_static);
}
// the same rows into the caller's columns (tmpc_stack_linearize_topology_columns): where.count rows, where.t.col[3 j + w]
__global__ void tmpc_linearize_topology_columns_kernel(Dims d, int B, const double *x0, double *params, const double *obst,
                                                       const int *scene_of, const double *state_x, double robot_radius,
                                                       const uint8_t *is_original, int n_obs, const double *obst_radius, const double *stat, int n_static,
                                                       ColumnRows where)
{
    linearize_topology_rows(where, d, B, x0, params, obst, scene_of, state_x, robot_radius, is_original, n_obs, obst_radius, stat, n_static);
}

// ---- a5 / f-1: Contouring's road constraints on device (contouring.cpp:181-262, `contouring/add_road_constraints`) ----------------
// one thread per (scene, stage).  For stage k = 1 .. N-1 of scene q (stage 0 gets nothing, :204, :247) with b = main_of[q] the batch entry
// that stands for the scene's MAIN solver, s_k = its warm start's spline state (`_solver->getEgoPrediction(k, "spline")`, :208, :250) and the
// path window of its parameter row of stage k (spline_x{i}_{a..d}, spline_y{i}_{a..d}, spline{i}_start):
//   centreline mode (bounds == nullptr; :191-235): tmpc_arith::road_rows_centreline of the path at s_k; off_first = times half - r, off_second = half - r
//   bounds mode (:237-262): road_row_left_bound / road_row_right_bound of the left / right bound spline at the same s_k -- bounds
//       [n_scenes][2][S][8] = (ax bx cx dx ay by cy dy), on the centreline's knots (:142-149) --, off_first = off_second = r.
// The rows are tmpc_arith's (prep_arithmetic.h: the assumptions of DESIGN.md U12 too), the source Contouring compiles as well: bit-equal to the
// independent modules.py::road_halfspaces(_from_bounds).  The cubic is that of segment i = max{j : start_j <= s} (0 below the first knot; the
// last segment's cubic continues beyond the window).
// Rows first_row, first_row + 1 of stat [n_scenes][N][n_static][3] -- what tmpc_linearize_topology_kernel copies -- and nothing else.
// Where: the path window is read at the layout's ip_spline (LayoutEnvRows) or at the caller's columns (ColumnEnvRows, where.count segments;
// the eight coefficients are gathered into a local array in the layout's order before the same tmpc_arith call).
template <class Where>
__device__ __forceinline__ void road_halfspace_rows(const Where &where, const Dims &d, int B, int n_scenes, const double *x0, const double *params,
                                                    const int *main_of, const double *bounds, double off_first, double off_second, double *stat,
                                                    int n_static, int first_row)
{
#pragma clang fp contract(off)
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = d.N, S = where.n_segments(d);
    if (e >= n_scenes * N) return;
    const int sc = e / N, k = e - sc * N;
    const int b = main_of[sc];
    if (k == 0 || b < 0 || b >= B) return;                              // (an entry outside the batch: nothing is read, nothing written)
    const double *p = params + ((size_t)b * N + k) * d.npar;
    const double s = x0[((size_t)b * (N + 1) + k) * ext_nv(d) + ZS];
    int i = 0;
    for (int j = 0; j < S; j++) if (p[where.spline(d, j, 8)] <= s) i = j;   // (a comparison, nothing is rounded: the kernel's own)
    const double t = s - p[where.spline(d, i, 8)];
    double *row = stat + (((size_t)sc * N + k) * n_static + first_row) * 3;
    if (bounds == nullptr) where.centreline_rows(d, p, i, t, off_first, off_second, row);
    else {
        const double *bl = bounds + (((size_t)sc * 2 + 0) * S + i) * 8, *br = bounds + (((size_t)sc * 2 + 1) * S + i) * 8;
        tmpc_arith::road_row_left_bound(bl, t, off_first, row);
        tmpc_arith::road_row_right_bound(br, t, off_second, row + 3);
    }
}
__global__ void tmpc_road_halfspaces_kernel(Dims d, int B, int n_scenes, const double *x0, const double *params, const int *main_of,
                                            const double *bounds, double off_first, double off_second, double *stat, int n_static, int first_row)
{
    road_halfspace_rows(LayoutEnvRows{0}, d, B, n_scenes, x0, params, main_of, bounds, off_first, off_second, stat, n_static, first_row);
}
// the same rows from the path window in the caller's columns (tmpc_stack_road_halfspaces)
__global__ void tmpc_road_halfspaces_columns_kernel(Dims d, int B, int n_scenes, const double *x0, const double *params, const int *main_of,
                                                    const double *bounds, double off_first, double off_second, double *stat, int n_static, int first_row,
                                                    ColumnEnvRows where)
{
    road_halfspace_rows(where, d, B, n_scenes, x0, params, main_of, bounds, off_first, off_second, stat, n_static, first_row);
}

// ---- obstacle preparation on device (mpc_planner/src/data_preparation.cpp; what a wrapper's obstacle callback does before solveMPC) -----------
// one workgroup per scene q: the scene's raw obstacle list (count[q] clipped to [0, R] of R slots) becomes exactly M prepared obstacles.
//   predictions   raw_vel: step i = pos + (vel dt) i, angle 0, major = minor = (probabilistic ? noise : 0), GAUSSIAN iff probabilistic
//                 (getConstantVelocityPrediction, :58-79);  raw_pred [R][N][5] = (x, y, angle, major, minor): as given, GAUSSIAN iff probabilistic
//                 and the last step's major != 0 (ros1_jackalsimulator.cpp:331-334)
//   filter        max_dist > 0: a slot whose current position is not closer to the robot than max_dist does not exist (removeDistantObstacles, :81-93)
//   selection     more than M left: the M with the smallest key  min_k ((k + 1) 0.6) |pred_k - (p + (v k) (cos psi, sin psi))|, from 1e5, in
//                 ascending (key, raw index) order (ensureObstacleSize, :104-150; the lower raw index wins a tie);
//                 M or fewer: raw order, then dummies at (x + 100, y + 100), radius 0, zero velocity, with the constant-velocity prediction
//                 whatever the input mode (:49-56, :151-165)
//   propagation   `passes` times over GAUSSIAN predictions: major_k = sqrt(major_{k-1}^2 + (sigma_k dt)^2) sequentially over k, the same for
//                 minor (propagatePredictionUncertainty, :170-186) -- one lane per (obstacle, axis), the passes fused: pass p + 1 consumes step k
//                 of pass p as soon as it exists, so no intermediate prediction is stored.
// Slot i's key and validity go into LDS (slots [0, count) only: the only ones read); a slot's rank is the number of smaller (key, index)
// pairs, O(R^2) per scene, which at R <= 1024 is nothing and needs no sort network; then all lanes write the M x N prediction entries.
// cos / sin of the device may differ from libm's in the last bits: they enter the ranking key only, never an output value.
// The arithmetic is tmpc_arith's, the source mpc_planner/data_preparation.h compiles too: every output is bit-equal to the independent
// modules.py::prepare_obstacles.
constexpr int PREP_MAX_SLOTS = 1024, PREP_THREADS = 256;
__global__ __launch_bounds__(PREP_THREADS) void tmpc_prepare_obstacles_kernel(int N, double dt, int R, int M, const int *count, const double *state,
                                                                            const double *raw_pos, const double *raw_radius, const double *raw_vel,
                                                                            const double *raw_pred, int probabilistic, double noise, int passes,
                                                                            double max_dist, double *out_pos, double *out_shape, double *out_radius,
                                                                            uint8_t *out_gauss, int *out_sel)
{
#pragma clang fp contract(off)
    __shared__ double s_key[PREP_MAX_SLOTS];
    __shared__ unsigned char s_valid[PREP_MAX_SLOTS];
    __shared__ int s_nvalid;
    extern __shared__ int s_sel[];                                       // [M]: raw slot of prepared obstacle m, -1 = dummy
    const int q = blockIdx.x, tid = threadIdx.x;
    int cnt = count[q];
    cnt = cnt < 0 ? 0 : (cnt > R ? R : cnt);
    const double x = state[(size_t)q * 4], y = state[(size_t)q * 4 + 1], psi = state[(size_t)q * 4 + 2], v = state[(size_t)q * 4 + 3];
    const double *rp = raw_pos + (size_t)q * R * 2, *rv = raw_vel ? raw_vel + (size_t)q * R * 2 : nullptr;
    const double *pr = raw_pred ? raw_pred + (size_t)q * R * N * 5 : nullptr;
    const double sigma = probabilistic ? noise : 0.0;
    if (tid == 0) s_nvalid = 0;
    for (int m = tid; m < M; m += PREP_THREADS) s_sel[m] = -1;
    __syncthreads();
    const double c = cos(psi), s = sin(psi);
    for (int i = tid; i < cnt; i += PREP_THREADS) {
        const double px = rp[i * 2], py = rp[i * 2 + 1];
        bool valid = true;
        if (max_dist > 0.0) valid = tmpc_arith::within_distance(px, py, x, y, max_dist);
        double best = tmpc_arith::SELECTION_KEY_START;
        for (int k = 0; k < N; k++) {
            const double ox = pr ? pr[((size_t)i * N + k) * 5] : tmpc_arith::cv_step(px, rv[i * 2], dt, k);
            const double oy = pr ? pr[((size_t)i * N + k) * 5 + 1] : tmpc_arith::cv_step(py, rv[i * 2 + 1], dt, k);
            const double dist = tmpc_arith::selection_key_term(k, ox, oy, x, y, v, c, s);
            if (dist < best) best = dist;
        }
        s_key[i] = best; s_valid[i] = valid ? 1 : 0;
        if (valid) atomicAdd(&s_nvalid, 1);
    }
    __syncthreads();
    const bool closest = s_nvalid > M;
    for (int i = tid; i < cnt; i += PREP_THREADS) {
        if (!s_valid[i]) continue;
        const double ki = s_key[i];
        int rank = 0;
        if (closest) { for (int j = 0; j < cnt; j++) if (s_valid[j] && (s_key[j] < ki || (s_key[j] == ki && j < i))) rank++; }    // (counted to the end: stopping at M smaller pairs was measured 30 % slower at R = 1024 -- the exit test breaks up the LDS reads)
        else for (int j = 0; j < i; j++) rank += s_valid[j];
        if (rank < M) s_sel[rank] = i;
    }
    __syncthreads();
    auto is_gaussian = [&](int i) { return probabilistic && (i < 0 || !pr || pr[((size_t)i * N + (N - 1)) * 5 + 3] != 0.0); };
    for (int e = tid; e < M * N; e += PREP_THREADS) {
        const int m = e / N, k = e - m * N, i = s_sel[m];
        const size_t o = ((size_t)q * M + m) * N + k;
        double ox, oy, ang = 0.0, major = sigma, minor = sigma;
        if (i < 0) { ox = tmpc_arith::dummy_coordinate(x); oy = tmpc_arith::dummy_coordinate(y); }
        else if (pr) { const double *g = pr + ((size_t)i * N + k) * 5; ox = g[0]; oy = g[1]; ang = g[2]; major = g[3]; minor = g[4]; }
        else { ox = tmpc_arith::cv_step(rp[i * 2], rv[i * 2], dt, k); oy = tmpc_arith::cv_step(rp[i * 2 + 1], rv[i * 2 + 1], dt, k); }
        out_pos[o * 2] = ox; out_pos[o * 2 + 1] = oy;
        out_shape[o * 3] = ang;
        if (passes == 0 || !is_gaussian(i)) { out_shape[o * 3 + 1] = major; out_shape[o * 3 + 2] = minor; }     // (else: the chain below writes them)
        if (k == 0) {
            out_radius[(size_t)q * M + m] = i < 0 ? 0.0 : raw_radius[(size_t)q * R + i];
            out_gauss[(size_t)q * M + m] = is_gaussian(i) ? 1 : 0;
            out_sel[(size_t)q * M + m] = i;
        }
    }
    if (passes > 0)
        for (int t = tid; t < 2 * M; t += PREP_THREADS) {
            const int m = t >> 1, axis = t & 1, i = s_sel[m];
            if (!is_gaussian(i)) continue;
            double acc0 = 0.0, acc1 = 0.0;
            for (int k = 0; k < N; k++) {
                double val = (i < 0 || !pr) ? sigma : pr[((size_t)i * N + k) * 5 + 3 + axis];
                const double a0 = tmpc_arith::propagate_step(acc0, val, dt);
                acc0 = a0; val = a0;
                if (passes > 1) { const double a1 = tmpc_arith::propagate_step(acc1, val, dt); acc1 = a1; val = a1; }
                out_shape[(((size_t)q * M + m) * N + k) * 3 + 1 + axis] = val;
            }
        }
}

// ---- the collision columns of the current batch's parameter rows from prepared obstacles (tmpc_prepare_obstacles' four buffers) --------------
// one thread per (trajectory, stage, obstacle).  row_model 0: EllipsoidConstraints::update + setParameters (ellipsoid_constraints.cpp:24-90) --
// stage 0 the dummies (x + 50, y + 50, 0, 0, 0, 1, 0.1) in the column order x, y, psi, major, minor, chi, r; stage k >= 1 prediction step k - 1;
// a DETERMINISTIC obstacle major = minor = 0, chi = 1 whatever the shape buffer holds (:72-77), a GAUSSIAN one its radii and chi =
// ExponentialQuantile(0.5, 1 - risk), evaluated by the HOST (no device logarithm enters).  row_model 1: GaussianConstraints as
// modules.py::gaussian_set_parameters has it (gaussian_constraints.cpp:22-79): stage 0 (x + 100, y + 100, 0.1, 0.1, 0.05, 0.1), then x, y,
// major, minor (0 for a DETERMINISTIC obstacle, like the mirror fed by modules.py::prepare_obstacles), risk and the CONFIGURED obstacle radius.  ego_disc_radius / ego_disc_0_offset at every stage.  Nothing else is touched.
template <class Where>
__device__ __forceinline__ void set_obstacle_rows(const Where &where, const Dims &d, int B, double *params, const double *opos, const double *oshape,
                                                  const double *oradius, const uint8_t *ogauss, const int *scene_of, const double *state,
                                                  double robot_radius, double disc_offset, double chi, double risk, double config_radius)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = d.N, M = where.n_obstacles(d);
    if (e >= B * N * M) return;
    const int j = e % M, k = (e / M) % N, b = e / (M * N);
    const int sc = scene_of[b];
    double *p = params + ((size_t)b * N + k) * d.npar;
    if (j == 0) { p[where.disc_radius(d)] = robot_radius; p[where.disc_offset(d)] = disc_offset; }
    const double x = state[(size_t)sc * 4], y = state[(size_t)sc * 4 + 1];
    const size_t o = (((size_t)sc * M + j) * N + (k > 0 ? k - 1 : 0));
    const bool gaussian = ogauss[(size_t)sc * M + j] != 0;
    if (where.row_model(d) == 0) {
        double val[7] = {x + 50.0, y + 50.0, 0.0, 0.0, 0.0, 1.0, 0.1};
        if (k > 0) {
            val[0] = opos[o * 2]; val[1] = opos[o * 2 + 1]; val[2] = oshape[o * 3];
            val[3] = gaussian ? oshape[o * 3 + 1] : 0.0; val[4] = gaussian ? oshape[o * 3 + 2] : 0.0; val[5] = gaussian ? chi : 1.0;
            val[6] = oradius[(size_t)sc * M + j];
        }
#pragma unroll
        for (int w = 0; w < 7; w++) p[where.ellipsoid(d, j, w)] = val[w];
    } else {
        double val[6] = {x + 100.0, y + 100.0, 0.1, 0.1, 0.05, 0.1};
        if (k > 0) {
            val[0] = opos[o * 2]; val[1] = opos[o * 2 + 1]; val[2] = gaussian ? oshape[o * 3 + 1] : 0.0; val[3] = gaussian ? oshape[o * 3 + 2] : 0.0;
            val[4] = risk; val[5] = config_radius;
        }
#pragma unroll
        for (int w = 0; w < 6; w++) p[where.gauss(d, j, w)] = val[w];
    }
}
__global__ void tmpc_set_obstacle_parameters_kernel(Dims d, int B, double *params, const double *opos, const double *oshape, const double *oradius,
                                                    const uint8_t *ogauss, const int *scene_of, const double *state, double robot_radius,
                                                    double disc_offset, double chi, double risk, double config_radius)
{
    set_obstacle_rows(LayoutRows{}, d, B, params, opos, oshape, oradius, ogauss, scene_of, state, robot_radius, disc_offset, chi, risk, config_radius);
}
// the same values into the caller's columns (tmpc_stack_set_obstacle_columns): where.count obstacles per scene, row model where.model
__global__ void tmpc_set_obstacle_columns_kernel(Dims d, int B, double *params, const double *opos, const double *oshape, const double *oradius,
                                                 const uint8_t *ogauss, const int *scene_of, const double *state, double robot_radius,
                                                 double disc_offset, double chi, double risk, double config_radius, ColumnRows where)
{
    set_obstacle_rows(where, d, B, params, opos, oshape, oradius, ogauss, scene_of, state, robot_radius, disc_offset, chi, risk, config_radius);
}

// ---- Contouring::update on a whole reference path (contouring.cpp:28-48, setSplineParameters :94-124) ---------------------------------------
// RosTools::Spline2D::findClosestPoint is not in the reference tree: restated, assumptions in DESIGN.md U14.  The arithmetic is tmpc_arith's, the
// source mpc_planner_modules/reference_path.h compiles too: every output is bit-equal to the independent modules.py::track_path.
constexpr int PATH_MAX_SEGMENTS = 1024;

// one wave per scene q; lane l takes the candidate segments first + l, first + l + 64, ... (a local search has at most 63 candidates: one per
// lane).  segment[q] < 0: every segment of the path is a candidate; otherwise [max(0, prev - R), min(n - 1, prev + R)], prev clamped into
// [0, n - 1] (the reference's _closest_segment protocol, contouring.cpp:37, :155).  Winner: the smallest D, the lowest segment on ties -- a
// 64-lane __shfl_xor argmin on the pair (D, segment) compared lexicographically, so the result does not depend on the lane order.  The
// mirror's sequential scan starts from the first candidate and replaces on strict `<`: a NaN D never wins unless it is the first candidate's,
// which then stays -- reproduced here by leaving NaN out of the reduction and letting a NaN first candidate (lane 0 holds it) take the result.
// Then the lanes copy the window: slot w < S = segment winner + w as given, or, beyond the last segment, the straight continuation along the
// end tangent (0, 0, x'(end), X(end), 0, 0, y'(end), Y(end)), start = length (U14-3); the bound cubics [n_scenes][2][n_seg_max][8] the same way
// from their own last cubics into bound_window [n_scenes][2][S][8], the layout tmpc_road_halfspaces_kernel reads.  A scene with count <= 0
// writes nothing.
__global__ __launch_bounds__(64) void tmpc_track_path_kernel(int S, int n_seg_max, int R, const double *path, const int *count, const double *length,
                                                             const double *bounds, const double *pos, int pos_stride, int *segment, double *closest_s,
                                                             double *window, double *bound_window, uint8_t *reached)
{
#pragma clang fp contract(off)
    const int q = blockIdx.x, lane = threadIdx.x;
    int n = count[q];
    n = n > n_seg_max ? n_seg_max : n;
    if (n <= 0) return;
    const double *pq = path + (size_t)q * n_seg_max * 9;
    const double len = length[q];
    const double px = pos[(size_t)q * pos_stride], py = pos[(size_t)q * pos_stride + 1];
    int first = 0, last = n - 1;
    int prev = segment[q];
    if (prev >= 0) {
        prev = prev > n - 1 ? n - 1 : prev;
        first = prev - R > 0 ? prev - R : 0;
        last = prev + R < n - 1 ? prev + R : n - 1;
    }
    double bD = 0.0, bt = 0.0, D_first = 0.0, t_first = 0.0;
    int bi = -1;
    for (int i = first + lane; i <= last; i += 64) {                     // ascending i per lane: strict '<' keeps the lowest index
        const double *c = pq + (size_t)i * 9;
        const double L = (i + 1 < n ? pq[(size_t)(i + 1) * 9 + 8] : len) - c[8];
        double D, t;
        tmpc_arith::closest_on_segment(c, L, px, py, D, t);
        if (i == first) { D_first = D; t_first = t; }
        if (D == D && (bi < 0 || D < bD)) { bD = D; bt = t; bi = i; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double ov = __shfl_xor(bD, o, 64), ot = __shfl_xor(bt, o, 64); const int oi = __shfl_xor(bi, o, 64);
        const bool take = (oi >= 0) && (bi < 0 || ov < bD || (ov == bD && oi < bi));
        if (take) { bD = ov; bt = ot; bi = oi; }
    }
    D_first = __shfl(D_first, 0, 64); t_first = __shfl(t_first, 0, 64);
    if (D_first != D_first || bi < 0) { bi = first; bt = t_first; }
    // the end of the path: its last cubic at t = L_last
    const double L_last = len - pq[(size_t)(n - 1) * 9 + 8];
    double ex, ey, edx, edy;
    tmpc_arith::cubic(pq + (size_t)(n - 1) * 9, L_last, ex, ey, edx, edy);
    if (lane == 0) {
        segment[q] = bi;
        closest_s[q] = pq[(size_t)bi * 9 + 8] + bt;
        if (reached) reached[q] = tmpc_arith::within_distance(ex, ey, px, py, 1.0) ? 1 : 0;                               // isObjectiveReached, :167-175
    }
    for (int e = lane; e < S * 9; e += 64) {
        const int w = e / 9, col = e - w * 9, i = bi + w;
        double v;
        if (i < n) v = pq[(size_t)i * 9 + col];
        else v = tmpc_arith::padding_entry(col, ex, ey, edx, edy, len);
        window[((size_t)q * S + w) * 9 + col] = v;
    }
    if (bounds && bound_window)
        for (int side = 0; side < 2; side++) {
            const double *bq = bounds + ((size_t)q * 2 + side) * n_seg_max * 8;
            double bx, by, bdx, bdy;
            tmpc_arith::cubic(bq + (size_t)(n - 1) * 8, L_last, bx, by, bdx, bdy);
            for (int e = lane; e < S * 8; e += 64) {
                const int w = e >> 3, col = e & 7, i = bi + w;
                double v;
                if (i < n) v = bq[(size_t)i * 8 + col];
                else v = tmpc_arith::padding_entry(col, bx, by, bdx, bdy);
                bound_window[(((size_t)q * 2 + side) * S + w) * 8 + col] = v;
            }
        }
}

// ---- the spline columns of the current batch's parameter rows from the windows tmpc_track_path_kernel wrote (setSplineParameters, :94-124) ----
// one thread per (trajectory, stage, window slot): the nine columns ip_spline(d, slot, 0..8) of stage k < N of entry b from window
// [n_scenes][S][9] of scene scene_of[b]; an entry whose scene is outside [0, n_scenes) is left untouched.  With closest_s and state
// [B][nx]: state[b][spline] = closest_s[scene] (state.set("spline", closest_s), :42).  Nothing else is written; both models' strides.
template <class Where>
__device__ __forceinline__ void set_path_rows(const Where &where, const Dims &d, int B, double *params, const double *window, const int *scene_of,
                                              int n_scenes, const double *closest_s, double *state)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = d.N, S = where.n_segments(d);
    if (e >= B * N * S) return;
    const int w = e % S, k = (e / S) % N, b = e / (S * N);
    const int sc = scene_of[b];
    if (sc < 0 || sc >= n_scenes) return;
    double *p = params + ((size_t)b * N + k) * d.npar;
    const double *src = window + ((size_t)sc * S + w) * 9;
#pragma unroll
    for (int c = 0; c < 9; c++) p[where.spline(d, w, c)] = src[c];
    if (k == 0 && w == 0 && closest_s && state) state[(size_t)b * ext_nx(d) + (ZS - NU)] = closest_s[sc];
}
__global__ void tmpc_set_path_parameters_kernel(Dims d, int B, double *params, const double *window, const int *scene_of, int n_scenes,
                                                const double *closest_s, double *state)
{
    set_path_rows(LayoutEnvRows{0}, d, B, params, window, scene_of, n_scenes, closest_s, state);
}
// the same window into the caller's columns (tmpc_stack_set_path_columns): where.count segments, where.t.col[9 i + c]
__global__ void tmpc_set_path_columns_kernel(Dims d, int B, double *params, const double *window, const int *scene_of, int n_scenes,
                                             const double *closest_s, double *state, ColumnEnvRows where)
{
    set_path_rows(where, d, B, params, window, scene_of, n_scenes, closest_s, state);
}

// ---- waypoints -> cubic segments: Contouring::onDataReceived (contouring.cpp:126-157), PathReferenceVelocity::onDataReceived -----------------
// (path_reference_velocity.cpp:28-40).  RosTools::Spline2D and tk::spline are not in the reference tree: the natural cubic spline is restated
// as DESIGN.md U15.  The rows and Thomas steps are tmpc_arith's, the source ReferencePathSpline::fitCubic compiles too: every output is bit-equal
// to the independent modules.py::path_knots / fit_cubic / fit_path.
constexpr int FIT_MAX_POINTS = 1025, FIT_CHUNK = 8;

// one curve of a scene: n values `stride_in` doubles apart, and its (a b c d) columns in rows `stride_out` doubles apart
struct FitCurve { const double *in; int stride_in; double *out; int stride_out; };

// curve k of scene q: 0, 1 = x, y of the centreline (columns 0-3 and 4-7 of path [.][9]); then, with bounds, 2 .. 5 = left x, left y, right x,
// right y (bounds [2][.][8]); then, with a velocity profile, v (velocity [.][4])
__device__ inline FitCurve fit_curve(int k, int q, int n_pts_max, int n_seg_max, const double *xy, const double *left_xy, const double *right_xy,
                                     const double *v_in, double *path, double *bounds, double *velocity)
{
    const size_t pts = (size_t)q * n_pts_max;
    if (k < 2) return FitCurve{xy + pts * 2 + k, 2, path + (size_t)q * n_seg_max * 9 + 4 * k, 9};
    if (bounds && k < 6) {
        const int side = (k - 2) >> 1, comp = (k - 2) & 1;
        return FitCurve{(side ? right_xy : left_xy) + pts * 2 + comp, 2, bounds + ((size_t)q * 2 + side) * n_seg_max * 8 + 4 * comp, 8};
    }
    return FitCurve{v_in + pts, 1, velocity + (size_t)q * n_seg_max * 4, 4};
}

// One wave per scene q.  (1) Knots into LDS: the given s, or the chord lengths by all lanes and their running sum by lane 0, strictly left
// to right (a scan would round differently).  (2) h_i = t_{i+1} - t_i by all lanes; the scene is INVALID if n < 2 or any h_i fails
// h_i > 0 && h_i < inf: count = 0, status = 1, nothing else is written.  (3) All lanes: up_i = h_i / 3, di_i = (2 (h_{i-1} + h_i)) / 3, the
// `start` column, and the right-hand sides r_i of every curve into the curve's own b column.  (4) Lanes 0 .. K-1 take one curve each (K <= 7)
// through the forward sweep -- den_i = di_i - lo_i cp_{i-1}, cp_i = up_i / den_i, g_i = (r_i - lo_i g_{i-1}) / den_i; every lane carries the
// same cp recurrence in registers, lane 0 keeps it in LDS -- and the back substitution m_i = g_i - cp_i m_{i+1}; g_i, then m_i, sit in the
// b column, read and written FIT_CHUNK rows at a time so that the loads do not wait on the recurrence.  (5) All lanes: a, c, d of every
// row.  LDS: five arrays of 1025 doubles, 41 KB.  Rows at or beyond count are not touched.
__global__ __launch_bounds__(64) void tmpc_fit_path_kernel(int n_pts_max, int n_seg_max, const double *xy, const int *count, const double *s_in,
                                                           const double *left_xy, const double *right_xy, const double *v_in, double *path,
                                                           int *path_count, double *path_length, double *bounds, double *velocity,
                                                           double *road_width, uint8_t *status)
{
#pragma clang fp contract(off)
    __shared__ double s_t[FIT_MAX_POINTS], s_h[FIT_MAX_POINTS], s_up[FIT_MAX_POINTS], s_di[FIT_MAX_POINTS], s_cp[FIT_MAX_POINTS];
    const int q = blockIdx.x, lane = threadIdx.x;
    int n = count[q];
    n = n < 0 ? 0 : (n > n_pts_max ? n_pts_max : n);
    if (n < 2) {                                                         // (uniform over the block: nobody reaches a barrier)
        if (lane == 0) { path_count[q] = 0; if (status) status[q] = 1; }
        return;
    }
    const double *pq = xy + (size_t)q * n_pts_max * 2;
    if (s_in) {
        for (int i = lane; i < n; i += 64) s_t[i] = s_in[(size_t)q * n_pts_max + i];
    } else {
        for (int i = lane; i < n - 1; i += 64) {
            const double dx = pq[2 * (i + 1)] - pq[2 * i], dy = pq[2 * (i + 1) + 1] - pq[2 * i + 1];
            s_h[i] = sqrt(dx * dx + dy * dy);
        }
        __syncthreads();
        if (lane == 0) {
            double t = 0.0;
            s_t[0] = 0.0;
            for (int i = 1; i < n; i++) { t = t + s_h[i - 1]; s_t[i] = t; }
        }
    }
    __syncthreads();
    bool bad = false;
    for (int i = lane; i < n - 1; i += 64) {
        const double h = s_t[i + 1] - s_t[i];
        if (!tmpc_arith::spacing_valid(h)) bad = true;
        s_h[i] = h;
    }
    if (__syncthreads_or(bad ? 1 : 0)) {
        if (lane == 0) { path_count[q] = 0; if (status) status[q] = 1; }
        return;
    }
    const int K = 2 + (bounds ? 4 : 0) + (velocity ? 1 : 0);
    if (lane == 0) {
        path_count[q] = n - 1;
        path_length[q] = s_t[n - 1];
        if (status) status[q] = 0;
        if (road_width && bounds) {
            const size_t o = (size_t)q * n_pts_max * 2;
            const double ex = left_xy[o] - right_xy[o], ey = left_xy[o + 1] - right_xy[o + 1];
            road_width[q] = sqrt(ex * ex + ey * ey);
        }
    }
    for (int i = lane; i < n - 1; i += 64) {
        s_up[i] = tmpc_arith::spline_off(s_h[i]);
        if (i >= 1) s_di[i] = tmpc_arith::spline_diag(s_h[i - 1], s_h[i]);
        path[((size_t)q * n_seg_max + i) * 9 + 8] = s_t[i];
    }
    for (int k = 0; k < K; k++) {
        const FitCurve c = fit_curve(k, q, n_pts_max, n_seg_max, xy, left_xy, right_xy, v_in, path, bounds, velocity);
        for (int i = 1 + lane; i <= n - 2; i += 64) {
            const double ym = c.in[(size_t)(i - 1) * c.stride_in], y0 = c.in[(size_t)i * c.stride_in], yp = c.in[(size_t)(i + 1) * c.stride_in];
            c.out[(size_t)i * c.stride_out + 1] = tmpc_arith::spline_rhs(ym, y0, yp, s_h[i - 1], s_h[i]);
        }
    }
    __syncthreads();
    const FitCurve mine = fit_curve(lane < K ? lane : 0, q, n_pts_max, n_seg_max, xy, left_xy, right_xy, v_in, path, bounds, velocity);
    double *bcol = mine.out + 1;
    const size_t so = (size_t)mine.stride_out;
    if (lane < K) {
        double g = 0.0, cp = 0.0;
        for (int i0 = 1; i0 <= n - 2; i0 += FIT_CHUNK) {
            double r[FIT_CHUNK];
#pragma unroll
            for (int j = 0; j < FIT_CHUNK; j++) r[j] = i0 + j <= n - 2 ? bcol[(size_t)(i0 + j) * so] : 0.0;
#pragma unroll
            for (int j = 0; j < FIT_CHUNK; j++) {
                const int i = i0 + j;
                if (i <= n - 2) {
                    tmpc_arith::thomas_forward(s_up[i - 1], s_di[i], s_up[i], r[j], cp, g);
                    bcol[(size_t)i * so] = g;
                    if (lane == 0) s_cp[i] = cp;
                }
            }
        }
    }
    __syncthreads();
    if (lane < K) {
        double m = 0.0;                                                  // m_{n-1}
        for (int i0 = n - 2; i0 >= 1; i0 -= FIT_CHUNK) {
            double gg[FIT_CHUNK];
#pragma unroll
            for (int j = 0; j < FIT_CHUNK; j++) gg[j] = i0 - j >= 1 ? bcol[(size_t)(i0 - j) * so] : 0.0;
#pragma unroll
            for (int j = 0; j < FIT_CHUNK; j++) {
                const int i = i0 - j;
                if (i >= 1) { m = tmpc_arith::thomas_backward(gg[j], s_cp[i], m); bcol[(size_t)i * so] = m; }
            }
        }
        bcol[0] = 0.0;                                                   // m_0
    }
    __syncthreads();
    for (int k = 0; k < K; k++) {
        const FitCurve c = fit_curve(k, q, n_pts_max, n_seg_max, xy, left_xy, right_xy, v_in, path, bounds, velocity);
        for (int i = lane; i < n - 1; i += 64) {
            double *o = c.out + (size_t)i * c.stride_out;
            const double m0 = o[1], m1 = i + 1 < n - 1 ? o[c.stride_out + 1] : 0.0, h = s_h[i];
            const double y0 = c.in[(size_t)i * c.stride_in], y1 = c.in[(size_t)(i + 1) * c.stride_in];
            tmpc_arith::spline_row(m0, m1, h, y0, y1, o[0], o[2], o[3]);
        }
    }
}

// ---- the velocity profile along the path: PathReferenceVelocity::setParameters (path_reference_velocity.cpp:59-95) and the value the guidance
// planner is given, path_velocity(state.spline) (guidance_constraints.cpp:91-94).  tk::spline::operator() is not in the reference tree: the
// evaluation is restated as DESIGN.md U17.  Bit-equal to the independent modules.py::path_velocity_window / path_velocity_at.
constexpr int VELOCITY_MAX_WINDOW = 64;

// One wave per scene q.  A scene has a profile iff velocity is given, its flag (all ones if has_velocity is NULL) is set and count > 0.
// With one: slot w < S of window [n_scenes][S][4] = velocity segment seg + w, seg = segment[q] clamped into [0, n - 1], or (0, 0, 0, 0) at or
// beyond n ("brake at the end"); v_ref[q] = the cubic of segment i = max{j < n : start_j <= s} (0 if there is none, U12's lookup) at
// t = s - start_i, s = closest_s[q] -- the lanes test start_j <= s sixty-four segments at a time, a ballot gives the highest j of each
// round, so 1024 segments cost 16 comparisons per lane and the result does not depend on the knots being sorted.  Without one: every slot
// (0, 0, 0, reference_velocity), v_ref = reference_velocity.  The lanes stride over the S x 4 copies; lane 0 evaluates the cubic.  No LDS.
__global__ __launch_bounds__(64) void tmpc_path_velocity_window_kernel(int S, int n_seg_max, const double *velocity, const double *path, const int *count,
                                                                       const int *segment, const double *closest_s, const uint8_t *has_velocity,
                                                                       double reference_velocity, double *window, double *v_ref)
{
#pragma clang fp contract(off)
    const int q = blockIdx.x, lane = threadIdx.x;
    int n = count[q];
    n = n > n_seg_max ? n_seg_max : n;
    const bool profile = velocity != nullptr && n > 0 && (has_velocity == nullptr || has_velocity[q] != 0);
    double *wq = window + (size_t)q * S * 4;
    if (!profile) {
        for (int e = lane; e < S * 4; e += 64) wq[e] = (e & 3) == 3 ? reference_velocity : 0.0;
        if (v_ref && lane == 0) v_ref[q] = reference_velocity;
        return;
    }
    const double *vq = velocity + (size_t)q * n_seg_max * 4;
    int seg = segment[q];
    seg = seg < 0 ? 0 : (seg > n - 1 ? n - 1 : seg);
    for (int e = lane; e < S * 4; e += 64) {
        const int i = seg + (e >> 2);
        wq[e] = i < n ? vq[(size_t)i * 4 + (e & 3)] : 0.0;
    }
    if (!v_ref) return;
    const double *pq = path + (size_t)q * n_seg_max * 9;
    const double s = closest_s[q];
    int found = 0;
    for (int base = 0; base < n; base += 64) {                             // n is the scene's: every lane of the wave runs the same rounds
        const int j = base + lane;
        const unsigned long long hit = __ballot(j < n && pq[(size_t)j * 9 + 8] <= s);
        if (hit) found = base + 63 - __builtin_clzll(hit);                 // ascending rounds: the last hit is the highest j
    }
    if (lane == 0) v_ref[q] = tmpc_arith::cubic_value(vq + (size_t)found * 4, s - pq[(size_t)found * 9 + 8]);
}

// ---- caller-chosen columns of the current batch's parameter rows: the writer for generated solvers, whose column numbers the caller has in the
// stack's parameter map.  The column list (ScatterCols, above) travels by value (at most 128 entries: 516 bytes of kernel arguments).
// one thread per (entry b, stage k < N, listed column c): params[b][k][col[c]] = values[scene_of[b]][c] (per_stage 0: values [n_scenes][n_cols])
// or values[scene_of[b]][k][c] (per_stage 1: values [n_scenes][N][n_cols]); an entry whose scene is outside [0, n_scenes) is left untouched.
// The host has checked every column against npar and the list for duplicates, so no two threads write one address.  Both models' strides.
__global__ void tmpc_scatter_parameters_kernel(Dims d, int B, double *params, ScatterCols cols, const double *values, const int *scene_of, int n_scenes,
                                               int per_stage)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = d.N, nc = cols.n;
    if (e >= B * N * nc) return;
    const int c = e % nc, k = (e / nc) % N, b = e / (nc * N);
    const int sc = scene_of[b];
    if (sc < 0 || sc >= n_scenes) return;
    const double *src = values + (per_stage ? ((size_t)sc * N + k) * nc : (size_t)sc * nc);
    params[((size_t)b * N + k) * d.npar + cols.col[c]] = src[c];
}

// ---- the guidance hand-off: what GuidanceConstraints does with the output of the guidance search either side of the solve.
// The arithmetic and the bookkeeping are tmpc_arith's, shared with mpc_planner_modules/guidance_handoff.h; bit-equal to the independent
// modules.py::sample_guidance / guidance_plan / guidance_decide.
constexpr int GUIDANCE_MAX_NODES = 64;
constexpr int GUIDANCE_MAX_PATHS = 63;                                     // P = n_paths + 1 <= 64: the planner sets are 64-bit masks

// One wave per guidance trajectory j: nodes [n_traj][n_nodes_max][3] = (t, x, y), count[j] of them (n_nodes_max <= 64: one lane per node).
// (1) knots into LDS, h_i by the lanes; INVALID if the count is outside [2, n_nodes_max] or any h_i fails spacing_valid: status 1, both
// rows zeros.  (2) the right-hand sides of x and y by the lanes, (3) lanes 0 / 1 carry x / y through the Thomas recurrence of U15 (both
// compute the same cp, lane 0 keeps it), (4) the lanes write the rows (a b c d) into LDS, (5) one lane per sample k <= N (strided): the
// segment i = max{j <= count - 2 : t_j <= k dt}, 0 if none, tau = k dt - t_i, position and velocity in Horner form.  LDS 5.5 KB.
__global__ __launch_bounds__(64) void tmpc_sample_guidance_kernel(int N, double dt, int n_nodes_max, const double *nodes, const int *count,
                                                                  double *gpos, double *gvel, int *status)
{
#pragma clang fp contract(off)
    __shared__ double s_t[GUIDANCE_MAX_NODES], s_h[GUIDANCE_MAX_NODES], s_cp[GUIDANCE_MAX_NODES], s_c[2][GUIDANCE_MAX_NODES][4];
    const int j = blockIdx.x, lane = threadIdx.x;
    const int n = count[j];
    const double *nq = nodes + (size_t)j * n_nodes_max * 3;
    double *pos = gpos + (size_t)j * (N + 1) * 2, *vel = gvel + (size_t)j * (N + 1) * 2;
    bool invalid = n < 2 || n > n_nodes_max;                               // (uniform over the block)
    if (!invalid) {
        if (lane < n) s_t[lane] = nq[lane * 3];
        __syncthreads();
        bool bad = false;
        if (lane < n - 1) {
            const double h = s_t[lane + 1] - s_t[lane];
            bad = !tmpc_arith::spacing_valid(h);
            s_h[lane] = h;
        }
        invalid = __syncthreads_or(bad ? 1 : 0) != 0;
    }
    if (invalid) {
        for (int e = lane; e < (N + 1) * 2; e += 64) { pos[e] = 0.0; vel[e] = 0.0; }
        if (lane == 0) status[j] = 1;
        return;
    }
    if (lane >= 1 && lane <= n - 2)
        for (int c = 0; c < 2; c++)
            s_c[c][lane][1] = tmpc_arith::spline_rhs(nq[(lane - 1) * 3 + 1 + c], nq[lane * 3 + 1 + c], nq[(lane + 1) * 3 + 1 + c], s_h[lane - 1], s_h[lane]);
    __syncthreads();
    if (lane < 2) {
        double g = 0.0, cp = 0.0;
        for (int i = 1; i <= n - 2; i++) {
            tmpc_arith::thomas_forward(tmpc_arith::spline_off(s_h[i - 1]), tmpc_arith::spline_diag(s_h[i - 1], s_h[i]), tmpc_arith::spline_off(s_h[i]),
                                       s_c[lane][i][1], cp, g);
            s_c[lane][i][1] = g;
            if (lane == 0) s_cp[i] = cp;
        }
    }
    __syncthreads();
    if (lane < 2) {
        double m = 0.0;                                                    // m_{n-1}
        for (int i = n - 2; i >= 1; i--) { m = tmpc_arith::thomas_backward(s_c[lane][i][1], s_cp[i], m); s_c[lane][i][1] = m; }
        s_c[lane][0][1] = 0.0;                                             // m_0
    }
    __syncthreads();
    if (lane < n - 1)
        for (int c = 0; c < 2; c++) {
            const double m0 = s_c[c][lane][1], m1 = lane + 1 < n - 1 ? s_c[c][lane + 1][1] : 0.0;
            tmpc_arith::spline_row(m0, m1, s_h[lane], nq[lane * 3 + 1 + c], nq[(lane + 1) * 3 + 1 + c], s_c[c][lane][0], s_c[c][lane][2], s_c[c][lane][3]);
        }
    __syncthreads();
    for (int k = lane; k <= N; k += 64) {
        const double t = tmpc_arith::sample_time(k, dt);
        int i = 0;
        for (int jj = 0; jj <= n - 2; jj++) if (s_t[jj] <= t) i = jj;
        const double tau = t - s_t[i];
        for (int c = 0; c < 2; c++) {
            pos[k * 2 + c] = tmpc_arith::cubic_value(s_c[c][i], tau);
            vel[k * 2 + c] = tmpc_arith::cubic_slope(s_c[c][i], tau);
        }
    }
    if (lane == 0) status[j] = 0;
}

// the options of tmpc_guidance_plan / tmpc_guidance_decide, by value
struct GuidanceOptions { int n_paths, use_tmpcpp, warmstart_with_mpc_solution, shift; double weight_consistency; };

// One thread per scene q (the mapping is a sequential scan over the scene's planners: nothing to share between lanes); entry b = q P + p.
__global__ void tmpc_guidance_plan_kernel(int n_scenes, GuidanceOptions o, const int *traj_count, const int *topology_class,
                                          const uint8_t *previously_selected, const int *planner_ids, const int *selection, int *mode, int *src,
                                          uint8_t *init_enabled, uint8_t *rows_dummy, uint8_t *disabled, int *guidance_id, double *weight)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_scenes) return;
    const int P = o.n_paths + (o.use_tmpcpp ? 1 : 0);
    const size_t f = (size_t)q * P;
    tmpc_arith::guidance_plan_scene((int)f, o.n_paths, o.use_tmpcpp, o.warmstart_with_mpc_solution, o.shift, o.weight_consistency, traj_count[q],
                                    topology_class + (size_t)q * o.n_paths, previously_selected ? previously_selected + (size_t)q * o.n_paths : nullptr,
                                    planner_ids + f, selection + (size_t)q * 3, mode + f, src + f, init_enabled + f, rows_dummy + f, disabled + f,
                                    guidance_id + f, weight + f);
}

// One thread per scene q: FindBestPlanner over its P entries, the exit code, the command, the state commit.
__global__ void tmpc_guidance_decide_kernel(int n_scenes, GuidanceOptions o, int N, int nxe, const double *pobj, const int *exit_code,
                                            const uint8_t *disabled, const int *guidance_id, const double *weight, const double *state,
                                            const double *xtraj, const double *utraj, double deceleration, double control_dt, int enable_output,
                                            int *best, int *exit_out, double *cmd, int *planner_ids, int *selection)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_scenes) return;
    const int P = o.n_paths + (o.use_tmpcpp ? 1 : 0);
    const size_t f = (size_t)q * P;
    const int x_entry = (N + 1) * nxe, u_entry = N * NU;
    tmpc_arith::guidance_decide_scene(P, o.use_tmpcpp, pobj + f, exit_code + f, disabled + f, guidance_id + f, weight + f, xtraj + f * x_entry, x_entry,
                                      nxe, utraj + f * u_entry, u_entry, state[(size_t)q * nxe + 3], deceleration, control_dt, enable_output, best + q,
                                      exit_out + q, cmd + (size_t)q * 2, planner_ids + f, selection + (size_t)q * 3);
}

// ---- the episode step (include/tmpc_hip_episode.h): plant, obstacle motion, intrusion, termination, log, restart ----------------
// the options of tmpc_episode_step, by value
struct EpisodeOptions { int substeps, timeout_ticks, max_episodes; double control_dt, max_acceleration, max_angular_velocity, robot_radius, goal_x; };
constexpr int EPISODE_MAX_SLOTS = 1024, EPISODE_MAX_SUBSTEPS = 16, EPISODE_MAX_LOG = 4096;

// One wave per scene q.  The plant, the verdict and the counters are functions of the scene's own few numbers: every lane evaluates them on
// the same operands (wave-uniform: no branch, nothing to broadcast, the same bits in every lane) and lane 0 stores them.  Lane l moves the
// obstacle slots l, l + 64, ... (at most 16 at R = 1024) and takes their intrusion candidates; a 64-lane __shfl_xor maximum on strict `>`
// from 0.0 gives the tick's intrusion -- no NaN enters and a maximum does not depend on the order, so the result is the mirror's sequential
// scan's.  On a reset the same lane restores the same slots it moved: one lane, the same addresses, program order.  The state outputs are
// strided over the lanes.  Plain loads and stores: a scene belongs to one wave.  The arithmetic is tmpc_arith's, the source
// mpc_planner/episode.h compiles too: every output is bit-equal to the independent modules.py::episode_step.
__global__ __launch_bounds__(64) void tmpc_episode_step_kernel(int R, int P, int nx, EpisodeOptions o, const double *cmd, double *plant,
                                                               const double *plant0, const int *count, double *raw_pos, double *raw_vel,
                                                               const double *raw_radius, const double *raw_pos0, const double *raw_vel0,
                                                               const double *box, const double *goal, int *episode, double *episode_f, double *log,
                                                               uint8_t *was_reset, double *state4, double *state_nx, double *state_batch,
                                                               int *planner_ids, int *selection, int *segment)
{
#pragma clang fp contract(off)
    const int q = blockIdx.x, lane = threadIdx.x;
    int cnt = count[q];
    cnt = cnt < 0 ? 0 : (cnt > R ? R : cnt);
    // 1. the plant
    double p[6];
#pragma unroll
    for (int i = 0; i < 6; i++) p[i] = plant[(size_t)q * 6 + i];
    const double cmd_v = cmd[(size_t)q * 2], cmd_w = cmd[(size_t)q * 2 + 1];
    const double h = o.control_dt / (double)o.substeps;
    for (int it = 0; it < o.substeps; it++) tmpc_arith::plant_substep(cmd_v, cmd_w, h, o.max_acceleration, o.max_angular_velocity, p);
    // 2. the obstacles, 3. the intrusion
    const bool boxed = box != nullptr;
    double xlo = 0.0, xhi = 0.0, ylo = 0.0, yhi = 0.0;
    if (boxed) { xlo = box[(size_t)q * 4]; xhi = box[(size_t)q * 4 + 1]; ylo = box[(size_t)q * 4 + 2]; yhi = box[(size_t)q * 4 + 3]; }
    double *rp = raw_pos + (size_t)q * R * 2, *rv = raw_vel + (size_t)q * R * 2;
    double intrusion = 0.0;
    for (int i = lane; i < cnt; i += 64) {
        double ox = rp[i * 2], oy = rp[i * 2 + 1], vx = rv[i * 2], vy = rv[i * 2 + 1];
        tmpc_arith::obstacle_step(ox, vx, o.control_dt, boxed, xlo, xhi);
        tmpc_arith::obstacle_step(oy, vy, o.control_dt, boxed, ylo, yhi);
        rp[i * 2] = ox; rp[i * 2 + 1] = oy; rv[i * 2] = vx; rv[i * 2 + 1] = vy;
        const double cand = tmpc_arith::intrusion_candidate(o.robot_radius, raw_radius[(size_t)q * R + i], ox, oy, p[0], p[1]);
        if (cand > intrusion) intrusion = cand;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const double other = __shfl_xor(intrusion, s, 64);
        if (other > intrusion) intrusion = other;
    }
    // 4. the counters, 5. the verdict (wave-uniform)
    int ticks = episode[(size_t)q * 4] + 1, collisions = episode[(size_t)q * 4 + 1] + (intrusion > 0.0 ? 1 : 0), finished = episode[(size_t)q * 4 + 2];
    double max_intrusion = episode_f[(size_t)q * 2];
    if (intrusion > max_intrusion) max_intrusion = intrusion;
    bool completed = p[0] > o.goal_x;
    if (goal) completed = completed || tmpc_arith::within_distance(p[0], p[1], goal[(size_t)q * 3], goal[(size_t)q * 3 + 1], goal[(size_t)q * 3 + 2]);
    const bool reset = completed || (o.timeout_ticks > 0 && ticks >= o.timeout_ticks);
    // 6. the log and the restart
    if (reset) {
        if (lane == 0 && finished >= 0 && finished < o.max_episodes) {
            double *row = log + ((size_t)q * o.max_episodes + finished) * 4;
            row[0] = (double)ticks * o.control_dt; row[1] = completed ? 1.0 : 0.0; row[2] = (double)collisions; row[3] = max_intrusion;
        }
        finished += 1;
#pragma unroll
        for (int i = 0; i < 6; i++) p[i] = plant0[(size_t)q * 6 + i];
        for (int i = lane; i < cnt; i += 64) {
            const double *rp0 = raw_pos0 + (size_t)q * R * 2, *rv0 = raw_vel0 + (size_t)q * R * 2;
            rp[i * 2] = rp0[i * 2]; rp[i * 2 + 1] = rp0[i * 2 + 1]; rv[i * 2] = rv0[i * 2]; rv[i * 2 + 1] = rv0[i * 2 + 1];
        }
        ticks = 0; collisions = 0; max_intrusion = 0.0;
        if (planner_ids) for (int e = lane; e < P; e += 64) planner_ids[(size_t)q * P + e] = -1;
        if (lane == 0) {
            if (selection) { selection[(size_t)q * 3] = -1; selection[(size_t)q * 3 + 1] = 0; selection[(size_t)q * 3 + 2] = -1; }
            if (segment) segment[q] = -1;
        }
    }
    if (lane == 0) {
        episode[(size_t)q * 4] = ticks; episode[(size_t)q * 4 + 1] = collisions; episode[(size_t)q * 4 + 2] = finished; episode[(size_t)q * 4 + 3] = 0;
        episode_f[(size_t)q * 2] = max_intrusion; episode_f[(size_t)q * 2 + 1] = intrusion;
        was_reset[q] = reset ? 1 : 0;
#pragma unroll
        for (int i = 0; i < 6; i++) plant[(size_t)q * 6 + i] = p[i];
#pragma unroll
        for (int i = 0; i < 4; i++) state4[(size_t)q * 4 + i] = p[i];
    }
    // 7. the planner's states: entries 0 .. 3 from the plant, the rest zeroed on a reset only
    auto entry = [&](int col) { return col == 0 ? p[0] : col == 1 ? p[1] : col == 2 ? p[2] : p[3]; };     // (selects: p stays in registers)
    if (state_nx)
        for (int e = lane; e < nx; e += 64) {
            if (e < 4) state_nx[(size_t)q * nx + e] = entry(e);
            else if (reset) state_nx[(size_t)q * nx + e] = 0.0;
        }
    if (state_batch) {
        const size_t total = (size_t)P * nx;
        for (size_t e = lane; e < total; e += 64) {
            const int col = (int)(e % (size_t)nx);
            if (col < 4) state_batch[(size_t)q * total + e] = entry(col);
            else if (reset) state_batch[(size_t)q * total + e] = 0.0;
        }
    }
}


// ---- f-3: scenario -> polygon on device (SH-MPC, BASELINE config 5) ------------------------------------------------
// The reference delegates this to the external scenario_module (scenario_constraints.cpp:47,76-79; source absent), so
// this restates the host mirror mpc_planner_amd/modules.py::scenario_halfspaces: for stage k >= 1 of trajectory b every
// sampled obstacle position o (n_pts = obstacles x scenarios of the trajectory's scene, prediction step k-1) gives the
// halfspace a = (o - p)/|o - p|, b = a.o - radius around the guess p = x0[b][k](x, y); the constraints of the stage are
// the halfspaces that form the boundary of the intersection polygon (all others are redundant), closest first, at most
// n_rows of them; unused rows and stage 0 get the dummy row (1, 0, x + 100) (decomp_constraints.cpp:153-169 pattern).
// One workgroup per (trajectory, stage), in two parts:
//   FILTER (free to be anything conservative: a halfspace whose boundary line misses the polygon of SOME of the
//      halfspaces -- the "seeds" -- cannot touch the smaller polygon of all of them, and dropping such halfspaces
//      changes neither the polygon nor which halfspaces are its edges).  On registers: the closest halfspace of each of
//      256 direction sectors is a seed (LDS table, atomicMin on an order-preserving key of the margin, then on the
//      index); a halfspace is clipped by the seed of its own sector and the two nearest seeds on either side only --
//      those decide, 5 clips instead of one per seed, the interval kept as two fractions compared by cross-multiplication
//      (no division); the survivors (~100 of 2048 on the SH-MPC scenes) are appended to a compact LDS list, on which a
//      second round with 2048 sectors and every seed clipping leaves ~11.
//   EDGE TEST (the definition, same per-pair arithmetic as the mirror): candidate i is an edge iff the piece of its line
//      inside all other candidates' halfspaces has positive length; its row index is its rank by (margin, sample index).
// The samples of a stage are contiguous ([scene][N][n_pts][2]): a coalesced stream shared through L2 by the scene's
// trajectories.  The edge test is written without FMA contraction, so the rows equal the mirror's bit for bit.
constexpr double POLY_EPS_PARALLEL = 1e-12, POLY_TOL_EDGE = 1e-9, POLY_SEED_MARGIN = 1e-6;
constexpr int POLY_IDX_MASK = 0x1fff, POLY_DROP_FLAG = 1 << 29;     // a candidate's index word during the second filter round
constexpr int POLY_SEC1 = 256;                        // direction sectors of round 1 (32 per octant, in angular order)
constexpr int POLY_NONE = 0x7fffffff;
constexpr int POLY_LIST_CAP = 1024;                 // candidate list of the first pass.  512 until round 4: on the cfg-5 scenes (8 x 256 samples per stage) enough units kept
                                                    // more than 512 candidates that the second pass cost another 250 us per tick; with 1024 none overflows there
                                                    // (second pass 4 us, the tick 2.06 -> 1.80 ms), and 28 KB of list still leave 4 workgroups per CU

__device__ __forceinline__ int poly_sector(double ax, double ay, int bins)        // octant x bins of min(|ax|,|ay|)/max: a partition of the directions
{
    const double u = fabs(ax), v = fabs(ay);
    const int oct = (ax < 0.0 ? 1 : 0) | (ay < 0.0 ? 2 : 0) | (v > u ? 4 : 0);
    const double t = (v > u ? u : v) / (v > u ? v : u);
    int sub = (int)(t * (double)bins);
    sub = sub > bins - 1 ? bins - 1 : sub;
    return oct * bins + sub;
}

__device__ __forceinline__ int poly_sector_angular(double ax, double ay)          // the same partition with 32 bins, numbered counter-clockwise
{
    const double u = fabs(ax), v = fabs(ay);
    const bool steep = v > u;
    const double t = (steep ? u : v) / (steep ? v : u);
    int bin = (int)(t * 32.0);
    bin = bin > 31 ? 31 : bin;
    const int quad = ax >= 0.0 ? (ay >= 0.0 ? 0 : 3) : (ay >= 0.0 ? 1 : 2);
    const bool second = ((quad & 1) == 0) == steep;           // second half (45..90 deg) of the quadrant
    const bool rising = ((quad & 1) == 0) != steep;           // t grows with the angle in this half
    return quad * 64 + (second ? 32 : 0) + (rising ? bin : 31 - bin);
}

__device__ __forceinline__ unsigned long long poly_key(double x)          // order-preserving map of a double to an unsigned integer
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// ---- SH-MPC scenario sampler (f-3; scenario_constraints.cpp:121-131: every solver draws its own scenarios,
// scenario_module.GetSampler().IntegrateAndTranslateToMeanAndVariance -- the scenario_module is absent from the reference tree, so this
// restates what the call's name and its inputs say: unit samples translated to the mean and the integrated variance of every prediction
// step).  One scenario = one joint draw for all obstacles over the horizon.  For obstacle m of solver (scene) q and scenario s:
// a mode of the obstacle's Gaussian mixture is drawn from its probabilities, then ONE standard-normal pair (xi1, xi2) places the obstacle
// on every step k of that mode:  o_k = mean_k + R(angle_k) (major_k xi1, minor_k xi2)  (PredictionStep: position, angle, major / minor
// radius = the integrated standard deviations, data_types.h:42-54).
// Counter-based and bit-reproducible: the random bits are a splitmix64 hash of (seed, solver, obstacle, scenario, draw), the normal
// deviates come from the inverse normal CDF (Acklam's rational approximation, |error| < 1.2e-9) evaluated with +, x, /, sqrt and a
// logarithm built from the same operations (det_log), no FMA contraction -- so modules.sample_scenarios reproduces every sample
// bit for bit and the polygon rows of a device-sampled tick can be checked exactly.  The rotation enters as (cos, sin) computed by
// the caller: trigonometric functions are not reproducible across libraries.
__host__ __device__ inline unsigned long long smp_mix(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ inline double smp_uniform(unsigned long long key, unsigned long long ctr)      // in (0, 1), 53 bits
{
    const unsigned long long r = smp_mix(key + (ctr + 1ull) * 0x9E3779B97F4A7C15ull);
    return ((double)(r >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}
__device__ inline double det_log(double x)                   // natural logarithm from +, x, / only (x > 0, normal): ~1e-14 relative
{
#pragma clang fp contract(off)
    int e;
    double m = frexp(x, &e);                                  // x = m 2^e, m in [0.5, 1)
    if (m < 0.70710678118654752) { m = m * 2.0; e = e - 1; }  // m in [sqrt(1/2), sqrt(2))
    const double f = (m - 1.0) / (m + 1.0), w = f * f;
    double p = 1.0 / 19.0;
    p = p * w + 1.0 / 17.0; p = p * w + 1.0 / 15.0; p = p * w + 1.0 / 13.0; p = p * w + 1.0 / 11.0; p = p * w + 1.0 / 9.0;
    p = p * w + 1.0 / 7.0; p = p * w + 1.0 / 5.0; p = p * w + 1.0 / 3.0; p = p * w + 1.0;
    return (double)e * 0.69314718055994531 + 2.0 * f * p;
}
__device__ inline double smp_normal(double u)                // inverse normal CDF (Acklam), u in (0, 1)
{
#pragma clang fp contract(off)
    const double a0 = -3.969683028665376e+01, a1 = 2.209460984245205e+02, a2 = -2.759285104469687e+02, a3 = 1.383577518672690e+02,
                 a4 = -3.066479806614716e+01, a5 = 2.506628277459239e+00;
    const double b0 = -5.447609879822406e+01, b1 = 1.615858368580409e+02, b2 = -1.556989798598866e+02, b3 = 6.680131188771972e+01,
                 b4 = -1.328068155288572e+01;
    const double c0 = -7.784894002430293e-03, c1 = -3.223964580411365e-01, c2 = -2.400758277161838e+00, c3 = -2.549732539343734e+00,
                 c4 = 4.374664141464968e+00, c5 = 2.938163982698783e+00;
    const double d0 = 7.784695709041462e-03, d1 = 3.224671290700398e-01, d2 = 2.445134137142996e+00, d3 = 3.754408661907416e+00;
    const double lo = 0.02425;
    if (u < lo) {
        const double q = sqrt(-2.0 * det_log(u));
        return (((((c0 * q + c1) * q + c2) * q + c3) * q + c4) * q + c5) / ((((d0 * q + d1) * q + d2) * q + d3) * q + 1.0);
    }
    if (u > 1.0 - lo) {
        const double q = sqrt(-2.0 * det_log(1.0 - u));
        return -(((((c0 * q + c1) * q + c2) * q + c3) * q + c4) * q + c5) / ((((d0 * q + d1) * q + d2) * q + d3) * q + 1.0);
    }
    const double q = u - 0.5, r = q * q;
    return (((((a0 * r + a1) * r + a2) * r + a3) * r + a4) * r + a5) * q / (((((b0 * r + b1) * r + b2) * r + b3) * r + b4) * r + 1.0);
}
// pred [n_solvers][M][n_modes][N][6] = (x, y, cos angle, sin angle, major, minor) per prediction step; prob [n_solvers][M][n_modes];
// out [n_solvers][N][M * S][2] (the layout tmpc_scenario_halfspaces reads: step k - 1 for stage k, sample m * S + s)
__global__ void tmpc_sample_scenarios_kernel(int N, int n_solvers, int M, int n_modes, int S, unsigned long long seed, const double *pred,
                                             const double *prob, double *out)
{
#pragma clang fp contract(off)
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_solvers * M * S) return;
    const int s = idx % S, m = (idx / S) % M, q = idx / (S * M);
    const unsigned long long key = smp_mix(seed ^ smp_mix((unsigned long long)q + 0x51ED270B1ull));
    const unsigned long long ctr = ((unsigned long long)m * (unsigned long long)S + (unsigned long long)s) * 4ull;
    const double um = smp_uniform(key, ctr);
    const double *pr = prob + ((size_t)q * M + m) * n_modes;
    int mode = n_modes - 1;
    double cum = 0.0;
    for (int j = 0; j < n_modes; j++) { cum = cum + pr[j]; if (um < cum) { mode = j; break; } }
    const double xi1 = smp_normal(smp_uniform(key, ctr + 1ull)), xi2 = smp_normal(smp_uniform(key, ctr + 2ull));
    const double *ps = pred + (((size_t)q * M + m) * n_modes + mode) * N * 6;
    for (int k = 0; k < N; k++) {
        const double *e = ps + (size_t)k * 6;
        const double a = e[4] * xi1, b = e[5] * xi2;
        double *o = out + (((size_t)q * N + k) * ((size_t)M * S) + (size_t)m * S + s) * 2;
        o[0] = (e[0] + e[2] * a) - e[3] * b;
        o[1] = (e[1] + e[3] * a) + e[2] * b;
    }
}

// ---- scenario removal (SH-MPC discards a fixed number of scenarios before building the constraints and pays for it in the bound:
// the discarded scenarios count into the compression set, modules.scenario_risk(removed=...)).  The scenario_module's own policy is
// not in the reference tree; restated as the greedy rule of the method's paper: the scenarios that constrain the previous plan most --
// smallest clearance  min over obstacles m, stages k >= 1 of |o_{m,s,k-1} - p_k| - radius  -- go first (lowest scenario index on ties).
// One workgroup per trajectory: clearance per scenario in LDS, then n_discard rounds of a block-wide argmin.  discard [B][S] (1 = out).
__global__ __launch_bounds__(256) void tmpc_scenario_discard_kernel(Dims d, int B, const double *x0, const double *samples, int n_pts, int S,
                                                                 const int *scene_of, double radius, int n_discard, unsigned char *discard)
{
#pragma clang fp contract(off)
    extern __shared__ double s_clear[];                               // [S]
    __shared__ unsigned long long s_min;
    __shared__ int s_arg;
    const int b = blockIdx.x, tid = threadIdx.x, N = d.N;
    if (b >= B) return;
    const int sc = scene_of[b], M = n_pts / S;
    for (int s = tid; s < S; s += 256) {
        double best = 1e300;
        for (int k = 1; k < N; k++) {
            const double px = x0[((size_t)b * (N + 1) + k) * ext_nv(d) + ZX], py = x0[((size_t)b * (N + 1) + k) * ext_nv(d) + ZY];
            const double2 *o = reinterpret_cast<const double2 *>(samples) + ((size_t)sc * N + (k - 1)) * n_pts;
            for (int m = 0; m < M; m++) {
                const double2 q = o[m * S + s];
                const double dx = q.x - px, dy = q.y - py;
                const double c = sqrt(dx * dx + dy * dy) - radius;
                best = c < best ? c : best;
            }
        }
        s_clear[s] = best;
        discard[(size_t)b * S + s] = 0;
    }
    __syncthreads();
    for (int r = 0; r < n_discard && r < S; r++) {
        if (tid == 0) { s_min = ~0ull; s_arg = 0x7fffffff; }
        __syncthreads();
        for (int s = tid; s < S; s += 256) if (!discard[(size_t)b * S + s]) atomicMin(&s_min, poly_key(s_clear[s]));
        __syncthreads();
        for (int s = tid; s < S; s += 256) if (!discard[(size_t)b * S + s] && poly_key(s_clear[s]) == s_min) atomicMin(&s_arg, s);
        __syncthreads();
        if (tid == 0) discard[(size_t)b * S + s_arg] = 1;
        __syncthreads();
    }
}


// halfspace j = (aj1, aj2, dmj) clips the boundary line of halfspace i, q_i + t perp_i, to  c t <= rhs
struct PolyClip { double lo, hi; bool kill; };
__device__ __forceinline__ void poly_clip(PolyClip &w, double ai1, double ai2, double dmi, int i, double aj1, double aj2, double dmj, int j)
{
#pragma clang fp contract(off)
    const double c = aj1 * (-ai2) + aj2 * ai1;
    const double dot = aj1 * ai1 + aj2 * ai2;
    const double rhs = dmj - dmi * dot;
    // hi = min(hi, rhs / c), lo = max(lo, rhs / c); the division only when the bound may move: a quotient that is clearly (1e-9
    // relative) on the far side of the current bound leaves it as it is, so the result equals the plain min / max
    // (one code path for both signs of c -- round 6: as two branches the lanes of a wave diverged and every clip paid for two divisions; the expressions
    //  evaluated per case are the same: bit for bit the same bounds)
    const bool pos = c > POLY_EPS_PARALLEL;
    if (pos || c < -POLY_EPS_PARALLEL) {
        const double t = (pos ? w.hi : w.lo) * c;                 // c < 0:  rhs / c > lo  <=>  rhs < lo c
        if (!(rhs > t + 1e-9 * fabs(t))) {
            const double r = rhs / c;
            const double nhi = r < w.hi ? r : w.hi, nlo = r > w.lo ? r : w.lo;
            w.hi = pos ? nhi : w.hi; w.lo = pos ? w.lo : nlo;
        }
    } else if (dot > 0.0 ? (dmj < dmi || (dmj == dmi && j < i)) : rhs < 0.0) w.kill = true;   // parallel: same direction -> the closer one (lowest index) wins
}

// The filter's clip: the same interval kept as two fractions, hi = nh / dh and lo = nl / dl (dh, dl >= 0; 1/0 and -1/0 are the
// infinities), compared by cross-multiplication -- no division.  Nearly parallel seeds (|c| < 1e-6) are skipped, which keeps every
// quotient below ~1e8 m and the rounding of the products (1e-16 relative) far inside the filter's margin; skipping only loosens it.
struct PolyFrac { double nh, dh, nl, dl; };
__device__ __forceinline__ void poly_clip_fast(PolyFrac &w, double ai1, double ai2, double dmi, double aj1, double aj2, double dmj)
{
    const double c = aj1 * (-ai2) + aj2 * ai1;
    const double rhs = dmj - dmi * (aj1 * ai1 + aj2 * ai2);
    if (c > 1e-6) { if (rhs * w.dh < w.nh * c) { w.nh = rhs; w.dh = c; } }
    else if (c < -1e-6) { if (-rhs * w.dl > w.nl * -c) { w.nl = -rhs; w.dl = -c; } }
}
__device__ __forceinline__ bool poly_frac_alive(const PolyFrac &w) { return w.nh * w.dl - w.nl * w.dh >= -POLY_SEED_MARGIN * (w.dh * w.dl); }   // (>=: both sides are 0 while a bound is infinite)

#ifdef TMPC_POLY_PROFILE
#define POLY_T(n) do { __syncthreads(); if (tid == 0) { const long long t_ = wall_clock64(); if (t_ - t_prev > 2500) printf("poly unit %d seg %d: %lld (x10 ns) nk %d ns %d ne %d\n", unit, n, t_ - t_prev, s_nk, s_ns, s_ne); t_prev = wall_clock64(); } } while (0)
#else
#define POLY_T(n) do { } while (0)
#endif
// one (trajectory, stage) = `unit` by one workgroup of 256 threads.  Where: the rows and ego_disc_0_offset go to the layout's ip_slk / ip_disc_offset
// (LayoutEnvRows{0}) or to the caller's columns (ColumnEnvRows, where.count = n_rows; include/tmpc_hip_stack_scenario.h) -- every write of a
// parameter, and nothing else, goes through it.
template <class Where>
__device__ __forceinline__ void poly_stage(const Where &where, int unit, const Dims &d, int B, const double *x0, double *params, const double *samples, int n_pts,
                                           int n_rows, const int *scene_of, const double *state_x, double radius, double disc_offset,
                                           int *row_sample, int cap, int *overflow, int *empty_stages, const unsigned char *discard, int n_scen)
{
#pragma clang fp contract(off)
    extern __shared__ double s_dyn[];                                    // the candidates, compact: normal, margin, sample index (~index: not an edge)
    __shared__ unsigned long long s_best[POLY_SEC1];
    __shared__ double sd_ax[POLY_SEC1], sd_ay[POLY_SEC1], sd_dm[POLY_SEC1];
    __shared__ int s_seed[POLY_SEC1], s_pick[POLY_SEC1];
    __shared__ short s_next[POLY_SEC1], s_prev[POLY_SEC1];              // nearest sector with a seed, counter-clockwise / clockwise (-1: none)
    __shared__ int s_nk, s_ns, s_nw, s_ne;
    __shared__ unsigned long long s_mask[4];
    double *c_ax = s_dyn, *c_ay = s_dyn + cap, *c_dm = s_dyn + 2 * (size_t)cap;
    int *c_idx = reinterpret_cast<int *>(s_dyn + 3 * (size_t)cap);
    const int N = d.N;
    const int b = unit / N, k = unit - b * N;
    const int sc = scene_of[b];
    double *p = params + ((size_t)b * N + k) * d.npar;
    const int tid = threadIdx.x;
    int *which = row_sample + (size_t)unit * n_rows;                  // the sample behind each row (-1: dummy), for tmpc_scenario_support
    if (tid == 0) p[where.disc_offset(d)] = disc_offset;
    if (k == 0) {
        if (tid < n_rows) { p[where.slk(d, tid, 0)] = 1.0; p[where.slk(d, tid, 1)] = 0.0; p[where.slk(d, tid, 2)] = state_x[sc] + 100.0; which[tid] = -1; }
        return;
    }
    long long t_prev = 0; (void)t_prev;
#ifdef TMPC_POLY_PROFILE
    t_prev = wall_clock64();
#endif
    s_best[tid] = ~0ull; s_seed[tid] = POLY_NONE;
    if (tid == 0) { s_nk = 0; s_ne = 0; s_ns = 0; }
    __syncthreads();
    const double px = x0[((size_t)b * (N + 1) + k) * ext_nv(d) + ZX], py = x0[((size_t)b * (N + 1) + k) * ext_nv(d) + ZY];
    const double2 *o = reinterpret_cast<const double2 *>(samples) + ((size_t)sc * N + (k - 1)) * n_pts;
    auto halfspace = [&](int i, double &ax, double &ay, double &dm) {
        const double2 q = o[i];
        const double dx = q.x - px, dy = q.y - py;
        const double dist = sqrt(dx * dx + dy * dy);
        ax = dx / dist; ay = dy / dist; dm = dist - radius;
    };
    // ---- round 1 on registers: the first CACHE halfspaces of a thread are kept, the rest (n_pts > 2048) recomputed per pass
    constexpr int CACHE = 8;
    double r_ax[CACHE], r_ay[CACHE], r_dm[CACHE]; int r_sec[CACHE];
    // discarded scenarios (tmpc_scenario_discard; scenario of sample i = i % n_scen) do not exist for this trajectory's polygons
    auto alive = [&](int i) { return discard == nullptr || discard[(size_t)b * n_scen + i % n_scen] == 0; };
    unsigned r_alive = 0;
#pragma unroll
    for (int c = 0; c < CACHE; c++)
        if (tid + c * 256 < n_pts && alive(tid + c * 256)) { r_alive |= 1u << c; halfspace(tid + c * 256, r_ax[c], r_ay[c], r_dm[c]); r_sec[c] = poly_sector_angular(r_ax[c], r_ay[c]); }
    auto every_sample = [&](auto &&f) {
#pragma unroll
        for (int c = 0; c < CACHE; c++) if (r_alive >> c & 1) f(tid + c * 256, r_ax[c], r_ay[c], r_dm[c], r_sec[c]);
        for (int i = tid + CACHE * 256; i < n_pts; i += 256) if (alive(i)) { double ax, ay, dm; halfspace(i, ax, ay, dm); f(i, ax, ay, dm, poly_sector_angular(ax, ay)); }
    };
    POLY_T(0);
    every_sample([&](int, double, double, double dm, int sec) { atomicMin(&s_best[sec], poly_key(dm)); });
    __syncthreads();
    every_sample([&](int i, double, double, double dm, int sec) { if (poly_key(dm) == s_best[sec]) atomicMin(&s_seed[sec], i); });
    __syncthreads();
    every_sample([&](int i, double ax, double ay, double dm, int sec) { if (s_seed[sec] == i) { sd_ax[sec] = ax; sd_ay[sec] = ay; sd_dm[sec] = dm; } });
    {   // nearest sectors with a seed on either side of sector tid: from the four ballot words of the table (wave w holds sectors 64w..64w+63)
        const unsigned long long mine = __ballot(s_seed[tid] != POLY_NONE);
        if ((tid & 63) == 0) s_mask[tid >> 6] = mine;
        __syncthreads();
        const int w0 = tid >> 6, bit = tid & 63;
        int nx = -1, pv = -1;
#pragma unroll
        for (int step = 0; step <= 4; step++) {                   // own word above the bit, the three other words, own word below the bit
            const int wn = (w0 + step) & 3, wp = (w0 - step) & 3;
            unsigned long long xn = s_mask[wn], xp = s_mask[wp];
            if (step == 0) { xn &= bit == 63 ? 0ull : ~0ull << (bit + 1); xp &= (1ull << bit) - 1ull; }
            if (step == 4) { xn &= (1ull << bit) - 1ull; xp &= bit == 63 ? 0ull : ~0ull << (bit + 1); }
            if (nx < 0 && xn) nx = wn * 64 + __ffsll((long long)xn) - 1;
            if (pv < 0 && xp) pv = wp * 64 + 63 - __clzll((long long)xp);
        }
        s_next[tid] = (short)nx; s_prev[tid] = (short)pv;
    }
    __syncthreads();
    POLY_T(1);
    // a halfspace is clipped by the seed of its own sector and the two nearest seeds on either side; the interval only shrinks,
    // so once it is empty the halfspace is out, whatever other seeds would do
    every_sample([&](int i, double ax, double ay, double dm, int sec) {
        const int n1 = s_next[sec], p1 = s_prev[sec];
        const int at[5] = {sec, n1, p1, n1 >= 0 ? s_next[n1] : -1, p1 >= 0 ? s_prev[p1] : -1};
        PolyFrac w = {1.0, 0.0, -1.0, 0.0};
#pragma unroll
        for (int q = 0; q < 5; q++)
            if (at[q] >= 0 && poly_frac_alive(w) && s_seed[at[q]] != i) poly_clip_fast(w, ax, ay, dm, sd_ax[at[q]], sd_ay[at[q]], sd_dm[at[q]]);
        if (poly_frac_alive(w)) { const int e = atomicAdd(&s_nk, 1); if (e < cap) { c_ax[e] = ax; c_ay[e] = ay; c_dm[e] = dm; c_idx[e] = i; } }
    });
    __syncthreads();
    POLY_T(2);
    if (s_nk > cap) { if (tid == 0) overflow[1 + atomicAdd(&overflow[0], 1)] = unit; return; }          // (uniform: s_nk is final after the barrier; only in the first pass)
    // ---- filter, second round, on the list (~100 -> ~11): seeds = the closest candidate of each of 2048 sectors (pairwise comparison:
    //      the list is short; the sector rides in bits 13-23 of the index word), every seed clips every candidate -- G threads per
    //      candidate, each taking every G-th seed, the fractions combined over the G lanes --, then the list is compacted in place
    {
        const int nk1 = s_nk;
        for (int ci = tid; ci < nk1; ci += 256) c_idx[ci] |= poly_sector(c_ax[ci], c_ay[ci], 256) << 13;
        if (tid == 0) { s_ns = 0; s_nw = 0; }
        __syncthreads();
        // Seeds by table (round 6): one pass per octant over the 256 bins of the octant -- keys in s_best, the lowest sample index among equal keys in s_pick --
        // O(nk1) where the pairwise comparison of rounds 2-5 was O(nk1^2 / 256): the units that keep 300 - 600 candidates (stage 1 of a horizon: the 256
        // scenarios of an obstacle still nearly coincide) took 400 us and with them the whole launch, 27 % of cfg 5's step.  (Both forms behind a branch on nk1
        // cost the kernel 20 B of scratch more and the saturated launch 6 %: one form.)
        for (int oct = 0; oct < 8; oct++) {
            s_best[tid] = ~0ull; s_pick[tid] = POLY_NONE;
            __syncthreads();
            for (int ci = tid; ci < nk1; ci += 256) {
                const int sec = c_idx[ci] >> 13;
                if ((sec >> 8) == oct) atomicMin(&s_best[sec & 255], poly_key(c_dm[ci]));
            }
            __syncthreads();
            for (int ci = tid; ci < nk1; ci += 256) {
                const int me = c_idx[ci], sec = me >> 13;
                if ((sec >> 8) == oct && poly_key(c_dm[ci]) == s_best[sec & 255]) atomicMin(&s_pick[sec & 255], me & POLY_IDX_MASK);
            }
            __syncthreads();
            for (int ci = tid; ci < nk1; ci += 256) {
                const int me = c_idx[ci], i = me & POLY_IDX_MASK, sec = me >> 13;
                if ((sec >> 8) == oct && s_pick[sec & 255] == i) {   // (the round-1 seed table is free; seeds beyond its size are not used: a looser filter)
                    const int e = atomicAdd(&s_ns, 1);
                    if (e < POLY_SEC1) { sd_ax[e] = c_ax[ci]; sd_ay[e] = c_ay[ci]; sd_dm[e] = c_dm[ci]; s_seed[e] = i; }
                }
            }
            __syncthreads();
        }
        const int ns = s_ns < POLY_SEC1 ? s_ns : POLY_SEC1;
        int G = 1;
        while (G < 64 && 2 * G * nk1 <= 256) G *= 2;
        const int g = tid & (G - 1);
        for (int base = 0; base < nk1; base += 256 / G) {
            const int ci = base + tid / G;
            const bool valid = ci < nk1;
            const double ax = valid ? c_ax[ci] : 1.0, ay = valid ? c_ay[ci] : 0.0, dm = valid ? c_dm[ci] : 0.0;
            const int i = valid ? c_idx[ci] & POLY_IDX_MASK : -1;
            PolyFrac w = {1.0, 0.0, -1.0, 0.0};
            if (valid)
                for (int q = g; q < ns; q += G)
                    if (s_seed[q] != i) poly_clip_fast(w, ax, ay, dm, sd_ax[q], sd_ay[q], sd_dm[q]);
            for (int m = 1; m < G; m <<= 1) {                     // the lower upper bound, the higher lower bound
                const double onh = __shfl_xor(w.nh, m, 64), odh = __shfl_xor(w.dh, m, 64), onl = __shfl_xor(w.nl, m, 64), odl = __shfl_xor(w.dl, m, 64);
                if (onh * w.dh < w.nh * odh) { w.nh = onh; w.dh = odh; }
                if (onl * w.dl > w.nl * odl) { w.nl = onl; w.dl = odl; }
            }
            if (valid && g == 0 && !poly_frac_alive(w)) c_idx[ci] |= POLY_DROP_FLAG;
        }
        __syncthreads();
        POLY_T(4);
        for (int c0 = 0; c0 < nk1; c0 += 256) {                   // in-place compaction, chunk-wise: read, then append below the chunk
            const int ci = c0 + tid;
            double ax = 0.0, ay = 0.0, dm = 0.0; int me = POLY_DROP_FLAG;
            if (ci < nk1) { ax = c_ax[ci]; ay = c_ay[ci]; dm = c_dm[ci]; me = c_idx[ci]; }
            __syncthreads();
            if (!(me & POLY_DROP_FLAG)) { const int e = atomicAdd(&s_nw, 1); c_ax[e] = ax; c_ay[e] = ay; c_dm[e] = dm; c_idx[e] = me & POLY_IDX_MASK; }
            __syncthreads();
        }
        if (tid == 0) s_nk = s_nw;
        __syncthreads();
    }
    POLY_T(5);
    // ---- edge test among the candidates, G threads per candidate (G = 256 / candidates, rounded down to a power of two): each takes
    //      every G-th of the other candidates, then min / max / or across the G lanes.  Every candidate clips every other, like in
    //      the mirror, and a quotient is the same whichever thread computes it, so the split does not change the result.  A
    //      candidate found redundant stays in the list as ~index (readers decode it): it still clips the others.
    const int nk = s_nk;
    // G by cost (round 6): trips x (clips per thread + combination) = ceil(nk G / 256) (ceil(nk / G) + ...).  One thread per candidate (the rule until round 5 for nk > 128) leaves a long
    // list -- stage 1 of a horizon, where the 256 scenarios of an obstacle still nearly coincide and ~300 nearly parallel candidates pass the filter -- with two
    // trips of nk sequential clips, the second with 44 busy threads: the tail of the whole launch.  (A pre-test against the seeds alone was tried and prunes nothing
    // there: the near-duplicates of an edge are near-edges.)
    int G = 1;
    {
        int best = ((nk + 255) / 256) * nk * 100;                    // (a clip ~ 100 instructions, a combination step over the G lanes ~ 15)
        for (int cand = 2, lg = 1; cand <= 64; cand *= 2, lg++) {
            const int cost = ((nk * cand + 255) / 256) * (((nk + cand - 1) / cand) * 100 + 15 * lg);
            if (cost < best) { best = cost; G = cand; }
        }
    }
    const int g = tid & (G - 1);
    for (int base = 0; base < nk; base += 256 / G) {                 // (several trips when nk G > 256)
        const int ci = base + tid / G;
        const bool valid = ci < nk;
        const int i = valid ? c_idx[ci] : -1;                         // (entry ci is rewritten only below, by this group)
        const double ai1 = valid ? c_ax[ci] : 1.0, ai2 = valid ? c_ay[ci] : 0.0, dmi = valid ? c_dm[ci] : 0.0;
        PolyClip w = {-HUGE_VAL, HUGE_VAL, false};
        if (valid)
            for (int cj = g; cj < nk; cj += G) {
                int j = c_idx[cj];
                j = j < 0 ? ~j : j;
                if (cj != ci) poly_clip(w, ai1, ai2, dmi, i, c_ax[cj], c_ay[cj], c_dm[cj], j);
            }
        int kill = w.kill ? 1 : 0;
        for (int m = 1; m < G; m <<= 1) {
            const double hi = __shfl_xor(w.hi, m, 64), lo = __shfl_xor(w.lo, m, 64);
            w.hi = hi < w.hi ? hi : w.hi; w.lo = lo > w.lo ? lo : w.lo; kill |= __shfl_xor(kill, m, 64);
        }
        if (valid && g == 0) {
            if (!kill && w.hi - w.lo > POLY_TOL_EDGE) atomicAdd(&s_ne, 1);
            else c_idx[ci] = ~i;
        }
    }
    __syncthreads();
    POLY_T(6);
    // ---- rows: an edge's row is its rank by (margin, sample index)
    for (int ci = tid; ci < nk; ci += 256) {
        const int i = c_idx[ci];
        if (i < 0) continue;
        const double dmi = c_dm[ci];
        int rank = 0;
        for (int cj = 0; cj < nk; cj++) {
            const int j = c_idx[cj];
            if (j >= 0 && (c_dm[cj] < dmi || (c_dm[cj] == dmi && j < i))) rank++;
        }
        if (rank < n_rows) {
            const double2 q = o[i];
            const double a1 = c_ax[ci], a2 = c_ay[ci];
            p[where.slk(d, rank, 0)] = a1; p[where.slk(d, rank, 1)] = a2; p[where.slk(d, rank, 2)] = a1 * q.x + a2 * q.y - radius;
            which[rank] = i;
        }
    }
    POLY_T(7);
    int n_real = s_ne;
    if (s_ne == 0 && n_pts > 0) {
        // EMPTY polygon: the halfspaces contradict each other (the guess sits in the overlap of inflated discs on opposite sides).
        // Leaving the stage unconstrained would certify the most dangerous geometry as safe, so the stage keeps the n_rows CLOSEST
        // halfspaces of all samples (lowest index on ties) -- contradictory rows: the QP is infeasible, or pays slack, and the solve
        // reports it -- and the unit is counted in empty_stages[b] (tmpc_scenario_empty_stages), which the callers turn into "not
        // eligible".  n_rows rounds of a block-wide argmin over (margin, index) above the previous pick; a rare path.
        unsigned long long prev_key = 0ull; int prev_idx = -1;
        const int rounds = n_rows < n_pts ? n_rows : n_pts;
        for (int r = 0; r < rounds; r++) {
            if (tid == 0) { s_best[0] = ~0ull; s_seed[0] = POLY_NONE; }
            __syncthreads();
            every_sample([&](int i, double, double, double dm, int) {
                const unsigned long long key = poly_key(dm);
                if (prev_idx < 0 || key > prev_key || (key == prev_key && i > prev_idx)) atomicMin(&s_best[0], key);
            });
            __syncthreads();
            every_sample([&](int i, double, double, double dm, int) {
                const unsigned long long key = poly_key(dm);
                if (key == s_best[0] && (prev_idx < 0 || key > prev_key || i > prev_idx)) atomicMin(&s_seed[0], i);
            });
            __syncthreads();
            every_sample([&](int i, double ax, double ay, double, int) {
                if (i == s_seed[0]) {
                    const double2 q = o[i];
                    p[where.slk(d, r, 0)] = ax; p[where.slk(d, r, 1)] = ay; p[where.slk(d, r, 2)] = ax * q.x + ay * q.y - radius;
                    which[r] = i;
                }
            });
            prev_key = s_best[0]; prev_idx = s_seed[0];
            __syncthreads();
        }
        n_real = rounds;
        if (tid == 0 && empty_stages) atomicAdd(&empty_stages[b], 1);
    }
    if (tid < n_rows && tid >= n_real) { p[where.slk(d, tid, 0)] = 1.0; p[where.slk(d, tid, 1)] = 0.0; p[where.slk(d, tid, 2)] = state_x[sc] + 100.0; which[tid] = -1; }
}


// The candidate list (`cap` entries of dynamic LDS) is what bounds the workgroups per CU, and the filter leaves ~100 candidates of 2048
// samples: the first pass (one workgroup per unit) runs with a short list (POLY_LIST_CAP) and records the rare unit whose candidates do
// not fit (overflow[0] = their number, overflow[1..] = the units); the second pass, a few workgroups with room for every sample, redoes
// only those.
template <class Where>
__device__ __forceinline__ void poly_units(const Where &where, const Dims &d, int B, const double *x0, double *params, const double *samples, int n_pts, int n_rows,
                                           const int *scene_of, const double *state_x, double radius, double disc_offset, int *row_sample, int cap, int *overflow,
                                           int second_pass, int *empty_stages, const unsigned char *discard, int n_scen)
{
    const int n_units = second_pass ? overflow[0] : B * d.N;
    for (int q = blockIdx.x; q < n_units; q += gridDim.x) {      // (first pass: one unit per workgroup)
        poly_stage(where, second_pass ? overflow[1 + q] : q, d, B, x0, params, samples, n_pts, n_rows, scene_of, state_x, radius, disc_offset, row_sample, cap, overflow, empty_stages, discard, n_scen);
        __syncthreads();                                          // (the LDS tables are reused by the next unit)
    }
}
__global__ __launch_bounds__(256, 4) void tmpc_scenario_halfspaces_kernel(Dims d, int B, const double *x0, double *params,
                                                                       const double *samples, int n_pts, int n_rows,
                                                                       const int *scene_of, const double *state_x,
                                                                       double radius, double disc_offset, int *row_sample, int cap, int *overflow, int second_pass,
                                                                       int *empty_stages, const unsigned char *discard, int n_scen)
{
    poly_units(LayoutEnvRows{0}, d, B, x0, params, samples, n_pts, n_rows, scene_of, state_x, radius, disc_offset, row_sample, cap, overflow, second_pass, empty_stages, discard, n_scen);
}
// the same stages into the caller's columns (tmpc_stack_scenario_halfspaces): a function of its own, so its static LDS and its dynamic-LDS
// attribute are its own too (csrc/tmpc_stack_scenario.hpp applies both to the kernel it launches)
__global__ __launch_bounds__(256, 4) void tmpc_scenario_halfspaces_columns_kernel(Dims d, int B, const double *x0, double *params,
                                                                               const double *samples, int n_pts, int n_rows,
                                                                               const int *scene_of, const double *state_x,
                                                                               double radius, double disc_offset, int *row_sample, int cap, int *overflow, int second_pass,
                                                                               int *empty_stages, const unsigned char *discard, int n_scen, ColumnEnvRows where)
{
    poly_units(where, d, B, x0, params, samples, n_pts, n_rows, scene_of, state_x, radius, disc_offset, row_sample, cap, overflow, second_pass, empty_stages, discard, n_scen);
}


// Support of a scenario program's solution (the scenarios whose constraints are active at it; SH-MPC bounds the collision
// probability of the plan through the size of this set -- ScenarioSolver::support / ::status, scenario_constraints.h:38-40; the
// scenario_module that fills them is absent, so this restates the definition of the method the reference cites, README.md:22):
// scenario s = sample index % n_scenarios (samples are [obstacle][scenario]: one scenario is one joint draw of all obstacles over
// the horizon); a row is active when  a.p_disc - (b + slack) >= -tol  at the solution.  One wave per trajectory; the set is a
// bitmask in LDS.  support[b] = number of distinct active scenarios, active_rows[b] = number of active rows.
// Where: the rows and ego_disc_0_offset are read at the layout's offsets or at the caller's columns, like poly_stage writes them.
template <class Where>
__device__ __forceinline__ void scenario_support_rows(const Where &where, const Dims &d, int B, const double *params, const double *xtraj, const int *row_sample,
                                                      int n_rows, int n_scenarios, double tol, int *support, int *active_rows)
{
#pragma clang fp contract(off)
    __shared__ unsigned int s_mask[256];                                // up to 8192 scenarios
    __shared__ int s_rows;
    const int b = blockIdx.x, tid = threadIdx.x, N = d.N, nxe = ext_nx(d);
    if (b >= B) return;
    for (int w = tid; w < 256; w += 64) s_mask[w] = 0u;
    if (tid == 0) s_rows = 0;
    __syncthreads();
    for (int e = tid; e < (N - 1) * n_rows; e += 64) {
        const int k = 1 + e / n_rows, r = e - (k - 1) * n_rows;
        const int smp = row_sample[((size_t)b * N + k) * n_rows + r];
        if (smp < 0) continue;
        const double *p = params + ((size_t)b * N + k) * d.npar;
        const double *x = xtraj + ((size_t)b * (N + 1) + k) * nxe;
        const double off = p[where.disc_offset(d)], slack = d.slack ? x[NX] : 0.0;
        const double px = x[0] + off * cos(x[2]), py = x[1] + off * sin(x[2]);
        const double h = p[where.slk(d, r, 0)] * px + p[where.slk(d, r, 1)] * py - (p[where.slk(d, r, 2)] + slack);
        if (h >= -tol) {
            const int s = smp % n_scenarios;
            atomicOr(&s_mask[s >> 5], 1u << (s & 31));
            atomicAdd(&s_rows, 1);
        }
    }
    __syncthreads();
    int cnt = 0;
    for (int w = tid; w < 256; w += 64) cnt += __popc(s_mask[w]);
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
    if (tid == 0) { support[b] = cnt; if (active_rows) active_rows[b] = s_rows; }
}
__global__ __launch_bounds__(64) void tmpc_scenario_support_kernel(Dims d, int B, const double *params, const double *xtraj, const int *row_sample,
                                                                  int n_rows, int n_scenarios, double tol, int *support, int *active_rows)
{
    scenario_support_rows(LayoutEnvRows{0}, d, B, params, xtraj, row_sample, n_rows, n_scenarios, tol, support, active_rows);
}
__global__ __launch_bounds__(64) void tmpc_scenario_support_columns_kernel(Dims d, int B, const double *params, const double *xtraj, const int *row_sample,
                                                                          int n_rows, int n_scenarios, double tol, int *support, int *active_rows, ColumnEnvRows where)
{
    scenario_support_rows(where, d, B, params, xtraj, row_sample, n_rows, n_scenarios, tol, support, active_rows);
}


// ---- free-space decomposition on device: DecompConstraints::update (decomp_constraints.cpp:52-148) ---------------------------------------
// DecompUtil is not in the reference tree: upstream DecompUtil's LineSegment algorithm is restated in the frame of the segment, DESIGN.md U16.
// The arithmetic is tmpc_arith's decomp_*, the source mpc_planner_modules/free_space.h compiles too: every output is bit-equal to the
// independent modules.py::costmap_points / decomp_halfspaces.
constexpr int DECOMP_THREADS = 256, DECOMP_MAX_POINTS = 16384, DECOMP_MAX_ROWS = 64, COSTMAP_MAX_CELLS = 1 << 20;

// getOccupiedGridCells (:122-148).  one workgroup per scene q: the cells in the reference's order e = mx size_y + my (mx outer, my inner), 256 per
// sweep; an occupied cell's place in the list = occupied cells before the sweep + those of the lower waves (four counts through LDS) + those of
// the lower lanes of its wave (popcount of the ballot below the lane): an order-preserving compaction without atomics.  The first n_pts_max
// are written, nothing at or beyond count; the sweeps stop once the list has overflowed.
__global__ __launch_bounds__(DECOMP_THREADS) void tmpc_costmap_points_kernel(int size_x, int size_y, double resolution, int n_pts_max, const uint8_t *cost,
                                                                           const double *origin, double *points, int *count, uint8_t *overflow)
{
    __shared__ int s_wave[2][4];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_cells = size_x * size_y;
    const uint8_t *cq = cost + (size_t)q * n_cells;
    const double ox = origin[(size_t)q * 2], oy = origin[(size_t)q * 2 + 1];
    double *pq = points + (size_t)q * n_pts_max * 2;
    int total = 0;
    for (int base = 0, it = 0; base < n_cells && total <= n_pts_max; base += DECOMP_THREADS, it++) {
        const int e = base + tid;
        int mx = 0, my = 0;
        bool occ = false;
        if (e < n_cells) { mx = e / size_y; my = e - mx * size_y; occ = cq[(size_t)my * size_x + mx] != 0; }
        const unsigned long long m = __ballot(occ);
        if (lane == 0) s_wave[it & 1][wave] = __popcll(m);
        __syncthreads();                                                  // (double-buffered counts: one barrier per sweep)
        int before = total, all = 0;
        for (int w = 0; w < 4; w++) { const int c = s_wave[it & 1][w]; all += c; if (w < wave) before += c; }
        const int at = before + __popcll(m & ((1ull << lane) - 1ull));
        if (occ && at < n_pts_max) {
            pq[(size_t)at * 2] = tmpc_arith::cell_centre(ox, mx, resolution);
            pq[(size_t)at * 2 + 1] = tmpc_arith::cell_centre(oy, my, resolution);
        }
        total += all;
    }
    if (tid == 0) {
        count[q] = total < n_pts_max ? total : n_pts_max;
        if (overflow) overflow[q] = total > n_pts_max ? 1 : 0;
    }
}

// the (key, index) argmin of a workgroup of four waves: lexicographic, so the result does not depend on the order of the reduction; index
// DECOMP_NONE = nobody.  s_key / s_idx: four partials; the barrier in front protects them from the previous call's readers.
constexpr int DECOMP_NONE = 0x7fffffff;
__device__ inline void decomp_block_argmin(double &key, int &idx, double *s_key, int *s_idx)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double ok = __shfl_xor(key, o, 64); const int oi = __shfl_xor(idx, o, 64);
        if (ok < key || (ok == key && oi < idx)) { key = ok; idx = oi; }
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { s_key[threadIdx.x >> 6] = key; s_idx[threadIdx.x >> 6] = idx; }
    __syncthreads();
    key = s_key[0]; idx = s_idx[0];
#pragma unroll
    for (int w = 1; w < 4; w++) {
        const double ok = s_key[w]; const int oi = s_idx[w];
        if (ok < key || (ok == key && oi < idx)) { key = ok; idx = oi; }
    }
}

// P(s) on a whole path (n segments, rows of 9, `len` the last knot): the cubic of segment i = max{j < n : start_j <= s} (0 below the first knot)
// at t = s - start_i; from `len` on straight along the end tangent (U14-3).  The lookup runs over all lanes; s_key / s_idx as above.
__device__ inline void decomp_path_point(const double *pq, int n, double len, double s, double &x, double &y, double *s_key, int *s_idx)
{
    if (s >= len) {
        double ex, ey, edx, edy;
        tmpc_arith::cubic(pq + (size_t)(n - 1) * 9, len - pq[(size_t)(n - 1) * 9 + 8], ex, ey, edx, edy);
        x = tmpc_arith::continue_straight(ex, edx, s, len); y = tmpc_arith::continue_straight(ey, edy, s, len);
        return;
    }
    int i = 0;
    for (int j = threadIdx.x; j < n; j += DECOMP_THREADS) if (pq[(size_t)j * 9 + 8] <= s) i = j;
    double key = 0.0; int neg = -i;                                        // the largest i = the smallest -i
    decomp_block_argmin(key, neg, s_key, s_idx);
    i = -neg;
    double dx, dy;
    tmpc_arith::cubic(pq + (size_t)i * 9, s - pq[(size_t)i * 9 + 8], x, y, dx, dy);
}

// one workgroup per (scene q, stage k).  Stage 0: dummies, count 0, status 0.  Stage k >= 1: the segment P(s_{k-1}) -> P(s_k) with s_0 = s0[q],
// s_{j+1} = s_j + v_j dt, v_j the warm start of batch entry main_of[q] (`_solver->getEgoPrediction(j, "v")`, :79).  The scene's points (count
// clipped to [0, n_pts_max]) are streamed from global memory on every pass and u, w, d2 recomputed, never stored; point i belongs to lane
// i % 64 of wave (i / 64) % 4, which keeps its bit of the three sets (box, inside the ellipse, remaining) in LDS words only that wave touches
// -- a ballot per 64 points, no atomics.  A wave skips a word that is empty.  The ellipse loop removes at least the chosen point per pass, the
// polygon loop ends after n_rows rows: no loop without a bound.  Every lane computes the frame, the ellipse and the rows from the same
// values in the same order, so they agree without a broadcast.
__global__ __launch_bounds__(DECOMP_THREADS) void tmpc_decomp_halfspaces_kernel(Dims d, int B, int n_scenes, const double *x0, const int *main_of, int n_seg_max,
                                                                              const double *path, const int *path_count, const double *path_length,
                                                                              const double *s0, const double *state_x, const double *points, const int *count,
                                                                              int n_pts_max, double R, int n_rows, double *rows, int *row_count, uint8_t *status)
{
#pragma clang fp contract(off)
    __shared__ unsigned long long s_box[DECOMP_MAX_POINTS / 64], s_set[DECOMP_MAX_POINTS / 64];
    __shared__ double s_key[4], s_row[(DECOMP_MAX_ROWS + 4) * 3];
    __shared__ int s_idx[4], s_written;
    const int N = d.N, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x / N, k = blockIdx.x - q * N;
    if (q >= n_scenes) return;
    const int b = main_of[q];
    int n = path_count[q];
    n = n > n_seg_max ? n_seg_max : n;
    if (b < 0 || b >= B || n <= 0) return;                               // (uniform over the workgroup: nothing is read, nothing written)
    const size_t unit = (size_t)q * N + k;
    double *out = rows + unit * n_rows * 3;
    const double dummy_b = tmpc_arith::dummy_coordinate(state_x[q]);
    int found = 0, limit = 0;
    bool valid = false;
    if (k > 0) {
        int cnt = count[q];
        cnt = cnt < 0 ? 0 : (cnt > n_pts_max ? n_pts_max : cnt);
        const double *pts = points + (size_t)q * n_pts_max * 2;
        const double *pq = path + (size_t)q * n_seg_max * 9;
        const double len = path_length[q];
        double s = s0[q];
        for (int j = 0; j < k - 1; j++) s = tmpc_arith::advance(s, x0[((size_t)b * (N + 1) + j) * ext_nv(d) + ZV], d.dt);
        const double s_next = tmpc_arith::advance(s, x0[((size_t)b * (N + 1) + (k - 1)) * ext_nv(d) + ZV], d.dt);
        double p1x, p1y, p2x, p2y, ex, ey, cx, cy, f;
        decomp_path_point(pq, n, len, s, p1x, p1y, s_key, s_idx);
        decomp_path_point(pq, n, len, s_next, p2x, p2y, s_key, s_idx);
        valid = tmpc_arith::decomp_frame(p1x, p1y, p2x, p2y, ex, ey, cx, cy, f);
        if (valid) {
            const int n_words = (cnt + 63) >> 6;
            double a = f, bb = f;
            for (int c = wave; c < n_words; c += 4) {
                const int i = c * 64 + lane;
                bool in_box = false, inside = false;
                if (i < cnt) {
                    double u, w;
                    tmpc_arith::decomp_local(pts[(size_t)i * 2], pts[(size_t)i * 2 + 1], cx, cy, ex, ey, u, w);
                    in_box = tmpc_arith::decomp_in_box(u, w, f, R);
                    inside = in_box && tmpc_arith::decomp_inside_first(tmpc_arith::decomp_d2(u, w, a, bb));
                }
                const unsigned long long mb = __ballot(in_box), mi = __ballot(inside);
                if (lane == 0) { s_box[c] = mb; s_set[c] = mi; }
            }
            __syncthreads();                                                 // (after every rewrite of the sets: the words are read again below)
            // the ellipse: shrink through the closest inside point until none is left
            for (int pass = 0; pass < cnt; pass++) {
                double key = __builtin_huge_val(); int idx = DECOMP_NONE;
                for (int c = wave; c < n_words; c += 4) {
                    const unsigned long long m = s_set[c];
                    if (m == 0ull) continue;
                    const int i = c * 64 + lane;
                    if ((m >> lane) & 1ull) {
                        double u, w;
                        tmpc_arith::decomp_local(pts[(size_t)i * 2], pts[(size_t)i * 2 + 1], cx, cy, ex, ey, u, w);
                        const double kk = tmpc_arith::decomp_key(tmpc_arith::decomp_d2(u, w, a, bb));
                        if (kk < key || idx == DECOMP_NONE) { key = kk; idx = i; }      // ascending i per lane: strict '<' keeps the lowest index
                    }
                }
                decomp_block_argmin(key, idx, s_key, s_idx);
                if (idx == DECOMP_NONE) break;
                double us, ws;
                tmpc_arith::decomp_local(pts[(size_t)idx * 2], pts[(size_t)idx * 2 + 1], cx, cy, ex, ey, us, ws);
                bb = tmpc_arith::decomp_shrink(us, ws, a, bb);
                for (int c = wave; c < n_words; c += 4) {
                    const unsigned long long m = s_set[c];
                    if (m == 0ull) continue;
                    const int i = c * 64 + lane;
                    bool keep = false;
                    if ((m >> lane) & 1ull) {
                        double u, w;
                        tmpc_arith::decomp_local(pts[(size_t)i * 2], pts[(size_t)i * 2 + 1], cx, cy, ex, ey, u, w);
                        keep = i != idx && tmpc_arith::decomp_inside(tmpc_arith::decomp_d2(u, w, a, bb));
                    }
                    const unsigned long long mk = __ballot(keep);
                    if (lane == 0) s_set[c] = mk;
                }
                __syncthreads();
            }
            // the polygon: the tangent row through the closest remaining point, which removes everything behind it
            for (int c = wave; c < n_words; c += 4) if (lane == 0) s_set[c] = s_box[c];
            __syncthreads();
            for (; found < n_rows; found++) {
                double key = __builtin_huge_val(); int idx = DECOMP_NONE;
                for (int c = wave; c < n_words; c += 4) {
                    const unsigned long long m = s_set[c];
                    if (m == 0ull) continue;
                    const int i = c * 64 + lane;
                    if ((m >> lane) & 1ull) {
                        double u, w;
                        tmpc_arith::decomp_local(pts[(size_t)i * 2], pts[(size_t)i * 2 + 1], cx, cy, ex, ey, u, w);
                        const double kk = tmpc_arith::decomp_key(tmpc_arith::decomp_d2(u, w, a, bb));
                        if (kk < key || idx == DECOMP_NONE) { key = kk; idx = i; }
                    }
                }
                decomp_block_argmin(key, idx, s_key, s_idx);
                if (idx == DECOMP_NONE) break;
                const double sx = pts[(size_t)idx * 2], sy = pts[(size_t)idx * 2 + 1];
                double us, ws, nx, ny, beta;
                tmpc_arith::decomp_local(sx, sy, cx, cy, ex, ey, us, ws);
                tmpc_arith::decomp_row(us, ws, a, bb, ex, ey, sx, sy, nx, ny, beta);
                for (int c = wave; c < n_words; c += 4) {
                    const unsigned long long m = s_set[c];
                    if (m == 0ull) continue;
                    const int i = c * 64 + lane;
                    bool keep = false;
                    if ((m >> lane) & 1ull)
                        keep = i != idx && tmpc_arith::decomp_side(nx, ny, pts[(size_t)i * 2], pts[(size_t)i * 2 + 1], sx, sy) < 0.0;
                    const unsigned long long mk = __ballot(keep);
                    if (lane == 0) s_set[c] = mk;
                }
                __syncthreads();
                tmpc_arith::decomp_flip(cx, cy, nx, ny, beta);
                if (tid == 0) { s_row[found * 3] = nx; s_row[found * 3 + 1] = ny; s_row[found * 3 + 2] = beta; }
            }
            if (tid == 0) tmpc_arith::decomp_box_rows(p1x, p1y, p2x, p2y, ex, ey, R, s_row + found * 3);
            found += 4;
            limit = found < n_rows ? found : n_rows;
        }
    }
    // the copy (:90-114): rows until the first terminator, dummies behind it
    if (tid == 0) {
        int written = 0;
        while (written < limit && !tmpc_arith::decomp_terminator(s_row[written * 3], s_row[written * 3 + 1])) written++;
        s_written = written;
        row_count[unit] = written;
        status[unit] = k == 0 ? 0 : (!valid || written < limit) ? 2 : (found > n_rows ? 1 : 0);
    }
    __syncthreads();
    const int written = s_written;
    for (int e = tid; e < n_rows * 3; e += DECOMP_THREADS) {
        const int r = e / 3, col = e - r * 3;
        out[e] = r < written ? s_row[e] : (col == 0 ? 1.0 : col == 1 ? 0.0 : dummy_b);
    }
}

// DecompConstraints::setParameters (:150-189) from tmpc_decomp_halfspaces_kernel's rows: one thread per (trajectory, stage, row): row r of stage k
// of scene scene_of[b] into slack row first_row + r of entry b, and ego_disc_0_offset; an entry whose scene is outside [0, n_scenes) is left
// untouched.  Nothing else is written.
template <class Where>
__device__ __forceinline__ void set_halfspace_rows(const Where &where, const Dims &d, int B, double *params, const double *rows, int n_rows,
                                                   const int *scene_of, int n_scenes, double disc_offset)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = d.N;
    if (e >= B * N * n_rows) return;
    const int r = e % n_rows, k = (e / n_rows) % N, b = e / (n_rows * N);
    const int sc = scene_of[b];
    if (sc < 0 || sc >= n_scenes) return;
    double *p = params + ((size_t)b * N + k) * d.npar;
    const double *src = rows + (((size_t)sc * N + k) * n_rows + r) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) p[where.slk(d, r, c)] = src[c];
    if (r == 0) p[where.disc_offset(d)] = disc_offset;
}
__global__ void tmpc_set_halfspace_rows_kernel(Dims d, int B, double *params, const double *rows, int n_rows, int first_row, const int *scene_of,
                                               int n_scenes, double disc_offset)
{
    set_halfspace_rows(LayoutEnvRows{first_row}, d, B, params, rows, n_rows, scene_of, n_scenes, disc_offset);
}
// the same rows into the caller's columns (tmpc_stack_set_halfspace_columns): where.t.col[0] the disc offset, where.t.col[1 + 3 r + c] row r
__global__ void tmpc_set_halfspace_columns_kernel(Dims d, int B, double *params, const double *rows, int n_rows, const int *scene_of, int n_scenes,
                                                  double disc_offset, ColumnEnvRows where)
{
    set_halfspace_rows(where, d, B, params, rows, n_rows, scene_of, n_scenes, disc_offset);
}

// ---- f-2: cross-tick state on device ------------------------------------------------------------------------------
// Warm start of the next tick from the previous tick's solution, without a host round trip.  One thread per
// (trajectory, node).  mode[b]:
//   0  leave x0[b] alone (the caller loads a guidance trajectory, tmpc_init_with_guidance)
//   1  Solver::initializeWarmstart(state, shift = true)   (acados_solver_interface.cpp:344-364):
//        [state, out_2, ..., out_{N-1}, out_{N-1}, out_{N-1}]
//   2  Solver::initializeWarmstart(state, shift = false)  (:365-375): x0[k] = out_k for k < N
//   3  Solver::initializeWithBraking(state)               (:303-342): constant deceleration roll-out
// out_k is the previous solution of trajectory src[b] (src = NULL: b itself -- a planner re-uses its own last output,
// guidance_constraints.cpp:310-311).  xinit[b] <- state[b] (Solver::setXinit).
// In mode 1 the reference fills the INPUT entries of node 0 from State::get(<input name>), which indexes the state
// vector at -2 / -1 (state.cpp:21-24: index - nu) -- an out-of-bounds read; this restatement writes 0 there.
__global__ void tmpc_warmstart_kernel(Dims d, int B, const double *state, const int *mode, const int *src, const double *xtraj,
                                      const double *utraj, double *x0, double *xinit, double decel)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = d.N, nxe = ext_nx(d), nve = ext_nv(d);
    if (e >= B * (N + 1)) return;
    const int b = e / (N + 1), k = e - b * (N + 1);
    const double *st = state + (size_t)b * nxe;
    if (k == 0) for (int i = 0; i < nxe; i++) xinit[(size_t)b * nxe + i] = st[i];
    const int m = mode ? mode[b] : 1;
    if (m == 0) return;
    double *z = x0 + ((size_t)b * (N + 1) + k) * nve;
    const int sb = src ? src[b] : b;
    const double *xo = xtraj + (size_t)sb * (N + 1) * nxe, *uo = utraj + (size_t)sb * N * NU;
    if (m == 1) {
        if (k == 0) {
            for (int i = 0; i < NU; i++) z[i] = 0.0;
            for (int i = 0; i < nxe; i++) z[NU + i] = st[i];
        } else {
            const int ko = (k >= N - 1) ? N - 1 : k + 1;
            for (int i = 0; i < NU; i++) z[i] = uo[ko * NU + i];
            for (int i = 0; i < nxe; i++) z[NU + i] = xo[ko * nxe + i];
        }
    } else if (m == 2) {
        if (k < N) {
            for (int i = 0; i < NU; i++) z[i] = uo[k * NU + i];
            for (int i = 0; i < nxe; i++) z[NU + i] = xo[k * nxe + i];
        }
    } else if (m == 3) {
        double x = st[0], y = st[1], v = st[3], spline = st[4];
        const double psi = st[2], a = -fabs(decel);
        double sn, cs;
        sincos(psi, &sn, &cs);
        for (int j = 1; j <= k; j++) {                       // same recursion order as the reference's loop (:322-331)
            x += v * d.dt * cs; y += v * d.dt * sn; spline += v * d.sdt;      // (sdt = 0: the model without a spline state keeps its padded slot)
            v += a * d.dt; v = fmax(v, 0.0);
        }
        z[ZA] = a; z[ZW] = 0.0; z[ZX] = x; z[ZY] = y; z[ZPSI] = psi; z[ZV] = v; z[ZS] = spline;
        for (int i = NX; i < nxe; i++) z[NU + i] = st[i];    // initializeWithState: remaining states = initial state
    }
}

// GuidanceConstraints::initializeSolverWithGuidance (guidance_constraints.cpp:390-414): k = 1..N-1: x, y from the guidance
// trajectory at t = k dt, psi = atan2(vy, vx), v = |vel|.  gpos / gvel: [B][N+1][2]; enabled[b] == 0 skips b.
__global__ void tmpc_init_with_guidance_kernel(Dims d, int B, const double *gpos, const double *gvel, const uint8_t *enabled, double *x0)
{
#pragma clang fp contract(off)
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = d.N;
    if (e >= B * (N + 1)) return;
    const int b = e / (N + 1), k = e - b * (N + 1);
    if (k < 1 || k > N - 1 || (enabled && !enabled[b])) return;
    double *z = x0 + ((size_t)b * (N + 1) + k) * ext_nv(d);
    const double vx = gvel[(size_t)e * 2], vy = gvel[(size_t)e * 2 + 1];
    z[ZX] = gpos[(size_t)e * 2]; z[ZY] = gpos[(size_t)e * 2 + 1];
    z[ZPSI] = atan2(vy, vx);
    z[ZV] = sqrt(vx * vx + vy * vy);
}

// ---- persistent state: a solve that did not succeed resets the reference's capsule (Solver_acados_reset + reset_qp_memory,
// acados_solver_interface.cpp:187-191): the slot's multipliers go back to zero (the primal iterate is overwritten by the next
// loadWarmstart anyway) ----
__global__ void tmpc_state_finalize_kernel(int n_pi, int n_lam, const int *__restrict__ exit_code, double *__restrict__ pi,
                                           double *__restrict__ lamh, const int *__restrict__ slot)
{
    const int b = blockIdx.x;
    if (exit_code[b] == 1) return;
    const int sb = slot ? slot[b] : b;                      // the batch entry's state slot (tmpc_set_slots)
    for (int e = threadIdx.x; e < n_pi; e += blockDim.x) pi[(size_t)sb * n_pi + e] = 0.0;
    for (int e = threadIdx.x; e < n_lam; e += blockDim.x) lamh[(size_t)sb * n_lam + e] = 0.0;
}

// ---- debug: stage functions on device -----------------------------------------------------------
__global__ void tmpc_debug_eval_kernel(Dims d, int n, const double *z, const double *p, const double *pi, const double *lamh,
                                       double *cost, double *cgrad, double *chess, double *hval, double *hjac,
                                       double *xnext, double *xjac, double *lag, double *mir)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int nh = d.n_up + d.M;
    const double *ze = z + (size_t)e * ext_nv(d); const double *pe = p + (size_t)e * d.npar;
    double zz[NV];
    for (int i = 0; i < NV; i++) zz[i] = ze[i];
    const double slack = d.slack ? ze[NV] : 0.0;
    // rows are reported in the reference's order [topology | ellipsoids | slack rows] (module order)
    auto ext = [&](int r) { return r < d.n_lin ? r : (r < d.n_up ? d.M + r : r - d.n_slk); };
    double Wc[NV][NV], cg[NV];
    for (int i = 0; i < NV; i++) for (int j = 0; j < NV; j++) Wc[i][j] = 0.0;
#ifndef TMPC_GENERATED_STAGE
    if (d.cost_model == 1) {
        CostOutCA co;
        cost_eval_ca(d, zz, pe, 1, co, true, slack);
        cost[e] = co.val;
        cost_add_hessian_ca(co, 1.0, Wc);
        for (int i = 0; i < NV; i++) cg[i] = co.g[i];
    } else
#endif
    {
        CostOut co;
        cost_eval(d, zz, pe, 1, co, true, slack);
        cost[e] = co.val;
        cost_add_hessian(co, 1.0, Wc);
        for (int i = 0; i < NV; i++) cg[i] = co.g[i];
    }
    for (int i = 0; i < NV; i++) {
        cgrad[(size_t)e * NV + i] = cg[i];
        for (int j = 0; j < NV; j++) chess[(size_t)e * NV * NV + i * NV + j] = Wc[i][j];
    }
    double W[NV][NV], g[NV], BA[NX * NV], xn[NX];
    auto lam = [&](int r) { return lamh ? lamh[(size_t)e * nh + ext(r)] : 0.0; };
    auto sink = [&](int r, const RowOut &ro) {
        hval[(size_t)e * nh + ext(r)] = ro.h;
        double *J = hjac + ((size_t)e * nh + ext(r)) * NV;
        for (int i = 0; i < NV; i++) J[i] = 0.0;
        J[ZX] = ro.gx; J[ZY] = ro.gy; J[ZPSI] = ro.gp;
    };
#ifndef TMPC_GENERATED_STAGE
    if (d.cost_model == 1 && d.row_model == 1) stage_linearise<3>(d, zz, pe, 1, pi ? pi[(size_t)e * NX] : 0.0, pi ? pi[(size_t)e * NX + 1] : 0.0, lam, sink, W, g, BA, xn, slack);
    else if (d.cost_model == 1) stage_linearise<1>(d, zz, pe, 1, pi ? pi[(size_t)e * NX] : 0.0, pi ? pi[(size_t)e * NX + 1] : 0.0, lam, sink, W, g, BA, xn, slack);
    else if (d.row_model == 1) stage_linearise<2>(d, zz, pe, 1, pi ? pi[(size_t)e * NX] : 0.0, pi ? pi[(size_t)e * NX + 1] : 0.0, lam, sink, W, g, BA, xn, slack);
    else
#endif
    stage_linearise(d, zz, pe, 1, pi ? pi[(size_t)e * NX] : 0.0, pi ? pi[(size_t)e * NX + 1] : 0.0, lam, sink, W, g, BA, xn, slack);
    for (int i = 0; i < NX; i++) xnext[(size_t)e * NX + i] = xn[i];
    for (int i = 0; i < NX * NV; i++) xjac[(size_t)e * NX * NV + i] = BA[i];
    for (int i = 0; i < NV; i++) for (int j = 0; j < NV; j++) lag[(size_t)e * NV * NV + i * NV + j] = W[i][j];
    mirror7(W, d.reg_eps);
    for (int i = 0; i < NV; i++) for (int j = 0; j < NV; j++) mir[(size_t)e * NV * NV + i * NV + j] = W[i][j];
}

}  // namespace tmpc
