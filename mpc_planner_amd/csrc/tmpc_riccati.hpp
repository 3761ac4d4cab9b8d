// Square-root Riccati recursion of the interior-point QP solve: factorisation (matrix recursion) and vector solves
// (backward / forward sweeps), one wave per trajectory, operands in LDS (struct Lds, tmpc_solve.hip / tmpc_fast.hpp).
// Included by tmpc_solve.hip after the LDS layout and the cross-lane helpers; shared by the generic and the fast kernels.
#pragma once

namespace tmpc {

// ---- optional coarse clock split of the sweeps (tools/profile_sweeps.py builds a separate library with this macro;
// the product library never defines it) ---------------------------------------------------------------------------
#ifdef TMPC_SWEEP_PROFILE
enum { SP_FACTOR_TERM = 0, SP_FACTOR_LOOP, SP_SOLVE_PRE, SP_SOLVE_BWD, SP_SOLVE_FWD, SP_SOLVE_POST, SP_CALLS_FACTOR, SP_CALLS_SOLVE, SP_COUNT };
__device__ unsigned long long g_sweep_prof[SP_COUNT];
#define SWEEP_T0(lead) long long sp_t = clock64(); const bool sp_lead = (lead)      // lead: the one lane that records
#define SWEEP_T(i) do { const long long sp_n = clock64(); if (sp_lead) atomicAdd(&g_sweep_prof[i], (unsigned long long)(sp_n - sp_t)); sp_t = sp_n; } while (0)
#define SWEEP_COUNT(i) do { if (tid == 0) atomicAdd(&g_sweep_prof[i], 1ull); } while (0)
#else
#define SWEEP_T0(lead)
#define SWEEP_T(i)
#define SWEEP_COUNT(i)
#endif

// Issue priority of the wave (s_setprio, round 5).  Two waves share a SIMD; when both have an instruction ready the one with the higher priority issues.
// A wave inside a SEQUENTIAL phase (the Riccati factorisation and sweeps: 8 of 64 lanes, every instruction on the trajectory's critical path) gets
// priority 3, the rest of an interior-point iteration 2, the linearisation 0 -- measured on the cfg 2 bench launch
// (profiles/round5_g_setprio_ab{,2}.jsonl): no priorities 27.53 ms, (3, 0) 27.15, (3, 1) 27.07, **(3, 2) 27.01** (+1.9 %), (3, 3) 27.20, (1, 1) 27.19,
// the reverse assignment (0, 3) 27.63; at 2-4 rounds per launch the same shape gains 4-8 % (round5_k_prio_vs_launch_size.jsonl).  Results are
// unaffected (it only orders issue between the waves of a SIMD).  Only where every SIMD hosts two waves: at 7 workgroups per CU (cfg 4's shape) one
// SIMD hosts a single wave, the priorities make the launch 6 % SLOWER (round5_j_prio_other_configs.jsonl: the starved waves set the makespan) --
// the host sets Dims::prio per launch (launch_solve) and the macros test it (a scalar branch).
#if defined(__HIP_DEVICE_COMPILE__)
#define TMPC_PRIO_HIGH() do { if (d.prio) __builtin_amdgcn_s_setprio(3); } while (0)
#define TMPC_PRIO_LOW() do { if (d.prio) __builtin_amdgcn_s_setprio(2); } while (0)
#define TMPC_PRIO_LINEARISE() do { if (d.prio) __builtin_amdgcn_s_setprio(0); } while (0)
#else
#define TMPC_PRIO_HIGH()
#define TMPC_PRIO_LOW()
#define TMPC_PRIO_LINEARISE()
#endif

// ---- Riccati recursion: factorisation --------------------------------------------------------------
// Lane i (< 7) owns ROW i of the stage matrix F_k = Hh_k + [B A]^T P_{k+1} [B A] in registers f[0..i].  The elimination runs entirely in
// registers: pivots and column entries are broadcast inside the 16-lane row (v_mov_b64_dpp row_newbcast), no LDS traffic and no barriers.
// Round 5: the elimination STOPS after the two input columns.  What is left in rows 2..6 is the Schur complement
// P_k = F_xx - Lxu Lxu^T -- the cost-to-go Hessian itself --, and the next stage uses it as it is (w = P [B A]_.,i per lane, F_ij = Hh_ij +
// sum_n w_n [B A]_nj) instead of re-factorising it into Lxx Lxx^T and forming G = Lxx^T [B A], F = Hh + G^T G (rounds 1-4: the square-root
// form, 7 pivots per stage).  The first two column eliminations are THE SAME operations in both forms, so P_k is the same matrix; what goes
// is the five state pivots (each: broadcast, v_rsq_f64 + Halley step, scale, column broadcasts, rank-1 update -- and v_rsq_f64 alone issues
// for 16 cycles, profiles/round5_chain_floor.json) and the triangular products: 227 -> ~150 VALU instructions per stage, two pivots on
// the chain instead of seven.  Numerics: tools/riccati_form_study.py ran both forms inside the oracle's interior-point method on the
// bench scenes -- at the reference's qp_tol = 1e-5 no exit code, SQP or interior-point iteration count changes on 2560 trajectories and the
// iterates agree to 4e-11 (the level of the kernels' rounding differences); profiles/round5_riccati_form_study.json.
// In place of Hh_k the "factor block" (28 doubles) is written for the vector solves:
//   [0..9]  Lxu (5x2, row-major)   [10] 1/L00   [11] L10   [12] 1/L11   [13..27] P_k (packed lower 5x5)
// (round 6: the vector sweeps apply Luu on lanes 0 and 1 only and broadcast the result: lane 0 needs (1/L00, L10), lane 1 (L10, 1/L11),
//  ONE two-double load with a per-lane base where every lane loaded all three, two instructions; the arithmetic is the same)
constexpr int FB_LXU = 0, FB_R0 = 10, FB_L10 = 11, FB_R1 = 12, FB_P = 13;

// L.scr: SCR_COMPACT doubles in the compact one-wave carve, SCR_FULL in every other one (tmpc_fast.hpp, tmpc_kernels.hpp).  The stage loops' stores of lanes
// outside a store group (factorisation and both vector sweeps) go to a dummy region of it that nobody reads: RDUM_EXTENT doubles from RDUM_BASE_COMPACT / RDUM_BASE_FULL -- the P row's five at
// RDUM_P (the sweeps' one double per stage goes there too), the pair's two at RDUM_PAIR -- below the two-wave kernels' flag L.scr[SCR_FULL - 1] and above
// what the other users of L.scr take (the block reductions' slots, the parallel-in-time factorisation's four doubles at 48).
constexpr int SCR_COMPACT = 8, SCR_FULL = 64;
constexpr int RDUM_P = 0, RDUM_PAIR = 5, RDUM_EXTENT = 7, RDUM_BASE_COMPACT = 0, RDUM_BASE_FULL = 56;
static_assert(RDUM_P + NX <= RDUM_PAIR && RDUM_PAIR + NU <= RDUM_EXTENT, "dummy slots of the stage loops' store groups");
static_assert(RDUM_BASE_COMPACT + RDUM_EXTENT <= SCR_COMPACT, "the dummy region must fit the compact carve's L.scr");
static_assert(RDUM_BASE_FULL >= 52 && RDUM_BASE_FULL + RDUM_EXTENT <= SCR_FULL - 1, "the dummy region must stay between scr + 48..51 and the flag scr[63]");

// Offset of stage k's block in Hh.  A stride of 28 doubles (56 dwords) puts the stages k, k + 8, k + 16 on the same LDS banks: the stage-parallel loops
// (one lane per stage: the node's 28 stores of Hh <- W, the 15 + 15 loads of P in the vector solves' prologue / epilogue, the row passes' ds_add_f64)
// ran every access in three passes; 29 is conflict-free and costs (N + 1) doubles of LDS.  The stride is a COMPILE-TIME fact of the instantiation --
// the layout parameter CP of the routines below: 0 fast / generic layouts (28), 1 compact (28), 2 compact with 29, 3 compact with 30 doubles of which the
// last two hold the stage's y (compact_layout(), tmpc_fast.hpp: the tuned one-wave shapes; 3 is (12,12)'s, whose seven-per-CU budget has 69 bytes to spare --
// 30 k is 2-way at worst for 21 stages, and dropping the y array pays for it) -- because a run-time stride, one more live SGPR in kernels that spill 250 of
// them, cost the two-wave compact kernels 3.7 %, and a bank swizzle k * 28 + (k >> 3) (no extra LDS) more than it saved (profiles/round5_q_*).  Measured: +2.4 % at cfg 2.
template <int CP> __host__ __device__ constexpr int hstride() { return CP == 2 ? NP28 + 1 : (CP == 3 ? NP28 + 2 : NP28); }
template <int CP> __device__ __forceinline__ int hoff(int k) { return k * hstride<CP>(); }
template <int CP> __device__ __forceinline__ int hoff_lane(int k) { return mul24(k, hstride<CP>()); }                             // (k per lane)
// y = Luu^-1 (...) of stage k, handed from the backward sweep (or the factorisation's extra row) to the forward sweep: its own array, or -- layout 3 --
// the two spare doubles of the stage's 30-double block
template <int CP> __device__ __forceinline__ double *ysl(const Lds &L, int k) { return CP == 3 ? L.Hh + hoff<CP>(k) + NP28 : L.y + k * NU; }

// (The sequential sweeps use lanes 0..7 of the wave and rows 1..3 run along on copies.  Switching those rows off for the sweeps -- the LDS unit is
// busy 70 % of the kernel time at eight trajectories per CU and the sweeps issue two thirds of its instructions -- was measured in round 5: 1.3 %
// SLOWER, profiles/round5_o_sweep_rows_ab.jsonl; an LDS instruction costs the same with 16 lanes as with 64 and the EXEC changes are not free.)

// ---- row broadcasts folded into the multiply-adds of the stage loops ---------------------------------------------------------------------
// Groups of v_fmac_f64_dpp behind ONE hazard pad (TMPC_FMAC_BCAST16, tmpc_kernels.hpp: why groups, the rounding, what the pad costs).  In every group
// the sources of the broadcasts are inputs that no instruction of the group writes, the accumulators are early-clobber, and the unfused expression
// was the same chain of FMAs -- explicit fma() or the contracted a += b * c, checked in the parent's assembly -- with the same operand roles in the
// same order: same bits.  Per stage of the factorisation 39 multiply-adds are fused and 29 of the 36 v_mov_b64_dpp are gone (left: column 0 of P, whose
// products open the w chains -- an fmac onto 0.0 would differ in the sign of a zero --, and the two pivots, which feed rsqrt_nr), 119 -> 90 VALU
// instructions and 4 pads; per stage of the backward sweep 5 of 9, 24 -> 19 and one pad: +5.2 % on the bench launch, lever by lever in
// profiles/riccati_fused_broadcast_ab.jsonl (tools/isa_loops.py counts `fused`, `nop`).  Not taken: the forward sweep's dx update, whose sources are
// written just before (a pad each) and whose accumulator is one of them (a register copy): -0.4 %.
// column c of chol_rows<0, NU>: f[j] -= bcast16<j>(f[c]) * f[c] for the rows j = c + 1 .. NV - 1 (f[c] was written just before: the pad is needed)
#define CH_T(i) TMPC_FMAC_BCAST16("%[a" #i "]", "-%[s]", "%[s]", "%[l" #i "]")
#define CH_A(i) [a##i] "+&v"(f[c + 1 + i])
#define CH_L(i) [l##i] "n"(c + 1 + i)
template <int c>
__device__ __forceinline__ void chol_column_update(double (&f)[NV])
{
    static_assert(NV == 7 && NU == 2 && c >= 0 && c < NU, "the two input columns: six and five rows below the pivot");
    if constexpr (c == 0)
        asm("s_nop 1\n\t" CH_T(0) CH_T(1) CH_T(2) CH_T(3) CH_T(4) CH_T(5)
            : CH_A(0), CH_A(1), CH_A(2), CH_A(3), CH_A(4), CH_A(5) : [s] "v"(f[c]), CH_L(0), CH_L(1), CH_L(2), CH_L(3), CH_L(4), CH_L(5));
    else
        asm("s_nop 1\n\t" CH_T(0) CH_T(1) CH_T(2) CH_T(3) CH_T(4)
            : CH_A(0), CH_A(1), CH_A(2), CH_A(3), CH_A(4) : [s] "v"(f[c]), CH_L(0), CH_L(1), CH_L(2), CH_L(3), CH_L(4));
}
#undef CH_T
#undef CH_A
#undef CH_L
// the terms m = 1 .. 4 of the five chains w_n = sum_m P_nm ba_m, P_nm = bcast16<NU + max(n, m)>(f[NU + min(n, m)]); w[n] comes in as the product
// P_n0 ba_0.  m outer, n inner: a chain's terms stay in the order m = 1, 2, 3, 4 and two instructions of one chain are five apart
#define W_T(n, m, lo, lane) TMPC_FMAC_BCAST16("%[w" #n "]", "%[p" #lo "]", "%[b" #m "]", #lane)
__device__ __forceinline__ void w_chains_update(double (&w)[NX], const double (&f)[NV], const double (&ba)[NX])
{
    static_assert(NU == 2 && NX == 5, "the literal lane numbers NU + max(n, m) below");
    asm("s_nop 1\n\t"
        W_T(0, 1, 0, 3) W_T(1, 1, 1, 3) W_T(2, 1, 1, 4) W_T(3, 1, 1, 5) W_T(4, 1, 1, 6)
        W_T(0, 2, 0, 4) W_T(1, 2, 1, 4) W_T(2, 2, 2, 4) W_T(3, 2, 2, 5) W_T(4, 2, 2, 6)
        W_T(0, 3, 0, 5) W_T(1, 3, 1, 5) W_T(2, 3, 2, 5) W_T(3, 3, 3, 5) W_T(4, 3, 3, 6)
        W_T(0, 4, 0, 6) W_T(1, 4, 1, 6) W_T(2, 4, 2, 6) W_T(3, 4, 3, 6) W_T(4, 4, 4, 6)
        : [w0] "+&v"(w[0]), [w1] "+&v"(w[1]), [w2] "+&v"(w[2]), [w3] "+&v"(w[3]), [w4] "+&v"(w[4])
        : [p0] "v"(f[NU + 0]), [p1] "v"(f[NU + 1]), [p2] "v"(f[NU + 2]), [p3] "v"(f[NU + 3]), [p4] "v"(f[NU + 4]),
          [b1] "v"(ba[1]), [b2] "v"(ba[2]), [b3] "v"(ba[3]), [b4] "v"(ba[4]));
}
#undef W_T
// the stage-dependent entries of [B A] in the F row: h_c += bcast16<c>(ba0) * w0, then h_c += bcast16<c>(ba1) * w1, for the columns c = a, w, psi, v
// (ba0, ba1: rows x, y of the lane's own column of [B A]; h_c comes in as Hh's entry)
#define F_T(c, s, y) TMPC_FMAC_BCAST16("%[h" #c "]", "%[" #s "]", "%[" #y "]", "%[l" #c "]")
__device__ __forceinline__ void f_row_update(double &ha, double &hw, double &hp, double &hv, double ba0, double ba1, double w0, double w1)
{
    asm("s_nop 1\n\t" F_T(a, s0, y0) F_T(w, s0, y0) F_T(p, s0, y0) F_T(v, s0, y0) F_T(a, s1, y1) F_T(w, s1, y1) F_T(p, s1, y1) F_T(v, s1, y1)
        : [ha] "+&v"(ha), [hw] "+&v"(hw), [hp] "+&v"(hp), [hv] "+&v"(hv)
        : [s0] "v"(ba0), [s1] "v"(ba1), [y0] "v"(w0), [y1] "v"(w1), [la] "n"(ZA), [lw] "n"(ZW), [lp] "n"(ZPSI), [lv] "n"(ZV));
}
#undef F_T
// backward sweep: fj += bcast16<NU + l>(Pb) * ba[l], l = 0 .. 4 in this order
#define B_T(l, lane) TMPC_FMAC_BCAST16("%[fj]", "%[pb]", "%[b" #l "]", #lane)
__device__ __forceinline__ void bwd_chain_update(double &fj, double Pb, const double (&ba)[NX])
{
    static_assert(NU == 2 && NX == 5, "the literal lane numbers NU + l below");
    asm("s_nop 1\n\t" B_T(0, 2) B_T(1, 3) B_T(2, 4) B_T(3, 5) B_T(4, 6)
        : [fj] "+&v"(fj) : [pb] "v"(Pb), [b0] "v"(ba[0]), [b1] "v"(ba[1]), [b2] "v"(ba[2]), [b3] "v"(ba[3]), [b4] "v"(ba[4]));
}
#undef B_T

// right-looking elimination of columns C0 .. C1-1 of the row-per-lane matrix
template <int C0, int C1 = NV>
__device__ __forceinline__ bool chol_rows(double (&f)[NV], int lane, double *r0, double *r1)
{
    bool bad = false;
    static_for<C0, C1>([&](auto c_) {
        constexpr int c = decltype(c_)::value;
        const double dpiv = bcast16<c>(f[c]);
        if (!(dpiv > 0.0)) bad = true;
        const double y = rsqrt_nr(dpiv);
        f[c] *= y;                                  // lane i >= c: L_ic (i == c: sqrt(d))
        if (c == 0 && r0) *r0 = y;
        if (c == 1 && r1) *r1 = y;
        // L_jc to the row's lanes and the update of column j.  The Schur-complement form's two input columns (every kernel's default path) fold the
        // broadcasts into the multiply-adds, one group per column; the square-root form's seven columns keep the pair (not measured there).
        if constexpr (C0 == 0 && C1 == NU) chol_column_update<c>(f);
        else static_for<c + 1, NV>([&](auto j_) {
            constexpr int j = decltype(j_)::value;
            const double ljc = bcast16<j>(f[c]);
            f[j] -= f[c] * ljc;
        });
    });
    (void)lane;                                       // entries above the diagonal are never read
    return bad;
}

// dyn8[k] = (Xa, Ya, Xw, Yw, Xp, Yp, Xv, Yv): the only non-constant entries of [B A] for the unicycle
// (tmpc_stage.hpp dyn_jacobian); the rest is identity / dt / dt^2/2.  A column's two entries are neighbours (one two-double load per
// lane in the sequential loops), a row's four are at stride 2.
enum { D8_XA = 0, D8_YA, D8_XW, D8_YW, D8_XP, D8_YP, D8_XV, D8_YV };

// Compact layout (no dense [B A] in LDS): a lane's column / row of [B A] through the table `tab` (ba_off, tmpc_solve.hip).
// Column j: entries 0, 1 are stage-dependent for j in {a, w, psi, v} (offset o0 + 8 k) and constants otherwise (stride 0), neighbours in
// the table either way (o0, o0 + 1); entries 2..4 are constants for every column, neighbours too (o1, o1 + 1, o1 + 2).
// Row i (state index) in dyn8 column order (a, w, psi, v) at o0, o0 + 2, o0 + 4, o0 + 6: stage-dependent for x, y.
struct BaLane { int o0, o1, st; };
__device__ __forceinline__ BaLane ba_column(int N, int j)
{
    BaLane c;
    c.o0 = j == ZA ? D8_XA : j == ZW ? D8_XW : j == ZPSI ? D8_XP : j == ZV ? D8_XV : N * 8 + (j == ZX ? BAP_X : j == ZY ? BAP_Y : BAP_S);
    c.o1 = N * 8 + (j == ZA ? BAT_A : j == ZW ? BAT_W : j == ZPSI ? BAT_PSI : j == ZV ? BAT_V : j == ZS ? BAT_S : BAT_XY);
    c.st = c.o0 < 8 ? 8 : 0;
    return c;
}
__device__ __forceinline__ BaLane ba_row4(int N, int i5)          // o0: base of (b_a, b_w, e_psi, e_v) of row i5 of [B E], E = A - I, at stride 2
{
    BaLane c;
    c.o0 = i5 < 2 ? i5 : N * 8 + (i5 == 2 ? BAR_PSI : i5 == 3 ? BAR_V : BAR_S); c.o1 = 0;
    c.st = i5 < 2 ? 8 : 0;
    return c;
}

// The sweeps below are strictly sequential over stages; to keep LDS latency off the critical path every
// operand of stage k-1 is (re)loaded into the same registers right after its last use in stage k, so the loads
// complete underneath the dependent Cholesky / readlane chain of stage k.
// NTH = threads per trajectory: 64, or 128 for the two-wave variant, in which the sweeps run on wave 0 alone (wave 1
// waits at the closing barrier) and only the stage-parallel loops use all threads.
// `sw`: which of the two waves sweeps (two-wave variant); the other one waits at the closing barrier.
// ---- the sequential parts work on 16-lane ROWS ---------------------------------------------------------------------------
// All cross-lane traffic of the sweeps is row-local (bcast16, row shifts), so a wave can run up to four trajectories' sweeps at
// once, one per row: `li` is the lane's index inside its row (li >= 16: idle lane), `L` the LDS view of the row's trajectory
// (per-lane pointers when rows differ) and `wr` enables the row's stores.  One trajectory per wave (the fast / compact kernels):
// li = lane, rows 1..3 idle.  Four per wave: the team kernels (tmpc_fast.hpp).
// VEC (the register-row kernels): the PREDICTOR's right-hand side rides through the factorisation as an extra row.  Lane 7 of the row
// holds the row [g_u g_x] of the bordered matrix [[F, g], [g^T, .]] (g = gh, the predictor right-hand side, complete before the
// factorisation starts): it takes part in every column update like the rows below the pivot and never becomes a pivot, so after the
// elimination of the two input columns it is  [y0 y1 | p_k]: y = Luu^-1 g_u is what the forward sweep needs, and the rest is the Schur
// complement of the border, i.e. the cost-to-go gradient p_k itself.  At the next stage the row's "own column" is the dynamics residual rb
// and p joins the product: w = P rb + p.  The separate backward vector sweep of the predictor (and its stage-parallel prologue P rb)
// disappear: one of the five sequential passes over the stages of an interior-point iteration.  Same algebra as the separate sweep; the
// operations associate differently (rounding-level differences).
// SQ (Dims::riccati_form = 1, tmpc_dims.riccati_form = TMPC_RICCATI_SQUARE_ROOT): the SQUARE-ROOT form of rounds 1-4 -- what acados' HPIPM runs in its
// default mode (square_root_alg = 1 [UPSTREAM]; solver_generator/generate_acados_solver.py:171 takes the defaults) -- kept as a selectable
// instantiation (round 6): all seven columns are eliminated, rows 2..6 hold Lxx with P_k = Lxx Lxx^T, the next stage forms G = Lxx^T [B A] and
// F = Hh + G^T G (no subtraction of large numbers), FB_P holds Lxx, and the extra row ends as [y0 y1 | lx] with p_k = Lxx lx.  At the
// reference's qp_tol = 1e-5 both forms give the same exit codes, iteration counts and iterates (profiles/round5_riccati_form_study.json); at
// qp_tol = 1e-9 a few solves per thousand end differently, which is why a run against a real acados at that tolerance (tools/acados_replay.py)
// should use this form.
template <int CP, bool VEC = false, bool SQ = false>
__device__ __forceinline__ bool riccati_factor_rows(const Lds &L, const Dims &d, int li, bool wr)
{
    const int N = d.N;
    const bool rowl = li < NV && wr;
    const bool vec = VEC && li == NV;                // the right-hand-side row
    const double vmask = vec ? 1.0 : 0.0;
    const int ls = li < NV ? li : 0;
    const int i5 = li - NU;                          // state index of lanes 2..6
    const double dt = d.dt, sdt = d.sdt, shdt2 = d.shdt2;      // (sdt, shdt2: the spline row of [B A]; zero for the model without a spline state)
    bool bad = false;
    // Operands of a stage.  The operands of stage k - 1 are loaded while stage k still needs some of its own (the scheduler computes rows 2..6 of
    // F after the pivots), so two register sets are live and the compiler copies the shadow set over at the back edge: 11 v_mov_b64 of the loop's
    // 138 instructions.  Naming the two sets and unrolling the stage loop by two (like the vector sweeps): no copies, 129 instructions per stage,
    // 4 % fewer cycles per factorisation on a lone wave -- and 0.7 % LESS throughput on the saturated compact kernel
    // (profiles/round5_m_factor_unroll_rotation_ab.jsonl).  So the one-wave-per-SIMD kernels (fast, profiled twins, CP == 0) run the unrolled
    // loop, the compact kernels (two waves per SIMD) the rolled one; the arithmetic is the same.  A property of the INSTANTIATION, so that every
    // translation unit gives a kernel the same body (round-5 advisor: a per-unit macro made the same template differ between units).
    struct Opnd { double hk[NV], ba[NX]; };
    double f[NV];
    const BaLane bc = ba_column(N, ls);
    double bac[NX];
    if constexpr (CP && !VEC) {                          // constant entries of the own column of [B A]
#pragma unroll
        for (int m = 2; m < NX; m++) bac[m] = L.tab[ba_off(N, 0, m, ls)];
    }
    // VEC: every lane loads hk[] / ba[] through per-lane (pointer, stride) pairs, so that the extra row reads gh / rb with the same loads.
    // Running pointers, stepped back by the lane's stride once per stage (round 4: the k * stride multiplications and per-entry index
    // arithmetic were ~17 of the stage loop's ~250 instructions): a lane reads hk[j] = row[j] at IMMEDIATE offsets from the start of its row of
    // the packed Hh block -- the entries j > own row index belong to the next row and are never used (chol_rows reads the lower triangle only).
    // (the same for ba[] -- running offsets or pointers, five more values live across the stage loop -- pushed the compact kernels into scratch
    // twice: ba[] keeps its (base + k * stride) form, which the compiler rematerialises)
    // Every stream of the stage loop -- loads and stores -- is a (base pointer, stride in BYTES) pair per lane, set up here, and its stage address is
    // at8(base, k, stride): one v_mad_u32_u24 (tmpc_kernels.hpp).  The hk[] stream used to be `hrow + (vec ? k * NV : hoff<CP>(k))`, k times a per-lane
    // select of two constants: a full 32-bit (quarter-rate) multiply per stage; it is the same pair form now.
    const double *hrow = nullptr;
    int hst = 0;
    const double *bo[NX] = {};
    int bst[NX] = {};
    if constexpr (VEC) {
        hrow = vec ? L.gh : L.Hh + pidx(ls, 0);       // (row start inside a stage's block)
        hst = (vec ? NV : hstride<CP>()) * B8;
        if constexpr (CP) {
            // the table keeps a column's entries of rows x, y and of rows psi, v, s next to each other, as rb is: two bases per lane, three loads
            // (2 + 2 + 1 doubles) where five bases took five
            bo[0] = vec ? L.rb : L.tab + bc.o0; bst[0] = (vec ? NX : bc.st) * B8;
            bo[2] = vec ? L.rb + 2 : L.tab + bc.o1; bst[2] = (vec ? NX : 0) * B8;
        } else {
#pragma unroll
            for (int m = 0; m < NX; m++) { bo[m] = vec ? L.rb + m : L.BA + m * NV + ls; bst[m] = (vec ? NX : NX * NV) * B8; }
        }
    }
    const double *tcb = CP ? L.tab + bc.o0 : nullptr;             // (non-VEC compact: rows x, y of the own column of [B A] in the table)
    const int tcs = bc.st * B8;
    // (load_stage reads stage k, then k - 1, ...; the last call re-loads stage 0)
    auto load_stage = [&](Opnd &o, int k) {
        // unconditional loads (clamped indices): entries above the diagonal / of idle lanes are never used
        if constexpr (VEC) {
            const double *hr = at8(hrow, k, hst);
#pragma unroll
            for (int j = 0; j < NV; j++) o.hk[j] = hr[j];
            if constexpr (CP) {
                const double *T0 = at8(bo[0], k, bst[0]), *T2 = at8(bo[2], k, bst[2]);
                o.ba[0] = T0[0]; o.ba[1] = T0[1]; o.ba[2] = T2[0]; o.ba[3] = T2[1]; o.ba[4] = T2[2];
            } else {
#pragma unroll
                for (int m = 0; m < NX; m++) o.ba[m] = *at8(bo[m], k, bst[m]);
            }
        } else {
            const double *Hk = at8u(L.Hh, k, hstride<CP>() * B8);
#pragma unroll
            for (int j = 0; j < NV; j++) o.hk[j] = Hk[pidx(ls, j <= ls ? j : ls)];
            if constexpr (CP) {
                { const double *Tc = at8(tcb, k, tcs); o.ba[0] = Tc[0]; o.ba[1] = Tc[1]; }       // rows x, y of the own column: one load
#pragma unroll
                for (int m = 2; m < NX; m++) o.ba[m] = bac[m];
            } else {
                const double *BA = at8u(L.BA, k, NX * NV * B8);
#pragma unroll
                for (int m = 0; m < NX; m++) o.ba[m] = BA[m * NV + ls];
            }
        }
    };
    // terminal node: P_N = the xx-block of Hh_N (rows/cols 2..6) as it is; the extra row starts as p_N = g_x of node N
#pragma unroll
    for (int j = 0; j < NV; j++) f[j] = (j >= NU) ? (vec ? L.gh[N * NV + j] : L.Hh[hoff<CP>(N) + pidx(ls, j <= ls ? j : ls)]) : 0.0;
    Opnd oa, ob;
    load_stage(oa, N - 1);
    if constexpr (SQ) bad |= chol_rows<NU>(f, li, nullptr, nullptr);       // square-root form: Cholesky of the xx block of node N
    // Store merging (round 6).  Stores of disjoint lane sets that hold the same registers at the same point of the loop can leave in ONE LDS instruction
    // with a per-lane address.  In the FACTORISATION -- p_{k+1} of the extra row with the rows of P_{k+1}, its [y0 y1] with the Lxu pairs: four LDS
    // instructions per stage fewer -- that is +1.4 % on the saturated cfg 2 launch.  In the vector sweeps (du of lanes 0, 1 with dx of lanes 2..6; y with p)
    // the merged store's value needs a select on the END of the stage's dependent chain: as PREDICATED stores with index arithmetic that was -3.4 %
    // (forward) and -2.0 % (backward) in round 6 (profiles/round6_saturated_levers_ab.jsonl).  With every stream a per-lane (base, stride) pair both signs
    // turned: the forward sweep's one store is +2.4 % (profiles/forward_sweep_fused_sum_ab.jsonl, one_store), the backward sweep's +1.3 %
    // (profiles/riccati_pivot_pair_store_ab.jsonl); results are bitwise the same either way.
    // End of stage k: ONE pair store of every lane, through one per-lane (base, stride) pair.  The Lxu pairs of lanes 2..6 and the extra row's [y0 y1] are
    // the registers f[0], f[1] of their lanes.  The pivots ride in it on lanes 0 and 1, which the Lxu / y pair leaves free: after chol_rows the reciprocal
    // pivots r0, r1 are row-uniform and lane 1's f[0] is L10, so lane 0 stores (1/L00, L10) at FB_R0 and lane 1 (L10, 1/L11) at FB_L10, both at the block
    // stride -- slot FB_L10 is written by both lanes, with identical bits; the block [Lxu | 1/L00 L10 1/L11 | P] and its readers are what they were.
    // Before, lane 1 stored the three doubles in two instructions through an address pair of its own: per stage two LDS instructions and one
    // v_mad_u32_u24 fewer for one row broadcast and six v_cndmask_b32 on loop-invariant lane masks, after the end of the stage's chain (nothing in the
    // next stage waits for this store): +1.6 % on the bench launch (profiles/riccati_pivot_pair_store_ab.jsonl).
    // (p_k follows at the top of stage k - 1; p_0 is never read.)
    // One straight-line store region per stage: the two store groups (the P row, the Lxu / y / pivot pair) are stores of EVERY lane through a
    // per-lane (offset, stride) pair -- evaluated once, here -- and the lanes outside a group write to a dummy slot of L.scr (stride 0) that nobody reads.
    // Predicated, each group was a divergent side block of the stage loop (saveexec / branch pairs, a lane compare re-evaluated per stage).
    const bool prl = rowl && li >= NU, vl = vec && wr;
    const bool pl0 = rowl && li == 0, pl1 = rowl && li == 1;
    double *const dum = L.scr + (CP ? RDUM_BASE_COMPACT : RDUM_BASE_FULL);
    double *const po = vl ? L.pr : prl ? L.Hh + FB_P + i5 * (i5 + 1) / 2 : dum + RDUM_P;
    const int pst = (vl ? NX : prl ? hstride<CP>() : 0) * B8;
    double *const qo = vl ? (CP == 3 ? L.Hh + NP28 : L.y) : prl ? L.Hh + FB_LXU + 2 * i5 : rowl ? L.Hh + FB_R0 + li : dum + RDUM_PAIR;
    const int qst = (vl ? (CP == 3 ? hstride<CP>() : NU) : rowl ? hstride<CP>() : 0) * B8;
    auto store_pairs = [&](int k, double r0, double r1) {
        const double l10 = bcast16<1>(f[0]);
        double *pp = at8(qo, k, qst);
        pp[0] = pl0 ? r0 : f[0]; pp[1] = pl0 ? l10 : (pl1 ? r1 : f[1]);
    };
    auto stage = [&](const Opnd &o, Opnd &nx, int k) {
        // broadcast P (lower triangle of the 5x5 cost-to-go Hessian of stage k+1: rows 2..6 after the elimination) to every lane of the row
        double Pm[NX][NX];
        static_for<0, NX>([&](auto m_) {
            constexpr int m = decltype(m_)::value;
#pragma unroll
            for (int l = 0; l <= m; l++) Pm[m][l] = bcast16<NU + m>(f[NU + l]);
        });
        // P_{k+1} (own row of lanes 2..6) is kept for the vector solves -- and the extra row's p_{k+1} (square-root form: lx) leaves in the SAME five store
        // instructions (round 6: the LDS unit is the busy one at eight trajectories per CU, and an LDS instruction costs the same with one lane as with six):
        // lane 7 holds it in the same registers f[2..6] at the same point of the loop; only the address differs per lane
        // The row is stored WITHOUT a select for the entries above the diagonal: every lane stores all five entries to Ln + l, in DESCENDING order of l.
        // Entry l > i5 of lane i5 lands on packed offset i5 (i5 + 1) / 2 + l, which is entry e < l of a later row j > i5: its owner writes it in a LATER
        // instruction of the same wave (LDS operations of a wave execute in order), so the junk is gone before anything reads the block.  The compiler
        // sees one thread: it may not re-order these stores or merge two of them into one instruction (a two-address store would put lane 0's junk and
        // lane 1's value on one address at once for the pairs (2, 1) and (1, 0)) -- hence the compiler barriers between them; only the pair (4, 3), whose
        // junk lands on junk or on entries <= 2, may share an instruction.
        // (Measured and left out: (4, 3) | (2, 1) | 0 in three instructions, with a dummy base for lane 2 -- i5 = 0, whose entries 1 and 2 are both junk --
        //  in the middle one, so that its junk entry 2 does not meet lane 3's valid entry 1; every other piece of junk is still overwritten by a later
        //  instruction.  One more per-lane address, zero scratch and bitwise the same results, +0.18 % at a spread of 0.39 %: inside the noise,
        //  profiles/riccati_pivot_pair_store_ab.jsonl.)
        {
            double *Ln = at8(po, k + 1, pst);
            Ln[4] = f[NU + 4]; Ln[3] = f[NU + 3];
            asm volatile("" ::: "memory");
            Ln[2] = f[NU + 2];
            asm volatile("" ::: "memory");
            Ln[1] = f[NU + 1];
            asm volatile("" ::: "memory");
            Ln[0] = f[NU + 0];
        }
        if constexpr (SQ) {
            // G = Lp^T [B A] (5 x 7), Lp = Pm (the lower triangle holds Lxx of stage k + 1).  Own column densely from ba[]; all columns (row-uniform)
            // from the sparse [B A]:  x: e0   y: e1   s: e4   psi: (Xp,Yp,1,0,0)   v: (Xv,Yv,0,1,sdt)   a: (Xa,Ya,0,dt,shdt2)   w: (Xw,Yw,dt,0,0)
            // F = Hh + G^T G keeps the square-root structure (a factor-level perturbation only).  The extra row: (Lp^T rb)_l + lx_l of stage k + 1.
            double Go[NX];
#pragma unroll
            for (int l = 0; l < NX; l++) {
                double acc = 0.0;
#pragma unroll
                for (int m = l; m < NX; m++) acc += Pm[m][l] * o.ba[m];
                Go[l] = VEC ? fma(vmask, f[NU + l], acc) : acc;
            }
            const double Xa = bcast16<ZA>(o.ba[0]), Ya = bcast16<ZA>(o.ba[1]), Xw = bcast16<ZW>(o.ba[0]), Yw = bcast16<ZW>(o.ba[1]);
            const double Xp = bcast16<ZPSI>(o.ba[0]), Yp = bcast16<ZPSI>(o.ba[1]), Xv = bcast16<ZV>(o.ba[0]), Yv = bcast16<ZV>(o.ba[1]);
            double Ga[NX], Gw[NX], Gp[3], Gv[NX];
            Ga[0] = ((Pm[0][0] * Xa + Pm[1][0] * Ya) + Pm[3][0] * dt) + Pm[4][0] * shdt2;
            Ga[1] = (Pm[1][1] * Ya + Pm[3][1] * dt) + Pm[4][1] * shdt2;
            Ga[2] = Pm[3][2] * dt + Pm[4][2] * shdt2;
            Ga[3] = Pm[3][3] * dt + Pm[4][3] * shdt2;
            Ga[4] = Pm[4][4] * shdt2;
            Gw[0] = (Pm[0][0] * Xw + Pm[1][0] * Yw) + Pm[2][0] * dt;
            Gw[1] = Pm[1][1] * Yw + Pm[2][1] * dt;
            Gw[2] = Pm[2][2] * dt; Gw[3] = 0.0; Gw[4] = 0.0;
            Gp[0] = (Pm[0][0] * Xp + Pm[1][0] * Yp) + Pm[2][0];
            Gp[1] = Pm[1][1] * Yp + Pm[2][1];
            Gp[2] = Pm[2][2];
            Gv[0] = ((Pm[0][0] * Xv + Pm[1][0] * Yv) + Pm[3][0]) + Pm[4][0] * sdt;
            Gv[1] = (Pm[1][1] * Yv + Pm[3][1]) + Pm[4][1] * sdt;
            Gv[2] = Pm[3][2] + Pm[4][2] * sdt;
            Gv[3] = Pm[3][3] + Pm[4][3] * sdt;
            Gv[4] = Pm[4][4] * sdt;
            double a0 = o.hk[ZA], a1 = o.hk[ZW], a2 = o.hk[ZX], a3 = o.hk[ZY], a4 = o.hk[ZPSI], a5 = o.hk[ZV], a6 = o.hk[ZS];
#pragma unroll
            for (int l = 0; l < NX; l++) {                       // F row `li`: F_ij = Hh_ij + sum_l G_l,li G_l,j
                a0 += Go[l] * Ga[l];
                if (l < 3) a1 += Go[l] * Gw[l];
                if (l < 1) a2 += Go[l] * Pm[0][0];
                if (l < 2) a3 += Go[l] * Pm[1][l];
                if (l < 3) a4 += Go[l] * Gp[l];
                a5 += Go[l] * Gv[l];
                a6 += Go[l] * Pm[4][l];
            }
            f[ZA] = a0; f[ZW] = a1; f[ZX] = a2; f[ZY] = a3; f[ZPSI] = a4; f[ZV] = a5; f[ZS] = a6;
            load_stage(nx, k > 0 ? k - 1 : 0);
            double r0 = 0.0, r1 = 0.0;
            bad |= chol_rows<0>(f, li, &r0, &r1);                 // all seven columns: rows 2..6 now hold Lxx of stage k (the extra row: lx)
            store_pairs(k, r0, r1);
            return;
        }
        // Schur-complement form (default): P_{k+1} enters the next stage's F unfactorised (its diagonal is tested after the loop, riccati_factor)
        // w = P [B A]_.,own (the lane's own column of [B A], densely from ba[]); the extra row: P rb + p_{k+1} -- as fma(1.0 or 0.0, f, acc):
        // exactly acc + f on the extra row and acc on the others (f is finite there), without the v_cndmask a select costs
        // (the first term of a chain is a plain product and keeps its bcast16; the other sixteen entries of Pm are used by the square-root form only)
        double w[NX];
#pragma unroll
        for (int n = 0; n < NX; n++) w[n] = Pm[n][0] * o.ba[0];
        w_chains_update(w, f, o.ba);
        if constexpr (VEC) {
#pragma unroll
            for (int n = 0; n < NX; n++) w[n] = fma(vmask, f[NU + n], w[n]);
        }
        // F row `li`: F_ij = Hh_ij + sum_n w_n [B A]_nj with the sparse columns of [B A] (row-uniform):
        //   x: e0   y: e1   s: e4   psi: (Xp,Yp,1,0,0)   v: (Xv,Yv,0,1,dt)   a: (Xa,Ya,0,dt,dt^2/2)   w: (Xw,Yw,dt,0,0)
        {
            // (round 6) the eight stage-dependent entries of [B A] are rows x, y of the columns a, w, psi, v -- which the lanes of those columns hold as
            // ba[0], ba[1] of their OWN column: eight row broadcasts instead of four row-uniform LDS loads of the dyn8 block (the LDS unit is the busy one)
            // (folded into the multiply-adds that open the four chains: Hh's entry + w0 X + w1 Y, accumulated on a copy of the hk operand)
            double ha = o.hk[ZA], hw = o.hk[ZW], hp = o.hk[ZPSI], hv = o.hk[ZV];
            f_row_update(ha, hw, hp, hv, o.ba[0], o.ba[1], w[0], w[1]);
            f[ZA] = fma(w[4], shdt2, fma(w[3], dt, ha));
            f[ZW] = fma(w[2], dt, hw);
            f[ZX] = o.hk[ZX] + w[0];
            f[ZY] = o.hk[ZY] + w[1];
            f[ZPSI] = hp + w[2];
            f[ZV] = fma(w[4], sdt, hv + w[3]);
            f[ZS] = o.hk[ZS] + w[4];
        }
        load_stage(nx, k > 0 ? k - 1 : 0);            // operands of the next stage, hidden under the elimination (unconditional, clamped;
                                                      // the pointers stop at stage 0, which the last pass re-loads and discards)
        double r0 = 0.0, r1 = 0.0;
        bad |= chol_rows<0, NU>(f, li, &r0, &r1);     // the two input columns; rows 2..6 now hold P_k (lanes 2..6) / p_k (the extra row)
        store_pairs(k, r0, r1);
    };
    if constexpr (CP == 0) {
        int k = N - 1;
        for (; k >= 1; k -= 2) {
            stage(oa, ob, k);
            stage(ob, oa, k - 1);
        }
        if (k == 0) stage(oa, ob, 0);
    } else {
        for (int k = N - 1; k >= 0; k--) stage(oa, oa, k);      // (one named set, re-loaded after its last use in source order)
    }
    return bad;
}

// NTH = threads per trajectory: 64, or 128 for the two-wave variant, in which the sweeps run on one wave (the other waits at the
// closing barrier) and only the stage-parallel loops use all threads.  `sw`: which of the two waves sweeps.
template <int NTH, int CP = 0, bool VEC = false, bool SQ = false>
__device__ __forceinline__ bool riccati_factor(const Lds &L, const Dims &d, int tid, int sw = 0)
{
    asm volatile("" : "+v"(tid));                    // opaque per call: lane-derived addresses are not shared with (kept live until) other phases
    bool anybad = false;
    SWEEP_T0(tid == 0); SWEEP_COUNT(SP_CALLS_FACTOR);
    if (NTH == 64 || (tid >> 6) == sw) {
        const int lane = tid & 63;
        TMPC_PRIO_HIGH();
        const bool bad = riccati_factor_rows<CP, VEC, SQ>(L, d, lane, true);
        TMPC_PRIO_LOW();
        bool bad_p = false;
        if constexpr (!SQ) {
            // Schur-complement form: P_k = F_xx - Lxu Lxu^T enters the next stage unfactorised, so nothing downstream would notice a diagonal entry that
            // cancellation has driven NEGATIVE (the square-root form's state pivots did; round-5 advisor).  Tested here, off the sequential chain: lane
            // k reads the sign bits of diag(P_{k+1}) from the factor blocks the loop has just written (same wave: LDS operations execute in order) --
            // five ds_read_b32 and three integer operations per factorisation.  (Inside the stage loop the same test cost the compact kernels, at 254
            // of 256 registers, their zero-scratch build.)  The oracle tests the same bits (oracle/qp_ipm.c riccati_factor_classical).
            const unsigned *Pd = reinterpret_cast<const unsigned *>(L.Hh + hoff_lane<CP>(lane < d.N ? lane + 1 : d.N) + FB_P) + 1;      // (high dwords)
            bad_p = (int)(Pd[2 * 0] | Pd[2 * 2] | Pd[2 * 5] | Pd[2 * 9] | Pd[2 * 14]) < 0;
        }
        anybad = __any((bad && lane < 16) || bad_p);  // (rows 1..3 of the wave compute on copies: their pivots mean nothing)
        if (NTH > 64 && lane == 0) L.scr[63] = anybad ? 1.0 : 0.0;
    }
    __syncthreads();
    SWEEP_T(SP_FACTOR_LOOP);
    if (NTH > 64) anybad = L.scr[63] != 0.0;
    return anybad;
}

// ---- square-root Riccati: vector solve (backward + forward), rhs gh / rb -> dv, dpi ------------------
// Stage-parallel parts (one lane per stage, `nth` lanes of the trajectory's own wave(s)):
//   pre   q_k = P_{k+1} rb_k for all stages at once (off the sequential chain); parked in dpi[k+1]
//   post  dpi_k = P_k dx_k + p_k, k = 1..N
// SQ (square-root form): FB_P holds Lxx, P x = Lxx (Lxx^T x)
template <int CP, bool SQ = false>
__device__ __forceinline__ void riccati_solve_pre(const Lds &L, const Dims &d, int tid, int nth)
{
    const int N = d.N;
    for (int k = tid; k < N; k += nth) {
        const double *Pn = L.Hh + hoff_lane<CP>(k + 1) + FB_P;              // P_{k+1}, packed lower triangle
        const double *r = L.rb + mul24(k, NX);
        double pp[15], rr[NX];
#pragma unroll
        for (int e = 0; e < 15; e++) pp[e] = Pn[e];
#pragma unroll
        for (int m = 0; m < NX; m++) rr[m] = r[m];
        if constexpr (SQ) {
            double tl[NX];
#pragma unroll
            for (int l = 0; l < NX; l++) {
                double acc = 0.0;
#pragma unroll
                for (int m = l; m < NX; m++) acc += pp[m * (m + 1) / 2 + l] * rr[m];
                tl[l] = acc;
            }
#pragma unroll
            for (int i = 0; i < NX; i++) {
                double acc = 0.0;
#pragma unroll
                for (int l = 0; l <= i; l++) acc += pp[i * (i + 1) / 2 + l] * tl[l];
                L.dpi[mul24(k + 1, NX) + i] = acc;
            }
            continue;
        }
#pragma unroll
        for (int i = 0; i < NX; i++) {
            double acc = 0.0;
#pragma unroll
            for (int m = 0; m < NX; m++) acc += pp[(m > i ? m * (m + 1) / 2 + i : i * (i + 1) / 2 + m)] * rr[m];
            L.dpi[mul24(k + 1, NX) + i] = acc;
        }
    }
}
// dpi_k = P_k dx_k + p_k, k = 1..N (L.pr holds p_k: from the backward sweep, or from the extra row of a VEC factorisation)
// SQ: dpi_k = Lxx (Lxx^T dx_k) + p_k
template <int CP, bool SQ = false>
__device__ __forceinline__ void riccati_solve_post(const Lds &L, const Dims &d, int tid, int nth)
{
    const int N = d.N;
    for (int kk = tid; kk < N; kk += nth) {
        const int k = kk + 1;
        const double *Pk = L.Hh + hoff_lane<CP>(k) + FB_P;
        const double *dxk = L.dv + mul24(k, NV) + NU;
        double pp[15], rr[NX], pk[NX];
#pragma unroll
        for (int e = 0; e < 15; e++) pp[e] = Pk[e];
#pragma unroll
        for (int m = 0; m < NX; m++) { rr[m] = dxk[m]; pk[m] = L.pr[mul24(k, NX) + m]; }
        if constexpr (SQ) {
            double tl[NX];
#pragma unroll
            for (int l = 0; l < NX; l++) {
                double acc = 0.0;
#pragma unroll
                for (int m = l; m < NX; m++) acc += pp[m * (m + 1) / 2 + l] * rr[m];
                tl[l] = acc;
            }
#pragma unroll
            for (int i = 0; i < NX; i++) {
                double acc = 0.0;
#pragma unroll
                for (int l = 0; l <= i; l++) acc += pp[i * (i + 1) / 2 + l] * tl[l];
                L.dpi[mul24(k, NX) + i] = acc + pk[i];
            }
            continue;
        }
#pragma unroll
        for (int i = 0; i < NX; i++) {
            double acc = 0.0;
#pragma unroll
            for (int m = 0; m < NX; m++) acc += pp[(m > i ? m * (m + 1) / 2 + i : i * (i + 1) / 2 + m)] * rr[m];
            L.dpi[mul24(k, NX) + i] = acc + pk[i];
        }
    }
}

// The two sequential sweeps on rows (see riccati_factor_rows for li / L / wr).  Lane j (< 7) of a row = component j of the stage
// vector [u; x]; the cost-to-go gradient p lives in lanes 2..6.  MID: what separates the sweeps (the forward sweep reads the y the
// backward sweep stored): a workgroup barrier in the one-trajectory kernels, a wave-level fence when one wave sweeps for a team.
template <int CP, bool BWD = true, typename MID>
__device__ __forceinline__ void riccati_sweeps_rows(const Lds &L, const Dims &d, int li, bool wr, bool sweeper, MID mid)
{
    const int N = d.N;
    const bool rowl = li < NV && wr, xl = rowl && li >= NU;
    const int ls = li < NV ? li : 0;
    const int i5 = (li >= NU && li < NV) ? li - NU : 0;
    SWEEP_T0(li == 0);
    if constexpr (BWD) {                                // (the fused predictor has done this part inside the factorisation)
    if (sweeper) {
    double p = L.gh[N * NV + ls];                       // p_N (lanes 2..6 meaningful)
    {
        // Two operand sets, filled alternately two stages ahead: a set is (re)loaded right after the stage that used it, so
        // its LDS latency passes underneath the other set's stage (with a single set the loads were issued at the end of
        // stage k and awaited at the top of stage k-1: ~120 exposed cycles per stage).
        // Compact layout: L.pr aliases L.dpi -- p_k takes the slot of q_{k-1} = (P rb)_{k-1}, which stage k - 1's operand load
        // (always issued before stage k runs: the sets are filled at least one stage ahead, and LDS operations of a wave
        // execute in order) has fetched by then; the closing loop adds P dx in place.
        // Operand merging: loads of disjoint lane sets leave in ONE LDS instruction with a per-lane address (an LDS instruction costs the same with one
        // lane as with 64, and at eight trajectories per CU the launch follows the LDS instruction count of these loops).  The pivot data is used by
        // lanes 0, 1 only and the Lxu pair by lanes 2..6 only, both sit in the stage's factor block: one pair (a0, a1) = lane 0 (1/L00, L10), lane 1
        // (L10, 1/L11), lane 2 + i (Lxu_i0, Lxu_i1).  The arithmetic on every lane that counts is what it was (profiles/sweep_operand_merge_ab.jsonl).
        // Addresses: every stream of the loop is at8(base, k, stride in bytes), base and stride set up here (tmpc_kernels.hpp): the per-lane strides
        // (gh / q, the table column) one v_mad_u32_u24 per stage, the block stride -- a compile-time fact -- a scalar product added to the lane's base.
        struct Ops { double ghj, ba[NX], a0, a1; };                        // (ghj: gh_j on lanes 0..6, q_i on lanes 8..12)
        const double *const fb = L.Hh + (li < NU ? FB_R0 + li : FB_LXU + 2 * i5);      // own pair in a factor block (lanes >= 7 follow lane 2: their values are not used)
        constexpr int HS8 = hstride<CP>() * B8, YS8 = (CP == 3 ? hstride<CP>() : NU) * B8;
        const BaLane bc = ba_column(N, ls);
        double bac[NX];
        if constexpr (CP) {
#pragma unroll
            for (int m = 2; m < NX; m++) bac[m] = L.tab[ba_off(N, 0, m, ls)];
        }
        // q rides in the gh load: lanes 8..12 of the row, idle in the sweeps, read q_i = dpi[(k + 1) NX + i] where they used to re-read gh[k NV] --
        // a per-lane (pointer, stride) pair --, and one row shift by six lanes hands it to lane 2 + i: the same value, one LDS load per stage fewer
        const bool ql = li >= 8 && li < 8 + NX;
        const double *ghq = ql ? L.dpi + NX + (li - 8) : L.gh + ls;
        const int ghs = (ql ? NX : NV) * B8;
        const double *const tcb = CP ? L.tab + bc.o0 : L.BA + ls;          // own column of [B A]: rows x, y in the table / the dense block
        const int tcs = bc.st * B8;
        // ONE store per stage, of EVERY lane through a per-lane (base, stride) pair, as in the factorisation and in the forward sweep: y0 and y1 are row
        // broadcasts (every lane has them), so lane 0 stores y0 to y_k[0], lane 1 y1 to y_k[1] -- layout 3: inside the stage's block, at the block
        // stride --, lanes 2..6 p to pr[k NX + i], and the other lanes write to a dummy slot of L.scr (stride 0), which nobody reads -- the sweeping
        // wave is the only one at work between the barriers around the sweeps.  Before, lane 0 stored the pair (y0, y1) and lanes 2..6 p in a second
        // instruction through an address pair of its own: per stage one LDS instruction and one v_mad_u32_u24 fewer for two selects (four
        // v_cndmask_b32); the same values at the same addresses, and p_k still takes the slot of q_{k-1} after that slot's load (above).  +1.3 % on the
        // bench launch, profiles/riccati_pivot_pair_store_ab.jsonl.  (History: predicated, each store was an s_and_saveexec / s_or pair around a block
        // of the stage loop, 18 -> 8 SALU instructions per trip of two stages, profiles/riccati_stage_addresses_ab.jsonl.)
        double *const dumb = L.scr + (CP ? RDUM_BASE_COMPACT : RDUM_BASE_FULL);
        const bool l0 = rowl && li == 0, l1 = rowl && li == 1;
        double *const pdb = xl ? L.pr + i5 : (l0 || l1) ? ysl<CP>(L, 0) + li : dumb + RDUM_P;
        const int pds = xl ? NX * B8 : (l0 || l1) ? YS8 : 0;
        auto load_stage = [&](Ops &o, int k) {
            const double *Fb = at8u(fb, k, HS8);
            o.ghj = *at8(ghq, k, ghs);
            if constexpr (CP) {
                { const double *Tc = at8(tcb, k, tcs); o.ba[0] = Tc[0]; o.ba[1] = Tc[1]; }       // rows x, y of the own column: one load
#pragma unroll
                for (int l = 2; l < NX; l++) o.ba[l] = bac[l];
            } else {
                const double *BA = at8u(tcb, k, NX * NV * B8);
#pragma unroll
                for (int l = 0; l < NX; l++) o.ba[l] = BA[l * NV];
            }
            o.a0 = Fb[0]; o.a1 = Fb[1];
        };
        auto stage = [&](const Ops &o, int k) {
            const double Pb = p + dpp_shift_zero<0x106>(o.ghj);           // row_shl:6: lane 2 + i takes lane 8 + i's q_i
            double fj = o.ghj;
            bwd_chain_update(fj, Pb, o.ba);                                // fj += sum_l ba[l] bcast16<NU + l>(Pb)
            const double y0 = bcast16<0>(fj * o.a0);                       // lane 0: fj 1/L00
            const double y1 = bcast16<1>((fj - o.a0 * y0) * o.a1);         // lane 1: (fj - L10 y0) 1/L11   (its a0 is L10)
            p = fj - o.a0 * y0 - o.a1 * y1;                                // lanes 2..6: fj - Lxu_i0 y0 - Lxu_i1 y1
            *at8(pdb, k, pds) = l0 ? y0 : (l1 ? y1 : p);
        };
        Ops oa, ob;
        load_stage(oa, N - 1);
        if (xl) L.pr[N * NX + i5] = p;                                    // (after the load of q_{N-1}: same slot when aliased)
        int k = N - 1;
        for (; k >= 1; k -= 2) {
            load_stage(ob, k - 1);
            stage(oa, k);
            load_stage(oa, k >= 2 ? k - 2 : 0);                           // unconditional (clamped): a branch here makes the
                                                                          // compiler wait for ALL outstanding LDS loads at the join
            stage(ob, k - 1);
        }
        if (k == 0) stage(oa, 0);
    }
    }
    mid();
    }
    SWEEP_T(SP_SOLVE_BWD);
    // forward sweep; dx_0 = 0 (dx lives in lanes 2..6).  dx+ = A dx + B du + rb with A = I + E (E: columns psi, v).
    if (sweeper) {
        double dx = 0.0;
        // Operand merging as in the backward sweep, two loads per stage fewer:
        //   yr        lane 0: y0, lane 8: y1, lanes 2..6 and 10..14: rb_i -- a per-lane (pointer, stride) pair, like the factorisation's hrow / bo[] / bst[];
        //             layout 3 keeps y inside the stage's block: another base and stride, the same load
        //   (a0, a1)  lane 0: (1/L00, L10), lane 8: (1/L11, -), lanes 2 + i: (Lxu_i0, -), lanes 10 + i: (Lxu_i1, -); a1 counts on lane 0 only.  (Before, the
        //             Lxu pair had ONE register set of its own, re-loaded right after its last use early in the stage, because two sets pushed the compact
        //             kernels into scratch; with y0, y1, rb_i in one register the merged pair fits the double-buffered set: 14 doubles where 9 + 9 + 2 were live.)
        // Two lane groups: the second column of Lxu has a SHADOW group on the row's upper half, which the forward sweep left idle.  Group A (lanes 0..6) is the
        // stage vector as everywhere; in group B lane 8 plays the second input (y1, 1/L11) and lanes 10..14 run a copy of dx: the same rb_i, the same row of
        // [B E], the same broadcast u0, u1, dpsi, dv -- taken from group A --, so their dx is bit for bit group A's.  With a0 = column 0 of Lxu on group A and
        // column 1 on group B, ONE product a0 dx and ONE chain of five shifted adds reduce both columns at once (lane 0 sums lanes 2..6, lane 8 lanes 10..14,
        // each in the order m = 0..4 the two chains of row broadcasts had): per stage 1 multiply + 5 adds where 2 + 10 were, the same bits
        // (profiles/forward_sweep_half_row_ab.jsonl).  Only group A stores.
        struct Ops { double yr, a0, a1, a_psi, a_v, b_a, b_w; };
        const bool shb = li >= 8 && li < 8 + NV;                           // group B: lane 8 + j shadows lane j
        const int lj = shb ? li - 8 : ls, j5 = lj >= NU ? lj - NU : 0;     // (lj: the lane's role; lanes 1 and 9 load like lanes 0 and 8 and are not read)
        const double *yrb = lj < NU ? ysl<CP>(L, 0) + (shb ? 1 : 0) : L.rb + j5;
        const int yrs = (lj < NU ? (CP == 3 ? hstride<CP>() : NU) : NX) * B8;
        const double *const fb = L.Hh + (lj < NU ? (shb ? FB_R1 : FB_R0) : FB_LXU + 2 * j5 + (shb ? 1 : 0));
        constexpr int HS8 = hstride<CP>() * B8;
        const double i_psi = lj == ZPSI ? 1.0 : 0.0, i_v = lj == ZV ? 1.0 : 0.0;
        const BaLane br = ba_row4(N, j5);
        const double *const trb = CP ? L.tab + br.o0 : L.BA + j5 * NV;     // own row of [B E] in the table / of [B A] in the dense block
        const int trs = br.st * B8;
        // ONE store per stage, of every lane, with a dummy slot outside the group as in the backward sweep: lane j of the writing row stores component j of
        // the stage's step [du; dx] -- lane 0 u0, lane 1 u1 (both are row broadcasts: every lane has them), lanes 2..6 dx.  Before, lane 0 stored the pair
        // and lanes 2..6 dx in a second instruction through an address of its own: per stage one LDS instruction and one address multiply-add fewer for two
        // selects (four v_cndmask_b32); the same values at the same addresses.  The vector sweeps follow their LDS instructions, not their VALU count:
        // +2.4 % on the bench launch for 3 VALU instructions MORE per stage (profiles/forward_sweep_fused_sum_ab.jsonl, record one_store).
        double *const dumb = L.scr + (CP ? RDUM_BASE_COMPACT : RDUM_BASE_FULL);
        const bool l0 = rowl && li == 0;
        const bool l1 = rowl && li == 1;
        double *const vdb = rowl ? L.dv + ls : dumb + RDUM_P;
        const int vds = rowl ? NV * B8 : 0;
        auto load_stage = [&](Ops &o, int k) {
            const double *Fb = at8u(fb, k, HS8);
            o.yr = *at8(yrb, k, yrs);
            o.a0 = Fb[0]; o.a1 = Fb[1];
            if constexpr (CP) {
                const double *Tr = at8(trb, k, trs);                       // own row of [B E] as (b_a, b_w, e_psi, e_v), at stride 2
                o.a_psi = Tr[4]; o.a_v = Tr[6];
                o.b_a = Tr[0]; o.b_w = Tr[2];
            } else {
                const double *BAr = at8u(trb, k, NX * NV * B8);             // own row of [B A]
                o.a_psi = BAr[ZPSI]; o.a_v = BAr[ZV];                      // loads only: arithmetic here would wait for them
                o.b_a = BAr[ZA]; o.b_w = BAr[ZW];
            }
        };
        auto stage = [&](const Ops &o, int k) {
            // du = -Luu^-T (Lxu^T dx + y)
            // Round 6 (round-5 verdict next-2 (a)): a lane keeps ITS OWN pair of Lxu -- one LDS load per stage instead of the five row-uniform ones that gave
            // every lane all ten entries --, multiplies it by its own dx, and the ten products are summed by row broadcasts: 22 VALU instructions where the
            // product form (round 4) has 13, four LDS instructions fewer.  At eight trajectories per CU the LDS unit is the busier one (65 % of the kernel
            // time, most of it these sweeps): cfg 2 1.288 -> 1.343 M solves/s (+4.3 %, profiles/round6_saturated_levers_ab.jsonl).
            // Every kernel family takes it (the fast and the compact kernel of a shape stay bitwise equal); the sums associate differently: rounding level.
            // (the products are read from lanes 2..6 and 10..14 only, where a 0 / 1 lane mask that used to multiply them was 1.0: gone, same bits)
            const double pa = o.a0 * dx;                                   // lanes 2..6: Lxu_i0 dx_i, lanes 10..14: Lxu_i1 dx_i
            double s = o.yr;
            static_for<0, NX>([&](auto m_) { constexpr int m = decltype(m_)::value; s += dpp_shift_zero<0x100 + NU + m>(pa); });      // row_shl:(2 + m)
            double dxs[NX];
            dxs[ZPSI - NU] = bcast16<ZPSI>(dx); dxs[ZV - NU] = bcast16<ZV>(dx);
            const double u1 = bcast16<8>(-s * o.a0);                       // lane 8: -s1 1/L11
            const double u0 = bcast16<0>((-s - o.a1 * u1) * o.a0);         // lane 0: (-s0 - L10 u1) 1/L00   (its a1 is L10)
            *at8(vdb, k, vds) = l0 ? u0 : (l1 ? u1 : dx);
            const double dpsi = dxs[ZPSI - NU], dvv = dxs[ZV - NU];
            // compact layouts: the table rows hold E = A - I itself (ba_tab_init); the dense [B A] of the other layouts holds A
            const double e_psi = CP ? o.a_psi : o.a_psi - i_psi, e_v = CP ? o.a_v : o.a_v - i_v;
            dx = dx + e_psi * dpsi + e_v * dvv + o.b_a * u0 + o.b_w * u1 + o.yr;   // lanes 2..6 meaningful (their yr is rb_i)
        };
        Ops oa, ob;
        load_stage(oa, 0);
        int k = 0;
        for (; k + 1 < N; k += 2) {
            load_stage(ob, k + 1);
            stage(oa, k);
            load_stage(oa, k + 2 < N ? k + 2 : N - 1);                    // unconditional (clamped), see the backward sweep
            stage(ob, k + 1);
        }
        if (k < N) stage(oa, k);
        if (rowl) L.dv[N * NV + li] = xl ? dx : 0.0;
    }
    SWEEP_T(SP_SOLVE_FWD);
}

template <int NTH, int CP = 0, bool SQ = false>
__device__ __forceinline__ void riccati_solve(const Lds &L, const Dims &d, int tid, int sw = 1)
{
    asm volatile("" : "+v"(tid));                    // opaque per call (see riccati_factor): the two solves of an iteration do not share address registers
    // two-wave variant: the vector sweeps run on the wave that did not factorise, so that with two trajectories' waves
    // sharing a SIMD pair the sequential work is spread over both SIMDs
    const bool sweeper = NTH == 64 || (tid >> 6) == sw;
    const int lane = NTH == 64 ? tid : (sweeper ? (tid & 63) : 64);
    SWEEP_COUNT(SP_CALLS_SOLVE);
    riccati_solve_pre<CP, SQ>(L, d, tid, NTH);
    __syncthreads();
    TMPC_PRIO_HIGH();
    riccati_sweeps_rows<CP, true>(L, d, lane, true, sweeper, [] { __syncthreads(); });
    TMPC_PRIO_LOW();
    __syncthreads();
    riccati_solve_post<CP, SQ>(L, d, tid, NTH);
    __syncthreads();
}

// The rest of the predictor solve after a VEC factorisation: the forward sweep.
template <int NTH, int CP = 0>
__device__ __forceinline__ void riccati_forward(const Lds &L, const Dims &d, int tid, int sw = 1)
{
    asm volatile("" : "+v"(tid));
    const bool sweeper = NTH == 64 || (tid >> 6) == sw;
    const int lane = NTH == 64 ? tid : (sweeper ? (tid & 63) : 64);
    SWEEP_COUNT(SP_CALLS_SOLVE);
    TMPC_PRIO_HIGH();
    riccati_sweeps_rows<CP, false>(L, d, lane, true, sweeper, [] {});
    TMPC_PRIO_LOW();
    __syncthreads();
    // (round 6: no closing loop here.  dpi = P dx + p is the step of the dynamics multipliers, and the PREDICTOR's is never used -- the row passes between
    //  predictor and corrector read dv only, the update takes the corrector's dpi: one stage-parallel pass and one barrier per interior-point iteration less)
}

}  // namespace tmpc
