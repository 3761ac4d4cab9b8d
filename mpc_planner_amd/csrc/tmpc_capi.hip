// mpc_planner_amd/csrc/tmpc_capi.hip -- the C-ABI translation unit of libtmpc_hip.so (include/tmpc_hip.h): kernel dispatch tables, the handle, every
// exported entry point, and the small kernels around the solve (tmpc_aux_kernels.hpp: selection, records, gather, f-1 / f-2 / f-3 helpers).
// The solve kernels themselves are templates (tmpc_kernels.hpp) instantiated in the units of tmpc_solve.hip; this unit declares them `extern`
// (tmpc_instances.hpp) and only takes their addresses.  A GENERATED solver (-DTMPC_GENERATED_STAGE, mpc_planner_amd/codegen/build.py) and the
// experiment builds that pass -DTMPC_SINGLE_TU compile this file ALONE: without the extern declarations every kernel the tables name is
// instantiated here.
#include <algorithm>
#include <cstring>
#include <memory>
#include "tmpc_kernels.hpp"
#include "tmpc_handle_layout.hpp"
#include "tmpc_instances.hpp"
#if !defined(TMPC_GENERATED_STAGE) && !defined(TMPC_SINGLE_TU)
TMPC_ALL_INSTANCES(EXT)
extern template __global__ void tmpc::tmpc_solve_fast_kernel<8, 8, 6, 128, true, tmpc::ScanSolo>(TMPC_KARGS);
extern template __global__ void tmpc::tmpc_solve_fast_kernel<8, 8, 2, 64, true>(TMPC_KARGS);
#endif
#include "tmpc_aux_kernels.hpp"
// The lane-per-trajectory kernel family (tmpc_lanes.hip, tmpc_set_throughput_mode) is an OPTIONAL part of the library since round 5: it loses to
// the wave kernels on every shape measured and is kept for its persistent-state protocol on arbitrary shapes.  -DTMPC_WITH_LANES links
// it (__graft_entry__.build(with_lanes=True) / TMPC_BUILD_LANES=1); without it tmpc_set_throughput_mode reports that the build has no such kernels.
// Lab switches (kernel selection overrides for A/B measurements and for tests that have to reach one particular kernel family): environment variables
// TMPC_* read when a handle is created.  They exist ONLY in a library built with -DTMPC_LAB_SWITCHES (mpc_planner_amd/libtmpc_hip_lab.so, which
// __graft_entry__.build() links from the same kernel objects; tools/build_compact_variants.sh): the product library never reads the environment -- what a
// drop-in does depends on the C-ABI calls alone (round-5 verdict, next-8).  INTEGRATION.md section 7 lists them.  (Defined for every build, the lane
// family's included: tests/test_dispatch_table.py compiles this unit with and without -DTMPC_WITH_LANES.)
#ifdef TMPC_LAB_SWITCHES
static inline const char *lab_env(const char *name) { return getenv(name); }
#else
static inline const char *lab_env(const char *) { return nullptr; }
#endif
#ifdef TMPC_WITH_LANES
#include "tmpc_lanes_api.hpp"
#else
namespace tmpc {
namespace lanes {
struct Context;
static const char *const kAbsent = "this build of the library does not contain the lane-per-trajectory kernels (build with TMPC_BUILD_LANES=1 / build(with_lanes=True))";
static inline Context *create(const Dims &, int, std::string &err) { err = kAbsent; return nullptr; }
static inline void destroy(Context *) {}
static inline int stage_in(Context *, hipStream_t, int, const double *, const double *, const double *, bool, bool, std::string &err) { err = kAbsent; return 1; }
static inline int solve(Context *, hipStream_t, int, int, bool, bool, double *, double *, double *, int *, int *, int *, double *, int *, std::string &err) { err = kAbsent; return 1; }
static inline int reset_multipliers(Context *, hipStream_t, int, std::string &err) { err = kAbsent; return 1; }
static inline int clear_stopped(Context *, hipStream_t, int, std::string &err) { err = kAbsent; return 1; }
}  // namespace lanes
}  // namespace tmpc
#endif

// =================================================================================================
// C-ABI
// =================================================================================================
namespace tmpc {
typedef void (*SolveKernel)(Dims, int, const double *, const double *, const double *, double *, double *, double *, int *,
                            int *, int *, double *, int *, long long *, StateIO);
// ---- the solve-kernel slots of a handle ---------------------------------------------------------------------------------------------------------
// A handle holds up to six solve kernels, one per slot (the labels tmpc_kernel_info reports); launch_slot() chooses the one a launch runs.
enum Slot {
    SLOT_DEFAULT,   // the fast kernel of the shape, else the generic kernel; on a one-wave compact handle the compact kernel (pick_compact_kernel)
    SLOT_SMALL,     // one-wave compact handles: the fast one-wave kernel, for launches of AT MOST `bound` trajectories (what it holds resident at once)
    SLOT_CP2,       // beside a two-wave fast default: the compact two-wave kernel, for launches of MORE THAN `bound` trajectories (what the default
                    //   holds resident at once)
    SLOT_LAT1,      // latency mode 1: two waves per trajectory (pick_latency_kernel)
    SLOT_LAT2,      // latency mode 2: parallel-in-time Newton solve (pick_scan_kernel)
    SLOT_LAT3,      // latency mode 3: four waves per trajectory (pick_quad_kernel)
    SLOT_COUNT
};
struct KernelSlot {
    enum Kind { GENERIC, FAST, COMPACT };
    SolveKernel kernel = nullptr;   // nullptr: the slot is not filled
    SolveKernel twin = nullptr;     // the instrumented instantiation tmpc_debug_profile runs in its place (nullptr: none; the generic kernel is its own)
    const char *name = "";          // the instantiation (pick_*_kernel's names; "generic<CM>" for the generic kernel): tmpc_kernel_info reports it
    Kind kind = FAST;               // COMPACT: a persistent launch -- grid = min(B, resident), the handle's ws + ticket
    int threads = 0;                // threads per trajectory
    size_t lds_bytes = 0;
    int lay = 1;                    // compact kernels: the Hh layout (compact_layout, tmpc_fast.hpp)
    int dpad = 0;                   // Dims::dpad: compact kernels' stage-stride padding (choose_compact_pad); the fast layouts do not pad
    bool prio = false;              // Dims::prio: wave issue priorities (set_resident)
    int resident = 0;               // compact kernels: the workgroups the device holds at once
    int bound = 0;                  // small / cp2: the launch-size bound (Slot)
};
// Registered fast shapes (upper-bounded rows n_lin + n_slk, ellipsoids M) x lanes-per-stage; anything else runs the generic kernel.
// Only instantiations that compile WITHOUT scratch (zero VGPR spills) are registered: __graft_entry__.build() checks
// the compiler's resource remarks and fails otherwise.  Reason: with > ~100 spilled VGPRs this kernel was observed to
// return wrong iterates (spill/reload around partially-masked regions), see DESIGN.md section 5.  Shapes with more rows
// per lane ((8,8) at 2 lanes/stage for N > 21, (12,12) at 2 lanes/stage) therefore use the generic kernel for now.  The library is
// built with -mllvm -disable-machine-licm: hoisted constant materialisations were what pushed (12,12,3) into scratch.
// Every instantiation a pick_*_kernel function returns is written through one of the macros below.  Each fills the slot *s from the template
// arguments as written: the name "fast<NLIN,MM,LPS,NTH,TEAM,CM>" / "compact<NLIN,MM,LPS,NTH,CM>" (tests/test_dispatch_table.py reads the same
// macro calls from this file and requires a test case for each name), the threads (NTH), the kind, the compact layout and the profiled twin;
// it yields the production kernel.
//   TMPC_FAST(NLIN, MM, LPS, NTH)        MPCC + ellipsoid rows (TEAM = Solo, CM = 0), with a profiled twin
//   TMPC_FASTP(NLIN, MM, LPS, NTH, TEAM) another TEAM (CM = 0), with a profiled twin
//   TMPC_FASTX(NLIN, MM, LPS, NTH, TEAM, CM) no profiled twin
//   TMPC_CP(NLIN, MM, LPS, CM) / TMPC_CP2(NLIN, MM, LPS, CM)   compact one-wave / two-wave kernels (persistent: tmpc_debug_profile runs the fast kernel
//                                                              of the shape instead)
#define TMPC_INST(nm, nth, kind_, lay_, twin_, k) (s->name = (nm), s->threads = (nth), s->kind = KernelSlot::kind_, s->lay = (lay_), s->twin = (twin_), (k))
#define TMPC_FAST(a, b, c, t) TMPC_INST("fast<" #a "," #b "," #c "," #t ",Solo,0>", t, FAST, 1, (SolveKernel)(tmpc_solve_fast_kernel<a, b, c, t, true>), \
                                        (SolveKernel)(tmpc_solve_fast_kernel<a, b, c, t, false>))
#define TMPC_FASTP(a, b, c, t, team) TMPC_INST("fast<" #a "," #b "," #c "," #t "," #team ",0>", t, FAST, 1, (SolveKernel)(tmpc_solve_fast_kernel<a, b, c, t, true, team>), \
                                               (SolveKernel)(tmpc_solve_fast_kernel<a, b, c, t, false, team>))
#define TMPC_FASTX(a, b, c, t, team, m) TMPC_INST("fast<" #a "," #b "," #c "," #t "," #team "," #m ">", t, FAST, 1, nullptr, \
                                                  (SolveKernel)(tmpc_solve_fast_kernel<a, b, c, t, false, team, m>))
static SolveKernel pick_fast_kernel(const Dims &d, KernelSlot *s)
{
    if (lab_env("TMPC_FORCE_GENERIC")) return nullptr;
    const int lps = (3 * d.N <= NT) ? 3 : ((2 * d.N <= NT) ? 2 : 0);
#ifndef TMPC_GENERATED_STAGE
    if (d.cost_model == 1 && d.row_model == 1) return nullptr;      // curvature-aware cost AND Gaussian rows (CM = 3, round 6): the generic kernel and the four-wave tick kernel of 21 <= N <= 31
    if (d.cost_model == 1) {
        // curvature-aware contouring (BASELINE configs[2]): the cfg-3 shape on the two-wave kernel, every other row mix of N <= 20 on the
        // runtime-shape one-wave kernel, anything else on the generic kernel -- all instantiated with CM = 1 (no profiled twins)
        const int nrc = d.n_up + d.M + 14;
        if (lps != 3 && 4 * d.N <= 128 && d.n_up == 20 && d.M == 8 && !lab_env("TMPC_NO_TWO_WAVE")) return TMPC_FASTX(20, 8, 4, 128, Solo, 1);
        if (lps == 3 && nrc <= 3 * 13) return TMPC_FASTX(-1, 13, 3, 64, Solo, 1);
        return nullptr;
    }
    if (d.row_model == 1) {
        // Gaussian chance-constraint rows instead of the ellipsoids (mpc_planner_jackal's default: N = 30, 5 topology + 5 Gaussian rows):
        // runtime-shape instantiations with CM = 2 (no profiled twins) -- two-wave for 22 <= N <= 32, one-wave for N <= 21, else the generic kernel
        const int nrg = d.n_up + d.M + 14;
        // mpc_planner_jackal's default (generate_jackal_solver.py:53-73: N = 30, 5 + 5 rows) on ONE wave at two lanes per stage (round 6): twelve rows per lane
        // fit the registers, and eight one-wave trajectories per CU keep eight waves busy where four two-wave ones idle a wave through every Riccati sweep --
        // saturated +27 % (585 -> 741 k solves/s).  Its small-launch twin below, the compact kernel in pick_compact_kernel; ticks: latency modes 2 / 3.
        if (lps == 2 && d.n_up == 5 && d.M == 5 && !lab_env("TMPC_NO_ONE_WAVE_N30")) return TMPC_FASTX(5, 5, 2, 64, Solo, 2);
        if (lps != 3 && 4 * d.N <= 128 && !lab_env("TMPC_NO_TWO_WAVE")) {
            if (d.n_up == 5 && d.M == 5) return TMPC_FASTX(5, 5, 4, 128, Solo, 2);     // mpc_planner_jackal's default (generate_jackal_solver.py:53-73), tuned
            if (nrg <= 4 * 6) return TMPC_FASTX(-1, 6, 4, 128, Solo, 2);
            if (nrg <= 4 * 12) return TMPC_FASTX(-1, 12, 4, 128, Solo, 2);
        }
        if (lps == 3 && nrg <= 3 * 13) return TMPC_FASTX(-1, 13, 3, 64, Solo, 2);
        return nullptr;
    }
#endif
#ifdef TMPC_GENERATED_STAGE
    // generated solver: one row shape (tmpc_gen::NH upper-bounded rows); the fast instantiations are compiled only when the
    // generator's build found them free of scratch (TMPC_GEN_FAST / TMPC_GEN_FAST2 set by codegen/build.py)
#ifdef TMPC_GEN_FAST
    if (lps == 3) return TMPC_FAST(tmpc_gen::NH, 0, 3, 64);
#endif
#ifdef TMPC_GEN_FAST2
    if (lps != 3 && 4 * d.N <= 128) return TMPC_FAST(tmpc_gen::NH, 0, 4, 128);
#endif
    return nullptr;
#else
    const int nr = d.n_up + d.M + 14;                    // interior-point rows per stage
    // the jackalsimulator T-MPC stack at the horizon it ships with (8 + 8 rows, N = 30; settings.yaml) on ONE wave at two lanes per stage (round 6, like
    // mpc_planner_jackal's default above: fifteen rows per lane still fit the registers); its compact twin in pick_compact_kernel, its profiled twin
    // in tmpc_solve.hip (TMPC_TU_PROF)
    if (lps == 2 && d.n_up == 8 && d.M == 8 && !lab_env("TMPC_NO_ONE_WAVE_N30")) return TMPC_FAST(8, 8, 2, 64);
    if (lps != 3 && 4 * d.N <= 128 && !lab_env("TMPC_NO_TWO_WAVE")) {
        // two waves per trajectory, 4 lanes per stage (22 <= N <= 32: the reference's default N = 30 and BASELINE cfg 3)
        if (d.n_up == 8 && d.M == 8) return TMPC_FAST(8, 8, 4, 128);
        if (d.n_up == 12 && d.M == 12) return TMPC_FAST(12, 12, 4, 128);  // mpc_planner_jackalsimulator defaults (N = 30, 12 obstacles)
        if (d.n_up == 20 && d.M == 8) return TMPC_FAST(20, 8, 4, 128);    // cfg 3: 8 topology + 12 decomp rows + 8 ellipsoids
        if (nr <= 4 * 6) return TMPC_FAST(-1, 6, 4, 128);                 // any other row mix: runtime-shape instantiations
        if (nr <= 4 * 9) return TMPC_FAST(-1, 9, 4, 128);                 //   (e.g. mpc_planner_jackal: N = 30, 5 obstacles)
        if (nr <= 4 * 12) return TMPC_FAST(-1, 12, 4, 128);
    }
    if (lps == 3) {
        if (d.n_up == 0 && d.M == 4) return TMPC_FAST(0, 4, 3, 64);
        if (d.n_up == 8 && d.M == 8) return TMPC_FAST(8, 8, 3, 64);
        if (d.n_up == 12 && d.M == 12) return TMPC_FAST(12, 12, 3, 64);      // zero scratch only with machine-LICM off (build flag)
        if (d.n_up == 24 && d.M == 0) return TMPC_FAST(24, 0, 3, 64);        // SH-MPC: 24 scenario halfspaces (cfg 5)
        if (nr <= 3 * 7) return TMPC_FAST(-1, 7, 3, 64);                     // runtime-shape instantiations
        if (nr <= 3 * 10) return TMPC_FAST(-1, 10, 3, 64);
        if (nr <= 3 * 13) return TMPC_FAST(-1, 13, 3, 64);
        if (d.N <= 2 * (64 / 6) && nr <= 6 * 9 && !lab_env("TMPC_NO_TWO_WAVE"))    // more rows: two waves, 6 lanes per stage
            return TMPC_FAST(-1, 9, 6, 128);                                 //   (mpc_planner_rosnavigation T-MPC: 24 + 12 rows)
    } else if (lps == 2) {
        if (d.n_up == 0 && d.M == 4) return TMPC_FAST(0, 4, 2, 64);
    }
    return nullptr;
#endif
}
// Square-root form of the Riccati recursion (tmpc_dims.riccati_form = TMPC_RICCATI_SQUARE_ROOT; csrc/tmpc_riccati.hpp SQ): run-time-shape fast kernels only
// -- a comparison aid (HPIPM's default recursion) with one instantiation per kernel family member that the BASELINE shapes need, not a throughput path.
static SolveKernel pick_sqrt_kernel(const Dims &d, KernelSlot *s)
{
#ifndef TMPC_GENERATED_STAGE
    const int nr = d.n_up + d.M + 14, sm = stage_model(d);
    if (3 * d.N <= NT) {
        if (sm == 0 && nr <= 3 * 13) return TMPC_FASTX(-1, 13, 3, 64, SoloSqrt, 0);
        return nullptr;
    }
    if (4 * d.N <= 128 && nr <= 4 * 12) {
        if (sm == 0) return TMPC_FASTX(-1, 12, 4, 128, SoloSqrt, 0);
        if (sm == 1 && d.n_up == 20 && d.M == 8) return TMPC_FASTX(20, 8, 4, 128, SoloSqrt, 1);      // cfg 3 as named (CA-MPC)
    }
#endif
    (void)d; (void)s;
    return nullptr;
}
// Compact variant (tmpc_fast.hpp: tmpc_solve_compact_kernel): two waves per SIMD, eight trajectories per CU, persistent
// workgroups.  Bitwise the same results as the fast kernel of the shape (tools/ab_compare.py against TMPC_NO_COMPACT=1).
// Round 4: the shapes with 13 rows per lane ((12,12) and (24,0) at three lanes per stage: cfg 4, cfg 5) fit 256 registers too since the
// row passes are specialised by the compile-time kind of each row slot (FastCfg::KIND): 238 registers, zero scratch; their larger row tables
// allow 7 (cfg 4: 23.3 KB) and 6 (cfg 5: 25.2 KB) workgroups per CU.  The runtime-shape instantiation with 13 rows per lane still spills
// (168 B) and is not registered.
// The layout: the instantiation's Hh layout (compact_layout, tmpc_fast.hpp) -- evaluated on the template arguments where they are written, so that
// the host's LDS size and the kernel's layout cannot disagree
#define TMPC_CP(a, b, c, m) TMPC_INST("compact<" #a "," #b "," #c ",64," #m ">", 64, COMPACT, compact_layout(a, b, 64), nullptr, \
                                      (SolveKernel)(tmpc_solve_compact_kernel<a, b, c, false, 64, m>))
#define TMPC_CP2(a, b, c, m) TMPC_INST("compact<" #a "," #b "," #c ",128," #m ">", 128, COMPACT, compact_layout(a, b, 128), nullptr, \
                                       (SolveKernel)(tmpc_solve_compact_kernel<a, b, c, false, 128, m>))
static SolveKernel pick_compact_kernel(const Dims &d, KernelSlot *s)
{
#ifndef TMPC_GENERATED_STAGE
    if (!lab_env("TMPC_FORCE_GENERIC") && !lab_env("TMPC_NO_COMPACT") && !lab_env("TMPC_NO_ONE_WAVE_N30") && 2 * d.N <= NT && 3 * d.N > NT) {
        // 22 <= N <= 32 on one wave, two lanes per stage (pick_fast_kernel): mpc_planner_jackal's default, the jackalsimulator stack
        if (stage_model(d) == 2 && d.n_up == 5 && d.M == 5) return TMPC_CP(5, 5, 2, 2);
        if (stage_model(d) == 0 && d.n_up == 8 && d.M == 8) return TMPC_CP(8, 8, 2, 0);
    }
    if (lab_env("TMPC_FORCE_GENERIC") || lab_env("TMPC_NO_COMPACT") || d.N > 20 || (stage_model(d) != 0 && stage_model(d) != 2)) return nullptr;
    if (stage_model(d) == 2) {                       // Gaussian chance-constraint rows (round 6): the run-time-shape instantiation with up to ten rows per lane
        if (d.n_up + d.M + 14 <= 3 * 10) return TMPC_CP(-1, 10, 3, 2);
        return nullptr;
    }
    const int nr = d.n_up + d.M + 14;                    // interior-point rows per stage
    if (d.n_up == 8 && d.M == 8) return TMPC_CP(8, 8, 3, 0);
    if (d.n_up == 0 && d.M == 4) return TMPC_CP(0, 4, 3, 0);
    if (d.n_up == 12 && d.M == 12) return TMPC_CP(12, 12, 3, 0);
    if (d.n_up == 24 && d.M == 0) return TMPC_CP(24, 0, 3, 0);
    if (nr <= 3 * 7) return TMPC_CP(-1, 7, 3, 0);       // runtime-shape instantiations
    if (nr <= 3 * 10) return TMPC_CP(-1, 10, 3, 0);
#endif
    (void)d; (void)s;
    return nullptr;
}
// Two-wave compact variant (round 4: 22 <= N <= 32, four lanes per stage -- the reference's N = 30 defaults, cfg 3): the same kernel with
// NTH = 128.  236 / 251 registers, zero scratch, 27-39 KB of LDS: FOUR trajectories per CU (two waves each, two waves per SIMD) where the
// fast two-wave kernel (57-70 KB of LDS) holds two.  Bitwise the same results; a trajectory takes longer on it (NLP data in the global
// workspace, the linearisation on one of the two waves), so launch_solve uses it only for launches that the fast kernel could not hold
// resident at once (more than two trajectories per CU).  The runtime-shape instantiation with 12 rows per lane spills (144 B): not registered.
static SolveKernel pick_compact2_kernel(const Dims &d, KernelSlot *s)
{
#ifndef TMPC_GENERATED_STAGE
    if (lab_env("TMPC_FORCE_GENERIC") || lab_env("TMPC_NO_COMPACT") || lab_env("TMPC_NO_TWO_WAVE") || 3 * d.N <= NT || 4 * d.N > 128) return nullptr;
    const int nr = d.n_up + d.M + 14, sm = stage_model(d);
    if (sm == 1) return (d.n_up == 20 && d.M == 8) ? TMPC_CP2(20, 8, 4, 1) : nullptr;      // cfg 3 as named (CA-MPC)
    if (sm == 2) {                                                                                                                   // Gaussian chance-constraint rows
        if (d.n_up == 5 && d.M == 5) return TMPC_CP2(5, 5, 4, 2);                          // mpc_planner_jackal's default, tuned (round 5)
        return nr <= 4 * 6 ? TMPC_CP2(-1, 6, 4, 2) : nullptr;
    }
    if (sm != 0) return nullptr;
    if (d.n_up == 20 && d.M == 8) return TMPC_CP2(20, 8, 4, 0);
    if (d.n_up == 12 && d.M == 12) return TMPC_CP2(12, 12, 4, 0);
    if (d.n_up == 8 && d.M == 8) return TMPC_CP2(8, 8, 4, 0);
    if (nr <= 4 * 6) return TMPC_CP2(-1, 6, 4, 0);
    if (nr <= 4 * 9) return TMPC_CP2(-1, 9, 4, 0);
#endif
    (void)d; (void)s;
    return nullptr;
}
// Latency variant (tmpc_set_latency_mode): two waves per trajectory at 6 lanes per stage, built for two waves per SIMD
// (<= 256 registers, so four trajectories per CU stay resident).  The stage-parallel phases run on twice the lanes:
// -8 % kernel time on a 64-trajectory control tick; on a saturated GPU the one-wave kernel is as fast or faster, which is
// why it stays the default.  The variant is chosen by the caller, never by the batch size: a trajectory's result does
// not depend on what else is in the launch.
static SolveKernel pick_latency_kernel(const Dims &d, KernelSlot *s)
{
#ifndef TMPC_GENERATED_STAGE
    if (lab_env("TMPC_FORCE_GENERIC") || lab_env("TMPC_NO_TWO_WAVE") || d.N > 2 * (64 / 6) || stage_model(d) != 0) return nullptr;
    if (d.n_up == 8 && d.M == 8) return TMPC_FAST(8, 8, 6, 128);
#endif
    (void)d; (void)s;
    return nullptr;
}
// Latency variant 2 (tmpc_set_latency_mode(h, 2)): one wave per trajectory like the fast kernels, the interior-point Newton systems
// solved parallel in time (tmpc_scan.hpp) instead of by the sequential Riccati recursion.  One workgroup per CU is what a control
// tick gives it anyway: built for one wave per SIMD (all 512 registers, 73 KB of LDS).  Another factorisation of the same systems:
// steps agree with the recursion's to rounding (~1e-6 of a step on ill-conditioned late iterations, like the recursion itself
// against an exact solve), so iteration counts can differ by one where a residual sits at the tolerance -- the caller opts in.
// A profiled twin exists for the cfg-2 shape (8, 8) on two waves only.  *sl: the scan depth of the factorisation (tmpc_scan.hpp).
static SolveKernel pick_scan_kernel(const Dims &d, KernelSlot *s, int *sl)
{
    *sl = 3;
#ifndef TMPC_GENERATED_STAGE
    if (lab_env("TMPC_FORCE_GENERIC") || d.N > 31 || d.N < 2 || (stage_model(d) != 0 && stage_model(d) != 2)) return nullptr;
    const bool gauss = stage_model(d) == 2;                      // Gaussian chance-constraint rows (mpc_planner_jackal's default stack): the run-time-shape instantiations, CM = 2
    if (d.N > 20) {                                              // 21 <= N <= 31 (cfg 3, the reference's N = 30 defaults): two lanes per stage in the
        if (d.n_up + d.M + 14 > 4 * 12) return nullptr;          // Newton solve, the runtime-shape two-wave kernel (4 lanes per stage, up to 34 rows) around it
        *sl = 2;
        return gauss ? TMPC_FASTX(-1, 12, 4, 128, ScanSoloT<2>, 2) : TMPC_FASTX(-1, 12, 4, 128, ScanSoloT<2>, 0);
    }
    if (gauss) {
        if (d.N <= 2 * (64 / 6) && d.n_up + d.M + 14 <= 6 * 9) return TMPC_FASTX(-1, 9, 6, 128, ScanSolo, 2);
        return nullptr;
    }
    const char *w = lab_env("TMPC_SCAN_WAVES");               // A/B: "1" = one wave per trajectory
    if (d.n_up == 8 && d.M == 8 && d.N <= 2 * (64 / 6) && !(w && atoi(w) == 1)) return TMPC_FASTP(8, 8, 6, 128, ScanSolo);
    if (d.n_up == 8 && d.M == 8) return TMPC_FASTX(8, 8, 3, 64, ScanSolo, 0);
    if (d.N <= 2 * (64 / 6) && d.n_up + d.M + 14 <= 6 * 9)      // every other row mix of the one-wave shapes (cfg 1, cfg 4, cfg 5, ...): runtime row counts, two waves
        return TMPC_FASTX(-1, 9, 6, 128, ScanSolo, 0);
#else
    // generated solver: the slot stays empty.  The two-wave instantiations around emitted stage functions (dynamics and rows | emitted cost) were built and
    // measured: at every shape tried they were SLOWER than the library's default kernel (tmpc_cfg2 N = 20: 1.087 against 1.008 ms at 64 trajectories, 1.178
    // against 1.098 ms at 5; jackal_tmpc N = 30: 1.304 against 1.221 and 1.368 against 1.253 ms; profiles/generated_tick_kernels.json), so the project's rule
    // for a tick mode -- every run below every run of the default kernel -- keeps them out.  Mode 3 (pick_quad_kernel) is the generated tick kernel.
#endif
    (void)d; (void)s;
    return nullptr;
}
// Latency variant 3 (tmpc_set_latency_mode(h, 3), round 6): FOUR waves per trajectory -- a control tick of a few planners leaves a whole CU (four SIMDs,
// 160 KB of LDS) to every trajectory.  The stage evaluation is split four ways by content (dynamics | cost + halfspace rows | obstacle rows on two waves),
// the interior-point row passes run at twelve lanes per stage (three rows per lane instead of five), and the wide phases of the parallel-in-time
// factorisation (the stage phase: one column per lane instead of four; level 0 of the cyclic reduction: one instead of two) use all 256 lanes
// (csrc/tmpc_scan.hpp factor4).  Same algorithm as variant 2 (sums associate differently: rounding level).  N <= 20, hand-written MPCC stages.
// `ab`: TMPC_QUAD_AB=1 in a lab build picks the twin whose factorisation stays on one wave (A/B of the factorisation split alone).  *sl: as pick_scan_kernel.
static SolveKernel pick_quad_kernel(const Dims &d, bool ab, KernelSlot *s, int *sl)
{
    *sl = 3;
#ifndef TMPC_GENERATED_STAGE
    if (d.N > 20 && d.N <= 31 && !ab && d.n_up + d.M + 14 <= 8 * 6) {
        // 21 <= N <= 31 (the horizon the reference ships for jackal / jackalsimulator: N = 30): eight lanes per stage around the two-lanes-per-stage Newton solve;
        // every stage model (the four-wave linearisation regularises a coupled W -- curvature-aware cost -- on wave 0)
        *sl = 2;
        const int sm = stage_model(d);
        return sm == 0 ? TMPC_FASTX(-1, 6, 8, 256, ScanQuadT<2>, 0)
             : sm == 1 ? TMPC_FASTX(-1, 6, 8, 256, ScanQuadT<2>, 1)
             : sm == 2 ? TMPC_FASTX(-1, 6, 8, 256, ScanQuadT<2>, 2)
             : sm == 3 ? TMPC_FASTX(-1, 6, 8, 256, ScanQuadT<2>, 3) : nullptr;
    }
    if (d.N > 20 || d.N < 2 || (stage_model(d) != 0 && stage_model(d) != 2)) return nullptr;
    if (stage_model(d) == 2) return (d.n_up + d.M + 14 <= 12 * 4) ? TMPC_FASTX(-1, 4, 12, 256, ScanQuad, 2) : nullptr;      // Gaussian rows
    if (d.n_up == 8 && d.M == 8) return ab ? TMPC_FASTX(8, 8, 12, 256, ScanSolo, 0) : TMPC_FASTP(8, 8, 12, 256, ScanQuad);    // (a profiled twin: ScanQuad's only)
    if (d.n_up + d.M + 14 <= 12 * 4) return TMPC_FASTX(-1, 4, 12, 256, ScanQuad, 0);      // cfg 1, cfg 4, cfg 5, any row mix up to 34 rows
#else
    // generated solver: the run-time-shape instantiations around the emitted stage functions (tmpc_gen::NH upper-bounded rows, no ellipsoids), under the
    // product's row caps; compiled for the horizon ranges the emitted header names (GENERATED_STAGE_TICK_KERNELS, codegen/build.py tick_kernels).  A stack
    // without rows keeps the slot empty (no demo library covers it)
    if (tmpc_gen::NH == 0 || d.N > 31 || d.N < 2) return nullptr;
#if GENERATED_STAGE_TICK_KERNELS & 2
    if (d.N > 20) {
        if (d.n_up + d.M + 14 > 8 * 6) return nullptr;
        *sl = 2;
        return TMPC_FASTX(-1, 6, 8, 256, ScanQuadT<2>, 0);
    }
#endif
#if GENERATED_STAGE_TICK_KERNELS & 1
    if (d.N <= 20 && d.n_up + d.M + 14 <= 12 * 4) return TMPC_FASTX(-1, 4, 12, 256, ScanQuad, 0);
#endif
#endif
    (void)d; (void)ab; (void)s;
    return nullptr;
}
// ---- stage stride of the row Jacobians in LDS (Dims::dpad) --------------------------------------------------------------------
// LDS bank-conflict model of the row passes' coefficient loads (ipm_fast: coef()).  Lane (stage k, sub-lane c) of a wave owns the rows c, c + LPS, ...;
// per row slot the lanes read the row's three entries as three 8-byte accesses at  k * dstride + offset(row)  (rows without a Jacobian read the
// zero triple: one address, a broadcast).  64 banks of 4 bytes; an access costs as many passes as the most loaded bank has DISTINCT dwords.
// Returns the passes summed over the row slots and the three entries: with the bare strides (48 doubles for 8 + 8 rows, 40 packed) every second
// / fourth stage falls on the same banks -- 180 passes where 36 would do (fast (8,8) layout), 83 / 36 packed.  The model only ranks strides; the
// measured effect is in profiles/round5_p_dpad_ab.jsonl.
static int d_load_passes(int N, int n_pair, int nh, int threads, int dstride)
{
    const int lps = threads == 64 ? (3 * N <= 64 ? 3 : 2) : (N <= 21 ? 6 : 4);       // lanes per stage of the kernel families (pick_*_kernel)
    const int spw = 64 / lps, nk = N < spw ? N : spw;                                 // stages of one wave (two-wave kernels: each wave loads for its own)
    const int rpl = (nh + 14 + lps - 1) / lps;
    int total = 0;
    std::vector<int> dw;
    for (int s = 0; s < rpl && lps * s < nh; s++)
        for (int part = 0; part < 3; part++) {
            dw.clear();
            for (int k = 0; k < nk; k++)
                for (int c = 0; c < lps; c++) {
                    const int r = c + lps * s;
                    int a = N * dstride + part;                                       // zero triple
                    if (r < nh) {
                        const int off = r < n_pair ? 2 * r : 3 * r - n_pair;
                        if (part < 2 || r >= n_pair) a = k * dstride + off + part; else a = N * dstride + 2;
                    }
                    dw.push_back(2 * a); dw.push_back(2 * a + 1);
                }
            std::sort(dw.begin(), dw.end());
            dw.erase(std::unique(dw.begin(), dw.end()), dw.end());
            int load[64] = {0}, worst = 0;
            for (int x : dw) { const int b = ++load[x & 63]; if (b > worst) worst = b; }
            total += worst;
        }
    return total;
}
// the padding in 0 .. max_pad that the model likes best (ties: the smaller); `allowed(pad)`: the layout still fits what it has to fit
template <typename Allowed>
static int pick_d_pad(int N, int n_pair, int nh, int threads, int max_pad, Allowed allowed)
{
    if (const char *e = lab_env("TMPC_EXP_DPAD")) { const int v = atoi(e); return v >= 0 && v <= max_pad && allowed(v) ? v : 0; }   // experiments ("0": the bare strides)
    const int base = 2 * n_pair + 3 * (nh - n_pair);
    int best = 0, best_cost = d_load_passes(N, n_pair, nh, threads, base);
    for (int pad = 1; pad <= max_pad; pad++) {
        if (!allowed(pad)) continue;
        const int c = d_load_passes(N, n_pair, nh, threads, base + pad);
        if (c < best_cost) { best = pad; best_cost = c; }
    }
    return best;
}

// ---- filling a slot (tmpc_create) ---------------------------------------------------------------------------------------------------------------
constexpr size_t LDS_CAP = 160 * 1024;     // what one CU has: a slot that needs more is not filled
// The LDS a slot's kernel needs, from its kind and geometry; sl: the scan depth of the latency-2 / -3 kernels (pick_scan_kernel, pick_quad_kernel)
static size_t slot_lds(const Dims &d, int slot, const KernelSlot &s, int sl)
{
    const int nh = d.n_up + d.M;
    if (s.kind == KernelSlot::GENERIC) return sizeof(double) * (size_t)lds_doubles(d.N, nh);
    if (s.kind == KernelSlot::COMPACT) return sizeof(double) * (size_t)lds_doubles_compact(d.N, d.n_lin, nh, s.threads, s.dpad, s.lay);
    size_t n = lds_doubles_fast(d.N, nh);
    // two-wave (128-thread) fast kernels park wave 0's share of W per stage behind the layout while they linearise (the NTH = 128 form of linearise,
    // tmpc_kernels.hpp), and so do all latency kernels; the four-wave form parks wave 0's share there too (N x 28) and the row lanes' shares inside the
    // scan scratch (hand-written stages 36 N / 24 N doubles, emitted stages 12 N), which is dead then
    if (s.threads == 128 || slot >= SLOT_LAT1) n += (size_t)d.N * NP28;
    if (slot == SLOT_LAT2 || slot == SLOT_LAT3) n += sl == 3 ? scan::lds_doubles<3>(d.N) : scan::lds_doubles<2>(d.N);
    return sizeof(double) * n;
}
// Sets `lds` as the kernel's maximum dynamic LDS and returns how many workgroups of `threads` threads one CU holds at once (0: a call failed)
static int blocks_per_cu(SolveKernel k, int threads, size_t lds)
{
    int n = 0;
    if (hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void *)k, threads, lds) != hipSuccess) return 0;
    return n;
}
// A compact kernel's padding of the packed rows' stage stride (Dims::dpad): only what keeps the residency of no padding (LDS is what bounds it:
// 8 x 20 KB at cfg 2).  Sets s.dpad and s.lds_bytes.
static void choose_compact_pad(const Dims &d, int slot, KernelSlot &s)
{
    auto per_cu = [&](int pad) { s.dpad = pad; return blocks_per_cu(s.kernel, s.threads, slot_lds(d, slot, s, 0)); };
    const int per_cu0 = per_cu(0);
    const int pad = pick_d_pad(d.N, d.n_lin, d.n_up + d.M, s.threads, DPAD_MAX, [&](int p) { return p == 0 || (per_cu0 > 0 && per_cu(p) == per_cu0); });
    s.dpad = pad;
    s.lds_bytes = slot_lds(d, slot, s, 0);
}
// A compact slot's resident workgroups, and its wave issue priorities: only when the residency puts two waves on every SIMD (8 waves per CU) --
// with an odd count the waves that share a SIMD starve and set the makespan (tmpc_riccati.hpp)
static void set_resident(KernelSlot &s, int per_cu, int cus)
{
    if (const char *e = lab_env("TMPC_COMPACT_PER_CU")) { const int v = atoi(e); if (v > 0 && v < per_cu) per_cu = v; }   // experiments
    s.resident = per_cu * cus;
    s.prio = per_cu * (s.threads / 64) == 8;
}
static_assert(IO_NU == NU, "tmpc_handle_layout.hpp sizes utraj with the kernels' control count");
// ---- the persistent per-slot solver state of a handle (tmpc_solve_iterations) -------------------------------------------------------------------
// Five device arrays of B_max slots, allocated together on first use and zeroed: a slot holds what one Solver capsule of the reference keeps between solves.
struct SolverState {
    enum { Z, PI, LAMH, STOPPED, HAS, COUNT };
    // Z [N + 1][NV] the iterate; PI [N + 1][NX] equality multipliers; LAMH [N][n_up + M] row multipliers; STOPPED (i32) the iteration loop of the current
    // solve() has ended; HAS (i32) the slot holds state of an earlier tmpc_solve_iterations (set by the kernels' store)
    void *a[COUNT] = {};
    template <class T> T *get(int i) const { return static_cast<T *>(a[i]); }
    bool allocated() const { return a[Z] != nullptr; }
    // bytes of B slots of array i: what is copied, zeroed and -- for B_max slots -- allocated
    static size_t bytes(const Dims &d, size_t B, int i) { return B * (i <= LAMH ? slot_doubles(d, i) * sizeof(double) : sizeof(int)); }
    // doubles of one slot of Z, PI or LAMH (the kernels' strides)
    static size_t slot_doubles(const Dims &d, int i) { return i == Z ? (d.N + 1) * NV : i == PI ? (d.N + 1) * NX : d.N * (d.n_up + d.M); }
    void release() { for (void *&p : a) { if (p) (void)hipFree(p); p = nullptr; } }
    // All or nothing (a later call must not find half of the arrays), zeroed on `stream`.  LAMH is allocated one double longer than bytes() says: a problem
    // without inequality rows (n_up + M = 0) has no row multipliers, and a zero-size hipMalloc may hand back a null pointer -- the memset of it would then
    // fail the whole allocation, and the kernels would be given a null lamh.  That double is never read, copied or reset.
    bool allocate(const Dims &d, size_t B_max, hipStream_t stream)
    {
        bool ok = true;
        for (int i = 0; i < COUNT && ok; i++) {
            const size_t n = bytes(d, B_max, i) + (i == LAMH ? 8 : 0);
            ok = hipMalloc(&a[i], n) == hipSuccess && hipMemsetAsync(a[i], 0, n, stream) == hipSuccess;
        }
        if (!ok) release();
        return ok;
    }
};
}  // namespace tmpc

struct tmpc_handle {
    tmpc::Dims d{};
    int B_max = 0, B = 0, device = 0;
    hipStream_t stream = nullptr;
    // inputs: owned staging buffers (tmpc_set_batch) or borrowed device pointers (tmpc_set_batch_device)
    double *o_xinit = nullptr, *o_x0 = nullptr, *o_params = nullptr;
    const double *xinit = nullptr, *x0 = nullptr, *params = nullptr;
    double *xtraj = nullptr, *utraj = nullptr, *pobj = nullptr, *res_eq = nullptr, *d_weight = nullptr;
    int *exit_code = nullptr, *qp_status = nullptr, *sqp_iter = nullptr, *qp_iter = nullptr, *d_best = nullptr;
    uint8_t *d_disabled = nullptr;
    // The owned input buffers (+ the slot map) are ONE device allocation, the outputs another, laid out by `io` (tmpc_handle_layout.hpp); the typed pointers
    // above and d_slot point into them.  Control-tick handles (io.tick) mirror both in pinned host memory with the same layout -- tmpc_set_batch is one
    // asynchronous H2D copy instead of three staged ones, tmpc_set_slots needs no stream synchronisation, tmpc_get is one D2H copy instead of eight (round 6:
    // the C++ BatchContext's tick spent ~0.2 ms of 1.1 ms in those thirteen transfers).  Larger handles (the bench's 32768 trajectories) have no mirrors:
    // direct copies and a stream synchronisation.
    tmpc::IoLayout io;
    char *dev_in = nullptr, *dev_out = nullptr, *pin_in = nullptr, *pin_out = nullptr;
    hipEvent_t in_done = nullptr, slot_done = nullptr;    // the last H2D copies out of pin_in -- batch inputs / slot map: disjoint regions of the mirror, each rewritten only after ITS copy
    bool in_pending = false, slot_pending = false;
    tmpc::KernelSlot slot[tmpc::SLOT_COUNT];  // the solve kernels (tmpc::Slot)
    double *ws = nullptr;                     // [resident][ws_doubles(N)] per-workgroup NLP workspace of the compact slot
    int *ticket = nullptr;
    int latency_mode = 0;                     // 0: throughput kernels, 1-3: the latency slots (tmpc_set_latency_mode)
    bool throughput_mode = false;             // lane-per-trajectory kernels (tmpc_lanes.hip) instead of one wave per trajectory
    tmpc::lanes::Context *lanes = nullptr;    // their HBM workspace, created when the mode is first enabled
    tmpc::SolverState st;            // persistent per-slot solver state (tmpc_solve_iterations), allocated on first use
    int *d_slot = nullptr;           // [B_max] state slot of every batch entry (tmpc_set_slots): inside dev_in
    bool slots_set = false;
    int slots_B = 0;                 // batch size the slot map was given for: a map of another size is refused, never read past its end
    int *d_share = nullptr;          // [B_max] tmpc_set_param_sharing
    int share_B = 0;                 // batch size the sharing map was given for (0: none)
    bool share_strict = false;       // tmpc_set_param_sharing_ex(.., TMPC_SHARE_COPIES_NOT_MAINTAINED): a solve that cannot honour the map is an error
    bool st_valid = false;           // lane kernels (state = their workspace, per launch): it holds the result of a previous call ...
    int st_B = 0;                    // ... for slots [0, st_B)
    int solved_B = 0;                // entries the last solve launch covered; 0 after tmpc_set_batch* (tmpc_guidance_decide reads the solution)
    // SH-MPC bookkeeping: the sample behind each scenario row of the last tmpc_scenario_halfspaces (i32 [B][N][scn_rows])
    unsigned char *scn_discard = nullptr;     // [B_max][scn_discard_S] scenarios discarded for each trajectory (tmpc_scenario_discard); applies to the next tmpc_scenario_halfspaces
    int scn_discard_S = 0, scn_discard_B = 0, scn_discard_n = 0;
    size_t scn_discard_cap = 0;
    int *scn_sample = nullptr;
    size_t scn_cap = 0;
    int scn_rows = 0, scn_B = 0;
    bool scn_by_column = false;               // the rows of batch scn_B were written by tmpc_stack_scenario_halfspaces, into the caller's columns
    std::vector<hipEvent_t> ev;      // per-launch timing events (pairs)
    int ev_used = 0;
    bool timing = false;
    std::string err;

    tmpc_handle() = default;
    tmpc_handle(const tmpc_handle &) = delete;
    tmpc_handle &operator=(const tmpc_handle &) = delete;
    // The handle owns everything above but the borrowed batch pointers; a handle that tmpc_create gave up half-way is released the same way.  (So the early
    // failure paths of tmpc_create, hipSetDevice's own failure among them, now also set the calling thread's device -- to one the device count has confirmed
    // -- where a bare delete did not.)
    ~tmpc_handle()
    {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (void *p : {(void *)dev_in, (void *)dev_out, (void *)d_weight, (void *)d_best, (void *)d_disabled, (void *)d_share, (void *)scn_sample, (void *)scn_discard,
                        (void *)ws, (void *)ticket})
            if (p) (void)hipFree(p);
        st.release();
        if (pin_in) (void)hipHostFree(pin_in);
        if (pin_out) (void)hipHostFree(pin_out);
        if (in_done) (void)hipEventDestroy(in_done);
        if (slot_done) (void)hipEventDestroy(slot_done);
        for (auto &e : ev) (void)hipEventDestroy(e);
        tmpc::lanes::destroy(lanes);
        if (stream) (void)hipStreamDestroy(stream);
    }
    // all B_max slots of state array i, zeroed on the handle's stream
    hipError_t zero_state(int i) { return hipMemsetAsync(st.a[i], 0, tmpc::SolverState::bytes(d, B_max, i), stream); }
};

#define TMPC_HIP_CHECK(h, expr)                                                                     \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                           \
            return TMPC_ERR_HIP;                                                                    \
        }                                                                                           \
    } while (0)

// the entry points that write the hand-written kernels' parameter layout refuse in a generated solver, whose layout is the module stack's
#ifdef TMPC_GENERATED_STAGE
#define TMPC_NOT_IN_GENERATED_SOLVER(h, name) \
    do { if (h) (h)->err = name ": not available in a generated solver (its parameter layout is the module stack's)"; return TMPC_ERR_INVALID; } while (0)
#else
#define TMPC_NOT_IN_GENERATED_SOLVER(h, name) do { } while (0)
#endif

// An options struct of the C-ABI (its first field: uint32_t size).  `o` holds the defaults and keeps them when the caller passes NULL; like
// tmpc_create_v2, the caller's struct may be longer (a newer header) only with a zero tail, and shorter only at `first_revision`, the size of
// the struct before fields were appended to it: the appended fields then keep their defaults.
template <class Options> static bool read_options(tmpc_handle *h, const char *fn, const char *type, const Options *options, Options &o,
                                                  uint32_t first_revision = sizeof(Options))
{
    if (!options) return true;
    if (options->size < sizeof(o)) {
        if (options->size != first_revision) { h->err = std::string(fn) + ": options->size is smaller than " + type; return false; }
        memcpy(&o, options, first_revision);
        o.size = sizeof(o);
        return true;
    }
    const unsigned char *tail = reinterpret_cast<const unsigned char *>(options);
    for (uint32_t i = sizeof(o); i < options->size; i++)
        if (tail[i]) { h->err = std::string(fn) + ": options holds a non-zero field this library does not know"; return false; }
    o = *options;
    return true;
}

// Grow-on-demand scratch of a handle: afterwards *p holds at least `need` elements (the old contents are not kept).  The stream may still read the old buffer:
// it is synchronised before the buffer is freed; a failed allocation leaves no buffer and a capacity of 0.
template <class T> static int grow_scratch(tmpc_handle *h, T **p, size_t *cap, size_t need)
{
    if (need <= *cap) return TMPC_OK;
    if (*p) { TMPC_HIP_CHECK(h, hipStreamSynchronize(h->stream)); (void)hipFree(*p); *p = nullptr; *cap = 0; }
    TMPC_HIP_CHECK(h, hipMalloc(p, need * sizeof(T)));
    *cap = need;
    return TMPC_OK;
}

namespace {
// Scratch device buffers / events of the diagnostic entry points: released on every return path.
struct DevBufs {
    std::vector<void *> p;
    ~DevBufs() { for (void *q : p) if (q) (void)hipFree(q); }
    hipError_t alloc(double **out, size_t bytes) { hipError_t e = hipMalloc(out, bytes ? bytes : 8); if (e == hipSuccess) p.push_back(*out); return e; }
};
struct Events {
    std::vector<hipEvent_t> ev;
    ~Events() { for (auto &e : ev) if (e) (void)hipEventDestroy(e); }
};
}  // namespace

// the entry points of the device row writers, for the hand-written layout (tmpc_hip.h) and for the columns of generated solvers' module stacks
// (tmpc_hip_stack.h, tmpc_hip_stack_env.h, tmpc_hip_stack_scenario.h): one body per writer, two thin entry points; no_batch, launch_flat, read_stack_columns
#include "tmpc_row_entries.hpp"
// the world of a closed loop (tmpc_hip_episode.h): plant step, obstacle motion, episode log -- no parameter row, no batch
#include "tmpc_episode_entry.hpp"
// the guidance search (tmpc_hip_guidance_search.h): topology-distinct trajectories per scene -- no parameter row, no batch
#include "tmpc_guidance_search_entry.hpp"

extern "C" {

void tmpc_default_dims(tmpc_dims *d, int32_t N, int32_t S, int32_t n_lin, int32_t M) { tmpc_default_dims_ex(d, N, S, n_lin, M, 0, 0); }

void tmpc_default_dims_ex(tmpc_dims *d, int32_t N, int32_t S, int32_t n_lin, int32_t M, int32_t n_slk, int32_t slack)
{
    memset(d, 0, sizeof *d);
#ifdef TMPC_GENERATED_STAGE
    // generated solver: the row / parameter structure is fixed by the generated stage functions
    (void)n_lin; (void)M; (void)n_slk; (void)slack;
    n_lin = tmpc_gen::NH; M = 0; n_slk = 0; slack = tmpc_gen::SLACK;
#endif
    d->N = N; d->S = S; d->n_lin = n_lin; d->M = M; d->n_slk = n_slk; d->slack = slack ? 1 : 0;
    tmpc::Dims t{}; t.S = S; t.n_lin = n_lin; t.M = M; t.n_slk = n_slk; t.slack = d->slack;
    d->npar = tmpc::expected_npar(t);
    d->n_sqp = 10; d->qp_iter_max = 50; d->erk_steps = 3;
    d->dt = 0.2; d->qp_tol = 1e-5; d->reg_eps = 1e-4; d->ipm_mu0 = 0.01; d->ipm_thr0 = 0.01;
    const double lb[TMPC_NV] = {-2.0, -0.8, -2000.0, -2000.0, -M_PI * 4, -0.01, -1.0};
    const double ub[TMPC_NV] = {2.0, 0.8, 2000.0, 2000.0, M_PI * 4, 3.0, 10000.0};
    for (int i = 0; i < TMPC_NV; i++) { d->lb[i] = lb[i]; d->ub[i] = ub[i]; }
#ifdef TMPC_GENERATED_STAGE
    for (int i = 0; i < TMPC_NV; i++) { d->lb[i] = tmpc_gen::LB[i]; d->ub[i] = tmpc_gen::UB[i]; }     // the plugin model's own bounds (emit.py)
#endif
}

int tmpc_create_v2(tmpc_handle **out, const tmpc_dims *dims_in, uint32_t dims_size, int32_t B_max, int32_t device)
{
    // a caller built against an older header passes a SHORTER struct: the fields it does not know are the defaults (0), never garbage.  Only the
    // struct's revision boundaries are sizes a header of this library ever had (round-5 advisor: a size ending inside a field copied part of it)
    constexpr uint32_t kRev[] = {(uint32_t)offsetof(tmpc_dims, cost_model),         // rounds 1-3: up to n_slk / slack
                                 (uint32_t)offsetof(tmpc_dims, riccati_form),       // rounds 4-5: + cost_model, row_model
                                 (uint32_t)sizeof(tmpc_dims)};                      // round 6: + riccati_form
    if (!out || !dims_in || dims_size > 4096) return TMPC_ERR_INVALID;
    if (out) *out = nullptr;
    bool known = dims_size > sizeof(tmpc_dims);
    for (uint32_t r : kRev) known |= dims_size == r;
    if (!known) return TMPC_ERR_INVALID;
    if (dims_size > sizeof(tmpc_dims)) {                                           // a NEWER header: fields this library does not know must be unset
        const unsigned char *tail = (const unsigned char *)dims_in + sizeof(tmpc_dims);
        for (uint32_t i = 0; i < dims_size - (uint32_t)sizeof(tmpc_dims); i++) if (tail[i] != 0) return TMPC_ERR_INVALID;
    }
    tmpc_dims d;
    memset(&d, 0, sizeof d);
    memcpy(&d, dims_in, dims_size < sizeof d ? dims_size : sizeof d);
    return tmpc_create(out, &d, B_max, device);
}

// why the calling thread's last tmpc_create* was refused, where the refusal has a message: there is no handle to keep it in (tmpc_last_error(NULL))
static thread_local std::string g_create_error;

static int refuse_create(const std::string &why)
{
    g_create_error = why;
    return TMPC_ERR_INVALID;
}

int tmpc_create(tmpc_handle **out, const tmpc_dims *dims, int32_t B_max, int32_t device)
{
    g_create_error.clear();
    if (!out || !dims || B_max <= 0) return TMPC_ERR_INVALID;
    *out = nullptr;
    {
        tmpc::Dims t{}; t.S = dims->S; t.n_lin = dims->n_lin; t.M = dims->M; t.n_slk = dims->n_slk; t.slack = dims->slack; t.row_model = dims->row_model;
        if (dims->row_model != 0 && dims->row_model != 1) return TMPC_ERR_INVALID;
        if (dims->N < 2 || dims->N > tmpc::STAGE_MAX || dims->S < 1 || dims->M < 0 || dims->n_lin < 0 || dims->n_slk < 0 ||
            (dims->slack != 0 && dims->slack != 1) || dims->npar != tmpc::expected_npar(t) || dims->erk_steps < 1 ||
            dims->n_sqp < 1 || dims->qp_iter_max < 1 || !(dims->dt > 0.0) || !(dims->qp_tol > 0.0) || !(dims->reg_eps > 0.0) ||
            !(dims->ipm_mu0 > 0.0) || !(dims->ipm_thr0 > 0.0) || (dims->cost_model != 0 && dims->cost_model != 1) ||
            (dims->riccati_form != TMPC_RICCATI_SCHUR && dims->riccati_form != TMPC_RICCATI_SQUARE_ROOT))
            return TMPC_ERR_INVALID;
        // the model bounds: a NaN, or a box with nothing inside, is no problem to solve with (infinite bounds are not looked at here)
        static const char *const var[TMPC_NV] = {"a", "w", "x", "y", "psi", "v", "spline"};
        for (int i = 0; i < TMPC_NV; i++) {
            if (dims->lb[i] != dims->lb[i] || dims->ub[i] != dims->ub[i]) return refuse_create(std::string("tmpc_create: a bound of ") + var[i] + " is NaN");
            if (dims->lb[i] >= dims->ub[i])
                return refuse_create(std::string("tmpc_create: lb[") + std::to_string(i) + "] >= ub[" + std::to_string(i) + "] (" + var[i] + ": " +
                                     std::to_string(dims->lb[i]) + " >= " + std::to_string(dims->ub[i]) + ")");
        }
#ifdef TMPC_GENERATED_STAGE
        if (dims->n_lin != tmpc_gen::NH || dims->M != 0 || dims->n_slk != 0 || dims->slack != tmpc_gen::SLACK || dims->cost_model != 0 || dims->row_model != 0) return TMPC_ERR_INVALID;
#endif
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return TMPC_ERR_NO_DEVICE;
    std::unique_ptr<tmpc_handle> owner(new tmpc_handle());      // until *out takes it: every failure below is a plain return
    tmpc_handle *h = owner.get();
    h->device = device; h->B_max = B_max;
    tmpc::Dims &d = h->d;
    d.N = dims->N; d.S = dims->S; d.n_lin = dims->n_lin; d.M = dims->M; d.npar = dims->npar;
    d.n_slk = dims->n_slk; d.slack = dims->slack; d.cost_model = dims->cost_model; d.row_model = dims->row_model;
    d.n_sqp = dims->n_sqp; d.qp_iter_max = dims->qp_iter_max; d.erk_steps = dims->erk_steps;
    d.dt = dims->dt; d.qp_tol = dims->qp_tol; d.reg_eps = dims->reg_eps; d.mu0 = dims->ipm_mu0; d.thr0 = dims->ipm_thr0;
    for (int i = 0; i < TMPC_NV; i++) { d.lb[i] = dims->lb[i]; d.ub[i] = dims->ub[i]; }
#ifdef TMPC_GENERATED_STAGE
    d.model = tmpc_gen::MODEL;               // fixed by the module stack's model (emit.py): 1 = SecondOrderUnicycleModel, the fifth state slot inert
#else
    d.model = 0;
#endif
    d.riccati_form = dims->riccati_form;
    tmpc::derive_dims(d);
    d.split_rows = tmpc::split_rows_for(d.N, d.n_up + d.M) ? 1 : 0;
    using tmpc::KernelSlot;
    KernelSlot *slot = h->slot, &def = h->slot[tmpc::SLOT_DEFAULT];
    const bool schur = d.riccati_form == TMPC_RICCATI_SCHUR;      // the square-root form has its fast kernels only: no latency / compact variants
    def.kernel = schur ? tmpc::pick_fast_kernel(d, &def) : tmpc::pick_sqrt_kernel(d, &def);
    if (!schur && !def.kernel) return TMPC_ERR_INVALID;       // (no square-root instantiation for this shape: never a silent other form)
    if (const char *lm = lab_env("TMPC_LATENCY_MODE")) {      // experiments: latency variant regardless of the caller ("0" .. "3"; anything else is ignored)
        if (lm[0] >= '0' && lm[0] <= '3' && lm[1] == '\0') h->latency_mode = lm[0] - '0';
    }
    const bool fast = def.kernel != nullptr;
    if (!fast) {                                              // the generic kernel (rows in LDS): every shape; it is its own profiled twin
        static const char *const generic_names[4] = {"generic<0>", "generic<1>", "generic<2>", "generic<3>"};
        const int sm = tmpc::stage_model(d);
        def.kernel = def.twin = sm == 3 ? tmpc::tmpc_solve_kernel<3> : sm == 1 ? tmpc::tmpc_solve_kernel<1> : (sm == 2 ? tmpc::tmpc_solve_kernel<2> : tmpc::tmpc_solve_kernel<0>);
        def.name = generic_names[sm]; def.threads = tmpc::NT; def.kind = KernelSlot::GENERIC;
    }
    def.lds_bytes = tmpc::slot_lds(d, tmpc::SLOT_DEFAULT, def, 0);
    if (hipSetDevice(device) != hipSuccess) return TMPC_ERR_HIP;
    if (def.lds_bytes > tmpc::LDS_CAP) return TMPC_ERR_INVALID;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) cus = 0;
    // the latency slots: beside a fast one-wave default; lat2 and lat3 also beside a two-wave one at N > 20, lat3 also beside the generic kernel of
    // curvature-aware cost + Gaussian rows.  A slot whose LDS the kernel does not accept stays empty (lat1: one shape, far below the cap)
    const bool one_wave = schur && fast && def.threads == tmpc::NT, lat23_ok = def.threads == tmpc::NT || d.N > 20;
    int sl2 = 3, sl3 = 3;
    if (one_wave) slot[tmpc::SLOT_LAT1].kernel = tmpc::pick_latency_kernel(d, &slot[tmpc::SLOT_LAT1]);
    if (schur && fast && lat23_ok) slot[tmpc::SLOT_LAT2].kernel = tmpc::pick_scan_kernel(d, &slot[tmpc::SLOT_LAT2], &sl2);
    if (schur && (fast || tmpc::stage_model(d) == 3) && lat23_ok)
        slot[tmpc::SLOT_LAT3].kernel = tmpc::pick_quad_kernel(d, lab_env("TMPC_QUAD_AB") != nullptr, &slot[tmpc::SLOT_LAT3], &sl3);
    for (int i = tmpc::SLOT_LAT1; i <= tmpc::SLOT_LAT3; i++) {
        KernelSlot &s = slot[i];
        if (!s.kernel) continue;
#ifdef TMPC_GENERATED_STAGE
        // zero-scratch rule: the product's tick kernels are held to it by the build; around emitted stage functions the compiler decides per
        // stack, so a tick kernel that uses scratch is not offered -- tmpc_set_latency_mode then answers 1 as for a shape without the variant
        hipFuncAttributes fa;
        if (hipFuncGetAttributes(&fa, (const void *)s.kernel) != hipSuccess || fa.localSizeBytes > 0) { s = KernelSlot{}; continue; }
#endif
        s.lds_bytes = tmpc::slot_lds(d, i, s, i == tmpc::SLOT_LAT3 ? sl3 : sl2);
        if ((i != tmpc::SLOT_LAT1 && s.lds_bytes > tmpc::LDS_CAP) ||
            hipFuncSetAttribute((const void *)s.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s.lds_bytes) != hipSuccess)
            s = KernelSlot{};
    }
    KernelSlot cp;
    if (one_wave && (cp.kernel = tmpc::pick_compact_kernel(d, &cp)) != nullptr) {
        // the fast kernel of the shape (everything in LDS, four per CU) stays for launches it holds resident at once: bitwise the same results
        // (tests/test_gpu_compact2.py), a trajectory is ~10 % faster on it.  TMPC_COMPACT_MIN_B=0: the compact kernel for every launch (rounds 3-4)
        const int fast_per_cu = tmpc::blocks_per_cu(def.kernel, def.threads, def.lds_bytes);
        if (fast_per_cu > 0 && cus > 0) {
            slot[tmpc::SLOT_SMALL] = def;
            slot[tmpc::SLOT_SMALL].bound = fast_per_cu * cus;
            if (const char *e = lab_env("TMPC_COMPACT_MIN_B")) slot[tmpc::SLOT_SMALL].bound = atoi(e);                                 // experiments
        }
        def = cp;
        tmpc::choose_compact_pad(d, tmpc::SLOT_DEFAULT, def);
    }
    if (hipFuncSetAttribute((const void *)def.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)def.lds_bytes) != hipSuccess)
        return TMPC_ERR_NO_DEVICE;
    if (def.kind == KernelSlot::COMPACT) {
        const int per_cu = tmpc::blocks_per_cu(def.kernel, def.threads, def.lds_bytes);
        if (per_cu <= 0 || cus <= 0) return TMPC_ERR_HIP;
        tmpc::set_resident(def, per_cu, cus);
    }
    KernelSlot &cp2 = slot[tmpc::SLOT_CP2];
    if (schur && def.kind == KernelSlot::FAST && def.threads == 128 && (cp2.kernel = tmpc::pick_compact2_kernel(d, &cp2)) != nullptr) {
        tmpc::choose_compact_pad(d, tmpc::SLOT_CP2, cp2);
        const int per_cu = tmpc::blocks_per_cu(cp2.kernel, cp2.threads, cp2.lds_bytes);
        const int fast_per_cu = tmpc::blocks_per_cu(def.kernel, def.threads, def.lds_bytes);
        if (fast_per_cu <= 0 || cus <= 0 || per_cu <= fast_per_cu)
            cp2 = KernelSlot{};                              // (no gain in residency: the fast kernel stays alone)
        else {
            cp2.bound = fast_per_cu * cus;
            if (const char *e = lab_env("TMPC_COMPACT2_MIN_B")) cp2.bound = atoi(e);                                                   // experiments
            tmpc::set_resident(cp2, per_cu, cus);
        }
    }
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return TMPC_ERR_HIP;
    const size_t B = B_max;
    const tmpc::IoLayout &io = h->io = tmpc::io_layout(d.N, tmpc::ext_nx(d), tmpc::ext_nv(d), d.npar, B);
    bool ok = hipMalloc(&h->dev_in, io.in_total) == hipSuccess && hipMalloc(&h->dev_out, io.out_total) == hipSuccess;
    if (io.tick) {
        ok &= hipHostMalloc(&h->pin_in, io.in_total, hipHostMallocDefault) == hipSuccess && hipHostMalloc(&h->pin_out, io.out_total, hipHostMallocDefault) == hipSuccess;
        ok &= hipEventCreateWithFlags(&h->in_done, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&h->slot_done, hipEventDisableTiming) == hipSuccess;
    }
    if (!ok) return TMPC_ERR_HIP;
    auto in = [&](int i) { return (void *)(h->dev_in + io.in[i].offset); };
    auto res = [&](int i) { return (void *)(h->dev_out + io.out[i].offset); };
    h->o_xinit = (double *)in(tmpc::IN_XINIT); h->o_x0 = (double *)in(tmpc::IN_X0);
    h->o_params = (double *)in(tmpc::IN_PARAMS); h->d_slot = (int *)in(tmpc::IN_SLOT);
    h->xtraj = (double *)res(tmpc::OUT_XTRAJ); h->utraj = (double *)res(tmpc::OUT_UTRAJ);
    h->pobj = (double *)res(tmpc::OUT_POBJ); h->res_eq = (double *)res(tmpc::OUT_RES_EQ);
    h->exit_code = (int *)res(tmpc::OUT_EXIT_CODE); h->qp_status = (int *)res(tmpc::OUT_QP_STATUS);
    h->sqp_iter = (int *)res(tmpc::OUT_SQP_ITER); h->qp_iter = (int *)res(tmpc::OUT_QP_ITER);
    ok &= hipMalloc(&h->d_weight, B * 8) == hipSuccess;
    ok &= hipMalloc(&h->d_best, 4) == hipSuccess;
    ok &= hipMalloc(&h->d_disabled, B) == hipSuccess;
    if (const KernelSlot *p = def.kind == KernelSlot::COMPACT ? &def : cp2.kernel ? &cp2 : nullptr) {
        ok &= hipMalloc(&h->ws, (size_t)p->resident * tmpc::ws_doubles(d.N, p->threads == 128) * 8) == hipSuccess;
        ok &= hipMalloc(&h->ticket, 8 * 4) == hipSuccess;         // one work counter per XCD (next_trajectory)
    }
    if (!ok) return TMPC_ERR_HIP;
    *out = owner.release();
    return TMPC_OK;
}

void tmpc_destroy(tmpc_handle *h) { delete h; }

const char *tmpc_last_error(const tmpc_handle *h) { return h ? h->err.c_str() : g_create_error.empty() ? "null handle" : g_create_error.c_str(); }

int tmpc_set_batch(tmpc_handle *h, int32_t B, const double *xinit, const double *x0, const double *params)
{
    if (!h || B <= 0 || B > h->B_max || !xinit || !x0 || !params) { if (h) h->err = "tmpc_set_batch: bad argument"; return TMPC_ERR_INVALID; }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    const tmpc::IoRegion *r = h->io.in;
    const void *src[tmpc::IO_BATCH_ARRAYS] = {xinit, x0, params};
    auto copy = [&](const char *from_base, size_t i) {           // the first B trajectories of batch array i: out of the mirror (from_base) or the caller's array
        return hipMemcpyAsync(h->dev_in + r[i].offset, from_base ? from_base + r[i].offset : src[i], r[i].bytes(B), hipMemcpyHostToDevice, h->stream);
    };
    if (h->pin_in && h->io.batch_bytes(B) <= (512u << 10)) {       // (measured: at 64 trajectories = 1.4 MB the runtime's own path for pageable memory is 12 us faster than a host copy into the mirror)
        // through the pinned mirror: one asynchronous copy of [xinit | x0 | params of the first B trajectories] (the regions of B_max trajectories lie in this order)
        if (h->in_pending) { TMPC_HIP_CHECK(h, hipEventSynchronize(h->in_done)); h->in_pending = false; }
        for (size_t i = 0; i < tmpc::IO_BATCH_ARRAYS; i++) std::memcpy(h->pin_in + r[i].offset, src[i], r[i].bytes(B));
        const tmpc::IoRegion &last = r[tmpc::IN_PARAMS];
        if (last.offset <= (256u << 10)) {                          // (B_max close to B, as for a control tick's handle: the gaps cost less than two more copies)
            TMPC_HIP_CHECK(h, hipMemcpyAsync(h->dev_in, h->pin_in, last.offset + last.bytes(B), hipMemcpyHostToDevice, h->stream));
        } else {
            for (size_t i = 0; i < tmpc::IO_BATCH_ARRAYS; i++) TMPC_HIP_CHECK(h, copy(h->pin_in, i));
        }
        TMPC_HIP_CHECK(h, hipEventRecord(h->in_done, h->stream)); h->in_pending = true;
    } else {
        for (size_t i = 0; i < tmpc::IO_BATCH_ARRAYS; i++) TMPC_HIP_CHECK(h, copy(nullptr, i));
    }
    h->xinit = h->o_xinit; h->x0 = h->o_x0; h->params = h->o_params; h->B = B;
    h->solved_B = 0;
    h->scn_B = 0;                      // new parameter rows: the scenario-row bookkeeping of the previous batch no longer describes them
    h->scn_discard_B = 0;
    h->share_B = 0;                    // ... nor does a parameter-sharing map given for them
    return TMPC_OK;
}

int tmpc_set_batch_device(tmpc_handle *h, int32_t B, const void *d_xinit, const void *d_x0, const void *d_params)
{
    if (!h || B <= 0 || B > h->B_max || !d_xinit || !d_x0 || !d_params) { if (h) h->err = "tmpc_set_batch_device: bad argument"; return TMPC_ERR_INVALID; }
    h->xinit = (const double *)d_xinit; h->x0 = (const double *)d_x0; h->params = (const double *)d_params; h->B = B;
    h->solved_B = 0;
    h->scn_B = 0; h->scn_discard_B = 0; h->share_B = 0;
    return TMPC_OK;
}

// The slot (tmpc::Slot) a launch of the current batch runs (launch_solve; tmpc_debug_profile profiles the twin of that slot's instantiation).
static int launch_slot(const tmpc_handle *h)
{
    // mode 3 without a four-wave variant runs as mode 2, mode 2 without a scan variant as mode 1
    for (int m = h->latency_mode; m >= 1; m--)
        if (h->slot[tmpc::SLOT_LAT1 + m - 1].kernel) return tmpc::SLOT_LAT1 + m - 1;
    // compact <-> fast kernels of a shape compute bit for bit the same, so the launch size may choose between them: the fast kernel while it
    // holds the whole launch resident (lower latency per trajectory), the compact one (twice the residency) above that
    const tmpc::KernelSlot &cp2 = h->slot[tmpc::SLOT_CP2], &small = h->slot[tmpc::SLOT_SMALL];
    if (cp2.kernel && h->B > cp2.bound) return tmpc::SLOT_CP2;
    if (small.kernel && h->B <= small.bound) return tmpc::SLOT_SMALL;
    return tmpc::SLOT_DEFAULT;
}

// One launch over the current batch: n_iter RTI iterations per trajectory + completeOneIteration.  st_flags: ST_* (0 = fresh
// solver instances from the batch's warm start, nothing kept or stored: Solver::solve() of a new capsule).
static int launch_solve(tmpc_handle *h, int n_iter, int st_flags)
{
    const bool rec = h->timing && h->ev_used + 2 <= (int)h->ev.size();
    if (rec) TMPC_HIP_CHECK(h, hipEventRecord(h->ev[h->ev_used], h->stream));
    if (h->throughput_mode) {
        // lane-per-trajectory variant: transpose the reference-layout inputs into the lane-major workspace, then one launch of
        // the scalar-per-lane SQP_RTI program; the workspace itself is the persistent state
        if (tmpc::lanes::stage_in(h->lanes, h->stream, h->B, h->xinit, h->x0, h->params, !(st_flags & tmpc::ST_KEEP_ITERATE),
                                  !(st_flags & tmpc::ST_KEEP_MULTIPLIERS), h->err)) return TMPC_ERR_HIP;
        if (tmpc::lanes::solve(h->lanes, h->stream, h->B, n_iter, (st_flags & tmpc::ST_STORE) != 0, (st_flags & tmpc::ST_COMPLETE) != 0,
                               h->xtraj, h->utraj, h->pobj,
                               h->exit_code, h->qp_status, h->sqp_iter, h->res_eq, h->qp_iter, h->err)) return TMPC_ERR_HIP;
    } else {
        tmpc::Dims dd = h->d;
        dd.n_sqp = n_iter;
        using St = tmpc::SolverState;
        tmpc::StateIO io{h->st.get<double>(St::Z), h->st.get<double>(St::PI), h->st.get<double>(St::LAMH), h->st.get<int>(St::STOPPED), st_flags, h->ws, h->ticket,
                         (h->slots_set && h->slots_B == h->B) ? h->d_slot : nullptr, h->st.get<int>(St::HAS),
                         (h->share_B == h->B) ? h->d_share : nullptr};      // (a map given for another batch size is not applied)
        const tmpc::KernelSlot &k = h->slot[launch_slot(h)];
        const bool persistent = k.kind == tmpc::KernelSlot::COMPACT;
        dd.prio = k.prio;
        dd.dpad = k.dpad;      // (layout only: results do not depend on it)
        if (persistent) TMPC_HIP_CHECK(h, hipMemsetAsync(h->ticket, 0, 8 * 4, h->stream));    // the persistent launch's work counters (one per XCD)
        hipLaunchKernelGGL(k.kernel, dim3(persistent ? (h->B < k.resident ? h->B : k.resident) : h->B),   // (persistent launch: at most the resident workgroups)
                           dim3(k.threads), k.lds_bytes, h->stream, dd, h->B,
                           h->xinit, h->x0, h->params, h->xtraj, h->utraj, h->pobj, h->exit_code, h->qp_status,
                           h->sqp_iter, h->res_eq, h->qp_iter, (long long *)nullptr, io);
        TMPC_HIP_CHECK(h, hipGetLastError());
        if (st_flags & tmpc::ST_COMPLETE) {
            // a failed solve resets the reference's capsule (Solver_acados_reset, acados_solver_interface.cpp:187-191): zero multipliers
            const int n_pi = (int)St::slot_doubles(h->d, St::PI), n_lam = (int)St::slot_doubles(h->d, St::LAMH);
            hipLaunchKernelGGL(tmpc::tmpc_state_finalize_kernel, dim3(h->B), dim3(64), 0, h->stream, n_pi, n_lam, h->exit_code, io.pi, io.lamh,
                               (h->slots_set && h->slots_B == h->B) ? h->d_slot : nullptr);
            TMPC_HIP_CHECK(h, hipGetLastError());
        }
    }
    if (rec) { TMPC_HIP_CHECK(h, hipEventRecord(h->ev[h->ev_used + 1], h->stream)); h->ev_used += 2; }
    h->solved_B = h->B;
    return TMPC_OK;
}

// A caller that declared "the copies are not maintained" must never reach a kernel that reads them: the map has to be in force for the
// CURRENT batch (tmpc_set_batch* drops it) and the kernel family has to honour it.
static int share_check(tmpc_handle *h, const char *who)
{
    if (!h->share_strict) return TMPC_OK;
    if (h->share_B != h->B) { h->err = std::string(who) + ": the parameter-sharing map was declared with TMPC_SHARE_COPIES_NOT_MAINTAINED but is not in force for the "
                                       "current batch (tmpc_set_batch* drops it: give it again, or clear it with a null map)"; return TMPC_ERR_INVALID; }
    if (h->throughput_mode) { h->err = std::string(who) + ": the lane kernels read every entry's own parameter rows, the map says they are not maintained"; return TMPC_ERR_INVALID; }
    return TMPC_OK;
}

// the slots' persistent state no longer describes what the handle last solved
static int invalidate_state(tmpc_handle *h)
{
    h->st_valid = false; h->st_B = 0;
    if (h->st.allocated()) TMPC_HIP_CHECK(h, h->zero_state(tmpc::SolverState::HAS));
    return TMPC_OK;
}

int tmpc_solve(tmpc_handle *h)
{
    if (!h || h->B <= 0 || !h->xinit) { if (h) h->err = "tmpc_solve: no batch set"; return TMPC_ERR_INVALID; }
    if (int rc = share_check(h, "tmpc_solve")) return rc;
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    if (int rc = invalidate_state(h)) return rc;
    return launch_solve(h, h->d.n_sqp, 0);
}

int tmpc_solve_iterations(tmpc_handle *h, int32_t n_iter, int32_t flags)
{
    if (!h || h->B <= 0 || !h->xinit || n_iter < 0 || (flags & ~15)) { if (h) h->err = "tmpc_solve_iterations: no batch set / bad argument"; return TMPC_ERR_INVALID; }
    if (int rc = share_check(h, "tmpc_solve_iterations")) return rc;
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    if (h->throughput_mode && h->slots_set) { h->err = "tmpc_solve_iterations: slot maps (tmpc_set_slots) are not available with the lane kernels"; return TMPC_ERR_INVALID; }
    if (h->slots_set && h->slots_B != h->B) {
        // the map has one entry per batch entry: entries [slots_B, B) of a larger batch would be read from uninitialised memory
        h->err = "tmpc_solve_iterations: the slot map was given for a batch of " + std::to_string(h->slots_B) + " entries, the current batch has " +
                 std::to_string(h->B) + ": call tmpc_set_slots again after tmpc_set_batch (or clear it with a null map)";
        return TMPC_ERR_INVALID;
    }
    if (!h->throughput_mode && !h->st.allocated()) {
        if (!h->st.allocate(h->d, h->B_max, h->stream)) { h->err = "tmpc_solve_iterations: state allocation failed"; return TMPC_ERR_HIP; }
        h->st_valid = false; h->st_B = 0;
    }
    int st = tmpc::ST_STORE;
    if (h->throughput_mode) {
        // lane kernels keep their state per launch, not per slot: nothing to keep on the first call, and a grown batch starts fresh
        if (!h->st_valid) h->st_B = 0;
        if (h->B > h->st_B) h->st_valid = false;
        if (h->st_valid) {
            if (flags & TMPC_ITER_KEEP_ITERATE) st |= tmpc::ST_KEEP_ITERATE;
            if (flags & TMPC_ITER_KEEP_MULTIPLIERS) st |= tmpc::ST_KEEP_MULTIPLIERS;
        }
    } else {
        // wave kernels: the keep-flags apply per slot -- a slot without stored state (first call, grown batch, new slot of a map)
        // starts like a fresh capsule (slot_flags in the kernels)
        if (flags & TMPC_ITER_KEEP_ITERATE) st |= tmpc::ST_KEEP_ITERATE;
        if (flags & TMPC_ITER_KEEP_MULTIPLIERS) st |= tmpc::ST_KEEP_MULTIPLIERS;
    }
    if (flags & TMPC_ITER_COMPLETE) st |= tmpc::ST_COMPLETE;
    // a new solve() of the slots' Solvers: the "iteration loop has ended" marks belong to the previous solve (:105-106 is local to one solve())
    if ((flags & TMPC_ITER_NEW_SOLVE) && !h->throughput_mode && h->st.allocated()) TMPC_HIP_CHECK(h, h->zero_state(tmpc::SolverState::STOPPED));
    if ((flags & TMPC_ITER_NEW_SOLVE) && h->throughput_mode && h->lanes && tmpc::lanes::clear_stopped(h->lanes, h->stream, h->B_max, h->err)) return TMPC_ERR_HIP;
    const int rc = launch_solve(h, n_iter, st);
    if (rc == TMPC_OK && h->throughput_mode) { h->st_valid = true; if (h->B > h->st_B) h->st_B = h->B; }
    return rc;
}

int tmpc_reset_multipliers(tmpc_handle *h)
{
    if (!h) return TMPC_ERR_INVALID;
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    if (h->throughput_mode) {
        if (h->lanes && tmpc::lanes::reset_multipliers(h->lanes, h->stream, h->B_max, h->err)) return TMPC_ERR_HIP;
    } else if (h->st.allocated()) {
        TMPC_HIP_CHECK(h, h->zero_state(tmpc::SolverState::PI));
        TMPC_HIP_CHECK(h, h->zero_state(tmpc::SolverState::LAMH));
    }
    return TMPC_OK;
}

int tmpc_set_latency_mode(tmpc_handle *h, int32_t on)
{
    if (!h) return TMPC_ERR_INVALID;
    if (on < 0 || on > 3) return TMPC_ERR_INVALID;
    h->latency_mode = on;
    // 1: accepted, but this shape has no such variant (mode 3 then runs as mode 2, mode 2 as mode 1, if those exist)
    return (on == 0 || h->slot[tmpc::SLOT_LAT1 + on - 1].kernel) ? TMPC_OK : 1;
}

int tmpc_latency_mode_capacity(tmpc_handle *h, int32_t mode)
{
    if (!h || mode < 0 || mode > 3) return TMPC_ERR_INVALID;
    if (hipSetDevice(h->device) != hipSuccess) return TMPC_ERR_HIP;
    // mode 0: the throughput kernels of the handle -- the resident set of the persistent (compact) launch, or of the plain kernel
    const int i = mode ? tmpc::SLOT_LAT1 + mode - 1 : h->slot[tmpc::SLOT_CP2].kernel ? tmpc::SLOT_CP2 : tmpc::SLOT_DEFAULT;
    const tmpc::KernelSlot &k = h->slot[i];
    if (!k.kernel) return 0;
    if (k.kind == tmpc::KernelSlot::COMPACT) return k.resident;
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k.kernel, k.threads, k.lds_bytes) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess) { h->err = "tmpc_latency_mode_capacity: occupancy query failed"; return TMPC_ERR_HIP; }
    // variant 3 is built for ONE workgroup per CU (a wave on every SIMD): a second one fits (LDS, registers) but shares the SIMDs, and the launch is then
    // slower than variant 2's (measured, cfg 4's share of 8 = 512 trajectories: 1.79 ms against 1.31 ms, profiles/round6_cfg4_share8_*): its capacity is what
    // it serves well, not what the hardware would hold
    if (mode == 3 && per_cu > 1) per_cu = 1;
    return per_cu * cus;
}

int tmpc_set_slots(tmpc_handle *h, const int32_t *slots)
{
    if (!h) return TMPC_ERR_INVALID;
    if (!slots) { h->slots_set = false; h->slots_B = 0; return TMPC_OK; }
    if (h->B <= 0) { h->err = "tmpc_set_slots: set the batch first (the map has one entry per batch entry)"; return TMPC_ERR_INVALID; }
    std::vector<char> seen((size_t)h->B_max, 0);
    for (int b = 0; b < h->B; b++) {
        if (slots[b] < 0 || slots[b] >= h->B_max || seen[slots[b]]) { h->err = "tmpc_set_slots: slots must be distinct and in [0, B_max)"; return TMPC_ERR_INVALID; }
        seen[slots[b]] = 1;
    }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    const tmpc::IoRegion &r = h->io.in[tmpc::IN_SLOT];
    if (h->pin_in) {                                                // pinned mirror: asynchronous, nothing to wait for (the caller's array is copied here)
        if (h->slot_pending) { TMPC_HIP_CHECK(h, hipEventSynchronize(h->slot_done)); h->slot_pending = false; }      // (not the batch copy just enqueued: it reads other bytes)
        std::memcpy(h->pin_in + r.offset, slots, r.bytes(h->B));
        TMPC_HIP_CHECK(h, hipMemcpyAsync(h->d_slot, h->pin_in + r.offset, r.bytes(h->B), hipMemcpyHostToDevice, h->stream));
        TMPC_HIP_CHECK(h, hipEventRecord(h->slot_done, h->stream)); h->slot_pending = true;
    } else {
        TMPC_HIP_CHECK(h, hipMemcpyAsync(h->d_slot, slots, r.bytes(h->B), hipMemcpyHostToDevice, h->stream));
        TMPC_HIP_CHECK(h, hipStreamSynchronize(h->stream));        // (the caller's array may go away)
    }
    h->slots_set = true; h->slots_B = h->B;
    return TMPC_OK;
}

int tmpc_set_param_sharing(tmpc_handle *h, const int32_t *base_of) { return tmpc_set_param_sharing_ex(h, base_of, 0); }

int tmpc_set_param_sharing_ex(tmpc_handle *h, const int32_t *base_of, int32_t flags)
{
    if (!h || (flags & ~TMPC_SHARE_COPIES_NOT_MAINTAINED)) return TMPC_ERR_INVALID;
    if (!base_of) { h->share_B = 0; h->share_strict = false; return TMPC_OK; }
#ifdef TMPC_GENERATED_STAGE
    // generated stage functions read every parameter -- halfspace rows included -- from ONE row block (tmpc_gen::rows has no notion of
    // "own" rows), so the hint cannot be honoured: as a pure hint it is accepted and ignored, as include/tmpc_hip.h says; a caller that
    // does not maintain the copies is refused
    if (flags & TMPC_SHARE_COPIES_NOT_MAINTAINED) { h->err = "tmpc_set_param_sharing_ex: generated solvers read every entry's own rows (copies must be maintained)"; return TMPC_ERR_INVALID; }
    h->share_B = 0;
    return TMPC_OK;
#endif
    if ((flags & TMPC_SHARE_COPIES_NOT_MAINTAINED) && h->throughput_mode) { h->err = "tmpc_set_param_sharing_ex: the lane kernels read every entry's own rows (copies must be maintained)"; return TMPC_ERR_INVALID; }
    if (h->B <= 0) { h->err = "tmpc_set_param_sharing: set the batch first (the map has one entry per batch entry)"; return TMPC_ERR_INVALID; }
    for (int b = 0; b < h->B; b++)
        if (base_of[b] < 0 || base_of[b] >= h->B) { h->err = "tmpc_set_param_sharing: entries must be batch indices in [0, B)"; return TMPC_ERR_INVALID; }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    if (!h->d_share) TMPC_HIP_CHECK(h, hipMalloc(&h->d_share, (size_t)h->B_max * 4));
    TMPC_HIP_CHECK(h, hipMemcpyAsync(h->d_share, base_of, (size_t)h->B * 4, hipMemcpyHostToDevice, h->stream));
    TMPC_HIP_CHECK(h, hipStreamSynchronize(h->stream));            // (the caller's array may go away)
    h->share_B = h->B;
    h->share_strict = (flags & TMPC_SHARE_COPIES_NOT_MAINTAINED) != 0;
    return TMPC_OK;
}

int tmpc_copy_state(tmpc_handle *dst, tmpc_handle *src)
{
    if (!dst || !src || dst == src) return TMPC_ERR_INVALID;
    const tmpc::Dims &a = dst->d, &b = src->d;
    if (a.N != b.N || a.n_up != b.n_up || a.M != b.M || a.npar != b.npar || a.slack != b.slack || a.cost_model != b.cost_model || a.row_model != b.row_model ||
        dst->device != src->device || dst->throughput_mode || src->throughput_mode) {
        dst->err = "tmpc_copy_state: handles of different shape / device / kernel family"; return TMPC_ERR_INVALID;
    }
    if (!src->st.allocated()) return TMPC_OK;                                 // nothing stored yet
    TMPC_HIP_CHECK(dst, hipSetDevice(dst->device));
    TMPC_HIP_CHECK(dst, hipStreamSynchronize(src->stream));
    if (!dst->st.allocated() && !dst->st.allocate(a, dst->B_max, dst->stream)) { dst->err = "tmpc_copy_state: allocation failed"; return TMPC_ERR_HIP; }
    const size_t n = (size_t)(dst->B_max < src->B_max ? dst->B_max : src->B_max);
    for (int i = 0; i < tmpc::SolverState::COUNT; i++)
        TMPC_HIP_CHECK(dst, hipMemcpyAsync(dst->st.a[i], src->st.a[i], tmpc::SolverState::bytes(a, n, i), hipMemcpyDeviceToDevice, dst->stream));
    TMPC_HIP_CHECK(dst, hipStreamSynchronize(dst->stream));
    return TMPC_OK;
}

int tmpc_clear_slot(tmpc_handle *h, int32_t slot)
{
    if (!h || slot < 0 || slot >= h->B_max) { if (h) h->err = "tmpc_clear_slot: slot out of range"; return TMPC_ERR_INVALID; }
    if (h->throughput_mode) { h->err = "tmpc_clear_slot: the lane kernels keep their state per launch, not per slot"; return TMPC_ERR_INVALID; }
    if (!h->st.allocated()) return TMPC_OK;                                 // nothing stored yet: every slot is fresh
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    TMPC_HIP_CHECK(h, hipMemsetAsync(h->st.get<int>(tmpc::SolverState::HAS) + slot, 0, 4, h->stream));
    TMPC_HIP_CHECK(h, hipMemsetAsync(h->st.get<int>(tmpc::SolverState::STOPPED) + slot, 0, 4, h->stream));
    return TMPC_OK;
}

__global__ __launch_bounds__(256) void tmpc_poison_lds_kernel(int n_doubles)
{
    extern __shared__ __attribute__((aligned(16))) double poison_smem[];
    const unsigned long long pat = 0x7ff4dead0000beefull;                 // a signalling NaN
    for (int i = threadIdx.x; i < n_doubles; i += blockDim.x) poison_smem[i] = __builtin_bit_cast(double, pat);
    __syncthreads();
    if (poison_smem[(threadIdx.x * 97) % n_doubles] == 0.0) poison_smem[0] = 1.0;      // (keeps the stores alive)
}

int tmpc_has_lab_switches(void)
{
#ifdef TMPC_LAB_SWITCHES
    return 1;
#else
    return 0;
#endif
}

int tmpc_debug_poison_lds(tmpc_handle *h)
{
    if (!h) return TMPC_ERR_INVALID;
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    int cus = 0;
    TMPC_HIP_CHECK(h, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
    const int bytes = 160 * 1024;
    TMPC_HIP_CHECK(h, hipFuncSetAttribute((const void *)tmpc_poison_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    for (int round = 0; round < 4; round++) {                               // (one workgroup per CU fits at a time: a few rounds reach every CU whatever the dispatch order)
        hipLaunchKernelGGL(tmpc_poison_lds_kernel, dim3(cus * 2), dim3(256), bytes, h->stream, bytes / 8);
        TMPC_HIP_CHECK(h, hipGetLastError());
    }
    TMPC_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    return TMPC_OK;
}

int tmpc_debug_lds_passes(int32_t N, int32_t n_pair, int32_t nh, int32_t threads, int32_t dstride)
{
    if (N < 1 || N > 64 || nh < 0 || n_pair < 0 || n_pair > nh || (threads != 64 && threads != 128) || dstride < 2 * n_pair + 3 * (nh - n_pair)) return TMPC_ERR_INVALID;
    return tmpc::d_load_passes(N, n_pair, nh, threads, dstride);
}

int tmpc_has_lane_kernels(void)
{
#ifdef TMPC_WITH_LANES
    return 1;
#else
    return 0;
#endif
}

int tmpc_set_throughput_mode(tmpc_handle *h, int32_t on)
{
    if (!h) return TMPC_ERR_INVALID;
    if (on && tmpc::stage_model(h->d) != 0) { h->err = "tmpc_set_throughput_mode: the lane kernels have the MPCC contouring cost and ellipsoid rows only"; return TMPC_ERR_INVALID; }
    if (on && h->d.model != 0) { h->err = "tmpc_set_throughput_mode: the lane kernels integrate the contouring model (spline state) only"; return TMPC_ERR_INVALID; }
    if (on && h->share_strict) { h->err = "tmpc_set_throughput_mode: a parameter-sharing map with TMPC_SHARE_COPIES_NOT_MAINTAINED is registered and the lane kernels read every entry's own rows"; return TMPC_ERR_INVALID; }
    if (on && !h->lanes) {
        TMPC_HIP_CHECK(h, hipSetDevice(h->device));
        h->lanes = tmpc::lanes::create(h->d, h->B_max, h->err);
        if (!h->lanes) return TMPC_ERR_HIP;
    }
    if (h->throughput_mode != (on != 0)) { if (int rc = invalidate_state(h)) return rc; }      // the two kernel families keep their persistent state separately
    h->throughput_mode = on != 0;
    return TMPC_OK;
}

int tmpc_synchronize(tmpc_handle *h)
{
    if (!h) return TMPC_ERR_INVALID;
    TMPC_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    return TMPC_OK;
}

int tmpc_get(tmpc_handle *h, double *xtraj, double *utraj, double *pobj, int32_t *exit_code, int32_t *qp_status,
             int32_t *sqp_iter, double *res_eq, int32_t *qp_iter_total)
{
    if (!h || h->B <= 0) return TMPC_ERR_INVALID;
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    void *const dst[tmpc::OUT_COUNT] = {xtraj, utraj, pobj, res_eq, exit_code, qp_status, sqp_iter, qp_iter_total};      // in the table's order (tmpc::IoOut)
    const tmpc::IoRegion *r = h->io.out;
    const size_t B = h->B;
    if (h->pin_out && h->io.out_total <= (256u << 10)) {            // one D2H copy of the whole output block into its pinned mirror
        TMPC_HIP_CHECK(h, hipMemcpyAsync(h->pin_out, h->dev_out, h->io.out_total, hipMemcpyDeviceToHost, h->stream));
    } else {                                                        // the first B entries of every array the caller asked for: into the mirror (B_max well above a
        for (int i = 0; i < tmpc::OUT_COUNT; i++) {                 // tick's size), or -- a handle without mirrors -- into the caller's array
            if (!dst[i]) continue;
            void *to = h->pin_out ? (void *)(h->pin_out + r[i].offset) : dst[i];
            TMPC_HIP_CHECK(h, hipMemcpyAsync(to, h->dev_out + r[i].offset, r[i].bytes(B), hipMemcpyDeviceToHost, h->stream));
        }
    }
    TMPC_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    if (h->pin_out)                                                 // host copies of what was asked for
        for (int i = 0; i < tmpc::OUT_COUNT; i++) if (dst[i]) std::memcpy(dst[i], h->pin_out + r[i].offset, r[i].bytes(B));
    return TMPC_OK;
}

int tmpc_select_best(tmpc_handle *h, int32_t first, int32_t count, const double *weight, const uint8_t *disabled, int32_t *best)
{
    if (!h || !best || first < 0 || count <= 0 || first + count > h->B) { if (h) h->err = "tmpc_select_best: bad range"; return TMPC_ERR_INVALID; }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    if (weight) TMPC_HIP_CHECK(h, hipMemcpyAsync(h->d_weight, weight, (size_t)count * 8, hipMemcpyHostToDevice, h->stream));
    if (disabled) TMPC_HIP_CHECK(h, hipMemcpyAsync(h->d_disabled, disabled, (size_t)count, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(tmpc::tmpc_select_best_kernel, dim3(1), dim3(256), 0, h->stream, first, count, h->pobj, h->exit_code,
                       weight ? h->d_weight : nullptr, disabled ? h->d_disabled : nullptr, h->d_best);
    TMPC_HIP_CHECK(h, hipGetLastError());
    TMPC_HIP_CHECK(h, hipMemcpyAsync(best, h->d_best, 4, hipMemcpyDeviceToHost, h->stream));
    TMPC_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    return TMPC_OK;
}

int tmpc_get_stream(tmpc_handle *h, void **stream)
{
    if (!h || !stream) return TMPC_ERR_INVALID;
    *stream = (void *)h->stream;
    return TMPC_OK;
}

int tmpc_kernel_info(const tmpc_handle *h, char *buf, int32_t capacity)
{
    if (!h || !buf || capacity <= 0) return TMPC_ERR_INVALID;
    using tmpc::KernelSlot;
    const KernelSlot &def = h->slot[tmpc::SLOT_DEFAULT], &small = h->slot[tmpc::SLOT_SMALL], &cp2 = h->slot[tmpc::SLOT_CP2];
    const bool compact = def.kind == KernelSlot::COMPACT;
    const char *family = h->throughput_mode                ? "lanes (one lane per trajectory)"
                         : def.kind == KernelSlot::GENERIC ? "generic (one wave per trajectory, rows in LDS)"
                         : !compact                        ? (def.threads == 128 ? "fast, two waves per trajectory" : "fast (one wave per trajectory)")
                                                           : "compact (one wave per trajectory, two waves per SIMD)";
    const std::string sm = (small.kernel && small.bound > 0) ? "; launches of at most " + std::to_string(small.bound) + " trajectories: fast one-wave variant (LDS " +
                                                               std::to_string(small.lds_bytes) + " B, one workgroup per trajectory)" : "";
    const std::string cp = cp2.kernel ? "; launches of more than " + std::to_string(cp2.bound) + " trajectories: compact two-wave variant (LDS " +
                                        std::to_string(cp2.lds_bytes) + " B, persistent launch, resident workgroups " + std::to_string(cp2.resident) + ")" : "";
    // the instantiation of every filled slot, by the slot's label (tmpc::Slot)
    static const char *const label[tmpc::SLOT_COUNT] = {"default", "small", "cp2", "lat1", "lat2", "lat3"};
    std::string names = std::string("; kernels: default=") + def.name;
    for (int i = tmpc::SLOT_SMALL; i < tmpc::SLOT_COUNT; i++) if (h->slot[i].kernel) names += std::string(", ") + label[i] + "=" + h->slot[i].name;
    const int n = snprintf(buf, (size_t)capacity, "%s; trajectories per workgroup %d; LDS %zu B per workgroup; %s%s%s", family, 1,
                           def.lds_bytes, compact ? (std::string("persistent launch, resident workgroups ") + std::to_string(def.resident)).c_str()
                                                  : "one workgroup per trajectory", (cp + sm).c_str(), names.c_str());
    return n < capacity ? n : capacity - 1;
}

int tmpc_result_device_ptrs(tmpc_handle *h, void **d_pobj, void **d_exit_code)
{
    if (!h) return TMPC_ERR_INVALID;
    if (d_pobj) *d_pobj = h->pobj;
    if (d_exit_code) *d_exit_code = h->exit_code;
    return TMPC_OK;
}

int tmpc_pack_records(tmpc_handle *h, void *d_records, const void *d_guidance_id, const void *d_weight)
{
    if (!h || h->B <= 0 || !d_records) return TMPC_ERR_INVALID;
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(tmpc::tmpc_pack_records_kernel, dim3((h->B + 255) / 256), dim3(256), 0, h->stream, h->B, h->pobj,
                       h->exit_code, (const int *)d_guidance_id, (const double *)d_weight, (tmpc_record *)d_records);
    TMPC_HIP_CHECK(h, hipGetLastError());
    return TMPC_OK;
}

int tmpc_select_best_records(tmpc_handle *h, const void *d_records, int32_t n_ranks, int32_t n_scenes, int32_t per_rank, void *d_best)
{
    if (!h || !d_records || !d_best || n_ranks <= 0 || n_scenes <= 0 || per_rank <= 0) return TMPC_ERR_INVALID;
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(tmpc::tmpc_select_best_records_kernel, dim3(n_scenes), dim3(64), 0, h->stream,
                       (const tmpc_record *)d_records, n_ranks, n_scenes, per_rank, (int *)d_best);
    TMPC_HIP_CHECK(h, hipGetLastError());
    return TMPC_OK;
}

int tmpc_gather_best(tmpc_handle *h, const void *d_best, int32_t n_sets, int32_t set_size, int32_t index_offset, void *d_xtraj, void *d_utraj)
{
    if (!h || !d_best || !d_xtraj || !d_utraj || n_sets <= 0 || set_size <= 0 || index_offset < 0 || (int64_t)n_sets * set_size > h->B) {
        if (h) h->err = "tmpc_gather_best: bad argument (n_sets x set_size entries of the current batch)";
        return TMPC_ERR_INVALID;
    }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(tmpc::tmpc_gather_best_kernel, dim3(n_sets), dim3(64), 0, h->stream, (const int *)d_best, set_size, index_offset,
                       (int)h->io.out[tmpc::OUT_XTRAJ].doubles(), (int)h->io.out[tmpc::OUT_UTRAJ].doubles(), h->xtraj, h->utraj, (double *)d_xtraj, (double *)d_utraj);
    TMPC_HIP_CHECK(h, hipGetLastError());
    return TMPC_OK;
}

int tmpc_track_path(tmpc_handle *h, int32_t n_scenes, int32_t n_seg_max, const void *d_path, const void *d_path_count, const void *d_path_length,
                    const void *d_bounds, const void *d_pos, int32_t pos_stride, const tmpc_path_options *options, void *d_segment,
                    void *d_closest_s, void *d_window, void *d_bound_window, void *d_reached)
{
    if (!h) return TMPC_ERR_INVALID;
    tmpc_path_options o{};                                            // NULL: the defaults (search_range 2, the handle's S)
    o.size = sizeof(o); o.search_range = 2;
    if (!read_options(h, "tmpc_track_path", "tmpc_path_options", options, o, (uint32_t)offsetof(tmpc_path_options, window_segments))) return TMPC_ERR_INVALID;
    if (o.window_segments < 0 || o.window_segments > tmpc::VELOCITY_MAX_WINDOW) { h->err = "tmpc_track_path: 0 <= window_segments <= 64"; return TMPC_ERR_INVALID; }
#ifdef TMPC_GENERATED_STAGE
    if (o.window_segments == 0) TMPC_NOT_IN_GENERATED_SOLVER(h, "tmpc_track_path");     // such a handle has no S: the caller has to supply it
    const int S = o.window_segments;
#else
    if (o.window_segments != 0 && o.window_segments != h->d.S) { h->err = "tmpc_track_path: window_segments must be 0 or the handle's S"; return TMPC_ERR_INVALID; }
    const int S = h->d.S;
#endif
    if (n_scenes <= 0) { h->err = "tmpc_track_path: n_scenes must be positive"; return TMPC_ERR_INVALID; }
    if (n_seg_max < 1 || n_seg_max > tmpc::PATH_MAX_SEGMENTS) { h->err = "tmpc_track_path: 1 <= n_seg_max <= 1024"; return TMPC_ERR_INVALID; }
    if (o.search_range < 0 || o.search_range > 31) { h->err = "tmpc_track_path: 0 <= search_range <= 31"; return TMPC_ERR_INVALID; }
    if (pos_stride < 2) { h->err = "tmpc_track_path: pos_stride >= 2 (x and y first)"; return TMPC_ERR_INVALID; }
    if (S <= 0) { h->err = "tmpc_track_path: the problem has no path segments (S = 0)"; return TMPC_ERR_INVALID; }
    if (!d_path || !d_path_count || !d_path_length || !d_pos) { h->err = "tmpc_track_path: NULL input (d_path, d_path_count, d_path_length, d_pos)"; return TMPC_ERR_INVALID; }
    if (!d_segment || !d_closest_s || !d_window) { h->err = "tmpc_track_path: NULL output (d_segment, d_closest_s, d_window)"; return TMPC_ERR_INVALID; }
    if ((d_bounds == nullptr) != (d_bound_window == nullptr)) { h->err = "tmpc_track_path: d_bounds and d_bound_window go together (both or neither)"; return TMPC_ERR_INVALID; }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(tmpc::tmpc_track_path_kernel, dim3((unsigned)n_scenes), dim3(64), 0, h->stream, S, n_seg_max, o.search_range,
                       (const double *)d_path, (const int *)d_path_count, (const double *)d_path_length, (const double *)d_bounds, (const double *)d_pos,
                       pos_stride, (int *)d_segment, (double *)d_closest_s, (double *)d_window, (double *)d_bound_window, (uint8_t *)d_reached);
    TMPC_HIP_CHECK(h, hipGetLastError());
    return TMPC_OK;
}

int tmpc_path_velocity_window(tmpc_handle *h, int32_t n_scenes, int32_t n_seg_max, int32_t S, const void *d_velocity, const void *d_path,
                              const void *d_path_count, const void *d_path_length, const void *d_segment, const void *d_closest_s,
                              const void *d_has_velocity, double reference_velocity, void *d_window, void *d_v_ref)
{
    if (!h) return TMPC_ERR_INVALID;
    if (n_scenes <= 0) { h->err = "tmpc_path_velocity_window: n_scenes must be positive"; return TMPC_ERR_INVALID; }
    if (n_seg_max < 1 || n_seg_max > tmpc::PATH_MAX_SEGMENTS) { h->err = "tmpc_path_velocity_window: 1 <= n_seg_max <= 1024"; return TMPC_ERR_INVALID; }
    if (S < 1 || S > tmpc::VELOCITY_MAX_WINDOW) { h->err = "tmpc_path_velocity_window: 1 <= S <= 64"; return TMPC_ERR_INVALID; }
    if (!d_path || !d_path_count || !d_path_length || !d_segment || !d_closest_s) {
        h->err = "tmpc_path_velocity_window: NULL input (d_path, d_path_count, d_path_length, d_segment, d_closest_s)"; return TMPC_ERR_INVALID;
    }
    if (!d_window) { h->err = "tmpc_path_velocity_window: NULL output (d_window)"; return TMPC_ERR_INVALID; }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(tmpc::tmpc_path_velocity_window_kernel, dim3((unsigned)n_scenes), dim3(64), 0, h->stream, S, n_seg_max, (const double *)d_velocity,
                       (const double *)d_path, (const int *)d_path_count, (const int *)d_segment, (const double *)d_closest_s,
                       (const uint8_t *)d_has_velocity, reference_velocity, (double *)d_window, (double *)d_v_ref);
    TMPC_HIP_CHECK(h, hipGetLastError());
    return TMPC_OK;
}

int tmpc_scatter_parameters(tmpc_handle *h, const int32_t *cols, int32_t n_cols, const void *d_values, int32_t per_stage, const void *d_scene_of,
                            int32_t n_scenes)
{
    if (!h) return TMPC_ERR_INVALID;
    if (h->B <= 0 || !h->params) { h->err = "tmpc_scatter_parameters: no batch (call tmpc_set_batch* first)"; return TMPC_ERR_INVALID; }
    if (!cols || !d_values || !d_scene_of || n_scenes <= 0) { h->err = "tmpc_scatter_parameters: bad argument (cols, d_values, d_scene_of, n_scenes > 0)"; return TMPC_ERR_INVALID; }
    if (n_cols < 1 || n_cols > tmpc::SCATTER_MAX_COLS) { h->err = "tmpc_scatter_parameters: 1 <= n_cols <= 128"; return TMPC_ERR_INVALID; }
    if (per_stage != 0 && per_stage != 1) { h->err = "tmpc_scatter_parameters: per_stage is 0 or 1"; return TMPC_ERR_INVALID; }
    tmpc::ScatterCols list{};
    if (!read_stack_columns(h, "tmpc_scatter_parameters: ", cols, n_cols, list)) return TMPC_ERR_INVALID;
    return launch_flat(h, "tmpc_scatter_parameters: ", "B x N x n_cols", (int64_t)h->B * h->d.N * n_cols, tmpc::tmpc_scatter_parameters_kernel, h->d, h->B,
                       const_cast<double *>(h->params), list, (const double *)d_values, (const int *)d_scene_of, n_scenes, per_stage);
}

int tmpc_fit_path(tmpc_handle *h, int32_t n_scenes, int32_t n_pts_max, int32_t n_seg_max, const void *d_xy, const void *d_count, const void *d_s,
                  const void *d_left_xy, const void *d_right_xy, const void *d_v, void *d_path, void *d_path_count, void *d_path_length,
                  void *d_bounds, void *d_velocity, void *d_road_width, void *d_status)
{
    if (!h) return TMPC_ERR_INVALID;
    if (n_scenes <= 0) { h->err = "tmpc_fit_path: n_scenes must be positive"; return TMPC_ERR_INVALID; }
    if (n_pts_max < 2 || n_pts_max > tmpc::FIT_MAX_POINTS) { h->err = "tmpc_fit_path: 2 <= n_pts_max <= 1025"; return TMPC_ERR_INVALID; }
    if (n_seg_max < n_pts_max - 1 || n_seg_max > tmpc::PATH_MAX_SEGMENTS) { h->err = "tmpc_fit_path: n_pts_max - 1 <= n_seg_max <= 1024"; return TMPC_ERR_INVALID; }
    if (!d_xy || !d_count) { h->err = "tmpc_fit_path: NULL input (d_xy, d_count)"; return TMPC_ERR_INVALID; }
    if (!d_path || !d_path_count || !d_path_length) { h->err = "tmpc_fit_path: NULL output (d_path, d_path_count, d_path_length)"; return TMPC_ERR_INVALID; }
    if ((d_left_xy == nullptr) != (d_right_xy == nullptr) || (d_left_xy == nullptr) != (d_bounds == nullptr)) {
        h->err = "tmpc_fit_path: d_left_xy, d_right_xy and d_bounds go together (all or none)"; return TMPC_ERR_INVALID;
    }
    if ((d_v == nullptr) != (d_velocity == nullptr)) { h->err = "tmpc_fit_path: d_v and d_velocity go together (both or neither)"; return TMPC_ERR_INVALID; }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(tmpc::tmpc_fit_path_kernel, dim3((unsigned)n_scenes), dim3(64), 0, h->stream, n_pts_max, n_seg_max, (const double *)d_xy,
                       (const int *)d_count, (const double *)d_s, (const double *)d_left_xy, (const double *)d_right_xy, (const double *)d_v,
                       (double *)d_path, (int *)d_path_count, (double *)d_path_length, (double *)d_bounds, (double *)d_velocity,
                       (double *)d_road_width, (uint8_t *)d_status);
    TMPC_HIP_CHECK(h, hipGetLastError());
    return TMPC_OK;
}

int tmpc_costmap_points(tmpc_handle *h, int32_t n_scenes, int32_t size_x, int32_t size_y, const void *d_cost, const void *d_origin, double resolution,
                        int32_t n_pts_max, void *d_points, void *d_count, void *d_overflow)
{
    if (!h) return TMPC_ERR_INVALID;
    if (n_scenes <= 0) { h->err = "tmpc_costmap_points: n_scenes must be positive"; return TMPC_ERR_INVALID; }
    if (size_x < 1 || size_y < 1 || (int64_t)size_x * size_y > tmpc::COSTMAP_MAX_CELLS) { h->err = "tmpc_costmap_points: size_x, size_y >= 1 and size_x x size_y <= 2^20"; return TMPC_ERR_INVALID; }
    if (n_pts_max < 1 || n_pts_max > tmpc::DECOMP_MAX_POINTS) { h->err = "tmpc_costmap_points: 1 <= n_pts_max <= 16384"; return TMPC_ERR_INVALID; }
    if (!d_cost || !d_origin) { h->err = "tmpc_costmap_points: NULL input (d_cost, d_origin)"; return TMPC_ERR_INVALID; }
    if (!d_points || !d_count) { h->err = "tmpc_costmap_points: NULL output (d_points, d_count)"; return TMPC_ERR_INVALID; }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(tmpc::tmpc_costmap_points_kernel, dim3((unsigned)n_scenes), dim3(tmpc::DECOMP_THREADS), 0, h->stream, size_x, size_y, resolution, n_pts_max,
                       (const uint8_t *)d_cost, (const double *)d_origin, (double *)d_points, (int *)d_count, (uint8_t *)d_overflow);
    TMPC_HIP_CHECK(h, hipGetLastError());
    return TMPC_OK;
}

int tmpc_sample_scenarios(tmpc_handle *h, const void *d_pred, const void *d_prob, int32_t n_solvers, int32_t n_obstacles, int32_t n_modes,
                          int32_t n_scenarios, uint64_t seed, void *d_samples)
{
    if (!h || !d_pred || !d_prob || !d_samples || n_solvers <= 0 || n_obstacles <= 0 || n_modes <= 0 || n_scenarios <= 0) {
        if (h) h->err = "tmpc_sample_scenarios: bad argument";
        return TMPC_ERR_INVALID;
    }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    const int n = n_solvers * n_obstacles * n_scenarios;
    hipLaunchKernelGGL(tmpc::tmpc_sample_scenarios_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d.N, n_solvers, n_obstacles, n_modes,
                       n_scenarios, (unsigned long long)seed, (const double *)d_pred, (const double *)d_prob, (double *)d_samples);
    TMPC_HIP_CHECK(h, hipGetLastError());
    return TMPC_OK;
}

int tmpc_scenario_discard(tmpc_handle *h, const void *d_samples, int32_t n_pts, int32_t n_scenarios, int32_t n_discard, const void *d_scene_of, double radius)
{
    if (!h || h->B <= 0 || !h->x0 || !d_samples || !d_scene_of || n_pts <= 0 || n_scenarios <= 0 || n_pts % n_scenarios != 0 || n_discard < 0 ||
        n_discard >= n_scenarios || n_scenarios > 16384) {
        if (h) h->err = "tmpc_scenario_discard: bad argument / no batch (n_pts = obstacles x n_scenarios, 0 <= n_discard < n_scenarios <= 16384)";
        return TMPC_ERR_INVALID;
    }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    const size_t need = (size_t)h->B_max * n_scenarios;
    if (int rc = grow_scratch(h, &h->scn_discard, &h->scn_discard_cap, need)) return rc;
    const size_t lds = (size_t)n_scenarios * sizeof(double);
    if (lds > 48 * 1024)
        TMPC_HIP_CHECK(h, hipFuncSetAttribute(reinterpret_cast<const void *>(tmpc::tmpc_scenario_discard_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(tmpc::tmpc_scenario_discard_kernel, dim3(h->B), dim3(256), lds, h->stream, h->d, h->B, h->x0, (const double *)d_samples, n_pts,
                       n_scenarios, (const int *)d_scene_of, radius, n_discard, h->scn_discard);
    TMPC_HIP_CHECK(h, hipGetLastError());
    h->scn_discard_S = n_scenarios; h->scn_discard_B = h->B; h->scn_discard_n = n_discard;
    return TMPC_OK;
}

int tmpc_scenario_discarded(tmpc_handle *h, void *d_mask)
{
    if (!h || !d_mask || !h->scn_discard || h->scn_discard_B != h->B) { if (h) h->err = "tmpc_scenario_discarded: no discard set for the current batch"; return TMPC_ERR_INVALID; }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    TMPC_HIP_CHECK(h, hipMemcpyAsync(d_mask, h->scn_discard, (size_t)h->B * h->scn_discard_S, hipMemcpyDeviceToDevice, h->stream));
    return TMPC_OK;
}

int tmpc_scenario_empty_stages(tmpc_handle *h, void *d_count)
{
    if (!h || !d_count) return TMPC_ERR_INVALID;
    if (!h->scn_sample || h->scn_B != h->B || h->B <= 0) { h->err = "tmpc_scenario_empty_stages: the scenario rows of the current batch were not built by tmpc_scenario_halfspaces"; return TMPC_ERR_INVALID; }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    const size_t units = (size_t)h->B * h->d.N;
    TMPC_HIP_CHECK(h, hipMemcpyAsync(d_count, h->scn_sample + units * h->scn_rows + 1 + units, sizeof(int) * (size_t)h->B, hipMemcpyDeviceToDevice, h->stream));
    return TMPC_OK;
}

int tmpc_warmstart(tmpc_handle *h, const void *d_state, const void *d_mode, const void *d_src, double deceleration)
{
    if (!h || h->B <= 0 || !h->x0 || !h->xinit || !d_state) { if (h) h->err = "tmpc_warmstart: bad argument / no batch"; return TMPC_ERR_INVALID; }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    const int n = h->B * (h->d.N + 1);
    hipLaunchKernelGGL(tmpc::tmpc_warmstart_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d, h->B, (const double *)d_state,
                       (const int *)d_mode, (const int *)d_src, h->xtraj, h->utraj, const_cast<double *>(h->x0),
                       const_cast<double *>(h->xinit), deceleration);
    TMPC_HIP_CHECK(h, hipGetLastError());
    return TMPC_OK;
}

int tmpc_init_with_guidance(tmpc_handle *h, const void *d_gpos, const void *d_gvel, const void *d_enabled)
{
    if (!h || h->B <= 0 || !h->x0 || !d_gpos || !d_gvel) { if (h) h->err = "tmpc_init_with_guidance: bad argument / no batch"; return TMPC_ERR_INVALID; }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    const int n = h->B * (h->d.N + 1);
    hipLaunchKernelGGL(tmpc::tmpc_init_with_guidance_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d, h->B,
                       (const double *)d_gpos, (const double *)d_gvel, (const uint8_t *)d_enabled, const_cast<double *>(h->x0));
    TMPC_HIP_CHECK(h, hipGetLastError());
    return TMPC_OK;
}

int tmpc_sample_guidance(tmpc_handle *h, int32_t n_traj, int32_t n_nodes_max, const void *d_nodes, const void *d_node_count, void *d_gpos,
                         void *d_gvel, void *d_status)
{
    if (!h) return TMPC_ERR_INVALID;
    if (n_traj <= 0) { h->err = "tmpc_sample_guidance: n_traj must be positive"; return TMPC_ERR_INVALID; }
    if (n_nodes_max < 2 || n_nodes_max > tmpc::GUIDANCE_MAX_NODES) { h->err = "tmpc_sample_guidance: 2 <= n_nodes_max <= 64"; return TMPC_ERR_INVALID; }
    if (!d_nodes || !d_node_count) { h->err = "tmpc_sample_guidance: NULL input (d_nodes, d_node_count)"; return TMPC_ERR_INVALID; }
    if (!d_gpos || !d_gvel || !d_status) { h->err = "tmpc_sample_guidance: NULL output (d_gpos, d_gvel, d_status)"; return TMPC_ERR_INVALID; }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(tmpc::tmpc_sample_guidance_kernel, dim3((unsigned)n_traj), dim3(64), 0, h->stream, h->d.N, h->d.dt, n_nodes_max,
                       (const double *)d_nodes, (const int *)d_node_count, (double *)d_gpos, (double *)d_gvel, (int *)d_status);
    TMPC_HIP_CHECK(h, hipGetLastError());
    return TMPC_OK;
}

// the checks tmpc_guidance_plan and tmpc_guidance_decide share: the scene count and the options (NULL is refused: n_paths has no default)
static bool read_guidance_options(tmpc_handle *h, const char *fn, int32_t n_scenes, const tmpc_guidance_options *opt, tmpc::GuidanceOptions &g)
{
    if (n_scenes <= 0) { h->err = std::string(fn) + ": n_scenes must be positive"; return false; }
    if (!opt) { h->err = std::string(fn) + ": NULL options"; return false; }
    tmpc_guidance_options o{};
    if (!read_options(h, fn, "tmpc_guidance_options", opt, o)) return false;
    if (o.n_paths < 1 || o.n_paths > tmpc::GUIDANCE_MAX_PATHS) { h->err = std::string(fn) + ": 1 <= n_paths <= 63"; return false; }
    g = tmpc::GuidanceOptions{o.n_paths, o.use_tmpcpp ? 1 : 0, o.warmstart_with_mpc_solution ? 1 : 0, o.shift_previous_solution_forward ? 1 : 0,
                              o.selection_weight_consistency};
    return true;
}

int tmpc_guidance_plan(tmpc_handle *h, int32_t n_scenes, const tmpc_guidance_options *opt, const void *d_traj_count, const void *d_topology_class,
                       const void *d_previously_selected, const void *d_planner_ids, const void *d_selection, void *d_mode, void *d_src,
                       void *d_init_enabled, void *d_rows_dummy, void *d_disabled, void *d_guidance_id, void *d_weight)
{
    if (!h) return TMPC_ERR_INVALID;
    tmpc::GuidanceOptions g{};
    if (!read_guidance_options(h, "tmpc_guidance_plan", n_scenes, opt, g)) return TMPC_ERR_INVALID;
    if (!d_traj_count || !d_topology_class || !d_planner_ids || !d_selection) {
        h->err = "tmpc_guidance_plan: NULL input (d_traj_count, d_topology_class, d_planner_ids, d_selection)"; return TMPC_ERR_INVALID;
    }
    if (!d_mode || !d_src || !d_init_enabled || !d_rows_dummy || !d_disabled || !d_guidance_id || !d_weight) {
        h->err = "tmpc_guidance_plan: NULL output (d_mode, d_src, d_init_enabled, d_rows_dummy, d_disabled, d_guidance_id, d_weight)"; return TMPC_ERR_INVALID;
    }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(tmpc::tmpc_guidance_plan_kernel, dim3((unsigned)((n_scenes + 63) / 64)), dim3(64), 0, h->stream, n_scenes, g,
                       (const int *)d_traj_count, (const int *)d_topology_class, (const uint8_t *)d_previously_selected, (const int *)d_planner_ids,
                       (const int *)d_selection, (int *)d_mode, (int *)d_src, (uint8_t *)d_init_enabled, (uint8_t *)d_rows_dummy, (uint8_t *)d_disabled,
                       (int *)d_guidance_id, (double *)d_weight);
    TMPC_HIP_CHECK(h, hipGetLastError());
    return TMPC_OK;
}

int tmpc_guidance_decide(tmpc_handle *h, int32_t n_scenes, const tmpc_guidance_options *opt, const void *d_pobj, const void *d_exit_code,
                         const void *d_disabled, const void *d_guidance_id, const void *d_weight, const void *d_state, double deceleration,
                         double control_dt, int32_t enable_output, void *d_best, void *d_exit, void *d_cmd, void *d_planner_ids, void *d_selection)
{
    if (!h) return TMPC_ERR_INVALID;
    tmpc::GuidanceOptions g{};
    if (!read_guidance_options(h, "tmpc_guidance_decide", n_scenes, opt, g)) return TMPC_ERR_INVALID;
    if (!d_pobj || !d_exit_code || !d_disabled || !d_guidance_id || !d_weight || !d_state) {
        h->err = "tmpc_guidance_decide: NULL input (d_pobj, d_exit_code, d_disabled, d_guidance_id, d_weight, d_state)"; return TMPC_ERR_INVALID;
    }
    if (!d_best || !d_exit || !d_cmd || !d_planner_ids || !d_selection) {
        h->err = "tmpc_guidance_decide: NULL output (d_best, d_exit, d_cmd, d_planner_ids, d_selection)"; return TMPC_ERR_INVALID;
    }
    if (h->B <= 0 || h->solved_B != h->B) { h->err = "tmpc_guidance_decide: no solved batch (tmpc_solve after tmpc_set_batch*)"; return TMPC_ERR_INVALID; }
    if ((int64_t)n_scenes * (g.n_paths + g.use_tmpcpp) != h->B) { h->err = "tmpc_guidance_decide: the batch is not n_scenes x P entries"; return TMPC_ERR_INVALID; }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(tmpc::tmpc_guidance_decide_kernel, dim3((unsigned)((n_scenes + 63) / 64)), dim3(64), 0, h->stream, n_scenes, g, h->d.N,
                       tmpc::ext_nx(h->d), (const double *)d_pobj, (const int *)d_exit_code, (const uint8_t *)d_disabled, (const int *)d_guidance_id,
                       (const double *)d_weight, (const double *)d_state, h->xtraj, h->utraj, deceleration, control_dt, enable_output ? 1 : 0,
                       (int *)d_best, (int *)d_exit, (double *)d_cmd, (int *)d_planner_ids, (int *)d_selection);
    TMPC_HIP_CHECK(h, hipGetLastError());
    return TMPC_OK;
}

int tmpc_debug_get_x0(tmpc_handle *h, double *x0, double *xinit)
{
    if (!h || h->B <= 0 || !h->x0) return TMPC_ERR_INVALID;
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    TMPC_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    if (x0) TMPC_HIP_CHECK(h, hipMemcpy(x0, h->x0, h->io.in[tmpc::IN_X0].bytes(h->B), hipMemcpyDeviceToHost));
    if (xinit) TMPC_HIP_CHECK(h, hipMemcpy(xinit, h->xinit, h->io.in[tmpc::IN_XINIT].bytes(h->B), hipMemcpyDeviceToHost));
    return TMPC_OK;
}

int tmpc_enable_timing(tmpc_handle *h, int32_t max_records)
{
    if (!h || max_records < 0) return TMPC_ERR_INVALID;
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    for (auto &e : h->ev) (void)hipEventDestroy(e);
    h->ev.clear(); h->ev_used = 0; h->timing = max_records > 0;
    h->ev.resize(2 * (size_t)max_records);
    for (auto &e : h->ev) TMPC_HIP_CHECK(h, hipEventCreate(&e));
    return TMPC_OK;
}

int tmpc_get_timings(tmpc_handle *h, float *ms, int32_t capacity, int32_t *n_out)
{
    if (!h || !ms || !n_out) return TMPC_ERR_INVALID;
    TMPC_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    int n = h->ev_used / 2; if (n > capacity) n = capacity;
    for (int i = 0; i < n; i++) TMPC_HIP_CHECK(h, hipEventElapsedTime(&ms[i], h->ev[2 * i], h->ev[2 * i + 1]));
    *n_out = n; h->ev_used = 0;
    return TMPC_OK;
}

int tmpc_time_solve(tmpc_handle *h, int32_t reps, float *ms_each)
{
    if (!h || reps <= 0 || !ms_each) return TMPC_ERR_INVALID;
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    Events evs; evs.ev.assign(2 * (size_t)reps, nullptr);
    std::vector<hipEvent_t> &ev = evs.ev;
    for (auto &e : ev) TMPC_HIP_CHECK(h, hipEventCreate(&e));
    for (int i = 0; i < reps; i++) {
        TMPC_HIP_CHECK(h, hipEventRecord(ev[2 * i], h->stream));
        int rc = tmpc_solve(h);
        if (rc != TMPC_OK) return rc;
        TMPC_HIP_CHECK(h, hipEventRecord(ev[2 * i + 1], h->stream));
    }
    TMPC_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < reps; i++) TMPC_HIP_CHECK(h, hipEventElapsedTime(&ms_each[i], ev[2 * i], ev[2 * i + 1]));
    return TMPC_OK;
}

int tmpc_debug_get_params(tmpc_handle *h, double *params)
{
    if (!h || h->B <= 0 || !params || !h->params) return TMPC_ERR_INVALID;
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    TMPC_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    TMPC_HIP_CHECK(h, hipMemcpy(params, h->params, h->io.in[tmpc::IN_PARAMS].bytes(h->B), hipMemcpyDeviceToHost));
    return TMPC_OK;
}

int tmpc_debug_profile(tmpc_handle *h, int64_t *cycles, int32_t n_phases)
{
    if (!h || h->B <= 0 || !cycles || n_phases < tmpc::PH_COUNT) return TMPC_ERR_INVALID;
    if (h->share_strict) { h->err = "tmpc_debug_profile: the profiled twins read every entry's own parameter rows; a map with TMPC_SHARE_COPIES_NOT_MAINTAINED is registered"; return TMPC_ERR_INVALID; }
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    DevBufs bufs;
    double *dp_ = nullptr;
    const size_t n = (size_t)h->B * tmpc::PH_COUNT;
    TMPC_HIP_CHECK(h, bufs.alloc(&dp_, n * 8));
    long long *dp = (long long *)dp_;
    TMPC_HIP_CHECK(h, hipMemset(dp, 0, n * 8));
    // The instrumented twin of the instantiation a solve of the current batch runs (launch_slot), with that slot's threads and LDS: the generic kernel
    // profiles itself, the fast kernels have profiled twins for some shapes, a compact slot is profiled through the fast kernel of its shape (bitwise the
    // same results, one wave per SIMD): the small slot's, or for the two-wave one the default slot's.  A slot without a twin is refused -- never another
    // instantiation in its place.
    int slot = launch_slot(h);
    if (h->slot[slot].kind == tmpc::KernelSlot::COMPACT) slot = slot == tmpc::SLOT_CP2 ? tmpc::SLOT_DEFAULT : tmpc::SLOT_SMALL;
    const tmpc::KernelSlot &k = h->slot[slot];
    if (!k.twin) {
        h->err = std::string("tmpc_debug_profile: no profiled twin of ") + (*k.name ? k.name : "this kernel") + " (the launch of " + std::to_string(h->B) +
                 " trajectories in latency mode " + std::to_string(h->latency_mode) + ")";
        return TMPC_ERR_INVALID;
    }
    TMPC_HIP_CHECK(h, hipFuncSetAttribute((const void *)k.twin, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds_bytes));
    hipLaunchKernelGGL(k.twin, dim3(h->B), dim3(k.threads), k.lds_bytes, h->stream, h->d, h->B,
                       h->xinit, h->x0, h->params, h->xtraj, h->utraj, h->pobj, h->exit_code, h->qp_status,
                       h->sqp_iter, h->res_eq, h->qp_iter, dp, tmpc::StateIO{nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr});
    TMPC_HIP_CHECK(h, hipGetLastError());
    TMPC_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    std::vector<long long> host(n);
    TMPC_HIP_CHECK(h, hipMemcpy(host.data(), dp, n * 8, hipMemcpyDeviceToHost));
    for (int i = 0; i < tmpc::PH_COUNT; i++) {
        double acc = 0.0;
        for (int b = 0; b < h->B; b++) acc += (double)host[(size_t)b * tmpc::PH_COUNT + i];
        cycles[i] = (int64_t)(acc / h->B);
    }
    return TMPC_OK;
}

int tmpc_debug_eval_stage(tmpc_handle *h, int32_t n, const double *z, const double *p, const double *pi, const double *lamh,
                          double *cost, double *cost_grad, double *cost_hess, double *hval, double *h_jac,
                          double *x_next, double *x_jac, double *lag_hess, double *mirror)
{
    if (!h || n <= 0 || !z || !p) return TMPC_ERR_INVALID;
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    const int nh = h->d.n_up + h->d.M;
    const size_t sz_in[4] = {(size_t)n * tmpc::ext_nv(h->d) * 8, (size_t)n * h->d.npar * 8, (size_t)n * 5 * 8, (size_t)n * nh * 8};
    const void *src[4] = {z, p, pi, lamh};
    DevBufs bufs;
    double *din[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < 4; i++) {
        if (!src[i]) continue;
        TMPC_HIP_CHECK(h, bufs.alloc(&din[i], sz_in[i]));
        TMPC_HIP_CHECK(h, hipMemcpy(din[i], src[i], sz_in[i], hipMemcpyHostToDevice));
    }
    const size_t sz_out[9] = {(size_t)n * 8, (size_t)n * 7 * 8, (size_t)n * 49 * 8, (size_t)n * nh * 8, (size_t)n * nh * 7 * 8,
                              (size_t)n * 5 * 8, (size_t)n * 35 * 8, (size_t)n * 49 * 8, (size_t)n * 49 * 8};
    double *dout[9]; void *dst[9] = {cost, cost_grad, cost_hess, hval, h_jac, x_next, x_jac, lag_hess, mirror};
    for (int i = 0; i < 9; i++) TMPC_HIP_CHECK(h, bufs.alloc(&dout[i], sz_out[i]));
    hipLaunchKernelGGL(tmpc::tmpc_debug_eval_kernel, dim3((n + 63) / 64), dim3(64), 0, h->stream, h->d, n, din[0], din[1], din[2], din[3],
                       dout[0], dout[1], dout[2], dout[3], dout[4], dout[5], dout[6], dout[7], dout[8]);
    TMPC_HIP_CHECK(h, hipGetLastError());
    TMPC_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < 9; i++)
        if (dst[i]) TMPC_HIP_CHECK(h, hipMemcpy(dst[i], dout[i], sz_out[i], hipMemcpyDeviceToHost));
    return TMPC_OK;
}

#ifdef TMPC_SWEEP_PROFILE
// Profiling build only (not declared in tmpc_hip.h): read and reset the sweep clock accumulators.
int tmpc_debug_sweep_profile(tmpc_handle *h, uint64_t *out, int32_t n)
{
    if (!h || !out || n < tmpc::SP_COUNT) return TMPC_ERR_INVALID;
    TMPC_HIP_CHECK(h, hipSetDevice(h->device));
    TMPC_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    unsigned long long host[tmpc::SP_COUNT];
    TMPC_HIP_CHECK(h, hipMemcpyFromSymbol(host, HIP_SYMBOL(tmpc::g_sweep_prof), sizeof host));
    for (int i = 0; i < tmpc::SP_COUNT; i++) out[i] = host[i];
    memset(host, 0, sizeof host);
    TMPC_HIP_CHECK(h, hipMemcpyToSymbol(HIP_SYMBOL(tmpc::g_sweep_prof), host, sizeof host));
    return TMPC_OK;
}
#endif

}  // extern "C"

#ifdef TMPC_LAB_SWITCHES
// Lab library only (not part of include/tmpc_hip.h): the wave and workgroup reductions of the solve kernels (tmpc_kernels.hpp) on caller-supplied lane
// values, one case per workgroup of `threads` (64, 128 or 256) threads -- tests/test_gpu_wave_reductions.py compares every result bit for bit with a
// numpy restatement of the same pairing order.  in: [n_cases][5][threads] doubles (arrays 0 .. 3: the four residual maxima of blk_residuals, array 4:
// its sum; the single-array reductions take array 0).  out: [n_cases][LAB_RED_SCALARS + 3 threads]:
//   [0, 4) wave_max of wave w, [8, 12) wave_min, [12, 16) wave_sum (waves the block does not have: untouched), 16 blk_max, 18 blk_min, 19 blk_sum,
//   20 / 21 blk_residuals' worst / mu; [4, 8), [28, 32), [24, 28) maximum, minimum and sum of wave w by lab_reduce_identity, the network with the
//   operation's identity moved into the vacated lanes and fmax / fmin on the operands (the form the kernels had before the fill was dropped);
//   then per lane stage_sum3, stage_sum_quad<false>, stage_sum_quad<true>.
constexpr int LAB_RED_SCALARS = 32;
template <typename Op>
__device__ __forceinline__ double lab_reduce_identity(double x, double identity, Op op)
{
    x = op(x, tmpc::dpp_move<0x111, 0xf>(x, identity)); x = op(x, tmpc::dpp_move<0x112, 0xf>(x, identity));
    x = op(x, tmpc::dpp_move<0x114, 0xf>(x, identity)); x = op(x, tmpc::dpp_move<0x118, 0xf>(x, identity));
    x = op(x, tmpc::dpp_move<0x142, 0xa>(x, identity)); x = op(x, tmpc::dpp_move<0x143, 0xc>(x, identity));
    return __shfl(x, 63, 64);
}
template <int NTH>
__global__ __launch_bounds__(NTH) void tmpc_lab_reductions_kernel(const double *in, double *out)
{
    __shared__ double scr[64];
    const int tid = threadIdx.x, w = tid >> 6;
    const double *x = in + (size_t)blockIdx.x * 5 * NTH;
    double *o = out + (size_t)blockIdx.x * (LAB_RED_SCALARS + 3 * NTH);
    const double a = x[tid], b = x[NTH + tid], c = x[2 * NTH + tid], m = x[3 * NTH + tid], s = x[4 * NTH + tid];
    const double wmax = tmpc::wave_max(a), wmin = tmpc::wave_min(a), wsum = tmpc::wave_sum(a);
    const double imax = lab_reduce_identity(a, -__builtin_huge_val(), [](double p, double q) { return fmax(p, q); });
    const double imin = lab_reduce_identity(a, __builtin_huge_val(), [](double p, double q) { return fmin(p, q); });
    const double isum = lab_reduce_identity(a, 0.0, [](double p, double q) { return p + q; });
    if ((tid & 63) == 0) { o[w] = wmax; o[4 + w] = imax; o[8 + w] = wmin; o[12 + w] = wsum; o[24 + w] = isum; o[28 + w] = imin; }
    const double bmax = tmpc::blk_max<NTH>(a, scr, tid, 2), bmin = tmpc::blk_min<NTH>(a, scr, tid, 4), bsum = tmpc::blk_sum<NTH>(a, scr, tid, 5);
    double worst, mu = s;
    tmpc::blk_residuals<NTH>(worst, a, b, c, m, mu, scr, tid);
    if (tid == 0) { o[16] = bmax; o[18] = bmin; o[19] = bsum; o[20] = worst; o[21] = mu; }
    o[LAB_RED_SCALARS + tid] = tmpc::stage_sum3(a);
    o[LAB_RED_SCALARS + NTH + tid] = tmpc::stage_sum_quad<false>(a);
    o[LAB_RED_SCALARS + 2 * NTH + tid] = tmpc::stage_sum_quad<true>(a);
}

extern "C" int tmpc_lab_reductions(int32_t threads, int32_t n_cases, const double *in_host, double *out_host)
{
    if ((threads != 64 && threads != 128 && threads != 256) || n_cases < 1 || n_cases > 4096 || !in_host || !out_host) return TMPC_ERR_INVALID;
    const size_t n_in = (size_t)n_cases * 5 * threads, n_out = (size_t)n_cases * (LAB_RED_SCALARS + 3 * threads);
    double *din = nullptr, *dout = nullptr;
    hipError_t e = hipMalloc((void **)&din, n_in * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&dout, n_out * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(din, in_host, n_in * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dout, out_host, n_out * sizeof(double), hipMemcpyHostToDevice);      // (slots the kernel leaves alone keep the caller's values)
    if (e == hipSuccess) {
        if (threads == 64) hipLaunchKernelGGL(tmpc_lab_reductions_kernel<64>, dim3(n_cases), dim3(64), 0, 0, din, dout);
        else if (threads == 128) hipLaunchKernelGGL(tmpc_lab_reductions_kernel<128>, dim3(n_cases), dim3(128), 0, 0, din, dout);
        else hipLaunchKernelGGL(tmpc_lab_reductions_kernel<256>, dim3(n_cases), dim3(256), 0, 0, din, dout);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out_host, dout, n_out * sizeof(double), hipMemcpyDeviceToHost);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    return e == hipSuccess ? TMPC_OK : TMPC_ERR_HIP;
}
#endif
