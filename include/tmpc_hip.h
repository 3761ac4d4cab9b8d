/*
 * include/tmpc_hip.h -- C-ABI of the MI355X batched SQP/NLP solve path (libtmpc_hip.so).
 *
 * This is the drop-in boundary under tud-amr/mpc_planner's `MPCPlanner::Solver`
 * (mpc_planner_solver/include/mpc_planner_solver/acados_solver_interface.h:93-222).  It replaces the inner
 * acados C ABI the reference's Solver calls (all call sites in
 * mpc_planner_solver/src/acados_solver_interface.cpp) with ONE batch-first interface: B independent
 * trajectories (= B reference `Solver` instances, i.e. the `planners_` loop of
 * mpc_planner_modules/src/guidance_constraints.cpp:279-361) are solved by one kernel launch.
 *
 * Plain C: opaque handle, plain pointers and sizes, int error codes.  No torch / HIP types in signatures
 * (device pointers travel as void*), no CUDA-compat headers.
 *
 * Layouts (identical to the reference's host structs, so `Solver::_params` can be passed as-is):
 *   xinit  [B][nx]            AcadosParameters::xinit            (acados_solver_interface.h:53)
 *   x0     [B][(N+1)*nvar]    AcadosParameters::x0, [u_k; x_k]   (:54)
 *   params [B][N*npar]        AcadosParameters::all_parameters   (:56), row k = stage k, node N reuses row N-1
 *   xtraj  [B][(N+1)*nx]      AcadosOutput::xtraj                (:129)
 *   utraj  [B][N*nu]          AcadosOutput::utraj                (:130)
 * nx = 5, nu = 2, nvar = 7 (ContouringSecondOrderUnicycleModel, solver_generator/solver_model.py:193-214), or
 * nx = 6, nvar = 8 with dims.slack = 1 (ContouringSecondOrderUnicycleModelWithSlack, solver_model.py:274-298: the
 * slack state is the last column).  acados pins that state (x_0 = xinit covers it and slack' = 0), so the solve
 * treats it as the constant xinit[5]: the slack column of x0 is ignored, xtraj returns xinit[5] in it.
 *
 * Error convention: every function returns 0 on success, <0 on error (TMPC_ERR_*); tmpc_last_error()
 * gives the message.  Per-trajectory solver outcomes use the reference's Forces-style exit codes
 * (acados_solver_interface.cpp:197-203, 391-424): 1 success, 0 generic failure, 2 max iter, 3 min step,
 * 4 QP failure; qp_status 0 ok / 2 max iter / 3 min step / 4 NaN.
 */
#ifndef TMPC_HIP_H
#define TMPC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMPC_NU 2
#define TMPC_NX 5
#define TMPC_NV 7

#define TMPC_OK 0
#define TMPC_ERR_INVALID (-1)      /* bad argument / unsupported dimensions */
#define TMPC_ERR_HIP (-2)          /* HIP runtime error (message in tmpc_last_error) */
#define TMPC_ERR_NO_DEVICE (-3)    /* no gfx950 device / kernels missing */

/* Problem dimensions + solver options.  Replaces the compile-time SOLVER_* macros of the generated
 * acados solver and the options of solver_generator/generate_acados_solver.py:143-177. */
typedef struct tmpc_dims {
    int32_t N;            /* horizon (settings.yaml "N"); nodes 0..N */
    int32_t S;            /* contouring/num_segments */
    int32_t n_lin;        /* topology halfspace rows per stage (max_obstacles + add_halfspaces; 0 = no guidance module) */
    int32_t M;            /* ellipsoid rows per stage (max_obstacles, n_discs = 1) */
    int32_t npar;         /* parameters per stage; must equal the reference's count for these modules:
                             8 + slack + 9 S + 3 n_lin + (M ? 2 + 7 M : 0) + (n_slk ? (M ? 0 : 1) + 3 n_slk : 0) */
    int32_t n_sqp;        /* solver_settings/acados/iterations (RTI iterations per solve) */
    int32_t qp_iter_max;  /* qp_solver_iter_max = 50 */
    int32_t erk_steps;    /* sim_method_num_steps = 3 (ERK4) */
    double dt;            /* integrator_step */
    double qp_tol;        /* qp_tol = 1e-5 */
    double reg_eps;       /* MIRROR epsilon (acados default 1e-4) */
    double ipm_mu0;       /* interior-point initial barrier (0.01) */
    double ipm_thr0;      /* interior-point initial slack floor (0.01) */
    double lb[TMPC_NV];   /* model bounds, order [a,w,x,y,psi,v,spline] (solver_model.py:204-205) */
    double ub[TMPC_NV];
    int32_t n_slk;        /* decomp / scenario halfspace rows a1 x + a2 y - (b + slack) <= 0 per stage
                             (decomp_constraints.py:68-98, scenario_constraints.py:64-94); scenario rows first */
    int32_t slack;        /* 1: slack model (nx = 6, nvar = 8; MPCBase weighs the slack state) */
    int32_t cost_model;   /* 0: ContouringModule (MPCC: contouring.py:48-98); 1: CurvatureAwareContouringModule (CA-MPC:
                             curvature_aware_contouring.py:48-105; same parameter map, spline ODE s' = v -- BASELINE configs[2]).  Set by
                             tmpc_default_dims* to 0.  Hand-written kernels only (a generated solver's cost is its module stack's). */
    int32_t row_model;    /* what the M obstacle rows are.  0: EllipsoidConstraintModule (ellipsoid_constraints.py:66-110: 7 parameters per
                             obstacle, h >= 1); 1: GaussianConstraintModule (gaussian_constraints.py:33-113: 6 parameters per obstacle -- x, y,
                             major, minor, risk, r --, h >= 0; the collision-avoidance submodule of mpc_planner_jackal's default T-MPC,
                             generate_jackal_solver.py:53-73).  npar follows: 6 instead of 7 entries per obstacle.  Set by tmpc_default_dims* to 0.
                             Together with cost_model 1 (round 6): the generic kernel, and the four-wave tick kernel for 21 <= N <= 31.
                             Hand-written kernels only. */
    int32_t riccati_form; /* form of the Riccati recursion inside the interior-point QP solver (round 6).  TMPC_RICCATI_SCHUR (0, what
                             tmpc_default_dims* sets): the cost-to-go Hessian P_k is kept as the Schur complement F_xx - Lxu Lxu^T (HPIPM's
                             square_root_alg = 0 [UPSTREAM]) -- every kernel family, every latency mode.  TMPC_RICCATI_SQUARE_ROOT (1): P_k is
                             re-factorised at every stage (P_k = Lxx Lxx^T: HPIPM's square_root_alg = 1 [UPSTREAM], the default of the mode
                             acados configures, solver_generator/generate_acados_solver.py:171) -- the run-time-shape fast kernels only (N <= 32,
                             any row mix of cost_model 0; cost_model 1 at N > 20; no compact / latency variants: tmpc_set_latency_mode answers 1).
                             SUPPORTED qp_tol RANGE: at qp_tol >= 1e-7 the two forms give the same exit codes, iteration counts and iterates to
                             rounding (profiles/round5_riccati_form_study.json: 0 of 6400 solves differ at the reference's 1e-5); below that the
                             interior-point method runs into the conditioning of the barrier systems and 0.4-3.4 % of the solves end differently
                             at 1e-9 -- a comparison with a real acados at such a tolerance (tools/acados_replay.py --qp-tol 1e-9) should run form 1.
                             (The CPU oracle numbers its option the other way round: orc_problem.riccati_form 0 = square-root, 1 = Schur.) */
} tmpc_dims;
#define TMPC_RICCATI_SCHUR 0
#define TMPC_RICCATI_SQUARE_ROOT 1

typedef struct tmpc_handle tmpc_handle;

/* Defaults for the Jackal contouring unicycle (settings.yaml + generate_acados_solver.py). */
void tmpc_default_dims(tmpc_dims *d, int32_t N, int32_t S, int32_t n_lin, int32_t M);
/* Same with decomp / scenario rows and the slack model (configuration_safe_horizon,
 * generate_jackalsimulator_solver.py:67-90; rosnavigation configuration_tmpc, generate_rosnavigation_solver.py:86-108). */
void tmpc_default_dims_ex(tmpc_dims *d, int32_t N, int32_t S, int32_t n_lin, int32_t M, int32_t n_slk, int32_t slack);

/* Replaces Solver_acados_create_capsule + Solver_acados_create_with_discretization
 * (acados_solver_interface.cpp:17,33) for B_max solver instances at once.  Owns device buffers + stream. */
int tmpc_create(tmpc_handle **out, const tmpc_dims *dims, int32_t B_max, int32_t device);
/* Same, for callers that may have been built against another revision of this header: `dims_size` = the caller's sizeof(tmpc_dims).  Fields
 * the caller's struct does not have (it is shorter: cost_model / row_model were appended in round 4, riccati_form in round 6) take their
 * defaults (0) instead of being read from whatever follows the caller's struct.  Accepted sizes are exactly the struct's REVISION BOUNDARIES
 * (the size up to n_slk / slack, up to row_model, the current one): a size that ends inside a field is refused.  A LONGER struct (a newer header
 * than this library) is accepted only if every byte beyond this library's struct is zero -- a non-zero field the library does not know is an
 * option it cannot honour, and is refused (TMPC_ERR_INVALID) instead of being ignored.  New code should call this one:
 * tmpc_create(out, dims, ..) == tmpc_create_v2(out, dims, sizeof(tmpc_dims), ..) of the SAME header revision. */
int tmpc_create_v2(tmpc_handle **out, const tmpc_dims *dims, uint32_t dims_size, int32_t B_max, int32_t device);
/* Replaces Solver_acados_free + Solver_acados_free_capsule (:54,60). */
void tmpc_destroy(tmpc_handle *h);
/* h == NULL: why the calling thread's last tmpc_create* was refused, where the refusal has a message (the model bounds: a NaN, or
 * lb[i] >= ub[i]); "null handle" otherwise. */
const char *tmpc_last_error(const tmpc_handle *h);

/* Replaces, for B solvers: ocp_nlp_constraints_model_set(lbx/ubx = xinit) (:124-125),
 * Solver_acados_update_params (:127-135) and loadWarmstart's ocp_nlp_out_set (:274-284).
 * Host pointers, copied H2D on the handle's stream. */
int tmpc_set_batch(tmpc_handle *h, int32_t B, const double *xinit, const double *x0, const double *params);
/* Same, inputs already resident in HBM (device pointers, same layouts); no copy is made. */
int tmpc_set_batch_device(tmpc_handle *h, int32_t B, const void *d_xinit, const void *d_x0, const void *d_params);

/* Replaces Solver::solve() = initializeOneIteration + n_sqp x solveOneIteration + completeOneIteration
 * (:86-204) for all B trajectories: one kernel launch, asynchronous on the handle's stream. */
int tmpc_solve(tmpc_handle *h);
int tmpc_synchronize(tmpc_handle *h);

/* ---- persistent solver state: the "one iteration at a time" protocol and multipliers carried across ticks ---------------
 * The reference's capsules keep the NLP iterate and its multipliers between calls: Solver::solveOneIteration() = ONE
 * Solver_acados_solve continuing from them (acados_solver_interface.cpp:149-160; driven by SH-MPC's scenario module,
 * scenario_constraints.cpp:85), Solver::operator= copies parameters only (:67-77), loadWarmstart() overwrites the primal iterate
 * only (:274-284), and a solve that does not succeed resets the capsule (:187-191).  tmpc_solve_iterations does n_iter RTI
 * iterations for every trajectory slot of the current batch and then completeOneIteration (so tmpc_get is valid after every
 * call), starting
 *   from the batch's warm start x0 and zero multipliers                      flags = 0            (a fresh capsule)
 *   from the iterate the handle holds for the slot (no loadWarmstart)         TMPC_ITER_KEEP_ITERATE
 *   with the multipliers the handle holds for the slot                        TMPC_ITER_KEEP_MULTIPLIERS
 *   and, as the last call of a solve (completeOneIteration, :162-204)          TMPC_ITER_COMPLETE: slots whose exit code is
 *                                                                             not 1 get zero multipliers (the capsule reset, :187-191)
 * and stores iterate + multipliers of every slot afterwards.  A slot whose QP stopped with qp_status != 0 has left the reference's iteration loop (:105-106): further
 * KEEP_ITERATE calls leave it untouched until a call without KEEP_ITERATE loads a new warm start or a call with TMPC_ITER_NEW_SOLVE starts the next solve.  Slots the handle has no state for yet (a batch larger than any before) start fresh whatever the flags say.  n_iter calls with one
 * iteration each give bitwise the same result as one call with n_iter.  The first call on a handle has nothing to keep and
 * behaves like flags = 0, and so does the first call after tmpc_set_throughput_mode changed the kernel family (the wave kernels keep
 * the state in per-slot arrays, the lane kernels in their workspace).  tmpc_solve() itself never reads or writes this state. */
#define TMPC_ITER_KEEP_ITERATE 1
#define TMPC_ITER_KEEP_MULTIPLIERS 2
#define TMPC_ITER_COMPLETE 4
/* first call of a NEW solve() of the slots' Solvers: a slot's "left the iteration loop" mark (a QP that stopped with qp_status != 0) belongs
 * to the solve that set it -- the reference's loop exit is local to one solve() (:105-106) and every new solve() iterates again from the
 * capsule's state, warm start loaded or not. */
#define TMPC_ITER_NEW_SOLVE 8
int tmpc_solve_iterations(tmpc_handle *h, int32_t n_iter, int32_t flags);
/* State slots.  By default batch entry b uses state slot b.  A caller that owns one slot per Solver (the reference: one capsule
 * per Solver, acados_solver_interface.cpp:17,51-65) but launches a changing subset of them -- GuidanceConstraints::optimize skips
 * disabled planners (guidance_constraints.cpp:286-293) -- passes the slot of every entry of the CURRENT batch: slots[B], distinct,
 * in [0, B_max).  The map stays in force for the following tmpc_solve_iterations calls until it is replaced or cleared
 * (slots = NULL).  A slot nothing was stored in yet starts like a fresh capsule whatever the keep-flags say.  Wave kernels only. */
int tmpc_set_slots(tmpc_handle *h, const int32_t *slots);
/* Parameter-sharing hint for the current batch (optional; results are bitwise the same with and without it).  base_of[b] (host, one
 * entry per batch entry, values in [0, B)): entry b's parameter rows equal entry base_of[b]'s except for its own topology and
 * scenario halfspace rows (LinearizedConstraints / ScenarioConstraints::setParameters) -- which is how a guidance set comes about:
 * every planner's solver starts as a copy of the main solver (guidance_constraints.cpp:300 `*solver = *_solver`) and the shared
 * modules write the same values into each (:312-318).  The kernels then read everything but those rows from entry base_of[b]: a set's
 * 64 copies of the obstacle / spline / weight rows are fetched once instead of 64 times (the parameter rows are 2/3 of the path's
 * algorithmic bytes, and at eight trajectories per CU they no longer fit the L2 next to the solve's workspace).  The CALLER guarantees
 * the equality -- or, equivalently for the kernels that honour the hint, simply does not maintain the copies: a caller that keeps its
 * parameter tensor on the device writes a tick's shared rows ONCE per set, into entry base_of[b] (what bench.py's end-to-end step does), and the
 * other entries' shared columns are never read.  (The lane kernels and generated solvers ignore the hint and read every entry's own rows: such
 * a caller must not use them.)  The map belongs to the batch it was given for: it stays in force until it is replaced, cleared (NULL) or a tmpc_set_batch* call
 * names new inputs (kernels of this library that rewrite a batch's rows in place -- tmpc_linearize_topology, tmpc_scenario_halfspaces --
 * touch the entries' own rows only and keep it valid).  Ignored by the lane kernels
 * (tmpc_set_throughput_mode) and by generated solvers. */
int tmpc_set_param_sharing(tmpc_handle *h, const int32_t *base_of);
/* The "copies are not maintained" mode, made explicit (round-4 advisor): with TMPC_SHARE_COPIES_NOT_MAINTAINED the caller declares that the
 * shared columns of entries b != base_of[b] hold NO valid data.  From then on every path that would read them is an error instead of a silent
 * fallback: tmpc_solve / tmpc_solve_iterations return TMPC_ERR_INVALID while the map is not in force for the current batch (every tmpc_set_batch*
 * drops it: give it again), tmpc_set_throughput_mode (lane kernels) and tmpc_debug_profile (profiled twins) refuse, and generated solvers refuse
 * the flag itself.  Cleared by a NULL map.  flags = 0: tmpc_set_param_sharing (a pure hint, copies equal). */
#define TMPC_SHARE_COPIES_NOT_MAINTAINED 1
int tmpc_set_param_sharing_ex(tmpc_handle *h, const int32_t *base_of, int32_t flags);
/* Copy the persistent state of min(B_max) slots from another handle of the same shape and device (a caller that outgrew its handle). */
int tmpc_copy_state(tmpc_handle *dst, tmpc_handle *src);
/* Forget the persistent state of ONE slot: its next tmpc_solve_iterations starts like a fresh capsule whatever the keep-flags say
 * (a caller that hands the slot of a destroyed Solver to a new one: a new acados capsule, acados_solver_interface.cpp:17-33). */
int tmpc_clear_slot(tmpc_handle *h, int32_t slot);
/* Zero the multipliers of every slot (a new capsule / Solver_acados_reset). */
int tmpc_reset_multipliers(tmpc_handle *h);
/* Kernel variant for the following tmpc_solve calls: 0 (default) = throughput variant, 1 = latency variant (two waves per
 * trajectory; for control ticks of a few planners, like the 8 OpenMP threads of guidance_constraints.cpp:279), 2 = latency
 * variant with the interior-point Newton systems solved parallel in time (multiplier Schur complement + block cyclic reduction
 * over the stages, csrc/tmpc_scan.hpp) instead of by the stage-by-stage Riccati recursion that acados / HPIPM -- and modes 0, 1 --
 * use: 30-40 % less kernel time per tick; available for horizons N <= 31 of the hand-written model, at one workgroup per CU (a launch of
 * more than 256 trajectories per GPU takes several rounds: the default kernels are the better choice there).  Returns 0, or 1 if the handle's shape has no such variant (mode 2 then runs as mode 1,
 * mode 1 as the default kernel).  A trajectory's result is bitwise independent of the batch it is solved in.  Modes 0 and 1 agree
 * to rounding (1e-11), not bitwise.  Mode 2 is another factorisation of the same systems: its steps agree with the recursion's to
 * ~1e-6 on ill-conditioned late iterations (each is that far from an exact solve), trajectories agree within the 1e-4 parity
 * tolerance, and the interior-point iteration count of a solve can differ by one where a residual sits at the tolerance.
 * 3 (round 6) = FOUR waves per trajectory, for the launches that leave a whole CU to each trajectory (<= one workgroup per CU: the
 * reference's deployed 4 + 1 planners, a 64-trajectory tick): the algorithm of mode 2 with the stage evaluation split four ways by content,
 * the row passes at twelve (N <= 20) or eight (21 <= N <= 31: the horizon the reference ships, N = 30) lanes per stage and the wide phases of
 * the factorisation on all 256 lanes -- 10-15 % less kernel time per tick than mode 2 (measured ticks: DESIGN.md section 5), results equal to
 * mode 2's to rounding; N <= 20: MPCC or Gaussian rows; 21 <= N <= 31: every stage model, up to 34 rows per stage.  A shape without it runs
 * mode 2 (return value 1).  tmpc_latency_mode_capacity says how many trajectories a variant serves well in one launch.
 * GENERATED solver libraries (mpc_planner_amd/codegen, build_generated_solver(..., tick_kernels=True)) carry mode 3, for 2 <= N <= 31 and a
 * stack with at least one row and at most 34: the run-time-shape instantiations of the same four-wave kernels around the emitted stage
 * functions, the stage evaluation split over the waves by content (dynamics | emitted cost | the rows on two waves): 10-14 % less kernel time
 * than the library's default kernel on 5- and 64-trajectory ticks.  Modes 1 and 2 have no generated variant (return
 * value 1, the default kernel runs): mode 2's two-wave kernels around emitted stage functions measured slower than the default kernel.  A
 * tick kernel that the compiler could only build with scratch for a stack is not offered either: <name>_meta.json "tick_kernels" lists each
 * one's registers and scratch. */
int tmpc_set_latency_mode(tmpc_handle *h, int32_t on);
/* How many trajectories ONE launch of kernel variant `mode` (0 .. 3 as above) holds resident on this device (workgroups per CU x CUs; variant 3: ONE workgroup per CU, what it is built for), 0 if the
 * handle's shape has no such variant, < 0 on error.  A latency variant pays off while the launch fits (one dependent chain deep); above it the
 * throughput kernels win.  The library never switches variants by batch size (results would depend on the rest of the batch): the CALLER decides,
 * e.g. the C++ BatchContext (cpp/src/solver_interface.cpp) asks for the tick variant only for batches within this capacity. */
int tmpc_latency_mode_capacity(tmpc_handle *h, int32_t mode);
/* Throughput variant for large batches (many control ticks / scenario solvers per launch): one LANE per trajectory instead of
 * one wavefront -- every lane runs the scalar SQP_RTI program on its own trajectory, the per-trajectory state is streamed from a
 * lane-major HBM workspace (allocated for B_max trajectories on the first call: about 8 (N+1) (175 + 6 nh) + 8 N npar bytes
 * each), and the reference-layout inputs are transposed into it at the start of every tmpc_solve.  Same algorithm and stopping
 * rules as the default kernels: exit codes and iteration counts agree, trajectories agree to rounding (1e-10), and a
 * trajectory's result does not depend on the rest of the batch.  The default (0) stays the choice for control ticks of a few
 * planners; the mode is chosen by the caller, never by the batch size.  Returns 0, or <0 if the workspace cannot be allocated or if
 * this build of the lane kernel spills registers to scratch (possible in generated solvers: refused, tmpc_last_error says so). */
int tmpc_set_throughput_mode(tmpc_handle *h, int32_t on);
/* 1 if this build of the library contains the lane-per-trajectory kernels, 0 if not (the default build since round 5: the family is optional,
 * -DTMPC_WITH_LANES; tmpc_set_throughput_mode(h, 1) then fails with a message that says so). */
int tmpc_has_lane_kernels(void);

/* Replaces ocp_nlp_out_get / ocp_nlp_get / ocp_nlp_eval_cost of completeOneIteration (:162-204).
 * Any pointer may be NULL.  Synchronises the stream.  Host pointers. */
int tmpc_get(tmpc_handle *h, double *xtraj, double *utraj, double *pobj, int32_t *exit_code,
             int32_t *qp_status, int32_t *sqp_iter, double *res_eq, int32_t *qp_iter_total);

/* Replaces FindBestPlanner (guidance_constraints.cpp:416-434) on device for ONE planner set = the contiguous trajectories
 * [first, first+count) of the batch (one scene's local planners): argmin of pobj*weight among exit_code == 1 && !disabled; init 1e10,
 * strict '<' (lowest index wins ties).  Index convention: everything is RELATIVE TO `first`, like an index into the reference's
 * planners_ vector -- weight[i] / disabled[i] (host pointers, `count` entries, or NULL) belong to trajectory first + i, and *best
 * is in [0, count) (the batch index is first + *best), or -1 if none. */
int tmpc_select_best(tmpc_handle *h, int32_t first, int32_t count, const double *weight,
                     const uint8_t *disabled, int32_t *best);

/* Device-resident result records for the multi-GPU all-gather: pointers to the handle's
 * pobj[B] (f64) and exit_code[B] (i32) device arrays. */
int tmpc_result_device_ptrs(tmpc_handle *h, void **d_pobj, void **d_exit_code);
/* The HIP stream (hipStream_t) every launch of this handle is enqueued on, for callers that order their own work against it
 * without host synchronisation -- e.g. the multi-GPU step runs the record all-gather stream-ordered between tmpc_pack_records and
 * tmpc_select_best_records by making that stream the collective's current stream. */
int tmpc_get_stream(tmpc_handle *h, void **stream);
/* Which solve kernel this handle dispatches and how it is launched, as a short text for logs and benchmark records (kernel family,
 * trajectories per workgroup, LDS bytes per workgroup, resident workgroups of a persistent launch), ending in the template instantiation of
 * every kernel slot the handle fills: "; kernels: default=<name>[, small=<name>][, cp2=<name>][, lat1=<name>][, lat2=<name>][, lat3=<name>]"
 * with <name> "fast<NLIN,MM,LPS,NTH,TEAM,CM>", "compact<NLIN,MM,LPS,NTH,CM>" or "generic<CM>" (small: the fast kernel of a compact shape for
 * launches it holds resident; cp2: the two-wave compact kernel for larger launches; latN: tmpc_set_latency_mode(h, N)).  Returns the length written. */
int tmpc_kernel_info(const tmpc_handle *h, char *buf, int32_t capacity);

/* ---- multi-GPU sharding: a scene's trajectories are split over ranks; after the solve every rank
 * packs one 16-byte record per local trajectory, the host all-gathers the record arrays (RCCL over xGMI via
 * torch.distributed) and every rank runs the same deterministic selection over the gathered array. -------- */
typedef struct tmpc_record {
    double objective;     /* _info.pobj (x consistency weight if supplied) */
    int32_t exit_code;    /* SolverResult::exit_code (guidance_constraints.h:32-50) */
    int32_t guidance_id;  /* SolverResult::guidance_ID */
} tmpc_record;

/* Pack records of the handle's B trajectories into d_records[B] (device pointer, caller-owned).
 * d_guidance_id: device int32[B] or NULL (then the local trajectory index); d_weight: device f64[B] or NULL. */
int tmpc_pack_records(tmpc_handle *h, void *d_records, const void *d_guidance_id, const void *d_weight);

/* FindBestPlanner over gathered records laid out [n_ranks][n_scenes][per_rank] (device pointer): for each scene
 * the winner is the lowest GLOBAL index (rank*per_rank + t) among exit_code == 1 with the smallest objective
 * (init 1e10, strict '<').  d_best: device int32[n_scenes], -1 if none.  Runs on the handle's stream. */
int tmpc_select_best_records(tmpc_handle *h, const void *d_records, int32_t n_ranks, int32_t n_scenes,
                             int32_t per_rank, void *d_best);

/* The winners' trajectories in one compact buffer -- what GuidanceConstraints::optimize copies from the best planner into the main solver
 * (`_solver->_output = best_solver->_output`, guidance_constraints.cpp:382-384), for every set of the launch at once, so that ONE small
 * device-to-host copy brings a tick's (or many ticks') results back.  d_best: i32 [n_sets] as written by tmpc_select_best_records (index
 * inside the set, -1: no successful trajectory).  The batch holds the entries [index_offset, index_offset + set_size) of every set (one
 * rank's share; index_offset = rank * per_rank, 0 on one GPU): a winner outside that range is another rank's and its rows are left untouched,
 * a set without a winner gets NaNs.  d_xtraj f64 [n_sets][(N + 1) nx], d_utraj f64 [n_sets][N nu] (device).  Runs on the handle's stream. */
int tmpc_gather_best(tmpc_handle *h, const void *d_best, int32_t n_sets, int32_t set_size, int32_t index_offset, void *d_xtraj, void *d_utraj);

/* Per-launch timing: when enabled, every tmpc_solve is bracketed by HIP events recorded on the handle's stream.
 * tmpc_get_timings synchronises and returns the durations [ms] of the launches since enable/last read. */
int tmpc_enable_timing(tmpc_handle *h, int32_t max_records);
int tmpc_get_timings(tmpc_handle *h, float *ms, int32_t capacity, int32_t *n_out);

/* Timing helper: runs tmpc_solve `reps` times back-to-back on the handle's stream, each bracketed by HIP
 * events recorded on THAT stream, and returns the per-launch kernel durations in milliseconds. */
int tmpc_time_solve(tmpc_handle *h, int32_t reps, float *ms_each);

/* ---- next row f-1: LinearizedConstraints::update + setParameters on device -----------------------------------
 * For every trajectory b of the current batch, stage k = 1..N-1 and obstacle j < n_lin: project the guess position
 * x0[b][k].(x,y) out of the discs of radius (1e-3 + robot_radius) around the obstacle predictions (<= 3 sweeps,
 * LinearizedConstraints::projectToSafety, linearized_constraints.cpp:130-148 -- the Douglas-Rachford operator of
 * ros_tools is not in the reference tree; restated from the published operator, DESIGN.md U10 -- the identity for collision-free guesses), then
 * a = (o - p)/|o - p|, b = a.o - (1e-3 + robot_radius) (:84-105, guidance mode) and write lin_constraint_j_{a1,a2,b}
 * into params[b][k]; stage 0 and the rows of non-guided planners get the dummies (1, 0, state_x + 100) (:155-166,
 * guidance_constraints.cpp:301-305).  The batch's params buffer is modified IN PLACE (device memory).
 * ALL n_lin topology rows are treated as dynamic obstacles (d_obstacle_pos has n_lin entries per scene); tmpc_linearize_topology_ex
 * below covers fewer obstacles than rows, static halfspace rows and the disc mode.
 *   d_obstacle_pos : f64 [n_scenes][n_lin][N][2]   prediction step i of obstacle j (stage k uses step k-1)
 *   d_scene_of     : i32 [B]                       scene of trajectory b
 *   d_state_x      : f64 [n_scenes]                current state x (for the dummy b)
 *   d_is_original  : u8  [B] or NULL               1 = non-guided T-MPC++ planner (all rows dummy) */
int tmpc_linearize_topology(tmpc_handle *h, const void *d_obstacle_pos, const void *d_scene_of, const void *d_state_x,
                            double robot_radius, const void *d_is_original);
/* The whole of LinearizedConstraints::update / setParameters (linearized_constraints.cpp:49-189):
 *   rows 0 .. n_obstacles-1          dynamic obstacles, d_obstacle_pos f64 [n_scenes][n_obstacles][N][2]
 *   rows n_obstacles .. +n_static-1  static halfspaces of the stage, copied as given (`linearized_constraints/add_halfspaces`, :107-123):
 *                                    d_static_halfspaces f64 [n_scenes][N][n_static][3] = (a1, a2, b) for stage k (k = 0 unused)
 *   remaining rows up to n_lin       dummies (1, 0, state_x + 100) (:181-187); n_obstacles + n_static <= n_lin
 * d_obstacle_radius == NULL: guidance mode, every obstacle disc has radius 1e-3 + robot_radius (:99, :140).  Otherwise the
 * `_use_guidance == false` branch (:63-73): f64 [n_scenes][n_obstacles], obstacle j's own radius + robot_radius in the projection and
 * in b.  One disc at the robot's centre (n_discs = 1, offset 0: the Jackal configurations); rows of further discs are not generated.
 * A non-guided planner (d_is_original) is updated with empty data in the reference (guidance_constraints.cpp:301-305): zero obstacles, so its
 * static halfspaces are its rows 0 .. n_static-1 (:113-124, :173-179) and every row behind them is a dummy. */
int tmpc_linearize_topology_ex(tmpc_handle *h, const void *d_obstacle_pos, int32_t n_obstacles, const void *d_obstacle_radius,
                               const void *d_static_halfspaces, int32_t n_static, const void *d_scene_of, const void *d_state_x,
                               double robot_radius, const void *d_is_original);

/* ---- rows a5 / f-1: Contouring's road constraints on device (`contouring/add_road_constraints`; Contouring::constructRoadConstraints,
 * mpc_planner_modules/src/contouring.cpp:181-262).  For every scene q < n_scenes and stage k = 1..N-1 (stage 0 gets nothing) two halfspaces
 * a.p <= b that keep the robot between the road's edges, built at s_k = the spline state of the warm start of batch entry d_main_of[q] -- the
 * entry of the CURRENT batch that stands for the scene's main solver (`_solver->getEgoPrediction(k, "spline")`, :208, :250): its warm start in
 * the handle's x0 buffer (after tmpc_set_batch* or tmpc_warmstart; both models' strides), the path window (spline_x{i}_{a..d}, spline_y{i}_{a..d},
 * spline{i}_start) of its parameter row of stage k.  With P(s) the point and A(s) the unit normal of a spline at s:
 *   d_bound_segments == NULL, centreline mode (:191-235):  row 0 (A, A.(P + A offset_first)),  row 1 (-A, -A.(P - A offset_second))  of the path;
 *       offset_first = times * road/width / 2 - r (times = road/two_way ? 3 : 1), offset_second = road/width / 2 - r, r = robot_area[0].radius
 *   otherwise, bounds mode (:237-262):  row 0 (-A_l, -A_l.(P_l + A_l offset_first)),  row 1 (A_r, A_r.(P_r - A_r offset_second))  of the left /
 *       right bound spline at the same s_k, offset_first = offset_second = r;  d_bound_segments f64 [n_scenes][2][S][8] = (left, right) x segment x
 *       (ax bx cx dx ay by cy dy) on the centreline's knots (the bound splines are built on its knot vector, :142-149).
 * RosTools::Spline2D is not in the reference tree.  ASSUMED: (1) getOrthogonal(s) = (y'(s), -x'(s)) / |.|, the normal to the RIGHT
 * of travel -- the only sign for which bounds mode is a corridor between the two bounds; in centreline mode it puts the `times = 3` side on the
 * right; (2) P, x', y' are the plain piecewise cubics (no sigmoid glue: that belongs to the NLP) of segment i = max{j : start_j <= s}, i = 0 below
 * the first knot, and the last segment's cubic continues beyond the window.
 * Writes rows first_row and first_row + 1 of d_static_halfspaces f64 [n_scenes][N][n_static][3] -- the buffer tmpc_linearize_topology_ex reads --
 * for k >= 1 and touches nothing else (other rows, stage 0).  Stream-ordered on the handle's stream: no synchronisation, no allocation, so a
 * closed loop tmpc_warmstart -> tmpc_road_halfspaces -> tmpc_init_with_guidance -> tmpc_linearize_topology_ex -> tmpc_solve has no host round
 * trip.  Equal bit for bit to mpc_planner_amd.modules.road_halfspaces / road_halfspaces_from_bounds (no FMA contraction, same operation order).
 * d_main_of i32 [n_scenes] (device); an entry outside [0, B) leaves its scene's rows untouched.  TMPC_ERR_INVALID: no batch, NULL d_main_of /
 * d_static_halfspaces, n_scenes <= 0, first_row < 0, n_static < first_row + 2, S = 0, a generated solver. */
int tmpc_road_halfspaces(tmpc_handle *h, const void *d_main_of, int32_t n_scenes, const void *d_bound_segments, double offset_first,
                         double offset_second, void *d_static_halfspaces, int32_t n_static, int32_t first_row);

/* ---- obstacle preparation on device: what a wrapper's obstacle callback does before Planner::solveMPC (mpc_planner/src/data_preparation.cpp;
 * mpc_planner_jackal/src/ros1_jackal.cpp:313-332, mpc_planner_jackalsimulator/src/ros1_jackalsimulator.cpp:298-347).  For every scene q < n_scenes
 * the raw obstacle list becomes exactly max_obstacles prepared obstacles, in the layout tmpc_linearize_topology_ex and
 * tmpc_set_obstacle_parameters read.  Uses N, dt and the stream of the handle only: no batch is needed.  Stream-ordered, no allocation, no
 * synchronisation.  Inputs (device):
 *   d_count      i32 [n_scenes]                 raw obstacles of the scene, clipped to [0, n_slots]
 *   d_state      f64 [n_scenes][4]              (x, y, psi, v)
 *   d_raw_pos    f64 [n_scenes][n_slots][2]     current positions;  d_raw_radius f64 [n_scenes][n_slots]
 *   d_raw_vel    f64 [n_scenes][n_slots][2]     or NULL: constant-velocity mode -- prediction step i = pos + (vel dt) i, i < N, angle 0,
 *                                               major = minor = (probabilistic ? noise : 0), GAUSSIAN iff probabilistic
 *                                               (getConstantVelocityPrediction, data_preparation.cpp:58-79)
 *   d_raw_pred   f64 [n_scenes][n_slots][N][5]  or NULL: given predictions (x, y, angle, major, minor), taken as they are; GAUSSIAN iff
 *                                               probabilistic and the last step's major != 0 (ros1_jackalsimulator.cpp:331-334)
 * exactly one of d_raw_vel / d_raw_pred; n_slots <= 1024.  Then, restated from the cited lines:
 *   distance filter  max_obstacle_distance > 0: an obstacle whose CURRENT position is not closer to the robot than it is dropped
 *                    (removeDistantObstacles, :81-93; no wrapper the reference ships calls it: off by default)
 *   closest M        more than max_obstacles left: the max_obstacles with the smallest min_k ((k + 1) 0.6) |pred_k - (p + (v k)(cos psi, sin psi))|,
 *                    k < N, from min_dist = 1e5, in ascending order of it (ensureObstacleSize, :104-150; `v k` has no dt in the reference: kept).
 *                    std::sort leaves ties unspecified: here the lower raw index wins.  The device's cos / sin may differ from
 *                    libm's in the last bits; they enter this ranking only, never an output value.
 *   or fewer         the obstacles in raw order, then dummies at (x + 100, y + 100), radius 0, zero velocity, with the constant-velocity
 *                    prediction in either input mode (getDummyObstacle :49-56, :151-165)
 *   propagation      propagatePredictionUncertainty (:170-186) `propagate_passes` times over GAUSSIAN predictions, dummies included:
 *                    major_k = sqrt(major_{k-1}^2 + (sigma_k dt)^2) sequentially over k, the same for minor.  TWO passes is what ros1_jackal.cpp:324-332
 *                    really does in probabilistic mode (one inside getConstantVelocityPrediction, one in the wrapper); ONE is the simulator wrapper
 *                    with probabilistic/propagate_uncertainty (ros1_jackalsimulator.cpp:345-346).
 * Outputs (device, caller-owned, every entry written):
 *   d_obstacle_pos      f64 [n_scenes][max_obstacles][N][2]
 *   d_obstacle_shape    f64 [n_scenes][max_obstacles][N][3]   (angle, major, minor)
 *   d_obstacle_radius   f64 [n_scenes][max_obstacles]
 *   d_obstacle_gaussian u8  [n_scenes][max_obstacles]         1 = PredictionType::GAUSSIAN
 *   d_selected          i32 [n_scenes][max_obstacles]         raw slot, -1 = dummy
 * Equal bit for bit to mpc_planner_amd.modules.prepare_obstacles (no FMA contraction, same operation order).  options == NULL: the defaults below.
 * TMPC_ERR_INVALID: a NULL required pointer, both or neither of d_raw_vel / d_raw_pred, n_scenes <= 0, n_slots outside [0, 1024], max_obstacles
 * outside [1, 4096], propagate_passes outside 0..2, probabilistic outside 0 / 1, noise < 0, an options->size this library cannot honour (shorter
 * than its struct, or longer with a non-zero tail, like tmpc_create_v2), a generated solver. */
typedef struct tmpc_obstacle_options {
    uint32_t size;                 /* sizeof(tmpc_obstacle_options) of the caller's header */
    int32_t probabilistic;         /* probabilistic/enable: 0 (default) / 1 */
    int32_t propagate_passes;      /* 0 (default), 1 or 2 */
    int32_t reserved;              /* 0 */
    double noise;                  /* the reference's 0.3 (data_preparation.cpp:65); used in probabilistic mode only */
    double max_obstacle_distance;  /* <= 0 (default): no distance filter */
} tmpc_obstacle_options;
int tmpc_prepare_obstacles(tmpc_handle *h, int32_t n_scenes, int32_t n_slots, int32_t max_obstacles, const void *d_count, const void *d_state,
                           const void *d_raw_pos, const void *d_raw_radius, const void *d_raw_vel, const void *d_raw_pred,
                           const tmpc_obstacle_options *options, void *d_obstacle_pos, void *d_obstacle_shape, void *d_obstacle_radius,
                           void *d_obstacle_gaussian, void *d_selected);
/* The collision columns of the CURRENT batch's parameter rows, in place, from those four buffers (max_obstacles = dims.M obstacles per scene):
 * d_scene_of i32 [B], d_state f64 [n_scenes][4].  One thread per (trajectory, stage, obstacle); both models' parameter strides.
 *   row_model 0  EllipsoidConstraints::update + setParameters (ellipsoid_constraints.cpp:24-90): stage 0 the dummies (x + 50, y + 50, 0, 0, 0, 1, 0.1)
 *                in the column order x, y, psi, major, minor, chi, r; stage k >= 1 prediction step k - 1 and the obstacle's own radius; a
 *                DETERMINISTIC obstacle gets major = minor = 0, chi = 1 whatever the shape buffer holds (:72-77), a GAUSSIAN one its radii and
 *                `chi` = ExponentialQuantile(0.5, 1 - risk) = -log(risk) / 0.5, evaluated by the CALLER (no device logarithm enters)
 *   row_model 1  GaussianConstraints (gaussian_constraints.cpp:22-79) as mpc_planner_amd.modules.gaussian_set_parameters has it: stage 0
 *                (x + 100, y + 100, 0.1, 0.1, 0.05, 0.1), then x, y, major, minor (0 for a DETERMINISTIC obstacle), `risk`, and in the r column
 *                `obstacle_radius`, the CONFIGURED radius (CONFIG["obstacle_radius"], :74), not the prepared obstacle's own
 * and ego_disc_radius = robot_radius, ego_disc_0_offset = disc_offset at every stage.  No other column is touched.  Stream-ordered, no allocation,
 * no synchronisation.  TMPC_ERR_INVALID: no batch, a problem without obstacle rows (M = 0), a NULL pointer, a generated solver. */
int tmpc_set_obstacle_parameters(tmpc_handle *h, const void *d_obstacle_pos, const void *d_obstacle_shape, const void *d_obstacle_radius,
                                 const void *d_obstacle_gaussian, const void *d_scene_of, const void *d_state, double robot_radius,
                                 double disc_offset, double risk, double chi, double obstacle_radius);

/* ---- the reference path on device: what Contouring::update does every tick (mpc_planner_modules/src/contouring.cpp:28-48) and the segment
 * window setSplineParameters writes (:94-124).  RosTools::Spline2D::findClosestPoint is not in the reference tree: the search is restated, its
 * assumptions are DESIGN.md U14.  tmpc_track_path uses S and the stream of the handle only: no batch is needed.  Stream-ordered, no allocation,
 * no synchronisation.  Inputs (device):
 *   d_path         f64 [n_scenes][n_seg_max][9]     cubic segments (ax bx cx dx ay by cy dy start), the 9-tuple of the parameter rows
 *   d_path_count   i32 [n_scenes]                   segments of the scene's path, clipped to [0, n_seg_max];  n_seg_max <= 1024
 *   d_path_length  f64 [n_scenes]                   the knot behind the last segment: L_i = start_{i+1} - start_i, L_last = length - start_last
 *   d_bounds       f64 [n_scenes][2][n_seg_max][8]  or NULL: left / right bound cubics on the same knots (with d_bound_window, both or neither)
 *   d_pos          f64 [n_scenes][pos_stride]       x and y first, pos_stride >= 2: the 4-wide state of tmpc_prepare_obstacles or the 5- / 6-wide
 *                                                   state of tmpc_warmstart can be passed as they are
 * In / out:
 *   d_segment      i32 [n_scenes]                   the previous closest segment; < 0 requests the global search (a new path, a reset)
 * Closest point on segment i to p, D(t) = |P_i(t) - p|^2, g(t) = (P_i(t) - p).P_i'(t), Horner forms: coarse samples t_j = L_i (j / 8), j = 0..8;
 * j* = argmin D(t_j), the lowest j on ties; bracket lo = t_max(j*-1,0), hi = t_min(j*+1,8); g(lo) >= 0: t = lo; else g(hi) <= 0: t = hi; else
 * exactly 40 bisections (mid = (lo + hi) / 2, g(mid) > 0 ? hi = mid : lo = mid) and t = (lo + hi) / 2; the coarse sample wins if D(t_j*) < D(t).
 * Candidates (U14-1): every segment after a reset, else [max(0, prev - R), min(count - 1, prev + R)] with prev clamped into [0, count - 1]
 * and R = search_range.  The smallest D wins, the lowest segment on ties; the comparison starts from the first candidate and replaces on
 * strict `<`, so a NaN / inf position yields the first candidate, never an index out of range.
 * Outputs (device, caller-owned; every entry of a scene with count > 0 is written, a scene with count <= 0 writes nothing and keeps its segment):
 *   d_segment      the segment found
 *   d_closest_s    f64 [n_scenes]                   start_segment + t
 *   d_window       f64 [n_scenes][S][9]             slot w = segment + w as given (U14-2); beyond the last segment the path continues STRAIGHT
 *                                                   ALONG ITS END TANGENT (U14-3): (0, 0, x'(end), X(end), 0, 0, y'(end), Y(end)), start = length,
 *                                                   from the last cubic at t = L_last
 *   d_bound_window f64 [n_scenes][2][S][8]          or NULL: the bound cubics of the same slots, padded the same way from their own last cubics;
 *                                                   exactly what tmpc_road_halfspaces takes as d_bound_segments
 *   d_reached      u8  [n_scenes]                   or NULL: 1 iff |p - P(length)| < 1.0 (Contouring::isObjectiveReached, :167-175)
 * Equal bit for bit to mpc_planner_amd.modules.track_path (no FMA contraction, same operation order).  One wave per scene, one lane per
 * candidate segment (strided beyond 64 candidates), a 64-lane argmin on (D, segment).  options == NULL: the defaults below.
 * TMPC_ERR_INVALID: a NULL required pointer, one of d_bounds / d_bound_window without the other, n_scenes <= 0, n_seg_max outside [1, 1024],
 * search_range outside [0, 31], pos_stride < 2, an options->size this library cannot honour (like tmpc_obstacle_options; the 8-byte first
 * revision, without window_segments, is still taken), a problem without path segments (S = 0), window_segments outside [0, 64] or, in a
 * hand-written build, neither 0 nor the handle's S; a generated solver called without window_segments.
 * IN A GENERATED SOLVER the handle has no S: the caller supplies it as options->window_segments in [1, 64] (the stack's
 * contouring/num_segments), and the call then does exactly the above; with 0 or options == NULL it refuses. */
typedef struct tmpc_path_options {
    uint32_t size;                 /* sizeof(tmpc_path_options) of the caller's header */
    int32_t search_range;          /* R: segments either side of the previous one that are searched; default 2, 0 .. 31 */
    int32_t window_segments;       /* S of d_window / d_bound_window; default 0: the handle's S.  Since the second revision of this struct */
} tmpc_path_options;
int tmpc_track_path(tmpc_handle *h, int32_t n_scenes, int32_t n_seg_max, const void *d_path, const void *d_path_count, const void *d_path_length,
                    const void *d_bounds, const void *d_pos, int32_t pos_stride, const tmpc_path_options *options, void *d_segment,
                    void *d_closest_s, void *d_window, void *d_bound_window, void *d_reached);
/* The spline columns of the CURRENT batch's parameter rows, in place, from d_window [n_scenes][S][9] as tmpc_track_path wrote it: the 9 S
 * columns spline_x{i}_{a..d}, spline_y{i}_{a..d}, spline{i}_start of every stage k < N of every entry b with d_scene_of[b] (i32 [B]) inside
 * [0, n_scenes), and nothing else; an entry whose scene is outside that range is left untouched, so a caller with
 * TMPC_SHARE_COPIES_NOT_MAINTAINED can name the lead entries only.  A parameter-sharing map stays valid when every entry of a set names the
 * same scene: equal values go to all of them.  Both models' parameter strides.
 * Optional d_closest_s (f64 [n_scenes]) with d_state (f64 [B][nx], the layout tmpc_warmstart reads; both or neither): the `spline` entry
 * (index 4) of each named entry becomes its scene's closest_s -- state.set("spline", closest_s), contouring.cpp:42.
 * ORDER.  In the reference setXinit(state) and initializeWarmstart(state) run BEFORE the modules' update (planner.cpp:81-96): the `spline`
 * of xinit is the PREVIOUS tick's closest_s.  Call tmpc_warmstart(d_state) before tmpc_set_path_parameters(..., d_state) to reproduce that;
 * call it after to start the solve from the fresh value.
 * Stream-ordered, no allocation, no synchronisation.  TMPC_ERR_INVALID: no batch, a NULL d_window / d_scene_of, n_scenes <= 0, one of
 * d_closest_s / d_state without the other, a problem without path segments, a generated solver. */
int tmpc_set_path_parameters(tmpc_handle *h, const void *d_window, const void *d_scene_of, int32_t n_scenes, const void *d_closest_s,
                             void *d_state);

/* ---- the velocity profile along the reference path: what PathReferenceVelocity::setParameters (mpc_planner_modules/src/
 * path_reference_velocity.cpp:59-95) writes into the spline_v{i}_{a..d} columns every tick, and the value GuidanceConstraints::update hands to
 * the guidance planner, path_velocity(state.spline) (guidance_constraints.cpp:91-94).  tk::spline::operator() is not in the reference tree: the
 * evaluation is restated, DESIGN.md U17.  Needs no batch, uses the stream of the handle only, S is an argument (1 <= S <= 64): also available in
 * a generated solver.  Stream-ordered, no allocation, no synchronisation.  Inputs (device):
 *   d_velocity     f64 [n_scenes][n_seg_max][4]   (a b c d) of v(s) per segment as tmpc_fit_path writes it, or NULL: no scene has a profile
 *   d_path         f64 [n_scenes][n_seg_max][9]   the paths (only the `start` column is read);  1 <= n_seg_max <= 1024
 *   d_path_count   i32 [n_scenes]                 segments of the scene's path, clipped to [0, n_seg_max]
 *   d_path_length  f64 [n_scenes]                 the last knot; part of a path's triple and required, but not read: beyond it v continues the
 *                                                 last cubic (U17)
 *   d_segment      i32 [n_scenes]                 the closest segment as tmpc_track_path wrote it; clamped into [0, count - 1] before use, so that
 *                                                 -1 or a stale value never indexes out of range
 *   d_closest_s    f64 [n_scenes]                 as tmpc_track_path wrote it
 *   d_has_velocity u8  [n_scenes]                 or NULL: every scene has a profile if d_velocity is given (reference_path.hasVelocity())
 *   reference_velocity                            CONFIG["weights"]["reference_velocity"]
 * A scene is WITHOUT A PROFILE if d_velocity is NULL, its flag is 0 or its count <= 0.  Outputs (device, caller-owned, every entry written):
 *   d_window       f64 [n_scenes][S][4]           slot w = velocity segment `segment + w`; a slot at or beyond count is (0, 0, 0, 0) -- "brake at
 *                                                 the end" (:71-78); without a profile every slot is (0, 0, 0, reference_velocity) (:86-95)
 *   d_v_ref        f64 [n_scenes]                 or NULL: with a profile v(s) at s = closest_s -- the cubic of segment i = max{j <= count - 1 :
 *                                                 start_j <= s}, 0 if there is none, at t = s - start_i, ((a t + b) t + c) t + d in Horner form;
 *                                                 without a profile reference_velocity
 * Equal bit for bit to mpc_planner_amd.modules.path_velocity_window (called with a segment inside the path) and path_velocity_at (no FMA
 * contraction).  One wave per scene; the lookup is a ballot over strided start_j <= s tests.
 * TMPC_ERR_INVALID, before any launch: a NULL required pointer (d_path, d_path_count, d_path_length, d_segment, d_closest_s, d_window),
 * n_scenes <= 0, n_seg_max outside [1, 1024], S outside [1, 64]. */
int tmpc_path_velocity_window(tmpc_handle *h, int32_t n_scenes, int32_t n_seg_max, int32_t S, const void *d_velocity, const void *d_path,
                              const void *d_path_count, const void *d_path_length, const void *d_segment, const void *d_closest_s,
                              const void *d_has_velocity, double reference_velocity, void *d_window, void *d_v_ref);

/* ---- caller-chosen columns of the CURRENT batch's parameter rows, in place: the parameter writer of generated solvers, whose row layout is
 * the module stack's and whose column numbers the caller has in the stack's parameter map (<name>_meta.json "parameter_map"); available in
 * every build.  Nothing but the named columns is touched.
 *   cols           i32 [n_cols], HOST             1 <= n_cols <= 128, every entry in [0, npar), all distinct (a duplicate would make the value
 *                                                 written depend on thread order: refused); copied before the call returns
 *   d_values       f64 [n_scenes][n_cols]         per_stage 0: row of scene d_scene_of[b] into every stage k < N of entry b
 *                  f64 [n_scenes][N][n_cols]      per_stage 1: stage k from row k -- for rows produced per stage, such as those
 *                                                 tmpc_decomp_halfspaces and tmpc_road_halfspaces leave in caller buffers
 *   d_scene_of     i32 [B]                        an entry whose scene is outside [0, n_scenes) is left untouched
 * With cols = the spline columns and d_values = tmpc_track_path's d_window it writes what tmpc_set_path_parameters writes; with the
 * spline_v{i}_{a..d} columns and tmpc_path_velocity_window's d_window, PathReferenceVelocity::setParameters.  Parameter sharing as for
 * tmpc_set_path_parameters: a map stays valid when every entry of a set names the same scene, and a caller with
 * TMPC_SHARE_COPIES_NOT_MAINTAINED can name the lead entries only.  One thread per (entry, stage, column); both models' strides.
 * Stream-ordered, no allocation, no synchronisation.
 * TMPC_ERR_INVALID, before any launch: no batch, a NULL cols / d_values / d_scene_of, n_scenes <= 0, n_cols outside [1, 128], a column outside
 * [0, npar), a duplicate column, per_stage neither 0 nor 1. */
int tmpc_scatter_parameters(tmpc_handle *h, const int32_t *cols, int32_t n_cols, const void *d_values, int32_t per_stage, const void *d_scene_of,
                            int32_t n_scenes);

/* ---- reference paths fitted on device: waypoints -> the cubic segments tmpc_track_path reads.  What Contouring::onDataReceived
 * (mpc_planner_modules/src/contouring.cpp:126-157) and PathReferenceVelocity::onDataReceived (path_reference_velocity.cpp:28-40) do when a
 * path arrives: the centreline through the waypoints, the two bound curves and the velocity profile on the CENTRELINE's knots, road/width
 * from the bounds' first waypoints.  RosTools::Spline2D and tk::spline are not in the reference tree: the natural cubic spline (second
 * derivative zero at both ends) is restated, DESIGN.md U15.  Needs no batch, uses the stream of the handle only; also available in a
 * generated solver (no parameter layout is involved).  Stream-ordered, no allocation, no synchronisation.  Inputs (device):
 *   d_xy        f64 [n_scenes][n_pts_max][2]   waypoints;  2 <= n_pts_max <= 1025
 *   d_count     i32 [n_scenes]                 waypoints of the scene, clipped to [0, n_pts_max]
 *   d_s         f64 [n_scenes][n_pts_max]      or NULL.  Given: the knots t_i = s_i as supplied (not shifted).  NULL: chord lengths, t_0 = 0,
 *                                              t_{i+1} = t_i + sqrt(dx dx + dy dy), accumulated strictly left to right
 *   d_left_xy, d_right_xy                      as d_xy, or NULL: the bounds' waypoints, one per waypoint of the centreline (all of d_left_xy,
 *                                              d_right_xy, d_bounds or none of them)
 *   d_v         f64 [n_scenes][n_pts_max]      or NULL: the velocity at each waypoint (with d_velocity, both or neither)
 * Outputs (device, caller-owned), in exactly the layouts tmpc_track_path reads, rows n_seg_max apart, n_pts_max - 1 <= n_seg_max <= 1024, so
 * that one allocation serves both calls:
 *   d_path        f64 [n_scenes][n_seg_max][9]     (ax bx cx dx ay by cy dy start), x(t) = ((ax t + bx) t + cx) t + dx on t = s - start
 *   d_path_count  i32 [n_scenes]                   count - 1 segments
 *   d_path_length f64 [n_scenes]                   the last knot
 *   d_bounds      f64 [n_scenes][2][n_seg_max][8]  or NULL: left, right
 *   d_velocity    f64 [n_scenes][n_seg_max][4]     or NULL: (a b c d) of v(s)
 *   d_road_width  f64 [n_scenes]                   or NULL: sqrt(ex ex + ey ey) between the bounds' first waypoints (contouring.cpp:152); written
 *                                                  with bounds only
 *   d_status      u8  [n_scenes]                   or NULL: 0 fitted, 1 invalid
 * INVALID: fewer than 2 waypoints, or a knot spacing h_i = t_{i+1} - t_i for which h_i > 0 && h_i < inf is false (a duplicate waypoint, a
 * non-increasing s, NaN; tk::spline asserts there).  An invalid scene gets d_path_count = 0 and d_status = 1 and NOTHING else of it is
 * written; tmpc_track_path ignores a path with count <= 0.  Coordinates are not checked otherwise.  Rows at or beyond a scene's segment count
 * are not touched.  Equal bit for bit to mpc_planner_amd.modules.fit_path (no FMA contraction, same operation order).  One wave per scene:
 * the Thomas recurrence is sequential, one lane per curve (at most 7: x, y, four bound curves, v); everything else uses all lanes.
 * TMPC_ERR_INVALID, before any launch: a NULL required pointer (d_xy, d_count, d_path, d_path_count, d_path_length), a partial group
 * (d_left_xy / d_right_xy / d_bounds; d_v / d_velocity), n_scenes <= 0, n_pts_max outside [2, 1025], n_seg_max outside [n_pts_max - 1, 1024]. */
int tmpc_fit_path(tmpc_handle *h, int32_t n_scenes, int32_t n_pts_max, int32_t n_seg_max, const void *d_xy, const void *d_count, const void *d_s,
                  const void *d_left_xy, const void *d_right_xy, const void *d_v, void *d_path, void *d_path_count, void *d_path_length,
                  void *d_bounds, void *d_velocity, void *d_road_width, void *d_status);

/* ---- free-space decomposition on device: costmap -> the decomp rows.  What DecompConstraints::update and setParameters
 * (mpc_planner_modules/src/decomp_constraints.cpp:52-189) do for the static obstacles of the rosnavigation stack: the occupied cells of the
 * costmap become points, a polyline on the reference path is laid along the warm start's speeds, every segment of it gets one convex polygon
 * free of points, and the polygon's rows A p <= b go into the decomp rows of the stage behind the segment.  DecompUtil is not in the reference
 * tree, and the reference uses a modified copy nobody here has read: this is a RESTATEMENT OF UPSTREAM DecompUtil's LineSegment algorithm
 * (DESIGN.md U16), held bit for bit to mpc_planner_amd.modules (costmap_points, decomp_halfspaces) and by the tests to hand values and to the
 * geometric properties any correct decomposition has; parity with the reference's own DecompUtil is not pinned.  All three calls are
 * stream-ordered on the handle's stream, allocate nothing, do not synchronise, and check every argument before any launch. */
/* getOccupiedGridCells (:122-148).  Needs no batch; also available in a generated solver.  Inputs (device):
 *   d_cost     u8  [n_scenes][size_y][size_x]   the costmap_2d layout, index my * size_x + mx;  size_x, size_y >= 1, size_x * size_y <= 2^20
 *   d_origin   f64 [n_scenes][2]                world position of the map's corner
 *   resolution                                  cell size
 * Outputs (device, caller-owned):
 *   d_points   f64 [n_scenes][n_pts_max][2]     1 <= n_pts_max <= 16384
 *   d_count    i32 [n_scenes]
 *   d_overflow u8  [n_scenes]                   or NULL
 * A cell is occupied iff its cost is not 0 (costmap_2d::FREE_SPACE); its point is the cell centre (origin_x + (mx + 0.5) resolution,
 * origin_y + (my + 0.5) resolution) (Costmap2D::mapToWorld).  The points come in the reference's order, mx outer and my inner; the first
 * n_pts_max occupied cells are kept, d_count is their number and d_overflow 1 iff there were more.  Entries at or beyond d_count are not
 * touched.  One workgroup per scene: an order-preserving compaction (ballot and popcount prefix), no atomics.
 * TMPC_ERR_INVALID: a NULL d_cost / d_origin / d_points / d_count, n_scenes <= 0, a size < 1 or size_x * size_y > 2^20, n_pts_max outside
 * [1, 16384]. */
int tmpc_costmap_points(tmpc_handle *h, int32_t n_scenes, int32_t size_x, int32_t size_y, const void *d_cost, const void *d_origin, double resolution,
                        int32_t n_pts_max, void *d_points, void *d_count, void *d_overflow);
/* DecompConstraints::update (:52-118) for n_scenes scenes.  Needs a batch: v_k is read from the handle's warm start, as tmpc_road_halfspaces
 * reads the spline state; both models' strides.  Inputs (device):
 *   d_main_of      i32 [n_scenes]                 the batch entry that stands for the scene's MAIN solver
 *   d_path, d_path_count, d_path_length           the whole paths as tmpc_fit_path writes them, rows n_seg_max apart, 1 <= n_seg_max <= 1024
 *   d_s0           f64 [n_scenes]                 state["spline"]; tmpc_track_path's d_closest_s can be passed as it is
 *   d_state_x      f64 [n_scenes]                 the dummy's b = x + 100
 *   d_points       f64 [n_scenes][n_pts_max][2],  d_count i32 [n_scenes] clipped to [0, n_pts_max]: what tmpc_costmap_points wrote
 *   range                                         decomp/range: half width of the local box;  n_rows = decomp/max_constraints, 1 .. 64
 * Outputs (device, caller-owned; every entry of a processed scene is written, dummies included):
 *   d_rows         f64 [n_scenes][N][n_rows][3]   (a1, a2, b)
 *   d_row_count    i32 [n_scenes][N]              rows that are not dummies
 *   d_status       u8  [n_scenes][N]              0 complete; 1 truncated: more rows were found than n_rows (the reference logs a warning);
 *                                                 2 degenerate: the stage has FEWER rows than the polygon needs, or none -- see below
 * A scene whose d_main_of is outside [0, B) or whose path count is <= 0 is left wholly untouched.
 * THE POLYLINE (:68-82).  N points P(s_k), s_0 = d_s0, s_{k+1} = s_k + v_k dt accumulated left to right, v_k = the warm start's v of stage k.
 * P(s): the cubic of segment i = max{j < count : start_j <= s} (0 below the first knot) at t = s - start_i; for s >= length the path
 * continues straight along its end tangent, P(length) + (s - length) P'(length) (U14-3).  Segment k, P(s_k) -> P(s_{k+1}), goes to stage
 * k + 1; stage 0 is all dummies (1, 0, x + 100), count 0, status 0.
 * ONE SEGMENT (U16).  e = unit direction, h = (e_y, -e_x), c = midpoint, f = half length; a segment whose length is not positive and finite
 * is degenerate: all dummies, status 2 (DecompUtil's normals are NaN there and the reference's copy stops at row 0 -- a robot with v = 0 gets
 * no static constraints in the reference; kept, and reported).  Local coordinates of a point o: u = (o - c).e, w = (o - c).h.  Box: |w| <=
 * range + 1e-10 and |u| <= f + range + 1e-10.  Ellipse: a = b = f; while a box point has sqrt(d2) <= 1 (then: 1 - sqrt(d2) > 1e-10),
 * d2 = (u / a)^2 + (w / b)^2, the one with the smallest d2 is chosen, b = |w| / sqrt(1 - (u / a)^2) if u < a, and the chosen point leaves.
 * Polygon: among all box points, repeatedly the one with the smallest d2 gives the row (n, n.o) tangent to the ellipse through it, n = the
 * normalised (u / a^2, w / b^2) turned back into the world; it and every point with n.(o' - o) >= 0 leave; the row is negated if c violates
 * it; at most n_rows such rows.  Smallest d2: a NaN counts as +inf, the lowest point index wins among equals.  Then the four rows of the box:
 * (h, h.(p1 + range h)), (-h, -h.(p1 - range h)), (e, e.(p2 + range e)), (-e, -e.(p1 - range e)).
 * THE COPY (:90-114).  Of the rows found, the first min(found, n_rows) are copied until one has |A_i| < 1e-3 or a NaN first entry; that row and
 * every later one is the dummy (an obstacle point ON the segment does this: status 2).
 * One workgroup of 256 threads per (scene, stage); the points are streamed from global memory on every pass, the three sets are bitmasks in
 * LDS, the argmin a reduction on (d2, index); no atomics, no unbounded loop.
 * TMPC_ERR_INVALID: no batch, a NULL pointer, n_scenes <= 0, n_seg_max outside [1, 1024], n_pts_max outside [1, 16384], n_rows outside
 * [1, 64], a range that is negative or not finite, a generated solver. */
int tmpc_decomp_halfspaces(tmpc_handle *h, const void *d_main_of, int32_t n_scenes, int32_t n_seg_max, const void *d_path, const void *d_path_count,
                           const void *d_path_length, const void *d_s0, const void *d_state_x, const void *d_points, const void *d_count,
                           int32_t n_pts_max, double range, int32_t n_rows, void *d_rows, void *d_row_count, void *d_status);
/* DecompConstraints::setParameters (:150-189): the rows d_rows [n_scenes][N][n_rows][3] of EVERY stage, stage 0 included, into the slack rows
 * first_row .. first_row + n_rows - 1 (disc_0_decomp_{j}_a1 / _a2 / _b) of every entry b of the CURRENT batch with d_scene_of[b] (i32 [B])
 * inside [0, n_scenes), and ego_disc_0_offset = disc_offset at every stage of those entries; nothing else is touched, an entry whose scene is
 * outside that range not at all.  Requires first_row + n_rows <= the problem's slack rows (n_slk).  Parameter sharing as for
 * tmpc_set_path_parameters: the rows are an entry's own columns, a map stays valid when every entry of a set names the same scene, and a
 * caller with TMPC_SHARE_COPIES_NOT_MAINTAINED still names every entry, since the kernels read these rows from the entry itself.
 * TMPC_ERR_INVALID: no batch, a NULL d_rows / d_scene_of, n_scenes <= 0, n_rows < 1, first_row < 0, rows that do not fit, a generated solver. */
int tmpc_set_halfspace_rows(tmpc_handle *h, const void *d_rows, int32_t n_rows, int32_t first_row, const void *d_scene_of, int32_t n_scenes,
                            double disc_offset);

/* ---- scenario -> polygon construction of SH-MPC on device.  Replaces what the reference gets from the
 * external scenario_module (scenario_constraints.cpp:47 update, :76-79 setParameters; source absent -> restated, see
 * mpc_planner_amd/modules.py::scenario_halfspaces): for every trajectory b and stage k >= 1, each of the n_pts sampled
 * obstacle positions of prediction step k-1 gives a halfspace a.x <= b linearised around the guess x0[b][k]; the
 * halfspaces that form the boundary of their intersection polygon (all others are redundant) are written, closest first
 * and at most n_rows of them (<= 64), into the first n_rows decomp/scenario rows of the batch's parameter tensor together
 * with ego_disc_0_offset; unused rows and stage 0 = dummy rows.  n_pts <= about 5480 (a stage's halfspaces live in LDS next to the kernel's static tables; the call checks the exact bound).
 * Device pointers:
 *   d_samples  : f64 [n_scenes][N][n_pts][2]   sampled positions, n_pts = obstacles x scenarios (index i = step k-1)
 *   d_scene_of : i32 [B];  d_state_x : f64 [n_scenes]  (dummy b = x + 100)
 * Operates in place on the parameter tensor of the last tmpc_set_batch / tmpc_set_batch_device call. */
int tmpc_scenario_halfspaces(tmpc_handle *h, const void *d_samples, int32_t n_pts, int32_t n_rows, const void *d_scene_of,
                             const void *d_state_x, double radius, double disc_offset);

/* Support of each trajectory's solution after a solve on rows written by tmpc_scenario_halfspaces: the number of distinct
 * scenarios with an active constraint, a.p_disc - (b + slack) >= -tol at the solution (ScenarioSolver::support,
 * scenario_constraints.h:38-40; filled by the absent scenario_module, restated from the method's definition: the plan's
 * collision-probability certificate holds while the support stays within the bound the sample size was chosen for -- see
 * mpc_planner_amd/modules.py::scenario_risk / scenario_sample_size).  Scenario of sample i = i % n_scenarios (samples are
 * [obstacle][scenario]); n_scenarios <= 8192.
 * Valid only while the batch's scenario rows are the ones tmpc_scenario_halfspaces wrote (a later tmpc_set_batch* invalidates
 * the bookkeeping: TMPC_ERR_INVALID).
 *   d_support     : i32 [B] out    distinct active scenarios
 *   d_active_rows : i32 [B] out or NULL    active rows */
int tmpc_scenario_support(tmpc_handle *h, int32_t n_scenarios, double tol, void *d_support, void *d_active_rows);
/* SH-MPC scenario sampler on device (f-3; scenario_constraints.cpp:121-131: scenario_module.GetSampler().IntegrateAndTranslateToMeanAndVariance
 * per solver -- the scenario_module is absent, the sampler is restated from the call's inputs): for each of n_solvers solvers (scenes), each of
 * n_obstacles obstacles and each of n_scenarios scenarios, a mode of the obstacle's Gaussian mixture is drawn from d_prob
 * [n_solvers][n_obstacles][n_modes] and ONE standard-normal pair places the obstacle on every prediction step of that mode:
 * o_k = mean_k + R(angle_k) (major_k xi1, minor_k xi2), d_pred [n_solvers][n_obstacles][n_modes][N][6] = (x, y, cos angle, sin angle, major,
 * minor).  d_samples [n_solvers][N][n_obstacles * n_scenarios][2] is what tmpc_scenario_halfspaces / tmpc_scenario_discard read.
 * Counter-based (splitmix64 of seed, solver, obstacle, scenario) and free of library transcendentals: mpc_planner_amd.modules.sample_scenarios
 * reproduces every sample bit for bit. */
int tmpc_sample_scenarios(tmpc_handle *h, const void *d_pred, const void *d_prob, int32_t n_solvers, int32_t n_obstacles, int32_t n_modes,
                          int32_t n_scenarios, uint64_t seed, void *d_samples);
/* Scenario removal: for every trajectory of the current batch the n_discard scenarios that constrain its guess most (smallest clearance
 * min over obstacles and stages of |o - p_k| - radius; lowest scenario index on ties) are marked; the next tmpc_scenario_halfspaces on this
 * batch leaves their samples out.  The discarded scenarios count into the bound (modules.scenario_risk(removed = n_discard)).  The policy of
 * the absent scenario_module is not in the reference tree: this is the greedy rule of the method the reference cites (README.md:22).
 * tmpc_scenario_discarded copies the marks (uint8 [B][n_scenarios], device). */
int tmpc_scenario_discard(tmpc_handle *h, const void *d_samples, int32_t n_pts, int32_t n_scenarios, int32_t n_discard, const void *d_scene_of, double radius);
int tmpc_scenario_discarded(tmpc_handle *h, void *d_mask);
/* Stages of every trajectory whose sampled halfspaces CONTRADICT each other (an empty polygon: the guess sits in the overlap of inflated
 * discs on opposite sides).  Such a stage keeps the n_rows closest halfspaces instead of dummies -- the QP is then infeasible or pays
 * slack, never silently unconstrained -- and is counted here: d_count int32 [B] (device).  Callers treat a trajectory with a count
 * > 0 as not eligible (solver.optimize_scenarios: scenario_status 2). */
int tmpc_scenario_empty_stages(tmpc_handle *h, void *d_count);

/* ---- cross-tick state on device, so a closed loop runs without host round trips --------------------
 * tmpc_warmstart builds the next tick's warm start x0 and xinit of every trajectory of the current batch from the
 * solution the handle holds (last tmpc_solve) and the new state.  Device pointers:
 *   d_state : f64 [B][nx]   the new initial state of each trajectory (Solver::setXinit(State))
 *   d_mode  : i32 [B] or NULL (= all 1):  0 leave x0 alone; 1 Solver::initializeWarmstart(state, true)
 *             (acados_solver_interface.cpp:344-364); 2 initializeWarmstart(state, false) (:365-375);
 *             3 Solver::initializeWithBraking(state) (:303-342) with |deceleration| (CONFIG deceleration_at_infeasible)
 *   d_src   : i32 [B] or NULL (= identity): trajectory whose previous solution is shifted into b.
 * Mode 1 writes 0 into the inputs of node 0, where the reference reads State::get(<input>) out of bounds (state.cpp:21-24).
 * The warm start / xinit buffers of the current batch are rewritten in place: the handle's own copies after tmpc_set_batch,
 * the caller's device buffers after tmpc_set_batch_device (they must be writable). */
int tmpc_warmstart(tmpc_handle *h, const void *d_state, const void *d_mode, const void *d_src, double deceleration);
/* GuidanceConstraints::initializeSolverWithGuidance (guidance_constraints.cpp:390-414) for every enabled trajectory:
 * d_gpos, d_gvel f64 [B][N+1][2] (guidance position / velocity at t = k dt), d_enabled u8 [B] or NULL. */
int tmpc_init_with_guidance(tmpc_handle *h, const void *d_gpos, const void *d_gvel, const void *d_enabled);

/* ---- the guidance hand-off: what GuidanceConstraints does with the output of the guidance search either side of the solve.
 * The search itself (the external guidance_planner) stays with the caller: it delivers, per scene, a number of trajectories, each a handful of
 * space-time nodes with a topology class.  Three entries; all stream-ordered on the handle's stream, no allocation, no synchronisation; they
 * read no parameter column, so they are available in a generated solver too.  Every output equals the numpy mirrors
 * (mpc_planner_amd.modules.sample_guidance / guidance_plan / guidance_decide) bit for bit: + - x / and comparisons only, no FMA contraction.
 *
 * THE BATCH LAYOUT IS FIXED: entry b = q P + p is planner p of scene q, P = n_paths + (use_tmpcpp ? 1 : 0), and the non-guided T-MPC++ planner is
 * p = P - 1.  Planner p follows guidance trajectory p (planner.id).  A DISABLED planner keeps its entry: it is solved and ignored, so the launch
 * shape never changes.  Only `enable_constraints = true` is covered (with false every planner takes the non-guided branch, :299-303). */

/* Nodes -> time spline -> the samples tmpc_init_with_guidance reads (GetGuidanceTrajectory(id).spline.GetTrajectory() at t = k dt, :390-414).
 *   d_nodes       f64 [n_traj][n_nodes_max][3]   (t, x, y) per node;  2 <= n_nodes_max <= 64
 *   d_node_count  i32 [n_traj]
 *   d_gpos, d_gvel f64 [n_traj][N + 1][2]        position / velocity at t = k dt, k = 0 .. N, N and dt the handle's; with n_traj = B exactly
 *                                                what tmpc_init_with_guidance takes.  Every entry is written
 *   d_status      i32 [n_traj]                   0 ok; 1 INVALID: the count outside [2, n_nodes_max] or a knot spacing t_{i+1} - t_i that is not
 *                                                positive and finite -- both rows of such a trajectory are zeros
 * x(t) and y(t) are the natural cubic splines of U15 over the knots t_i (tmpc_fit_path's recurrence; two nodes: the straight line).  Sample k:
 * segment i = max{j <= count - 2 : t_j <= t}, 0 if there is none, tau = t - t_i, position ((a tau + b) tau + c) tau + d, velocity
 * (3 a tau + 2 b) tau + c; outside the node span the first / last cubic continues.  RosTools::Spline2D and the guidance planner's trajectory type
 * are not in the reference tree: a real guidance_planner may parametrise or extrapolate differently (U18), and a caller with its own samples
 * passes them to tmpc_init_with_guidance as before.  Needs no batch.  One wave per trajectory.
 * TMPC_ERR_INVALID, before any launch: a NULL pointer, n_traj <= 0, n_nodes_max outside [2, 64]. */
int tmpc_sample_guidance(tmpc_handle *h, int32_t n_traj, int32_t n_nodes_max, const void *d_nodes, const void *d_node_count, void *d_gpos,
                         void *d_gvel, void *d_status);

typedef struct tmpc_guidance_options {
    uint32_t size;                               /* sizeof(tmpc_guidance_options) of the caller's header (the rule of tmpc_create_v2) */
    int32_t n_paths;                             /* guidance_planner's n_paths: guided planners per scene, 1 .. 63 */
    int32_t use_tmpcpp;                          /* CONFIG["t-mpc"]["use_t-mpc++"]: a non-guided planner as the last of every scene */
    int32_t warmstart_with_mpc_solution;         /* CONFIG["t-mpc"]["warmstart_with_mpc_solution"] */
    int32_t shift_previous_solution_forward;     /* CONFIG shift_previous_solution_forward && enable_output (planner.cpp:78-79) */
    int32_t reserved;                            /* 0 */
    double selection_weight_consistency;         /* guidance_planner's selection_weight_consistency_ */
} tmpc_guidance_options;

/* Before the warm start: mapGuidanceTrajectoriesToPlanners (:192-250), the per-planner branches of optimize() (:283-317) and the main solver's
 * start (planner.cpp:78-86), per scene.  Pure: it reads the cross-tick state and may be called twice with the same result.  Needs no batch.
 *   d_traj_count          i32 [n_scenes]            NumberOfGuidanceTrajectories(), clipped to [0, n_paths]
 *   d_topology_class      i32 [n_scenes][n_paths]   class of trajectory i (entries at or beyond the count are not read)
 *   d_previously_selected u8  [n_scenes][n_paths]   the trajectory's previously_selected_, or NULL (below)
 *   d_planner_ids         i32 [n_scenes][P]         cross-tick state, caller-owned: result.guidance_ID of each planner's last tick; initialise
 *                                                   to -1 (SolverResult::Reset)
 *   d_selection           i32 [n_scenes][3]         cross-tick state: (selected guidance ID, selected was the non-guided planner, best index of
 *                                                   the last tick); initialise to (-1, 0, -1).  Both are written by tmpc_guidance_decide only
 * Outputs, [B] = [n_scenes P]:
 *   d_disabled     u8   p >= traj_count and p is not the non-guided planner (:286-293)
 *   d_mode, d_src  i32  for tmpc_warmstart.  The main solver's start: best index >= 0: mode = shift ? 1 : 2, src = q P + best; else mode 3
 *                       (braking), src = b; every planner copies it (`*solver = *_solver`).  A guided, enabled planner with
 *                       warmstart_with_mpc_solution && existing_guidance -- the mapping run on the old d_planner_ids, its missing `break`
 *                       kept -- restarts from its own solution instead: src = b, mode = shift ? 1 : 2 (:310-311)
 *   d_init_enabled u8   for tmpc_init_with_guidance: 1 for every other guided, enabled planner (:312-313); 0 for the non-guided and disabled ones
 *   d_rows_dummy   u8   non-guided || disabled: d_is_original of tmpc_linearize_topology_ex
 *   d_guidance_id  i32  2 n_paths for the non-guided planner (:349), topology_class[q][p] for a guided, enabled one, -1 for a disabled one
 *   d_weight       f64  selection_weight_consistency for a guided, enabled planner whose trajectory was previously selected, else 1.0 (:358-359).
 *                       Without d_previously_selected: class == selection[0] && selection[1] == 0 && selection[0] >= 0 -- what U18 assumes the
 *                       absent planner does with OverrideSelectedTrajectory
 * TMPC_ERR_INVALID, before any launch: a NULL required pointer (all but d_previously_selected), NULL options, n_scenes <= 0, n_paths outside
 * [1, 63], an options->size this library cannot honour. */
int tmpc_guidance_plan(tmpc_handle *h, int32_t n_scenes, const tmpc_guidance_options *opt, const void *d_traj_count, const void *d_topology_class,
                       const void *d_previously_selected, const void *d_planner_ids, const void *d_selection, void *d_mode, void *d_src,
                       void *d_init_enabled, void *d_rows_dummy, void *d_disabled, void *d_guidance_id, void *d_weight);

/* After the solve: recordResult (:343-360), decide (:366-387) and the wrapper's command (ros1_jackalsimulator.cpp:181-201), per scene.  Needs a
 * solved batch (tmpc_solve since the last tmpc_set_batch*) of B == n_scenes P entries.
 *   d_pobj f64 [B], d_exit_code i32 [B]   normally those of tmpc_result_device_ptrs; any device arrays will do
 *   d_disabled, d_guidance_id, d_weight   as tmpc_guidance_plan wrote them
 *   d_state  f64 [n_scenes][nx]           the robot's state (v = entry 3), for the braking command
 * Outputs:
 *   d_best  i32 [n_scenes]      FindBestPlanner (:416-434) over the scene's entries: disabled skipped, success exit_code == 1, objective
 *                               pobj x weight, initial value 1e10, strict '<' (the lowest index wins); relative to the set as tmpc_gather_best
 *                               reads it, -1 if none
 *   d_exit  i32 [n_scenes]      the winner's exit code; without one exit_code of planner 0, or -1 if planner 0 is disabled (:372, after Reset)
 *   d_cmd   f64 [n_scenes][2]   a winner and enable_output: (v of node 1, w of node 0) of the winner's solution in the handle; otherwise the
 *                               braking command (max(v - deceleration control_dt, 0), 0)
 *   d_planner_ids               [q][p] = d_guidance_id[b], whatever the solve's verdict (:347-356)
 *   d_selection                 (d_guidance_id[winner], winner is the non-guided planner, best); without a winner the first two stay and the
 *                               third is -1 (the early return of :369-373)
 * TMPC_ERR_INVALID, before any launch: as tmpc_guidance_plan (every pointer is required), no solved batch, B != n_scenes P. */
int tmpc_guidance_decide(tmpc_handle *h, int32_t n_scenes, const tmpc_guidance_options *opt, const void *d_pobj, const void *d_exit_code,
                         const void *d_disabled, const void *d_guidance_id, const void *d_weight, const void *d_state, double deceleration,
                         double control_dt, int32_t enable_output, void *d_best, void *d_exit, void *d_cmd, void *d_planner_ids, void *d_selection);

/* ---- test/debug entry points (used by tests/ to diff per-phase tensors against the oracle) -------- */
/* Copy the batch's (possibly device-built) warm start and xinit back: x0[B][(N+1)*nvar], xinit[B][nx]; either may be NULL. */
int tmpc_debug_get_x0(tmpc_handle *h, double *x0, double *xinit);
/* Evaluate the stage functions on device for n points: z[n][7], p[n][npar] (host pointers).
 * Outputs (host, may be NULL): cost[n], cost_grad[n][7], cost_hess[n][49], h[n][nh], h_jac[n][nh][7],
 * x_next[n][5], x_jac[n][5][7]; lag_hess[n][49] = dt*hess(l) + sum_j pi[j] hess(x_next_j) +
 * sum_r lamh[r] hess(h_r) (pi[n][5], lamh[n][nh] host inputs, NULL = zeros); mirror[n][49] = MIRROR(lag_hess). */
/* Copy the batch's (possibly device-modified) parameter tensor back: params[B][N*npar] host pointer. */
int tmpc_debug_get_params(tmpc_handle *h, double *params);

/* Mean shader-clock cycles per phase over the batch (one extra instrumented solve).  cycles[10]:
 * linearise, residuals, barrier Hessian, Riccati factor, rhs build, Riccati solve, row passes, update, final, total.
 * Runs the instrumented twin of the instantiation tmpc_solve would run for the current batch and latency mode (a compact kernel: the fast kernel
 * of its shape, bitwise the same results) and leaves that solve's results in the handle; TMPC_ERR_INVALID where no such twin exists. */
int tmpc_debug_profile(tmpc_handle *h, int64_t *cycles, int32_t n_phases);

/* The LDS bank-conflict model behind the compact kernels' layout padding (no handle, no GPU): the passes the row passes' coefficient loads
 * take per wave and interior-point row pass for a stage stride of `dstride` doubles -- N stages, nh general rows per stage of which the first
 * n_pair are stored as pairs, a kernel of `threads` (64 or 128) threads per trajectory.  tmpc_create picks, among the strides that keep the
 * kernel's residency, the one this function likes best (diagnostics: TMPC_EXP_DPAD in INTEGRATION.md section 7); results never depend on it. */
int tmpc_debug_lds_passes(int32_t N, int32_t n_pair, int32_t nh, int32_t threads, int32_t dstride);
/* Test aid (no reference counterpart): fills the LDS of every CU of the handle's device with signalling-NaN bit patterns (one 160 KB workgroup
 * per CU, several rounds) and waits.  LDS keeps its contents between kernels, so a solve kernel that reads a word it never wrote gives results
 * that depend on what ran before it -- in a fresh test process that is usually zeros and the bug stays invisible (round 6: a column slot the
 * four-wave factorisation multiplied by zero without ever writing it).  tests/test_gpu_lds_poison.py solves after this call and demands the
 * un-poisoned results bit for bit, for every kernel family. */
int tmpc_debug_poison_lds(tmpc_handle *h);
/* 1 if this build of the library reads the TMPC_* lab switches from the environment (libtmpc_hip_lab.so, -DTMPC_LAB_SWITCHES), 0 for the product library. */
int tmpc_has_lab_switches(void);

int tmpc_debug_eval_stage(tmpc_handle *h, int32_t n, const double *z, const double *p, const double *pi,
                          const double *lamh, double *cost, double *cost_grad, double *cost_hess,
                          double *hval, double *h_jac, double *x_next, double *x_jac, double *lag_hess,
                          double *mirror);

#ifdef __cplusplus
}
#endif
#endif
