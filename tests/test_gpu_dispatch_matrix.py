"""Every solve kernel the dispatcher can pick, at the edges of its regime, against the CPU oracle.

The HIP path is a dispatch table (pick_*_kernel in csrc/tmpc_capi.hip): horizon, row count nr = n_up + M + 14, stage model, latency mode,
riccati_form and launch size choose a template instantiation, and tmpc_kernel_info names the instantiation of every slot the handle fills.  Each
case of DISPATCH_CASES asserts
  (a) the library reports exactly the expected instantiation for the slot the launch runs;
  (b) the oracle's exit codes, SQP counts, QP status and interior-point counts, trajectories <= 1e-8 relative per stage next to the 1e-4 contract,
      FindBestPlanner bit-exact on the device's objectives (test_gpu_parity._compare / _check_selection; latency mode 2 keeps its interior-point
      count rule, test_gpu_parity._compare_relaxed_iterations, plus 1e-8 where the counts agree);
  (c) at least half of the trajectories succeed;
  (d) the same launch twice gives the same bits;
  (e) the first k trajectories solved alone give the bits of their rows in the full launch (for the launch-size cases: the previous size);
and then tmpc_debug_profile: where the running instantiation has a profiled twin (the TMPC_FAST / TMPC_FASTP shapes of the table, the generic
kernel) the phases are positive and the results it leaves in the handle are solve()'s bits; elsewhere it is refused.
tests/test_dispatch_table.py (CPU) requires a case here for every instantiation the pick functions name, or a reason in EXCLUDED."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("xtraj", "utraj", "pobj", "exit_code", "qp_status", "sqp_iter", "qp_iter_total", "res_eq")
VERDICT = ("exit_code", "qp_status", "sqp_iter", "qp_iter_total")


def case(cid, expect, N, n_lin, M, n_slk=0, S=5, cm=0, gauss=False, rf=0, mode=0, B=16, lab=None, scene=None, ids=(1,), refused=False, also=None, prev=None,
         doomed=(), disc_offset=0.0):
    """expect: the instantiation of the slot the launch runs; also: {slot: name} of other slots the handle must fill; lab: TMPC_* switches of the lab
    library; scene: make_scene keywords instead of the ones derived from the row counts; B: an int, or an expression of the thresholds tmpc_kernel_info
    reports (cp_min_B, cp2_min_B, grid_max); refused: set_latency_mode(mode) returns False (no such variant: the default kernels run); prev: the
    launch size of (e) (the other side of a threshold) instead of a few trajectories; doomed: batch entries given contradictory topology rows
    (test_gpu_parity._make_infeasible): their failure verdicts (exit code, QP status, SQP and interior-point counts) are compared with the oracle's too;
    disc_offset: ego_disc_0_offset of every stage (the scenes give 0): a non-zero offset couples psi with x, y in the rows' Hessian, so that W is not block
    diagonal and MIRROR takes its 7 x 7 iteration -- without the curvature-aware cost, no other case reaches that branch."""
    return dict(id=cid, expect=expect, N=N, n_lin=n_lin, M=M, n_slk=n_slk, S=S, cm=cm, gauss=gauss, rf=rf, mode=mode, B=B, lab=lab or {},
                scene=scene, ids=ids, refused=refused, also=also or {}, prev=prev, doomed=tuple(doomed), disc_offset=disc_offset)


CFG5 = dict(M=8, slack=True, n_scenario=24)                      # SH-MPC: 24 scenario halfspaces, dims n_lin 0, M 0, n_slk 24
CP0 = {"TMPC_COMPACT_MIN_B": "0"}                                 # lab: the compact one-wave kernel for every launch size
CP2_0 = {"TMPC_COMPACT2_MIN_B": "0"}                              # lab: the compact two-wave kernel for every launch size

DISPATCH_CASES = [
    # ---- latency mode 0, one wave, three lanes per stage (N <= 21); N <= 20: compact kernel (default slot) + its fast twin for small launches
    case("m0 (8,8) N=2", "fast<8,8,3,64,Solo,0>", 2, 8, 8, also={"default": "compact<8,8,3,64,0>"}),
    case("m0 (8,8) N=3", "fast<8,8,3,64,Solo,0>", 3, 8, 8),
    case("m0 (8,8) N=20", "fast<8,8,3,64,Solo,0>", 20, 8, 8, ids=(1, 2), also={"default": "compact<8,8,3,64,0>", "lat1": "fast<8,8,6,128,Solo,0>",
         "lat2": "fast<8,8,6,128,ScanSolo,0>", "lat3": "fast<8,8,12,256,ScanQuad,0>"}),
    case("m0 (8,8) N=20 compact", "compact<8,8,3,64,0>", 20, 8, 8, lab=CP0),
    case("m0 (8,8) N=21", "fast<8,8,3,64,Solo,0>", 21, 8, 8, also={"lat2": "fast<-1,12,4,128,ScanSoloT<2>,0>", "lat3": "fast<-1,6,8,256,ScanQuadT<2>,0>"}),
    case("m0 (0,4) N=20", "fast<0,4,3,64,Solo,0>", 20, 0, 4, ids=range(50, 66), also={"default": "compact<0,4,3,64,0>"}),
    case("m0 (0,4) N=20 compact", "compact<0,4,3,64,0>", 20, 0, 4, ids=range(50, 66), lab=CP0),
    case("m0 (12,12) N=20", "fast<12,12,3,64,Solo,0>", 20, 12, 12, also={"default": "compact<12,12,3,64,0>"}),
    case("m0 (12,12) N=20 compact", "compact<12,12,3,64,0>", 20, 12, 12, lab=CP0),
    case("m0 (24,0) N=20", "fast<24,0,3,64,Solo,0>", 20, 0, 0, n_slk=24, scene=CFG5, B=8, also={"default": "compact<24,0,3,64,0>"}),
    case("m0 (24,0) N=20 compact", "compact<24,0,3,64,0>", 20, 0, 0, n_slk=24, scene=CFG5, B=8, lab=CP0),
    # runtime-shape one-wave kernels <-1, R, 3>: nr = 3 R (every row slot used) and the first nr past the previous capacity
    case("m0 <-1,7,3> nr=21", "fast<-1,7,3,64,Solo,0>", 20, 3, 4, also={"default": "compact<-1,7,3,64,0>"}),
    case("m0 <-1,7,3> nr=21 compact", "compact<-1,7,3,64,0>", 20, 3, 4, lab=CP0),
    case("m0 <-1,10,3> nr=22", "fast<-1,10,3,64,Solo,0>", 20, 4, 4, also={"default": "compact<-1,10,3,64,0>"}),
    case("m0 <-1,10,3> nr=30", "fast<-1,10,3,64,Solo,0>", 20, 7, 9, also={"default": "compact<-1,10,3,64,0>"}),
    case("m0 <-1,10,3> nr=30 compact", "compact<-1,10,3,64,0>", 20, 7, 9, lab=CP0),
    case("m0 <-1,13,3> nr=31", "fast<-1,13,3,64,Solo,0>", 20, 8, 9),
    case("m0 <-1,13,3> nr=39", "fast<-1,13,3,64,Solo,0>", 20, 12, 13),
    case("m0 <-1,13,3> nr=39 N=21", "fast<-1,13,3,64,Solo,0>", 21, 12, 13),
    case("m0 N=21 nr=40 generic", "generic<0>", 21, 13, 13),
    case("m0 <-1,9,6> nr=40", "fast<-1,9,6,128,Solo,0>", 20, 13, 13),
    case("m0 <-1,9,6> nr=54", "fast<-1,9,6,128,Solo,0>", 20, 14, 14, n_slk=12),      # (the last fast capacity of N <= 20; the generic kernel past it: below)
    # ---- latency mode 0, 22 <= N <= 32: one wave at two lanes per stage for (8,8); two waves at four lanes per stage otherwise
    case("m0 (8,8) N=22", "fast<8,8,2,64,Solo,0>", 22, 8, 8, also={"default": "compact<8,8,2,64,0>"}),
    case("m0 (8,8) N=30", "fast<8,8,2,64,Solo,0>", 30, 8, 8, ids=(1, 2), also={"default": "compact<8,8,2,64,0>", "lat2": "fast<-1,12,4,128,ScanSoloT<2>,0>",
         "lat3": "fast<-1,6,8,256,ScanQuadT<2>,0>"}),
    case("m0 (8,8) N=30 compact", "compact<8,8,2,64,0>", 30, 8, 8, lab=CP0),
    case("m0 (8,8) N=31", "fast<8,8,2,64,Solo,0>", 31, 8, 8),
    case("m0 (8,8) N=32", "fast<8,8,2,64,Solo,0>", 32, 8, 8),
    case("m0 (8,8) N=30 two-wave", "fast<8,8,4,128,Solo,0>", 30, 8, 8, lab={"TMPC_NO_ONE_WAVE_N30": "1"}, also={"cp2": "compact<8,8,4,128,0>"}),
    case("m0 (8,8) N=30 two-wave cp2", "compact<8,8,4,128,0>", 30, 8, 8, lab={"TMPC_NO_ONE_WAVE_N30": "1", **CP2_0}),
    case("m0 (0,4) N=30 one-wave", "fast<0,4,2,64,Solo,0>", 30, 0, 4, ids=range(50, 66), lab={"TMPC_NO_TWO_WAVE": "1"}),
    case("m0 (12,12) N=30", "fast<12,12,4,128,Solo,0>", 30, 12, 12, also={"cp2": "compact<12,12,4,128,0>"}),
    case("m0 (12,12) N=30 cp2", "compact<12,12,4,128,0>", 30, 12, 12, lab=CP2_0),
    case("m0 (20,8) N=30", "fast<20,8,4,128,Solo,0>", 30, 8, 8, n_slk=12, also={"cp2": "compact<20,8,4,128,0>"}),
    case("m0 (20,8) N=30 cp2", "compact<20,8,4,128,0>", 30, 8, 8, n_slk=12, lab=CP2_0),
    case("m0 <-1,6,4> nr=24 N=22", "fast<-1,6,4,128,Solo,0>", 22, 5, 5, S=3, also={"cp2": "compact<-1,6,4,128,0>"}),
    case("m0 <-1,6,4> nr=24 N=30", "fast<-1,6,4,128,Solo,0>", 30, 5, 5, S=3),
    case("m0 <-1,6,4> nr=24 cp2", "compact<-1,6,4,128,0>", 30, 5, 5, S=3, lab=CP2_0),
    case("m0 <-1,9,4> nr=25", "fast<-1,9,4,128,Solo,0>", 30, 5, 6, also={"cp2": "compact<-1,9,4,128,0>"}),
    case("m0 <-1,9,4> nr=36", "fast<-1,9,4,128,Solo,0>", 32, 11, 11),
    case("m0 <-1,9,4> nr=36 cp2", "compact<-1,9,4,128,0>", 30, 11, 11, lab=CP2_0),
    case("m0 <-1,12,4> nr=37", "fast<-1,12,4,128,Solo,0>", 30, 11, 12),
    case("m0 <-1,12,4> nr=48", "fast<-1,12,4,128,Solo,0>", 31, 11, 11, n_slk=12),
    case("m0 N=30 nr=49 generic", "generic<0>", 30, 11, 12, n_slk=12),
    # ---- latency mode 1: two waves at six lanes per stage, (8,8), N <= 20
    case("m1 (8,8) N=20", "fast<8,8,6,128,Solo,0>", 20, 8, 8, mode=1),
    case("m1 (8,8) N=21 refused", "fast<8,8,3,64,Solo,0>", 21, 8, 8, mode=1, refused=True),
    case("m1 (8,8) N=32 refused", "fast<8,8,2,64,Solo,0>", 32, 8, 8, mode=1, refused=True),
    # ---- latency mode 2: the parallel-in-time Newton solve
    case("m2 (8,8) N=2", "fast<8,8,6,128,ScanSolo,0>", 2, 8, 8, mode=2),
    case("m2 (8,8) N=20", "fast<8,8,6,128,ScanSolo,0>", 20, 8, 8, mode=2),
    case("m2 (8,8) N=20 one wave", "fast<8,8,3,64,ScanSolo,0>", 20, 8, 8, mode=2, lab={"TMPC_SCAN_WAVES": "1"}),
    case("m2 (8,8) N=21", "fast<-1,12,4,128,ScanSoloT<2>,0>", 21, 8, 8, mode=2),
    case("m2 (8,8) N=31", "fast<-1,12,4,128,ScanSoloT<2>,0>", 31, 8, 8, mode=2),
    case("m2 <-1,12,4> nr=48 N=30", "fast<-1,12,4,128,ScanSoloT<2>,0>", 30, 11, 11, n_slk=12, mode=2),
    case("m2 N=30 nr=49 refused", "generic<0>", 30, 11, 12, n_slk=12, mode=2, refused=True),
    case("m2 <-1,9,6> (12,12) N=20", "fast<-1,9,6,128,ScanSolo,0>", 20, 12, 12, mode=2),
    # (N <= 20: the latency variants exist only next to a one-wave default kernel, nr <= 39 -- the runtime-shape ones would hold 54 / 48)
    case("m2 <-1,9,6> nr=39 N=20", "fast<-1,9,6,128,ScanSolo,0>", 20, 12, 13, mode=2),
    case("m2 N=20 nr=40 refused", "fast<-1,9,6,128,Solo,0>", 20, 13, 13, mode=2, refused=True),
    case("m2 (8,8) N=32 refused", "fast<8,8,2,64,Solo,0>", 32, 8, 8, mode=2, refused=True),
    # ---- latency mode 3: four waves per trajectory
    case("m3 (8,8) N=2", "fast<8,8,12,256,ScanQuad,0>", 2, 8, 8, mode=3),
    case("m3 (8,8) N=20", "fast<8,8,12,256,ScanQuad,0>", 20, 8, 8, mode=3),
    case("m3 (8,8) N=20 one-wave factorisation", "fast<8,8,12,256,ScanSolo,0>", 20, 8, 8, mode=3, lab={"TMPC_QUAD_AB": "1"}),
    case("m3 <-1,4,12> nr=39 N=20", "fast<-1,4,12,256,ScanQuad,0>", 20, 12, 13, mode=3),
    case("m3 N=20 nr=40 refused", "fast<-1,9,6,128,Solo,0>", 20, 13, 13, mode=3, refused=True),
    case("m3 (8,8) N=21", "fast<-1,6,8,256,ScanQuadT<2>,0>", 21, 8, 8, mode=3),
    case("m3 (8,8) N=31", "fast<-1,6,8,256,ScanQuadT<2>,0>", 31, 8, 8, mode=3),
    case("m3 <-1,6,8> nr=48 N=30", "fast<-1,6,8,256,ScanQuadT<2>,0>", 30, 11, 11, n_slk=12, mode=3),
    case("m3 (8,8) N=32 refused", "fast<8,8,2,64,Solo,0>", 32, 8, 8, mode=3, refused=True),
    # ---- curvature-aware cost (CM = 1)
    case("ca (20,8) N=30", "fast<20,8,4,128,Solo,1>", 30, 8, 8, n_slk=12, cm=1, also={"cp2": "compact<20,8,4,128,1>"}),
    case("ca (20,8) N=30 cp2", "compact<20,8,4,128,1>", 30, 8, 8, n_slk=12, cm=1, lab=CP2_0),
    case("ca (20,8) N=30 m3", "fast<-1,6,8,256,ScanQuadT<2>,1>", 30, 8, 8, n_slk=12, cm=1, mode=3),
    case("ca <-1,13,3> (8,8) N=20", "fast<-1,13,3,64,Solo,1>", 20, 8, 8, cm=1),
    case("ca <-1,13,3> nr=39 N=21", "fast<-1,13,3,64,Solo,1>", 21, 12, 13, cm=1),
    case("ca N=20 nr=40 generic", "generic<1>", 20, 13, 13, cm=1),
    # ---- Gaussian chance-constraint rows (CM = 2)
    case("g (5,5) N=30", "fast<5,5,2,64,Solo,2>", 30, 5, 5, S=3, gauss=True, also={"default": "compact<5,5,2,64,2>"}),
    case("g (5,5) N=30 compact", "compact<5,5,2,64,2>", 30, 5, 5, S=3, gauss=True, lab=CP0),
    case("g (5,5) N=30 two-wave", "fast<5,5,4,128,Solo,2>", 30, 5, 5, S=3, gauss=True, lab={"TMPC_NO_ONE_WAVE_N30": "1"}, also={"cp2": "compact<5,5,4,128,2>"}),
    case("g (5,5) N=30 two-wave cp2", "compact<5,5,4,128,2>", 30, 5, 5, S=3, gauss=True, lab={"TMPC_NO_ONE_WAVE_N30": "1", **CP2_0}),
    case("g <-1,6,4> nr=24 N=30", "fast<-1,6,4,128,Solo,2>", 30, 4, 6, gauss=True, also={"cp2": "compact<-1,6,4,128,2>"}),
    case("g <-1,6,4> nr=24 cp2", "compact<-1,6,4,128,2>", 30, 4, 6, gauss=True, lab=CP2_0),
    case("g <-1,12,4> nr=25 N=30", "fast<-1,12,4,128,Solo,2>", 30, 5, 6, gauss=True),
    case("g <-1,12,4> nr=48 N=32", "fast<-1,12,4,128,Solo,2>", 32, 17, 17, gauss=True),
    case("g N=30 nr=49 generic", "generic<2>", 30, 17, 18, gauss=True),
    case("g <-1,13,3> (8,8) N=20", "fast<-1,13,3,64,Solo,2>", 20, 8, 8, gauss=True, also={"default": "compact<-1,10,3,64,2>"}),
    case("g <-1,10,3> nr=30 compact", "compact<-1,10,3,64,2>", 20, 8, 8, gauss=True, lab=CP0),
    case("g <-1,13,3> nr=39 N=21", "fast<-1,13,3,64,Solo,2>", 21, 12, 13, gauss=True),
    case("g N=20 nr=40 generic", "generic<2>", 20, 13, 13, gauss=True),
    case("g m2 N=20", "fast<-1,9,6,128,ScanSolo,2>", 20, 8, 8, gauss=True, mode=2),
    case("g m2 N=30", "fast<-1,12,4,128,ScanSoloT<2>,2>", 30, 5, 5, S=3, gauss=True, mode=2),
    case("g m3 N=20", "fast<-1,4,12,256,ScanQuad,2>", 20, 8, 8, gauss=True, mode=3),
    case("g m3 N=30", "fast<-1,6,8,256,ScanQuadT<2>,2>", 30, 5, 5, S=3, gauss=True, mode=3),
    # ---- curvature-aware cost + Gaussian rows (CM = 3): the generic kernel, the four-wave kernel of 21 <= N <= 31
    case("cm3 N=30", "generic<3>", 30, 5, 5, S=3, cm=1, gauss=True),
    case("cm3 N=30 m3", "fast<-1,6,8,256,ScanQuadT<2>,3>", 30, 5, 5, S=3, cm=1, gauss=True, mode=3),
    # ---- square-root Riccati form (riccati_form = 1)
    case("sqrt <-1,13,3> N=20", "fast<-1,13,3,64,SoloSqrt,0>", 20, 8, 8, rf=1),
    case("sqrt <-1,12,4> N=30", "fast<-1,12,4,128,SoloSqrt,0>", 30, 8, 8, rf=1),
    case("sqrt ca (20,8) N=30", "fast<20,8,4,128,SoloSqrt,1>", 30, 8, 8, n_slk=12, cm=1, rf=1),
    # ---- the generic kernel past every register-row instantiation: 41 and more rows per stage, horizons 33 .. STAGE_MAX = 62, each at its entry point and
    #      at the row count where lds_doubles() reaches the 160 KB of a CU (test_gpu_parity.test_create_rejects_unsupported_dimensions: one row more is
    #      refused).  The reference is the wide build of the oracle (tests/test_oracle_wide.py)
    case("generic N=20 nr=55", "generic<0>", 20, 14, 15, n_slk=12),                  # first shape past fast<-1,9,6,128>
    case("generic N=20 nh=98 LDS cap", "generic<0>", 20, 49, 49),                    # 163,536 B; the largest row table (nrows 2230)
    case("generic N=21 nh=92 LDS cap", "generic<0>", 21, 46, 46),
    case("generic N=32 nh=50 LDS cap", "generic<0>", 32, 25, 25),
    case("generic N=32 (30,18) slack", "generic<0>", 32, 18, 18, n_slk=12),
    # doomed entries of the two cases below: chosen on the CPU, with all 16 entries doomed, so that the wide oracle gives the same exit code, QP status,
    # SQP count and interior-point count for them in all 36 of: built with and without -ffp-contract=off x either Riccati form (the kernels run the other
    # form than the oracle's default) x the inputs as they are and eight times with every parameter, warm-start value and initial state moved by a few
    # ulp (a factor 1 + 2^-50 N(0,1)).  A diverging QP ends on a pivot or a diagonal entry of P that exact arithmetic keeps positive, so its count can hang
    # on rounding: scene 1 at N = 33 has six entries on which the four builds agree (1, 6, 7, 10, 11, 13), and three that also survive the moved inputs
    # (1: QP status 2 at the limit of 50 iterations; 10, 11: status 4 after 5) -- on entry 6 the oracle itself gives 5 or 6.  At N = 62 scene 1 has one
    # entry on which the builds agree, so that case takes scene 6, which has seven (0, 1, 5, 6, 9, 11, 15), four under moved inputs too (0, 5, 9, 11:
    # status 4 after 5 iterations)
    case("generic N=33 (8,8)", "generic<0>", 33, 8, 8, doomed=(1, 10)),              # first horizon with no fast kernel
    case("generic N=33 nh=48 LDS cap", "generic<0>", 33, 24, 24),
    case("generic N=43 nh=30 LDS cap", "generic<0>", 43, 15, 15),
    case("generic N=48 (12,12)", "generic<0>", 48, 12, 12),
    case("generic N=61 (6,6)", "generic<0>", 61, 6, 6),
    case("generic N=62 (6,6) LDS cap", "generic<0>", 62, 6, 6, ids=(6,), doomed=(5, 9)),  # STAGE_MAX: lane 62 is the terminal node, lane 63 idle
    case("generic N=62 (0,4)", "generic<0>", 62, 0, 4, ids=range(50, 66)),
    case("generic N=62 (8,4) slack", "generic<0>", 62, 2, 4, n_slk=6),
    case("generic ca N=40 (8,8)", "generic<1>", 40, 8, 8, cm=1),
    case("generic g N=40 (8,8)", "generic<2>", 40, 8, 8, gauss=True),
    case("generic cm3 N=40 (5,5)", "generic<3>", 40, 5, 5, S=3, cm=1, gauss=True),
    case("m1 (8,8) N=33 refused", "generic<0>", 33, 8, 8, mode=1, refused=True),
    case("m2 (8,8) N=33 refused", "generic<0>", 33, 8, 8, mode=2, refused=True),
    case("m3 (8,8) N=33 refused", "generic<0>", 33, 8, 8, mode=3, refused=True),
    # ---- launch size, product library: the real thresholds (fast one-wave -> compact; fast two-wave -> compact two-wave), a persistent loop
    #      that wraps twice with a ragged tail
    case("B=cp_min_B (8,8) N=20", "fast<8,8,3,64,Solo,0>", 20, 8, 8, B="cp_min_B"),
    case("B=cp_min_B+1 (8,8) N=20", "compact<8,8,3,64,0>", 20, 8, 8, B="cp_min_B+1", prev="cp_min_B"),
    case("B=2*grid_max+3 (8,8) N=20", "compact<8,8,3,64,0>", 20, 8, 8, B="2*grid_max+3", prev="cp_min_B+1"),
    case("B=cp2_min_B (20,8) N=30", "fast<20,8,4,128,Solo,0>", 30, 8, 8, n_slk=12, B="cp2_min_B"),
    case("B=cp2_min_B+1 (20,8) N=30", "compact<20,8,4,128,0>", 30, 8, 8, n_slk=12, B="cp2_min_B+1", prev="cp2_min_B"),
    case("B=2*grid_max+3 (20,8) N=30", "compact<20,8,4,128,0>", 30, 8, 8, n_slk=12, B="2*grid_max+3", prev="cp2_min_B+1"),
    # ---- a disc offset: the coupled W (MIRROR's 7 x 7 iteration) of the plain cost, on every form of the linearisation -- two waves, four waves in both
    #      horizon ranges, one wave (mirror7_pair), two waves with the compact layout
    case("offset <-1,9,4> nr=25 N=22", "fast<-1,9,4,128,Solo,0>", 22, 5, 6, disc_offset=0.1),
    case("offset m3 <-1,4,12> nr=39 N=5", "fast<-1,4,12,256,ScanQuad,0>", 5, 12, 13, mode=3, disc_offset=0.1),
    case("offset m3 (8,8) N=21", "fast<-1,6,8,256,ScanQuadT<2>,0>", 21, 8, 8, mode=3, disc_offset=0.1),
    case("offset (8,8) N=5", "fast<8,8,3,64,Solo,0>", 5, 8, 8, disc_offset=0.1),
    case("offset <-1,9,4> nr=25 N=22 cp2", "compact<-1,9,4,128,0>", 22, 5, 6, lab=CP2_0, disc_offset=0.1),
]

# instantiations the pick functions name that no case above reaches
EXCLUDED = {
    "fast<tmpc_gen::NH,0,3,64,Solo,0>": "generated solvers only (-DTMPC_GENERATED_STAGE): test_gpu_parity.py test_generated_* and test_codegen",
    "fast<tmpc_gen::NH,0,4,128,Solo,0>": "generated solvers only (-DTMPC_GENERATED_STAGE): test_gpu_parity.py test_generated_* and test_codegen",
}

def case_names(c):
    return {c["expect"], *c["also"].values()}


def expected_names(cases=None):
    out = set()
    for c in DISPATCH_CASES if cases is None else cases:
        out |= case_names(c)
    return out


def _slots(info):
    """{slot: instantiation} and the launch-size thresholds from tmpc_kernel_info."""
    slots = dict(kv.split("=", 1) for kv in info.split("; kernels: ")[1].split(", "))
    num = lambda pat: int(re.search(pat, info).group(1)) if re.search(pat, info) else 0
    th = dict(cp_min_B=num(r"launches of at most (\d+) "), cp2_min_B=num(r"launches of more than (\d+) "), grid_max=num(r"resident workgroups (\d+)"))
    return slots, th


def _running(slots, mode, B, th):
    """The slot a launch of B trajectories in `mode` runs (launch_slot in csrc/tmpc_capi.hip)."""
    if mode == 3 and "lat3" in slots:
        return "lat3"
    if mode >= 2 and "lat2" in slots:
        return "lat2"
    if mode >= 1 and "lat1" in slots:
        return "lat1"
    if "cp2" in slots and B > th["cp2_min_B"]:
        return "cp2"
    if "small" in slots and B <= th["cp_min_B"]:
        return "small"
    return "default"


def _dims(c):
    from mpc_planner_amd import solver
    return solver.default_dims(N=c["N"], S=c["S"], n_lin=c["n_lin"], M=c["M"], n_slk=c["n_slk"], slack=int(c["n_slk"] > 0),
                               cost_model=c["cm"], row_model=int(c["gauss"]), riccati_form=c["rf"])


def _problem(c):
    import oracle_lib as O
    assert c["N"] <= O.WIDE_N and c["n_lin"] + c["n_slk"] + c["M"] <= O.WIDE_NH, "more stages or rows per stage than the wide oracle holds"
    M, ng = (0, c["M"]) if c["gauss"] else (c["M"], 0)
    return O.problem(N=c["N"], S=c["S"], n_lin=c["n_lin"], M=M, n_slk=c["n_slk"], slack=int(c["n_slk"] > 0), n_gauss=ng, cost_model=c["cm"],
                     riccati_form=c["rf"])


def _scenes(c, B):
    """B trajectories of the case's row mix: scenes with M obstacles (topology rows of the first n_lin kept, as in
    test_gpu_parity.test_runtime_shape_fast_kernels_match_oracle), n_slk decomposition rows with the slack model."""
    from mpc_planner_amd import scenes
    if c["scene"] is not None:
        skw = dict(c["scene"])
    else:
        skw = dict(M=c["M"], S=c["S"], chance=c["gauss"], guidance=c["n_lin"] > 0)
        if c["n_slk"]:
            skw.update(slack=True, n_decomp=c["n_slk"])
    ids = list(c["ids"])
    per = 1 if not skw.get("guidance", True) else max(1, min(64, -(-B // len(ids))))
    while len(ids) * per < B:
        ids.append(ids[-1] + 1 + len(ids))
    sc = scenes.make_batch(ids, N=c["N"], B=per, **skw)
    sc = {k: sc[k][:B] for k in ("xinit", "x0", "params")} | {"pm": sc["pm"]}
    assert sc["xinit"].shape[0] == B
    if c["disc_offset"]:
        sc["params"] = sc["params"].copy()
        sc["offset_col"] = sc["pm"].index("ego_disc_0_offset")
        sc["params"][:, :, sc["offset_col"]] = c["disc_offset"]
    if c["doomed"]:
        from test_gpu_parity import _make_infeasible
        sc = _make_infeasible(sc, list(c["doomed"]))
    if c["scene"] is None and c["n_lin"] < c["M"] and c["n_lin"] > 0:
        drop = tuple(f"lin_constraint_{j}_" for j in range(c["n_lin"], c["M"]))
        keep = [i for n, i in sc["pm"]._params.items() if not n.startswith(drop)]
        sc["params"] = np.ascontiguousarray(sc["params"][:, :, keep])
        if "offset_col" in sc:
            sc["offset_col"] = keep.index(sc["offset_col"])
    return sc


def _profiled_twins():
    from test_dispatch_table import pick_instantiations
    return {n for n, (macro, _) in pick_instantiations().items() if macro in ("TMPC_FAST", "TMPC_FASTP")}


def _solve(s, sc, lo=0, hi=None):
    s.set_batch(sc["xinit"][lo:hi], sc["x0"][lo:hi], sc["params"][lo:hi]); s.solve()
    return s.get()


def _b(c, th):
    return c["B"] if isinstance(c["B"], int) else int(eval(c["B"], {}, dict(th)))


@pytest.mark.parametrize("c", DISPATCH_CASES, ids=[c["id"] for c in DISPATCH_CASES])
def test_dispatch_case(c, request, monkeypatch):
    import oracle_lib as O
    from mpc_planner_amd import solver
    from test_gpu_parity import _check_selection, _compare, _compare_relaxed_iterations
    if c["lab"]:
        for k, v in c["lab"].items():
            monkeypatch.setenv(k, v)
        request.getfixturevalue("lab_library")
    dims = _dims(c)
    probe = solver.BatchedSolver(dims, B_max=1)                   # the thresholds the launch-size cases are made of
    _, th = _slots(probe.kernel_info()); probe.close()
    B = _b(c, th)
    assert B > 0, (c["B"], th)
    s = solver.BatchedSolver(dims, B_max=B)
    assert s.set_latency_mode(c["mode"]) == (not c["refused"]) or c["mode"] == 0
    slots, th = _slots(s.kernel_info())
    slot = _running(slots, c["mode"], B, th)
    # (a) the instantiation that runs, and the other slots the case names
    assert slots.get(slot) == c["expect"], (slot, slots)
    for k, v in c["also"].items():
        assert slots.get(k) == v, (k, slots)
    if c["refused"]:
        assert slot in ("default", "small"), (slot, slots)
    sc = _scenes(c, B)
    assert sc["params"].shape[2] == s.npar
    got = _solve(s, sc)
    # (b) against the oracle
    pb = _problem(c)
    assert pb.npar == s.npar
    xt, ut, info = O.solve_batch(pb, sc["xinit"], sc["x0"].reshape(B, -1), sc["params"].reshape(B, -1))
    ok = info["exit_code"] == 1
    if slot == "lat2":
        _compare_relaxed_iterations(got, xt, ut, info)
        same = ok & (got["qp_iter_total"] == info["qp_iter_total"])
        sx = np.maximum(np.abs(xt[same]).max(axis=2, keepdims=True), 1.0); su = np.maximum(np.abs(ut[same]).max(axis=2, keepdims=True), 1.0)
        worst = max((np.abs(got["xtraj"][same] - xt[same]) / sx).max(initial=0.0), (np.abs(got["utraj"][same] - ut[same]) / su).max(initial=0.0))
        assert worst < 1e-8, worst
    else:
        worst = max(_compare(got, xt, ut, info))
    _check_selection(s.select_best(), got, info)
    for b in c["doomed"]:                                           # the failure verdicts (_compare: exit code and SQP count of every entry)
        print(f"[dispatch] {c['id']}: doomed entry {b}: (exit code, QP status, SQP count, interior-point count) kernel "
              f"{tuple(int(got[f][b]) for f in VERDICT)} oracle {tuple(int(info[f][b]) for f in VERDICT)}")
    for b in c["doomed"]:
        assert info["exit_code"][b] != 1 and got["qp_status"][b] == info["qp_status"][b], (b, info["exit_code"][b], got["qp_status"][b], info["qp_status"][b])
        assert got["qp_iter_total"][b] == info["qp_iter_total"][b], (b, got["qp_iter_total"][b], info["qp_iter_total"][b])
    if c["disc_offset"]:
        # The offset reaches the kernel: the zero-offset solve of the same batch gives other bits.  No bound on the size of the change: at N = 5 no obstacle of the
        # scenes is within reach, the rows' multipliers stay near zero and the offset moves the result at rounding level only (2e-16, the oracle likewise) -- the
        # cross entries of W are non-zero all the same, which is all MIRROR's `coupled` test asks; at N = 21, 22 it moves the trajectories by tenths of a metre.
        zero = sc["params"].copy()
        assert (zero[:, :, sc["offset_col"]] == c["disc_offset"]).all()
        zero[:, :, sc["offset_col"]] = 0.0
        s.set_batch(sc["xinit"], sc["x0"], zero); s.solve()
        moved = np.abs(s.get()["xtraj"][ok] - got["xtraj"][ok]).max()
        print(f"[dispatch] {c['id']}: the offset moves the trajectories by {moved:.2e}")
        assert moved > 0.0
        got2 = _solve(s, sc)
        for f in FIELDS:
            assert np.array_equal(got2[f], got[f]), f
    # (c) the parity check is not made on nothing
    assert ok.sum() >= B / 2, (int(ok.sum()), B)
    # (d) launch to launch
    s.solve(); again = s.get()
    for k in FIELDS:
        assert np.array_equal(again[k], got[k]), k
    # (e) batch independence: the first k alone (launch-size cases: the previous size, the other side of the threshold)
    k = _b(dict(B=c["prev"]), th) if c["prev"] else max(1, min(4, B // 2))
    if k < B:
        part = _solve(s, sc, 0, k)
        for f in FIELDS:
            assert np.array_equal(part[f], got[f][:k]), (f, k)
        got = _solve(s, sc)
    # tmpc_debug_profile: the profiled twin of what runs, or a refusal; either way the handle keeps solve()'s results
    twin = slots.get("small") if slot in ("default", "small") and "small" in slots else (slots["default"] if slot == "cp2" else slots[slot])
    allowed = twin.startswith("generic<") and slot == "default" or twin in _profiled_twins()
    if allowed:
        ph = s.debug_profile()
        assert ph["total"] > 0 and all(v >= 0 for v in ph.values()) and sum(v for n, v in ph.items() if n != "total") > 0, ph
    else:
        with pytest.raises(solver.TmpcError):
            s.debug_profile()
    after = s.get()
    for f in FIELDS:
        assert np.array_equal(after[f], got[f]), f
    s.close()
    print(f"[dispatch] {c['id']}: {slot}={c['expect']} B {B} successes {int(ok.sum())}/{B} worst rel diff {worst:.2e} profile {'twin' if allowed else 'refused'}")
