"""ctypes binding of the C-ABI (include/tmpc_hip.h, libtmpc_hip.so) + the batched host-side solver object.

`BatchedSolver` is the batch-first counterpart of the reference's `MPCPlanner::Solver`
(mpc_planner_solver/include/mpc_planner_solver/acados_solver_interface.h:93-222): B solver instances'
`_params` (xinit / x0 / all_parameters) in, `_output` (xtraj / utraj) and `_info` out, with the reference's
exit-code convention.  There is NO CPU fallback: if the HIP library or a GPU is missing, construction raises.
"""
import ctypes as C
import os

import numpy as np

from . import _binding
from ._binding import TmpcError, _pointer  # noqa: F401  (solver.TmpcError, solver._pointer: the names callers and tests use)

NU, NX, NV = 2, 5, 7
_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TMPC_HIP_LIBRARY") or os.path.join(_HERE, "libtmpc_hip.so")     # (TMPC_HIP_LIBRARY: lab switch, an A/B build of the same C-ABI)
# The same kernels behind a C-ABI unit built with -DTMPC_LAB_SWITCHES: the only library that reads the TMPC_* kernel-selection overrides from the environment
# (tests that have to reach one kernel family, A/B tools).  The product library (LIB_PATH) ignores the environment.
LAB_LIB_PATH = os.path.join(_HERE, "libtmpc_hip_lab.so")


class TmpcDims(C.Structure):
    _fields_ = [("N", C.c_int32), ("S", C.c_int32), ("n_lin", C.c_int32), ("M", C.c_int32), ("npar", C.c_int32),
                ("n_sqp", C.c_int32), ("qp_iter_max", C.c_int32), ("erk_steps", C.c_int32),
                ("dt", C.c_double), ("qp_tol", C.c_double), ("reg_eps", C.c_double), ("ipm_mu0", C.c_double),
                ("ipm_thr0", C.c_double), ("lb", C.c_double * NV), ("ub", C.c_double * NV),
                ("n_slk", C.c_int32), ("slack", C.c_int32), ("cost_model", C.c_int32), ("row_model", C.c_int32),
                ("riccati_form", C.c_int32)]        # 0: Schur-complement recursion (default), 1: square-root recursion (include/tmpc_hip.h)

    @property
    def nx(self):            # external (model) state / variable counts: the slack model has one more state
        return NX + self.slack

    @property
    def nvar(self):
        return NV + self.slack

    @property
    def nh(self):
        return self.n_lin + self.M + self.n_slk


class TmpcObstacleOptions(C.Structure):
    """tmpc_obstacle_options (include/tmpc_hip.h)."""
    _fields_ = [("size", C.c_uint32), ("probabilistic", C.c_int32), ("propagate_passes", C.c_int32), ("reserved", C.c_int32),
                ("noise", C.c_double), ("max_obstacle_distance", C.c_double)]


class TmpcPathOptions(C.Structure):
    """tmpc_path_options (include/tmpc_hip.h)."""
    _fields_ = [("size", C.c_uint32), ("search_range", C.c_int32), ("window_segments", C.c_int32)]


class TmpcGuidanceOptions(C.Structure):
    """tmpc_guidance_options (include/tmpc_hip.h)."""
    _fields_ = [("size", C.c_uint32), ("n_paths", C.c_int32), ("use_tmpcpp", C.c_int32), ("warmstart_with_mpc_solution", C.c_int32),
                ("shift_previous_solution_forward", C.c_int32), ("reserved", C.c_int32), ("selection_weight_consistency", C.c_double)]


def guidance_options(n_paths, use_tmpcpp=True, warmstart_with_mpc_solution=False, shift_previous_solution_forward=True,
                     selection_weight_consistency=1.0):
    """A filled tmpc_guidance_options for BatchedSolver.guidance_plan / guidance_decide."""
    return TmpcGuidanceOptions(C.sizeof(TmpcGuidanceOptions), int(n_paths), int(bool(use_tmpcpp)), int(bool(warmstart_with_mpc_solution)),
                               int(bool(shift_previous_solution_forward)), 0, float(selection_weight_consistency))


_int, _i32, _u32, _u64, _f64, _vp = C.c_int, C.c_int32, C.c_uint32, C.c_uint64, C.c_double, C.c_void_p
_dims_p, _obstacle_p, _path_p, _guidance_p = C.POINTER(TmpcDims), C.POINTER(TmpcObstacleOptions), C.POINTER(TmpcPathOptions), C.POINTER(TmpcGuidanceOptions)

# The Python side of include/tmpc_hip.h, in the header's order: name -> (restype, argtypes).  Everything else follows from this table: EXPORTS,
# what load_library() sets on the library, how BatchedSolver._call() converts its arguments.  tests/test_binding_signatures.py holds it against
# the header's prototypes.  _vp: the handle and every data pointer (an integer address, a ctypes object or None = NULL).
_SIGNATURES = {
    "tmpc_default_dims": (None, [_dims_p, _i32, _i32, _i32, _i32]),
    "tmpc_default_dims_ex": (None, [_dims_p] + [_i32] * 6),
    "tmpc_create": (_int, [C.POINTER(_vp), _dims_p, _i32, _i32]),
    "tmpc_create_v2": (_int, [C.POINTER(_vp), _dims_p, _u32, _i32, _i32]),
    "tmpc_destroy": (None, [_vp]),
    "tmpc_last_error": (C.c_char_p, [_vp]),
    "tmpc_set_batch": (_int, [_vp, _i32, _vp, _vp, _vp]),
    "tmpc_set_batch_device": (_int, [_vp, _i32, _vp, _vp, _vp]),
    "tmpc_solve": (_int, [_vp]),
    "tmpc_synchronize": (_int, [_vp]),
    "tmpc_solve_iterations": (_int, [_vp, _i32, _i32]),
    "tmpc_set_slots": (_int, [_vp, _vp]),
    "tmpc_set_param_sharing": (_int, [_vp, _vp]),
    "tmpc_set_param_sharing_ex": (_int, [_vp, _vp, _i32]),
    "tmpc_copy_state": (_int, [_vp, _vp]),
    "tmpc_clear_slot": (_int, [_vp, _i32]),
    "tmpc_reset_multipliers": (_int, [_vp]),
    "tmpc_set_latency_mode": (_int, [_vp, _i32]),
    "tmpc_latency_mode_capacity": (_int, [_vp, _i32]),
    "tmpc_set_throughput_mode": (_int, [_vp, _i32]),
    "tmpc_has_lane_kernels": (_int, []),
    "tmpc_get": (_int, [_vp] + [_vp] * 8),
    "tmpc_select_best": (_int, [_vp, _i32, _i32, _vp, _vp, C.POINTER(_i32)]),
    "tmpc_result_device_ptrs": (_int, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "tmpc_get_stream": (_int, [_vp, C.POINTER(_vp)]),
    "tmpc_kernel_info": (_int, [_vp, C.c_char_p, _i32]),
    "tmpc_pack_records": (_int, [_vp, _vp, _vp, _vp]),
    "tmpc_select_best_records": (_int, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "tmpc_gather_best": (_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp]),
    "tmpc_enable_timing": (_int, [_vp, _i32]),
    "tmpc_get_timings": (_int, [_vp, _vp, _i32, C.POINTER(_i32)]),
    "tmpc_time_solve": (_int, [_vp, _i32, _vp]),
    "tmpc_linearize_topology": (_int, [_vp, _vp, _vp, _vp, _f64, _vp]),
    "tmpc_linearize_topology_ex": (_int, [_vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _f64, _vp]),
    "tmpc_road_halfspaces": (_int, [_vp, _vp, _i32, _vp, _f64, _f64, _vp, _i32, _i32]),
    "tmpc_prepare_obstacles": (_int, [_vp, _i32, _i32, _i32] + [_vp] * 6 + [_obstacle_p] + [_vp] * 5),
    "tmpc_set_obstacle_parameters": (_int, [_vp] + [_vp] * 6 + [_f64] * 5),
    "tmpc_track_path": (_int, [_vp, _i32, _i32] + [_vp] * 5 + [_i32, _path_p] + [_vp] * 5),
    "tmpc_set_path_parameters": (_int, [_vp, _vp, _vp, _i32, _vp, _vp]),
    "tmpc_path_velocity_window": (_int, [_vp, _i32, _i32, _i32] + [_vp] * 7 + [_f64, _vp, _vp]),
    "tmpc_scatter_parameters": (_int, [_vp, C.POINTER(_i32), _i32, _vp, _i32, _vp, _i32]),
    "tmpc_fit_path": (_int, [_vp, _i32, _i32, _i32] + [_vp] * 13),
    "tmpc_costmap_points": (_int, [_vp, _i32, _i32, _i32, _vp, _vp, _f64, _i32, _vp, _vp, _vp]),
    "tmpc_decomp_halfspaces": (_int, [_vp, _vp, _i32, _i32] + [_vp] * 7 + [_i32, _f64, _i32, _vp, _vp, _vp]),
    "tmpc_set_halfspace_rows": (_int, [_vp, _vp, _i32, _i32, _vp, _i32, _f64]),
    "tmpc_scenario_halfspaces": (_int, [_vp, _vp, _i32, _i32, _vp, _vp, _f64, _f64]),
    "tmpc_scenario_support": (_int, [_vp, _i32, _f64, _vp, _vp]),
    "tmpc_sample_scenarios": (_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _u64, _vp]),
    "tmpc_scenario_discard": (_int, [_vp, _vp, _i32, _i32, _i32, _vp, _f64]),
    "tmpc_scenario_discarded": (_int, [_vp, _vp]),
    "tmpc_scenario_empty_stages": (_int, [_vp, _vp]),
    "tmpc_warmstart": (_int, [_vp, _vp, _vp, _vp, _f64]),
    "tmpc_init_with_guidance": (_int, [_vp, _vp, _vp, _vp]),
    "tmpc_sample_guidance": (_int, [_vp, _i32, _i32] + [_vp] * 5),
    "tmpc_guidance_plan": (_int, [_vp, _i32, _guidance_p] + [_vp] * 12),
    "tmpc_guidance_decide": (_int, [_vp, _i32, _guidance_p] + [_vp] * 6 + [_f64, _f64, _i32] + [_vp] * 5),
    "tmpc_debug_get_x0": (_int, [_vp, _vp, _vp]),
    "tmpc_debug_get_params": (_int, [_vp, _vp]),
    "tmpc_debug_profile": (_int, [_vp, _vp, _i32]),
    "tmpc_debug_lds_passes": (_int, [_i32] * 5),
    "tmpc_debug_poison_lds": (_int, [_vp]),
    "tmpc_has_lab_switches": (_int, []),
    "tmpc_debug_eval_stage": (_int, [_vp, _i32] + [_vp] * 13),
}
EXPORTS = list(_SIGNATURES)

_CONVERT = _binding.converters(_SIGNATURES)      # per function, how BatchedSolver._call() converts each argument behind the handle


def has_lane_kernels(lib_path=None):
    """Does this build of the library carry the optional lane-per-trajectory kernels (tmpc_set_throughput_mode)?"""
    return load_library(lib_path).tmpc_has_lane_kernels() == 1


_libs = {}


def load_library(path=None):
    """Load libtmpc_hip.so -- or a generated per-configuration library with the same C-ABI (mpc_planner_amd/codegen) --;
    raises (never falls back) if it has not been built."""
    path = os.path.abspath(path) if path else LIB_PATH
    if path in _libs:
        return _libs[path]
    try:
        # If torch is going to be used in this process (device buffers, torch.distributed) its bundled HIP runtime must be the
        # one that gets loaded: libtmpc_hip.so resolves the same libamdhip64 SONAME, and whichever is loaded first serves both.
        # Loading the system runtime first has been seen to leave torch without devices ("No HIP GPUs are available").
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(path):
        raise TmpcError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(path)
    _binding.bind(lib, _SIGNATURES)
    _libs[path] = lib
    return lib


def default_dims(N=20, S=5, n_lin=8, M=8, n_slk=0, slack=0, lib_path=None, **opts):
    """lib_path: a generated library (its row / parameter structure overrides n_lin, M, n_slk, slack)."""
    d = TmpcDims()
    load_library(lib_path).tmpc_default_dims_ex(C.byref(d), N, S, n_lin, M, n_slk, int(bool(slack)))
    for k, v in opts.items():
        setattr(d, k, v)
    if d.row_model == 1 and "npar" not in opts:              # Gaussian rows: 6 parameters per obstacle instead of the ellipsoid's 7
        d.npar -= d.M
    return d


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def own_parameter_columns(dims):
    """Indices (within a stage's parameter row) of the entries a planner of a guidance / scenario set sets for itself: the topology
    halfspaces (LinearizedConstraints::setParameters) and the scenario / decomp halfspaces (csrc/tmpc_stage.hpp ip_lin, ip_slk)."""
    base = 8 + dims.slack + 9 * dims.S
    lin = np.arange(base, base + 3 * dims.n_lin)
    disc = base + 3 * dims.n_lin
    slk0 = (disc + 2 + (6 if dims.row_model == 1 else 7) * dims.M) if dims.M > 0 else disc + 1
    return np.concatenate([lin, np.arange(slk0, slk0 + 3 * dims.n_slk)]).astype(int)


def param_sharing_map(params, dims, set_size):
    """base_of for tmpc_set_param_sharing: consecutive groups of `set_size` batch entries (one guidance set each) share the rows of
    their first entry -- CHECKED here: an entry whose shared columns differ from its set's first entry keeps its own rows."""
    B = params.shape[0]
    p = params.reshape(B, dims.N, -1)
    mask = np.ones(p.shape[2], bool); mask[own_parameter_columns(dims)] = False
    out = np.arange(B, dtype=np.int32)
    for s0 in range(0, B, set_size):                                          # set by set: no batch-sized temporaries
        blk = p[s0:s0 + set_size]
        same = (blk[:, :, mask] == blk[0][None, :, mask]).all(axis=(1, 2))
        out[s0:s0 + set_size][same] = s0
    return out


class BatchedSolver:
    """B reference `Solver` instances behind one HIP launch."""

    def __init__(self, dims, B_max, device=0, lib_path=None):
        self.lib = load_library(lib_path)
        self.dims = dims
        self.B_max = int(B_max)
        self.B = 0
        self.device = int(device)
        self._h = C.c_void_p()
        rc = self.lib.tmpc_create(C.byref(self._h), C.byref(dims), self.B_max, int(device))
        if rc != 0:
            why = self.lib.tmpc_last_error(None).decode()          # (no handle: the refusal's message, where it has one)
            raise TmpcError(f"tmpc_create failed with code {rc} (-1 invalid dims, -2 HIP error, -3 no gfx950 device)" + ("" if why == "null handle" else f": {why}"))
        self.N, self.npar = dims.N, dims.npar

    def close(self):
        if self._h:
            self.lib.tmpc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        _binding.check(self.lib, self._h, rc, what)

    def _invoke(self, name, *args):
        """The one path into the library: entry `name` of _SIGNATURES on this handle, every argument converted as its type in the table
        says; returns the entry's code as it is (for the entries whose non-negative return is a value)."""
        return _binding.invoke(self.lib, self._h, name, _CONVERT, args)

    def _call(self, name, *args):
        """_invoke, and a non-zero code raises with the library's message."""
        self._check(self._invoke(name, *args), name)

    # --- inputs -----------------------------------------------------------------------------------
    def set_batch(self, xinit, x0, params):
        """Host arrays: xinit [B][nx], x0 [B][N+1][nvar], params [B][N][npar] (reference layouts; nx, nvar = 5, 7 or,
        with the slack model, 6, 8)."""
        xinit = np.ascontiguousarray(xinit, np.float64); x0 = np.ascontiguousarray(x0, np.float64)
        params = np.ascontiguousarray(params, np.float64)
        B = xinit.shape[0]
        if xinit.shape != (B, self.dims.nx) or x0.size != B * (self.N + 1) * self.dims.nvar \
                or params.size != B * self.N * self.npar:
            raise ValueError(f"set_batch: expected xinit [{B}][{self.dims.nx}], x0 [{B}][{self.N + 1}][{self.dims.nvar}], "
                             f"params [{B}][{self.N}][{self.npar}]; got {xinit.shape}, {x0.shape}, {params.shape}")
        self._keep = (xinit, x0, params)
        self._call("tmpc_set_batch", B, _p(xinit), _p(x0), _p(params))
        self.B = B

    def set_batch_device(self, B, d_xinit, d_x0, d_params):
        """Raw device pointers (ints), inputs already resident in HBM."""
        self._call("tmpc_set_batch_device", B, d_xinit, d_x0, d_params)
        self.B = int(B)

    # --- solve ------------------------------------------------------------------------------------
    def solve(self, sync=True):
        self._call("tmpc_solve")
        if sync:
            self._call("tmpc_synchronize")

    def set_latency_mode(self, on=True):
        """Kernel variant for small control ticks: True / 1 = two waves per trajectory, 2 = the Newton systems solved parallel in time
        (csrc/tmpc_scan.hpp), 3 = four waves per trajectory (round 6: the parallel-in-time solve with its wide phases, the stage evaluation and the
        row passes on 256 lanes; N <= 20), False / 0 = the throughput kernels; returns False if the shape has no such variant."""
        rc = self._invoke("tmpc_set_latency_mode", on)
        if rc < 0:
            self._check(rc, "tmpc_set_latency_mode")
        return rc == 0

    KEEP_ITERATE, KEEP_MULTIPLIERS, COMPLETE, NEW_SOLVE = 1, 2, 4, 8

    def solve_iterations(self, n_iter, keep_iterate=False, keep_multipliers=False, complete=True, sync=True, new_solve=False):
        """n_iter RTI iterations per trajectory slot from the state the handle keeps (tmpc_solve_iterations): the reference's
        initializeOneIteration / solveOneIteration / completeOneIteration protocol and multipliers carried across ticks."""
        flags = (self.KEEP_ITERATE if keep_iterate else 0) | (self.KEEP_MULTIPLIERS if keep_multipliers else 0) | (self.COMPLETE if complete else 0) \
            | (self.NEW_SOLVE if new_solve else 0)      # new_solve: first call of a new Solver::solve(): loop exits of the previous solve do not carry over
        self._call("tmpc_solve_iterations", n_iter, flags)
        if sync:
            self.synchronize()

    def set_slots(self, slots):
        """State slot of every entry of the current batch (tmpc_set_slots); None: entry b uses slot b."""
        if slots is None:
            self._call("tmpc_set_slots", None)
            return
        a = np.ascontiguousarray(slots, np.int32)
        assert a.size == self.B
        self._call("tmpc_set_slots", _p(a))

    def set_param_sharing(self, base_of, copies_not_maintained=False):
        """Hint (tmpc_set_param_sharing): entry b's parameter rows equal entry base_of[b]'s except for its own topology / scenario
        halfspace rows; the kernels read the rest from base_of[b] (same results, 1/64 of a guidance set's parameter traffic).  None clears.
        copies_not_maintained (tmpc_set_param_sharing_ex, TMPC_SHARE_COPIES_NOT_MAINTAINED): the caller writes a set's shared rows into the base
        entry only; every path that would read the other entries' copies then fails instead of falling back."""
        if base_of is None:
            self._call("tmpc_set_param_sharing", None)
            return
        a = np.ascontiguousarray(base_of, np.int32)
        assert a.size == self.B
        self._call("tmpc_set_param_sharing_ex", _p(a), 1 if copies_not_maintained else 0)

    def latency_mode_capacity(self, mode):
        """Trajectories one launch of kernel variant `mode` holds resident on this device (tmpc_latency_mode_capacity); 0: no such variant."""
        rc = self._invoke("tmpc_latency_mode_capacity", mode)
        if rc < 0:
            self._check(rc, "tmpc_latency_mode_capacity")
        return rc

    def clear_slot(self, slot):
        """Forget one slot's persistent state (tmpc_clear_slot): the slot's next solve_iterations starts like a fresh capsule."""
        self._call("tmpc_clear_slot", slot)

    def copy_state_from(self, other):
        self._call("tmpc_copy_state", other._h)

    def debug_poison_lds(self):
        """Test aid: fill every CU's LDS with NaN bit patterns (tmpc_debug_poison_lds): a kernel that reads a word it never wrote shows."""
        self._call("tmpc_debug_poison_lds")

    def kernel_info(self):
        """Which solve kernel the handle dispatches and how it is launched (text)."""
        buf = C.create_string_buffer(2048)
        n = self._invoke("tmpc_kernel_info", buf, 2048)
        return buf.value.decode() if n >= 0 else ""

    def stream_ptr(self):
        """hipStream_t of the handle (as an integer), e.g. for torch.cuda.ExternalStream."""
        st = C.c_void_p()
        self._call("tmpc_get_stream", C.byref(st))
        return st.value or 0

    def reset_multipliers(self):
        self._call("tmpc_reset_multipliers")

    def set_throughput_mode(self, on=True):
        """Lane-per-trajectory kernels for large batches (allocates the HBM workspace for B_max trajectories on first use)."""
        self._call("tmpc_set_throughput_mode", bool(on))

    def synchronize(self):
        self._call("tmpc_synchronize")

    def time_solve(self, reps):
        ms = np.zeros(reps, np.float32)
        self._call("tmpc_time_solve", reps, _p(ms))
        return ms

    # --- outputs ----------------------------------------------------------------------------------
    def get(self):
        B, N = self.B, self.N
        out = dict(xtraj=np.zeros((B, N + 1, self.dims.nx)), utraj=np.zeros((B, N, NU)), pobj=np.zeros(B),
                   exit_code=np.zeros(B, np.int32), qp_status=np.zeros(B, np.int32), sqp_iter=np.zeros(B, np.int32),
                   res_eq=np.zeros(B), qp_iter_total=np.zeros(B, np.int32))
        self._call("tmpc_get", *[_p(out[k]) for k in ("xtraj", "utraj", "pobj", "exit_code", "qp_status", "sqp_iter", "res_eq", "qp_iter_total")])
        return out

    def select_best(self, first=0, count=None, weight=None, disabled=None):
        count = self.B - first if count is None else count
        w = None if weight is None else np.ascontiguousarray(weight, np.float64)
        dis = None if disabled is None else np.ascontiguousarray(disabled, np.uint8)
        best = C.c_int32(-2)
        self._call("tmpc_select_best", first, count, _p(w), _p(dis), C.byref(best))
        return best.value

    def enable_timing(self, max_records):
        self._call("tmpc_enable_timing", max_records)

    def get_timings(self, capacity=4096):
        ms = np.zeros(capacity, np.float32); n = C.c_int32(0)
        self._call("tmpc_get_timings", _p(ms), capacity, C.byref(n))
        return ms[:n.value].copy()

    def pack_records(self, d_records, d_guidance_id=None, d_weight=None):
        """d_*: raw device pointers (ints). Packs {f64 objective, i32 exit_code, i32 guidance_id} per trajectory."""
        self._call("tmpc_pack_records", d_records, d_guidance_id, d_weight)

    def select_best_records(self, d_records, n_ranks, n_scenes, per_rank, d_best):
        self._call("tmpc_select_best_records", d_records, n_ranks, n_scenes, per_rank, d_best)

    def gather_best(self, d_best, n_sets, set_size, d_xtraj, d_utraj, index_offset=0):
        """The winners' trajectories of every set in one compact device buffer (tmpc_gather_best; raw device pointers)."""
        self._call("tmpc_gather_best", d_best, n_sets, set_size, index_offset, d_xtraj, d_utraj)

    def linearize_topology(self, d_obstacle_pos, d_scene_of, d_state_x, robot_radius, d_is_original=None):
        """Device LinearizedConstraints::update + setParameters (raw device pointers); modifies the batch params in place."""
        self._call("tmpc_linearize_topology", d_obstacle_pos, d_scene_of, d_state_x, robot_radius, d_is_original)

    def linearize_topology_ex(self, d_obstacle_pos, n_obstacles, d_scene_of, d_state_x, robot_radius, d_obstacle_radius=None,
                              d_static_halfspaces=None, n_static=0, d_is_original=None):
        """The whole of LinearizedConstraints::update / setParameters on device (tmpc_linearize_topology_ex): fewer obstacles than rows,
        static halfspace rows (`add_halfspaces`), per-obstacle radii (the `_use_guidance == false` branch)."""
        self._call("tmpc_linearize_topology_ex", d_obstacle_pos, n_obstacles, d_obstacle_radius, d_static_halfspaces, n_static, d_scene_of, d_state_x,
                   robot_radius, d_is_original)

    def road_halfspaces(self, d_main_of, n_scenes, offset_first, offset_second, d_static_halfspaces, n_static, first_row=0,
                        d_bound_segments=None):
        """Contouring's road constraints on device (tmpc_road_halfspaces; raw device pointers): rows first_row, first_row + 1 of
        d_static_halfspaces [n_scenes][N][n_static][3] -- the buffer linearize_topology_ex reads -- from the warm start and path window of batch
        entry d_main_of[scene].  d_bound_segments None: centreline mode, offsets = modules.road_offsets(width, radius, two_way); else
        [n_scenes][2][S][8] left / right bound cubics and offsets = (radius, radius).  Stream-ordered, no synchronisation."""
        self._call("tmpc_road_halfspaces", d_main_of, n_scenes, d_bound_segments, offset_first, offset_second, d_static_halfspaces, n_static, first_row)

    def prepare_obstacles(self, n_scenes, n_slots, max_obstacles, d_count, d_state, d_raw_pos, d_raw_radius, d_obstacle_pos, d_obstacle_shape,
                          d_obstacle_radius, d_obstacle_gaussian, d_selected, d_raw_vel=None, d_raw_pred=None, probabilistic=False, noise=0.3,
                          propagate_passes=0, max_obstacle_distance=0.0):
        """Obstacle preparation on device (tmpc_prepare_obstacles; raw device pointers): per scene the raw list d_raw_pos / d_raw_radius
        [n_scenes][n_slots] (d_count of them) with velocities d_raw_vel or given predictions d_raw_pred becomes exactly max_obstacles prepared
        obstacles -- distance filter, closest-M selection or dummies, uncertainty passes -- in d_obstacle_pos [n_scenes][M][N][2] (what
        linearize_topology_ex reads), d_obstacle_shape [..][N][3], d_obstacle_radius, d_obstacle_gaussian (u8), d_selected (i32) [n_scenes][M].
        Equal bit for bit to modules.prepare_obstacles.  Needs no batch.  Stream-ordered, no synchronisation."""
        opt = TmpcObstacleOptions(C.sizeof(TmpcObstacleOptions), int(probabilistic), int(propagate_passes), 0, float(noise),
                                  float(max_obstacle_distance))
        self._call("tmpc_prepare_obstacles", n_scenes, n_slots, max_obstacles, d_count, d_state, d_raw_pos, d_raw_radius, d_raw_vel, d_raw_pred,
                   C.byref(opt), d_obstacle_pos, d_obstacle_shape, d_obstacle_radius, d_obstacle_gaussian, d_selected)

    def set_obstacle_parameters(self, d_obstacle_pos, d_obstacle_shape, d_obstacle_radius, d_obstacle_gaussian, d_scene_of, d_state, robot_radius,
                                disc_offset=0.0, risk=0.05, obstacle_radius=0.0):
        """The collision columns of the current batch's parameter rows, in place, from prepare_obstacles' buffers (tmpc_set_obstacle_parameters;
        raw device pointers): EllipsoidConstraints (row_model 0) or GaussianConstraints (row_model 1; obstacle_radius = the configured radius of
        its r column), ego_disc_radius and ego_disc_0_offset.  chi = -log(risk) / 0.5 is evaluated here, on the host.  Stream-ordered."""
        chi = float(-np.log(risk) / 0.5)                              # ExponentialQuantile(0.5, 1 - risk), ellipsoid_constraints.cpp:80
        self._call("tmpc_set_obstacle_parameters", d_obstacle_pos, d_obstacle_shape, d_obstacle_radius, d_obstacle_gaussian, d_scene_of, d_state,
                   robot_radius, disc_offset, risk, chi, obstacle_radius)

    def track_path(self, n_scenes, n_seg_max, d_path, d_path_count, d_path_length, d_pos, pos_stride, d_segment, d_closest_s, d_window,
                   d_bounds=None, d_bound_window=None, d_reached=None, search_range=2, window_segments=0):
        """Contouring::update on whole reference paths (tmpc_track_path; raw device pointers): per scene the closest point of d_path
        [n_scenes][n_seg_max][9] (d_path_count segments, parameter length d_path_length) to d_pos [n_scenes][pos_stride] -- searched over
        every segment where d_segment is negative, else search_range segments either side of it -- into d_segment (in / out) and d_closest_s,
        the window of S segments from there into d_window [n_scenes][S][9] (padded straight along the end tangent), with d_bounds
        [n_scenes][2][n_seg_max][8] the bound cubics of the window into d_bound_window [n_scenes][2][S][8] (what road_halfspaces takes), and
        the objective-reached flag into d_reached (u8).  Equal bit for bit to modules.track_path.  Needs no batch.  Stream-ordered.
        window_segments: 0 = the handle's S; a generated solver has none and needs the stack's contouring/num_segments here (1 .. 64)."""
        opt = TmpcPathOptions(C.sizeof(TmpcPathOptions), int(search_range), int(window_segments))
        self._call("tmpc_track_path", n_scenes, n_seg_max, d_path, d_path_count, d_path_length, d_bounds, d_pos, pos_stride, C.byref(opt), d_segment,
                   d_closest_s, d_window, d_bound_window, d_reached)

    def set_path_parameters(self, d_window, d_scene_of, n_scenes, d_closest_s=None, d_state=None):
        """The spline columns of the current batch's parameter rows, in place, from track_path's d_window (tmpc_set_path_parameters; raw
        device pointers); entries whose d_scene_of is outside [0, n_scenes) are left untouched.  With d_closest_s and d_state [B][nx]: the
        spline entry of each named entry's state becomes its scene's closest_s -- before warmstart(d_state) the solve starts from the fresh
        value, after it from the previous tick's, as in the reference (planner.cpp:81-96).  Stream-ordered."""
        self._call("tmpc_set_path_parameters", d_window, d_scene_of, n_scenes, d_closest_s, d_state)

    def path_velocity_window(self, n_scenes, n_seg_max, S, d_path, d_path_count, d_path_length, d_segment, d_closest_s, d_window, d_velocity=None,
                             d_has_velocity=None, reference_velocity=0.0, d_v_ref=None):
        """PathReferenceVelocity::setParameters on device (tmpc_path_velocity_window; raw device pointers): per scene the S
        velocity cubics from d_segment on -- d_velocity [n_scenes][n_seg_max][4] as fit_path wrote it, d_segment / d_closest_s as track_path
        wrote them -- into d_window [n_scenes][S][4], (0, 0, 0, 0) at or beyond the path's end, (0, 0, 0, reference_velocity) for a scene
        without a profile (d_velocity None, d_has_velocity[scene] == 0 or count <= 0); with d_v_ref the profile's value at closest_s (or
        reference_velocity) into d_v_ref [n_scenes], what the guidance planner is given.  Equal bit for bit to modules.path_velocity_window
        and modules.path_velocity_at.  Needs no batch; also in a generated solver.  Stream-ordered."""
        self._call("tmpc_path_velocity_window", n_scenes, n_seg_max, S, d_velocity, d_path, d_path_count, d_path_length, d_segment, d_closest_s,
                   d_has_velocity, reference_velocity, d_window, d_v_ref)

    def scatter_parameters(self, cols, d_values, d_scene_of, n_scenes, per_stage=False):
        """Caller-chosen columns of the current batch's parameter rows, in place (tmpc_scatter_parameters; cols a host sequence of at most 128
        distinct column numbers, e.g. from a generated stack's meta["parameter_map"]; raw device pointers otherwise): d_values
        [n_scenes][len(cols)] into every stage of every entry whose d_scene_of is inside [0, n_scenes), or with per_stage d_values
        [n_scenes][N][len(cols)], stage k from row k; nothing else.  The parameter writer of generated solvers.  Equal bit for bit to
        modules.scatter_parameters.  Stream-ordered."""
        arr = None if cols is None else (C.c_int32 * max(len(cols), 1))(*[int(c) for c in cols])
        self._call("tmpc_scatter_parameters", arr, 0 if cols is None else len(cols), d_values, bool(per_stage), d_scene_of, n_scenes)

    def fit_path(self, n_scenes, n_pts_max, n_seg_max, d_xy, d_count, d_path, d_path_count, d_path_length, d_s=None, d_left_xy=None,
                 d_right_xy=None, d_v=None, d_bounds=None, d_velocity=None, d_road_width=None, d_status=None):
        """Waypoints to cubic segments on device (tmpc_fit_path; raw device pointers): per scene the natural cubic spline
        through d_count waypoints of d_xy [n_scenes][n_pts_max][2] -- on the knots d_s [n_scenes][n_pts_max], or on chord lengths -- into
        d_path [n_scenes][n_seg_max][9], d_path_count and d_path_length, the layouts track_path reads; with d_left_xy / d_right_xy the bound
        curves on the centreline's knots into d_bounds [n_scenes][2][n_seg_max][8] and the road width into d_road_width; with d_v the
        velocity profile into d_velocity [n_scenes][n_seg_max][4]; d_status (u8): 0 fitted, 1 invalid (count 0, nothing else written).
        Equal bit for bit to modules.fit_path.  Needs no batch.  Stream-ordered."""
        self._call("tmpc_fit_path", n_scenes, n_pts_max, n_seg_max, d_xy, d_count, d_s, d_left_xy, d_right_xy, d_v, d_path, d_path_count, d_path_length,
                   d_bounds, d_velocity, d_road_width, d_status)

    def costmap_points(self, n_scenes, size_x, size_y, d_cost, d_origin, resolution, n_pts_max, d_points, d_count, d_overflow=None):
        """Occupied costmap cells to points on device (tmpc_costmap_points; raw device pointers; getOccupiedGridCells,
        decomp_constraints.cpp:122-148): d_cost u8 [n_scenes][size_y][size_x], d_origin [n_scenes][2] -> the centres of the cells whose cost is
        not 0, mx outer and my inner, the first n_pts_max of them into d_points [n_scenes][n_pts_max][2], their number into d_count (i32),
        d_overflow (u8) 1 iff there were more.  Equal bit for bit to modules.costmap_points.  Needs no batch.  Stream-ordered."""
        self._call("tmpc_costmap_points", n_scenes, size_x, size_y, d_cost, d_origin, resolution, n_pts_max, d_points, d_count, d_overflow)

    def decomp_halfspaces(self, d_main_of, n_scenes, n_seg_max, d_path, d_path_count, d_path_length, d_s0, d_state_x, d_points, d_count, n_pts_max,
                          decomp_range, n_rows, d_rows, d_row_count, d_status):
        """DecompConstraints::update on device (tmpc_decomp_halfspaces; raw device pointers): per scene the polyline on the whole
        path d_path / d_path_count / d_path_length (fit_path's layout) from d_s0 along the speeds of the warm start of batch entry
        d_main_of[scene], one convex polygon per segment among the scene's d_count points of d_points [n_scenes][n_pts_max][2], its rows into
        d_rows [n_scenes][N][n_rows][3] (dummies (1, 0, d_state_x + 100) included), d_row_count (i32) and d_status (u8: 0 complete, 1
        truncated, 2 degenerate) [n_scenes][N].  Equal bit for bit to modules.decomp_halfspaces.  Stream-ordered, no synchronisation."""
        self._call("tmpc_decomp_halfspaces", d_main_of, n_scenes, n_seg_max, d_path, d_path_count, d_path_length, d_s0, d_state_x, d_points, d_count,
                   n_pts_max, decomp_range, n_rows, d_rows, d_row_count, d_status)

    def set_halfspace_rows(self, d_rows, n_rows, d_scene_of, n_scenes, first_row=0, disc_offset=0.0):
        """DecompConstraints::setParameters on device (tmpc_set_halfspace_rows; raw device pointers): d_rows [n_scenes][N][n_rows][3] of every
        stage into the slack rows first_row .. first_row + n_rows - 1 of every entry of the current batch whose d_scene_of is inside
        [0, n_scenes), and ego_disc_0_offset; nothing else.  Stream-ordered."""
        self._call("tmpc_set_halfspace_rows", d_rows, n_rows, first_row, d_scene_of, n_scenes, disc_offset)

    def scenario_halfspaces(self, d_samples, n_pts, n_rows, d_scene_of, d_state_x, radius, disc_offset=0.0):
        """Device scenario -> halfspace reduction of SH-MPC (raw device pointers; samples [n_scenes][N][n_pts][2]);
        modifies the batch params in place."""
        self._call("tmpc_scenario_halfspaces", d_samples, n_pts, n_rows, d_scene_of, d_state_x, radius, disc_offset)

    def scenario_support(self, n_scenarios, tol=1e-6):
        """Support of every trajectory's solution (distinct scenarios with an active row; tmpc_scenario_support) after a solve on
        rows built by scenario_halfspaces.  Returns (support [B], active_rows [B]) as numpy int32."""
        import torch
        out = torch.empty((2, self.B), dtype=torch.int32, device=f"cuda:{self.device}")
        self._call("tmpc_scenario_support", n_scenarios, tol, out[0].data_ptr(), out[1].data_ptr())
        self.synchronize()
        o = out.cpu().numpy()
        return o[0], o[1]

    def scenario_support_async(self, n_scenarios, tol, d_support, d_active_rows):
        """tmpc_scenario_support on raw device pointers (int32 [B] each), stream-ordered on the handle's stream, no synchronisation."""
        self._call("tmpc_scenario_support", n_scenarios, tol, d_support, d_active_rows)

    def sample_scenarios(self, d_pred, d_prob, n_solvers, n_obstacles, n_modes, n_scenarios, seed, d_samples):
        """Device scenario sampler (tmpc_sample_scenarios): raw device pointers; d_samples [n_solvers][N][n_obstacles * n_scenarios][2]."""
        self._call("tmpc_sample_scenarios", d_pred, d_prob, n_solvers, n_obstacles, n_modes, n_scenarios, seed, d_samples)

    def scenario_discard(self, d_samples, n_pts, n_scenarios, n_discard, d_scene_of, radius):
        """Scenario removal for the current batch (tmpc_scenario_discard); the next scenario_halfspaces leaves the discarded scenarios out."""
        self._call("tmpc_scenario_discard", d_samples, n_pts, n_scenarios, n_discard, d_scene_of, radius)

    def scenario_discarded(self, n_scenarios):
        import torch
        out = torch.zeros((self.B, n_scenarios), dtype=torch.uint8, device=f"cuda:{self.device}")
        self._call("tmpc_scenario_discarded", out.data_ptr())
        self.synchronize()
        return out.cpu().numpy().astype(bool)

    def scenario_empty_stages(self):
        """Per trajectory: the stages whose sampled halfspaces contradicted each other in the last scenario_halfspaces (empty polygon;
        such a stage keeps the closest halfspaces and the trajectory is not eligible)."""
        import torch
        out = torch.zeros(self.B, dtype=torch.int32, device=f"cuda:{self.device}")
        self._call("tmpc_scenario_empty_stages", out.data_ptr())
        self.synchronize()
        return out.cpu().numpy()

    def warmstart(self, d_state, d_mode=None, d_src=None, deceleration=3.0):
        """Device warm start of the next tick from the solution held by the handle (raw device pointers)."""
        self._call("tmpc_warmstart", d_state, d_mode, d_src, deceleration)

    def init_with_guidance(self, d_gpos, d_gvel, d_enabled=None):
        self._call("tmpc_init_with_guidance", d_gpos, d_gvel, d_enabled)

    def sample_guidance(self, n_traj, n_nodes_max, d_nodes, d_node_count, d_gpos, d_gvel, d_status):
        """Guidance nodes to the samples init_with_guidance reads (tmpc_sample_guidance; raw device pointers): per trajectory
        the natural cubic splines x(t), y(t) through d_nodes [n_traj][n_nodes_max][3] = (t, x, y) (d_node_count of them, at most 64), sampled
        at t = k dt, k = 0 .. N, into d_gpos / d_gvel [n_traj][N + 1][2]; d_status 1 and zero rows for an invalid node list.  Equal bit for
        bit to modules.sample_guidance.  Needs no batch.  Stream-ordered."""
        self._call("tmpc_sample_guidance", n_traj, n_nodes_max, d_nodes, d_node_count, d_gpos, d_gvel, d_status)

    def guidance_plan(self, n_scenes, options, d_traj_count, d_topology_class, d_planner_ids, d_selection, d_mode, d_src, d_init_enabled,
                      d_rows_dummy, d_disabled, d_guidance_id, d_weight, d_previously_selected=None):
        """What every planner of every scene does this tick (tmpc_guidance_plan; options from guidance_options(); raw device pointers): from
        the trajectory counts, the classes and the cross-tick state d_planner_ids [n_scenes][P] / d_selection [n_scenes][3] to d_mode / d_src
        (warmstart), d_init_enabled (init_with_guidance), d_rows_dummy (linearize_topology_ex's d_is_original), d_disabled, d_guidance_id and
        d_weight (guidance_decide), entry b = scene P + planner.  Equal to modules.guidance_plan.  Needs no batch.  Stream-ordered."""
        self._call("tmpc_guidance_plan", n_scenes, None if options is None else C.byref(options), d_traj_count, d_topology_class,
                   d_previously_selected, d_planner_ids, d_selection, d_mode, d_src, d_init_enabled, d_rows_dummy, d_disabled, d_guidance_id, d_weight)

    def guidance_decide(self, n_scenes, options, d_pobj, d_exit_code, d_disabled, d_guidance_id, d_weight, d_state, d_best, d_exit, d_cmd,
                        d_planner_ids, d_selection, deceleration=3.0, control_dt=0.05, enable_output=True):
        """The decision after the solve (tmpc_guidance_decide; raw device pointers): per scene FindBestPlanner over the enabled planners into
        d_best (as gather_best reads it), the exit code into d_exit, the command (v of node 1, w of node 0) of the winner or the braking
        command into d_cmd [n_scenes][2], and the cross-tick state d_planner_ids / d_selection for the next guidance_plan.  d_pobj /
        d_exit_code: result_device_ptrs(), or arrays of the caller's.  Equal bit for bit to modules.guidance_decide.  Stream-ordered."""
        self._call("tmpc_guidance_decide", n_scenes, None if options is None else C.byref(options), d_pobj, d_exit_code, d_disabled, d_guidance_id,
                   d_weight, d_state, deceleration, control_dt, bool(enable_output), d_best, d_exit, d_cmd, d_planner_ids, d_selection)

    def debug_get_x0(self):
        x0 = np.zeros((self.B, self.N + 1, self.dims.nvar)); xinit = np.zeros((self.B, self.dims.nx))
        self._call("tmpc_debug_get_x0", _p(x0), _p(xinit))
        return x0, xinit

    def debug_get_params(self):
        out = np.zeros((self.B, self.N, self.npar))
        self._call("tmpc_debug_get_params", _p(out))
        return out

    def result_device_ptrs(self):
        a, b = C.c_void_p(), C.c_void_p()
        self._call("tmpc_result_device_ptrs", C.byref(a), C.byref(b))
        return a.value, b.value

    # --- debug ------------------------------------------------------------------------------------
    PHASES = ["linearise", "residuals", "barrier_hessian", "riccati_factor", "rhs", "riccati_solve", "row_passes",
              "update", "final", "total"]

    def debug_profile(self):
        cyc = np.zeros(10, np.int64)
        self._call("tmpc_debug_profile", _p(cyc), 10)
        return dict(zip(self.PHASES, cyc.tolist()))

    def debug_eval_stage(self, z, p, pi=None, lamh=None):
        z = np.ascontiguousarray(z, np.float64).reshape(-1, self.dims.nvar); n = z.shape[0]
        p = np.ascontiguousarray(p, np.float64).reshape(n, self.npar)
        nh = self.dims.nh            # rows in the reference's order [topology | ellipsoids | decomp/scenario rows]
        pi = None if pi is None else np.ascontiguousarray(pi, np.float64).reshape(n, NX)
        lamh = None if lamh is None else np.ascontiguousarray(lamh, np.float64).reshape(n, nh)
        o = dict(cost=np.zeros(n), cost_grad=np.zeros((n, NV)), cost_hess=np.zeros((n, NV, NV)), h=np.zeros((n, nh)),
                 h_jac=np.zeros((n, nh, NV)), x_next=np.zeros((n, NX)), x_jac=np.zeros((n, NX, NV)),
                 lag_hess=np.zeros((n, NV, NV)), mirror=np.zeros((n, NV, NV)))
        self._call("tmpc_debug_eval_stage", n, _p(z), _p(p), _p(pi), _p(lamh), *[_p(a) for a in o.values()])
        return o


def optimize_batch(solver, scene_batch, tmpc_consistency_weight=None):
    """Batched counterpart of GuidanceConstraints::optimize (guidance_constraints.cpp:264-388) for one launch batch:
    load every local planner's parameters + warm start, solve all of them in one launch, then pick the best
    planner per scene (FindBestPlanner :416-434).  Returns (results dict, best index per scene)."""
    solver.set_batch(scene_batch["xinit"], scene_batch["x0"], scene_batch["params"])
    solver.solve()
    res = solver.get()
    scene_of = scene_batch.get("scene_of")
    if scene_of is None:
        return res, np.array([solver.select_best()])
    n_scenes = int(scene_of.max()) + 1
    best = np.zeros(n_scenes, np.int32)
    for s in range(n_scenes):
        idx = np.nonzero(scene_of == s)[0]
        best[s] = solver.select_best(first=int(idx[0]), count=len(idx))
    return res, best


def optimize_scenarios(solver, xinit, x0, params, n_iter=None, scenario=None):
    """Batched counterpart of ScenarioConstraints::optimize (scenario_constraints.cpp:58-108): the P parallel scenario solvers
    (each a copy of the main solver with its own scenario halfspaces in `params` [P][N][npar]; copying the main solver and
    scenario_module.setParameters happen on the caller's side, e.g. modules.halfspace_rows_set_parameters) are solved together,
    driven ONE RTI iteration at a time like the scenario module drives its solver (initializeOneIteration, solveOneIteration x n
    with the loop exit on qp_status != 0, completeOneIteration; :85), then the selection of :93-107: lowest objective among exit
    code 1 (init 1e9, strict '<': lowest index wins ties).  Returns (results dict, best index or -1, exit code the reference
    returns: the best solver's, or the first solver's when none succeeded).

    scenario = dict(d_samples, n_pts, n_rows, d_scene_of, d_state_x, radius, n_scenarios[, disc_offset, tol, max_support, n_discard]) builds
    the rows on device from the sampled scenarios (tmpc_scenario_halfspaces, scenario_module.update + setParameters) and adds the
    support bookkeeping of ScenarioSolver (scenario_constraints.h:38-40): res["support"], res["active_rows"], and with max_support
    (the bound on the support of the solution AFTER the removal, i.e. NOT counting the n_discard removed scenarios: the removed ones
    enter the certificate separately -- the sample size has to come from modules.scenario_sample_size(risk, max_support=max_support,
    removed=n_discard), which is what makes `support <= max_support` certify the risk; tests/test_host_scenario_bound.py)
    res["scenario_status"] (0 = within the bound the sample size was chosen for, 1 = support exceeded: no certificate, 2 = a stage's
    scenario halfspaces contradicted each other -- an empty polygon; res["empty_polygon_stages"] counts them) -- a solver
    with status 1 is then not eligible as the best one."""
    n_iter = solver.dims.n_sqp if n_iter is None else int(n_iter)
    solver.set_batch(xinit, x0, params)                               # *solver = *_solver; setParameters; loadWarmstart
    if scenario is not None:
        if scenario.get("n_discard"):                                  # scenario removal before the polygons; counts into the bound (scenario_risk(removed=...))
            solver.scenario_discard(scenario["d_samples"], scenario["n_pts"], scenario["n_scenarios"], scenario["n_discard"],
                                    scenario["d_scene_of"], scenario["radius"])
        solver.scenario_halfspaces(scenario["d_samples"], scenario["n_pts"], scenario["n_rows"], scenario["d_scene_of"],
                                   scenario["d_state_x"], scenario["radius"], scenario.get("disc_offset", 0.0))
    for it in range(n_iter):                                          # every slot stops by itself once its QP reports a status
        solver.solve_iterations(1, keep_iterate=it > 0, keep_multipliers=True, complete=False)
    solver.solve_iterations(0, keep_iterate=True, keep_multipliers=True, complete=True)
    res = solver.get()
    eligible = res["exit_code"] == 1
    if scenario is not None:
        res["support"], res["active_rows"] = solver.scenario_support(scenario["n_scenarios"], scenario.get("tol", 1e-6))
        res["empty_polygon_stages"] = solver.scenario_empty_stages()
        status = np.zeros(len(res["pobj"]), np.int32)
        if scenario.get("max_support") is not None:
            status[res["support"] > scenario["max_support"]] = 1
        status[res["empty_polygon_stages"] > 0] = 2                  # contradictory scenario halfspaces somewhere on the horizon: never eligible
        if scenario.get("max_support") is not None or (status == 2).any():
            res["scenario_status"] = status
        eligible = eligible & (status == 0)
    best, lowest = -1, 1e9
    for i in range(len(res["pobj"])):
        if eligible[i] and res["pobj"][i] < lowest:
            lowest, best = res["pobj"][i], i
    return res, best, int(res["exit_code"][best if best >= 0 else 0])
