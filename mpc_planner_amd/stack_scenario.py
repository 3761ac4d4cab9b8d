"""The scenario rows of include/tmpc_hip_stack_scenario.h: the SH-MPC polygons and the support of the solution of a generated solver on device.

A generated library's parameter layout belongs to its module stack, so BatchedSolver.scenario_halfspaces refuses on it, and scenario_support with
it.  StackScenario runs the same device code with the columns named by the caller -- the column numbers of the stack's parameter map -- on the
library a BatchedSolver already loaded:

    path, meta = ...                                    # build/generated/libtmpc_hip_safe_horizon.so, safe_horizon_meta.json
    s = solver.BatchedSolver(solver.default_dims(N=20, lib_path=path), B_max, lib_path=path)
    scn = StackScenario(s)
    cols = scenario_columns(meta["parameter_map"], 24)
    s.sample_scenarios(...); s.scenario_discard(...)    # these touch no parameter column: any handle
    scn.halfspaces(cols, d_samples, n_pts, d_scene_of, d_state_x, radius)
    s.solve_iterations(10); support, active_rows = scn.support(cols, n_scenarios, tol); s.scenario_empty_stages()

The same calls work on a hand-written shape with scenes.make_scene(...)["pm"]._params as the map."""
import ctypes as C

from ._binding import StackEntries, _cols, _column, _count

_int, _i32, _f64, _vp = C.c_int, C.c_int32, C.c_double, C.c_void_p

# The Python side of include/tmpc_hip_stack_scenario.h, in the header's order: name -> (restype, argtypes); tests/test_stack_scenario_header.py
# holds it against the header's prototypes.  Kept apart from the tables of the three older headers.
_SIGNATURES = {
    "tmpc_stack_scenario_halfspaces": (_int, [_vp, C.POINTER(_i32), _i32, _vp, _i32, _vp, _vp, _f64, _f64]),
    "tmpc_stack_scenario_support": (_int, [_vp, C.POINTER(_i32), _i32, _i32, _f64, _vp, _vp]),
}
EXPORTS = list(_SIGNATURES)


def scenario_columns(parameter_map, n_rows, disc=0):
    """cols of halfspaces / support from a stack's parameter map (name -> column): ego_disc_{disc}_offset, then
    disc_{disc}_scenario_constraint_{r}_{a1,a2,b}, r < n_rows."""
    return [_column(parameter_map, f"ego_disc_{int(disc)}_offset")] + \
           [_column(parameter_map, f"disc_{int(disc)}_scenario_constraint_{r}_{f}") for r in range(int(n_rows)) for f in ("a1", "a2", "b")]


class StackScenario(StackEntries):
    """The two entry points of tmpc_hip_stack_scenario.h on a BatchedSolver's library and handle (raw device pointers, like BatchedSolver's
    own wrappers).  Everything is enqueued on the handle's stream; a failure raises solver.TmpcError with the library's message."""
    _SIGNATURES = _SIGNATURES

    @staticmethod
    def _rows(cols):
        return _count(cols, 3, lead=1)

    def halfspaces(self, cols, d_samples, n_pts, d_scene_of, d_state_x, radius, disc_offset=0.0):
        """What BatchedSolver.scenario_halfspaces writes, for len(cols) // 3 rows: the polygon rows of d_samples [n_scenes][N][n_pts][2] and
        ego_disc_0_offset into the columns `cols` = scenario_columns(parameter_map, n_rows) of the current batch's rows
        (tmpc_stack_scenario_halfspaces).  The scenarios marked by scenario_discard for this batch are left out."""
        self._call("tmpc_stack_scenario_halfspaces", _cols(cols), self._rows(cols), d_samples, n_pts, d_scene_of, d_state_x, radius, disc_offset)

    def support(self, cols, n_scenarios, tol=1e-6):
        """What BatchedSolver.scenario_support returns -- (support [B], active_rows [B]) as numpy int32 -- after a solve on rows built by
        halfspaces(cols, ...), the rows read from the same columns (tmpc_stack_scenario_support)."""
        import torch
        s = self.solver
        out = torch.empty((2, s.B), dtype=torch.int32, device=f"cuda:{s.device}")
        self.support_async(cols, n_scenarios, tol, out[0].data_ptr(), out[1].data_ptr())
        s.synchronize()
        o = out.cpu().numpy()
        return o[0], o[1]

    def support_async(self, cols, n_scenarios, tol, d_support, d_active_rows):
        """tmpc_stack_scenario_support on raw device pointers (int32 [B] each), stream-ordered on the handle's stream, no synchronisation."""
        self._call("tmpc_stack_scenario_support", _cols(cols), self._rows(cols), n_scenarios, tol, d_support, d_active_rows)
