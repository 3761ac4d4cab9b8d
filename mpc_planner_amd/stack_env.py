"""The static environment of include/tmpc_hip_stack_env.h: the path window, the road rows and the free-space (decomp) rows of a generated
solver on device.

A generated library's parameter layout belongs to its module stack, so BatchedSolver.set_path_parameters / road_halfspaces / decomp_halfspaces /
set_halfspace_rows refuse on it.  StackEnvironment runs the same device code with the columns named by the caller -- the column numbers of the
stack's parameter map -- on the library a BatchedSolver already loaded:

    path, meta = ...                                    # build/generated/libtmpc_hip_road_decomp.so, road_decomp_meta.json
    s = solver.BatchedSolver(solver.default_dims(N=20, lib_path=path), B_max, lib_path=path)
    env = StackEnvironment(s)
    pcols = path_columns(meta["parameter_map"], 3)
    dcols = decomp_columns(meta["parameter_map"], 4)
    s.track_path(..., window_segments=3); env.set_path_columns(pcols, d_window, d_scene_of, n_scenes)
    env.road_halfspaces(pcols, d_main_of, n_scenes, ...); env.decomp_halfspaces(...); env.set_halfspace_columns(dcols, d_rows, d_scene_of, n_scenes)

Together with stack_writers.StackWriters this is every row of a contouring stack with guidance, road and decomp rows.  The same calls work on a
hand-written shape with scenes.make_scene(...)["pm"]._params as the map.  The scenario rows of generated stacks: stack_scenario.py."""
import ctypes as C

from ._binding import StackEntries, _cols, _column, _count

_int, _i32, _f64, _vp = C.c_int, C.c_int32, C.c_double, C.c_void_p

# The Python side of include/tmpc_hip_stack_env.h, in the header's order: name -> (restype, argtypes); tests/test_stack_env_header.py holds it
# against the header's prototypes.  Kept apart from solver._SIGNATURES (tmpc_hip.h) and stack_writers._SIGNATURES (tmpc_hip_stack.h).
_SIGNATURES = {
    "tmpc_stack_set_path_columns": (_int, [_vp, C.POINTER(_i32), _i32, _vp, _vp, _i32, _vp, _vp]),
    "tmpc_stack_road_halfspaces": (_int, [_vp, C.POINTER(_i32), _i32, _vp, _i32, _vp, _f64, _f64, _vp, _i32, _i32]),
    "tmpc_stack_decomp_halfspaces": (_int, [_vp, _vp, _i32, _i32] + [_vp] * 7 + [_i32, _f64, _i32, _vp, _vp, _vp]),
    "tmpc_stack_set_halfspace_columns": (_int, [_vp, C.POINTER(_i32), _i32, _vp, _vp, _i32, _f64]),
}
EXPORTS = list(_SIGNATURES)

SPLINE_COEFFICIENTS = ("a", "b", "c", "d")                                  # contouring.py: spline_x{i}_a .. spline_y{i}_d, spline{i}_start


def path_columns(parameter_map, n_segments):
    """cols of set_path_columns / road_halfspaces from a stack's parameter map (name -> column): per segment i < n_segments
    spline_x{i}_{a,b,c,d}, spline_y{i}_{a,b,c,d}, spline{i}_start."""
    return [_column(parameter_map, name) for i in range(int(n_segments))
            for name in [f"spline_{axis}{i}_{c}" for axis in "xy" for c in SPLINE_COEFFICIENTS] + [f"spline{i}_start"]]


def decomp_columns(parameter_map, n_rows, disc=0):
    """cols of set_halfspace_columns from a stack's parameter map: ego_disc_{disc}_offset, then disc_{disc}_decomp_{r}_{a1,a2,b}, r < n_rows."""
    return [_column(parameter_map, f"ego_disc_{int(disc)}_offset")] + \
           [_column(parameter_map, f"disc_{int(disc)}_decomp_{r}_{f}") for r in range(int(n_rows)) for f in ("a1", "a2", "b")]


class StackEnvironment(StackEntries):
    """The four entry points of tmpc_hip_stack_env.h on a BatchedSolver's library and handle (raw device pointers, like BatchedSolver's own
    wrappers).  Everything is enqueued on the handle's stream; a failure raises solver.TmpcError with the library's message."""
    _SIGNATURES = _SIGNATURES

    def set_path_columns(self, cols, d_window, d_scene_of, n_scenes, d_closest_s=None, d_state=None):
        """What BatchedSolver.set_path_parameters writes, for a stack with len(cols) / 9 path segments: track_path's d_window
        [n_scenes][n_segments][9] into the columns `cols` = path_columns(parameter_map, n_segments) of the current batch's rows
        (tmpc_stack_set_path_columns); d_closest_s / d_state as there."""
        self._call("tmpc_stack_set_path_columns", _cols(cols), _count(cols, 9), d_window, d_scene_of, n_scenes, d_closest_s, d_state)

    def road_halfspaces(self, cols, d_main_of, n_scenes, offset_first, offset_second, d_static_halfspaces, n_static, first_row=0,
                        d_bound_segments=None):
        """What BatchedSolver.road_halfspaces writes -- rows first_row, first_row + 1 of d_static_halfspaces [n_scenes][N][n_static][3], the
        buffer linearize_topology_columns reads -- with the path window read from the columns `cols` = path_columns(parameter_map,
        n_segments) of the main entry's rows (tmpc_stack_road_halfspaces); d_bound_segments [n_scenes][2][n_segments][8]: bounds mode."""
        self._call("tmpc_stack_road_halfspaces", _cols(cols), _count(cols, 9), d_main_of, n_scenes, d_bound_segments, offset_first, offset_second,
                   d_static_halfspaces, n_static, first_row)

    def decomp_halfspaces(self, d_main_of, n_scenes, n_seg_max, d_path, d_path_count, d_path_length, d_s0, d_state_x, d_points, d_count, n_pts_max,
                          decomp_range, n_rows, d_rows, d_row_count, d_status):
        """BatchedSolver.decomp_halfspaces (same arguments, same outputs), also in a generated solver (tmpc_stack_decomp_halfspaces)."""
        self._call("tmpc_stack_decomp_halfspaces", d_main_of, n_scenes, n_seg_max, d_path, d_path_count, d_path_length, d_s0, d_state_x, d_points, d_count,
                   n_pts_max, decomp_range, n_rows, d_rows, d_row_count, d_status)

    def set_halfspace_columns(self, cols, d_rows, d_scene_of, n_scenes, disc_offset=0.0):
        """What BatchedSolver.set_halfspace_rows writes, for len(cols) // 3 rows: d_rows [n_scenes][N][n_rows][3] of every stage and
        ego_disc_0_offset into the columns `cols` = decomp_columns(parameter_map, n_rows) of the current batch's rows
        (tmpc_stack_set_halfspace_columns).  The columns name the rows: there is no first_row."""
        self._call("tmpc_stack_set_halfspace_columns", _cols(cols), _count(cols, 3, lead=1), d_rows, d_scene_of, n_scenes, disc_offset)
