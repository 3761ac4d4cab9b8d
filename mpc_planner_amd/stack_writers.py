"""The module-stack writers of include/tmpc_hip_stack.h: the obstacle and topology rows of a generated solver on device.

A generated library's parameter layout belongs to its module stack, so BatchedSolver.prepare_obstacles / set_obstacle_parameters /
linearize_topology(_ex) refuse on it.  StackWriters runs the same device code with the destination named by the caller -- the column numbers
of the stack's parameter map -- on the library a BatchedSolver already loaded:

    path, meta = ...                                    # build/generated/libtmpc_hip_<name>.so, <name>_meta.json
    s = solver.BatchedSolver(solver.default_dims(N=30, lib_path=path), B_max, lib_path=path)
    w = StackWriters(s)
    ocols = obstacle_columns(meta["parameter_map"], 5, row_model=1)
    tcols = topology_columns(meta["parameter_map"], 5)
    w.prepare_obstacles(...); w.set_obstacle_columns(ocols, 1, 5, ...); w.linearize_topology_columns(tcols, ...); s.solve()

The same calls work on a hand-written shape with scenes.make_scene(...)["pm"]._params as the map.  The path window, the road rows and the decomp
rows of such stacks: stack_env.py.  Their scenario rows and the support of the solution: stack_scenario.py."""
import ctypes as C

import numpy as np

from . import solver as _solver
from ._binding import StackEntries, _cols, _column, _count

_int, _i32, _f64, _vp = C.c_int, C.c_int32, C.c_double, C.c_void_p

# The Python side of include/tmpc_hip_stack.h, in the header's order: name -> (restype, argtypes); tests/test_stack_header.py holds it against the
# header's prototypes.  Kept apart from solver._SIGNATURES, which is the Python side of tmpc_hip.h and nothing else.
_SIGNATURES = {
    "tmpc_stack_prepare_obstacles": (_int, [_vp, _i32, _i32, _i32] + [_vp] * 6 + [C.POINTER(_solver.TmpcObstacleOptions)] + [_vp] * 5),
    "tmpc_stack_set_obstacle_columns": (_int, [_vp, C.POINTER(_i32), _i32, _i32, _i32] + [_vp] * 6 + [_f64] * 5),
    "tmpc_stack_linearize_topology_columns": (_int, [_vp, C.POINTER(_i32), _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _f64, _vp]),
}
EXPORTS = list(_SIGNATURES)

ELLIPSOID_FIELDS = ("x", "y", "psi", "major", "minor", "chi", "r")          # ellipsoid_constraints.py:33-49
GAUSSIAN_FIELDS = ("x", "y", "major", "minor", "risk", "r")                 # gaussian_constraints.py:40-52


def obstacle_columns(parameter_map, max_obstacles, row_model):
    """cols of set_obstacle_columns from a stack's parameter map (name -> column): ego_disc_radius, ego_disc_0_offset, then per obstacle
    ellipsoid_obst_{j}_{x,y,psi,major,minor,chi,r} (row_model 0) or gaussian_obst_{j}_{x,y,major,minor,risk,r} (row_model 1)."""
    if row_model not in (0, 1):
        raise ValueError("row_model is 0 (ellipsoids) or 1 (Gaussian rows)")
    prefix, fields = (("ellipsoid_obst", ELLIPSOID_FIELDS), ("gaussian_obst", GAUSSIAN_FIELDS))[row_model]
    return [_column(parameter_map, "ego_disc_radius"), _column(parameter_map, "ego_disc_0_offset")] + \
           [_column(parameter_map, f"{prefix}_{j}_{f}") for j in range(int(max_obstacles)) for f in fields]


def topology_columns(parameter_map, n_rows):
    """cols of linearize_topology_columns from a stack's parameter map: lin_constraint_{j}_{a1,a2,b}, j < n_rows."""
    return [_column(parameter_map, f"lin_constraint_{j}_{f}") for j in range(int(n_rows)) for f in ("a1", "a2", "b")]


class StackWriters(StackEntries):
    """The three entry points of tmpc_hip_stack.h on a BatchedSolver's library and handle (raw device pointers, like BatchedSolver's own
    wrappers).  Everything is enqueued on the handle's stream; a failure raises solver.TmpcError with the library's message."""
    _SIGNATURES = _SIGNATURES

    def prepare_obstacles(self, n_scenes, n_slots, max_obstacles, d_count, d_state, d_raw_pos, d_raw_radius, d_obstacle_pos, d_obstacle_shape,
                          d_obstacle_radius, d_obstacle_gaussian, d_selected, d_raw_vel=None, d_raw_pred=None, probabilistic=False, noise=0.3,
                          propagate_passes=0, max_obstacle_distance=0.0):
        """BatchedSolver.prepare_obstacles (same arguments, same outputs, equal bit for bit to modules.prepare_obstacles), also in a generated
        solver (tmpc_stack_prepare_obstacles).  Needs no batch."""
        opt = _solver.TmpcObstacleOptions(C.sizeof(_solver.TmpcObstacleOptions), int(probabilistic), int(propagate_passes), 0, float(noise),
                                          float(max_obstacle_distance))
        self._call("tmpc_stack_prepare_obstacles", n_scenes, n_slots, max_obstacles, d_count, d_state, d_raw_pos, d_raw_radius, d_raw_vel, d_raw_pred,
                   C.byref(opt), d_obstacle_pos, d_obstacle_shape, d_obstacle_radius, d_obstacle_gaussian, d_selected)

    def set_obstacle_columns(self, cols, row_model, max_obstacles, d_obstacle_pos, d_obstacle_shape, d_obstacle_radius, d_obstacle_gaussian,
                             d_scene_of, d_state, robot_radius, disc_offset=0.0, risk=0.05, obstacle_radius=0.0):
        """What BatchedSolver.set_obstacle_parameters writes -- EllipsoidConstraints (row_model 0) or GaussianConstraints (row_model 1),
        ego_disc_radius and ego_disc_0_offset -- from prepare_obstacles' buffers with max_obstacles obstacles per scene, into the columns
        `cols` = obstacle_columns(parameter_map, max_obstacles, row_model) of the current batch's rows (tmpc_stack_set_obstacle_columns).
        chi = -log(risk) / 0.5 is evaluated here, on the host."""
        chi = float(-np.log(risk) / 0.5)                              # ExponentialQuantile(0.5, 1 - risk), ellipsoid_constraints.cpp:80
        self._call("tmpc_stack_set_obstacle_columns", _cols(cols), 0 if cols is None else len(cols), row_model, max_obstacles, d_obstacle_pos,
                   d_obstacle_shape, d_obstacle_radius, d_obstacle_gaussian, d_scene_of, d_state, robot_radius, disc_offset, risk, chi, obstacle_radius)

    def linearize_topology_columns(self, cols, d_obstacle_pos, n_obstacles, d_scene_of, d_state_x, robot_radius, d_obstacle_radius=None,
                                   d_static_halfspaces=None, n_static=0, d_is_original=None):
        """What BatchedSolver.linearize_topology_ex writes, for a stack with len(cols) / 3 topology rows, into the columns `cols` =
        topology_columns(parameter_map, n_rows) of the current batch's rows (tmpc_stack_linearize_topology_columns)."""
        self._call("tmpc_stack_linearize_topology_columns", _cols(cols), _count(cols, 3), d_obstacle_pos, n_obstacles, d_obstacle_radius, d_static_halfspaces,
                   n_static, d_scene_of, d_state_x, robot_radius, d_is_original)
