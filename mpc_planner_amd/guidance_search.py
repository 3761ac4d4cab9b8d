"""The guidance search on device, include/tmpc_hip_guidance_search.h: topology-distinct trajectories per scene.

tmpc_guidance_search produces what sample_guidance and guidance_plan read -- nodes, node counts, trajectory counts and topology classes --
from the obstacles prepare_obstacles just wrote and a set of goals, stream-ordered on the handle's stream.  It reads no parameter column and
needs no batch, so it works on any library a BatchedSolver loaded, generated ones included.  Where it sits in a tick, nothing read back:

    s = solver.BatchedSolver(dims, Q * P)
    search = GuidanceSearchState(s, Q, options=guidance_search_options(n_paths=4, n_samples=30, seed=1, robot_radius=0.325))
    for tick in range(ticks):
        world.step(d_cmd)                                   # tmpc_episode_step writes world.was_reset
        s.prepare_obstacles(Q, n_slots, M, ..., d_pos, d_shape, d_radius, d_gaussian, d_selected)
        search.search(n_goals, M, world.state4.data_ptr(), d_goals, d_pos, d_radius, d_selected, d_was_reset=world.was_reset.data_ptr())
        s.guidance_plan(Q, gopt, search.traj_count.data_ptr(), search.topology_class.data_ptr(), ...)
        s.warmstart(...)
        s.sample_guidance(Q * n_paths, R, search.nodes.data_ptr(), search.node_count.data_ptr(), d_gpos, d_gvel, d_status)
        ...

mpc_planner_amd.modules.guidance_search is the numpy mirror for one scene, bit for bit the device's."""
import ctypes as C

from ._binding import StackEntries

_int, _i32, _u32, _u64, _f64, _vp = C.c_int, C.c_int32, C.c_uint32, C.c_uint64, C.c_double, C.c_void_p


class TmpcGuidanceSearchOptions(C.Structure):
    """tmpc_guidance_search_options of include/tmpc_hip_guidance_search.h, field for field."""
    _fields_ = [("size", _u32), ("n_paths", _i32), ("n_samples", _i32), ("reserved", _i32), ("seed", _u64), ("n_nodes_max", _i32),
                ("max_expansions", _i32), ("robot_radius", _f64), ("max_velocity", _f64), ("margin", _f64), ("weight_length", _f64)]


# The Python side of include/tmpc_hip_guidance_search.h: name -> (restype, argtypes); tests/test_guidance_search_header.py holds it against
# the header's prototype.  Kept apart from the tables of the five older headers.
_SIGNATURES = {
    "tmpc_guidance_search": (_int, [_vp, _i32, _i32, _i32, C.POINTER(TmpcGuidanceSearchOptions)] + [_vp] * 15),
}
EXPORTS = list(_SIGNATURES)

# the pointer arguments of tmpc_guidance_search, in the header's order
ARRAYS = ("d_state4", "d_goals", "d_obstacle_pos", "d_obstacle_radius", "d_selected", "d_was_reset", "d_prev_traj", "d_prev_class", "d_prev_count",
          "d_next_class", "d_nodes", "d_node_count", "d_traj_count", "d_topology_class", "d_status")
OPTIONAL = ("d_was_reset",)


def guidance_search_options(n_paths=4, n_samples=30, seed=0, n_nodes_max=64, max_expansions=4096, robot_radius=0.325, max_velocity=3.0,
                            margin=0.5, weight_length=1.0):
    """A filled tmpc_guidance_search_options; n_paths and n_samples default to the reference's guidance_planner.yaml."""
    return TmpcGuidanceSearchOptions(C.sizeof(TmpcGuidanceSearchOptions), int(n_paths), int(n_samples), 0, int(seed), int(n_nodes_max),
                                     int(max_expansions), float(robot_radius), float(max_velocity), float(margin), float(weight_length))


class GuidanceSearch(StackEntries):
    """The entry point of tmpc_hip_guidance_search.h on a BatchedSolver's library and handle (raw device pointers, like BatchedSolver's own
    wrappers).  Enqueued on the handle's stream; a failure raises solver.TmpcError with the library's message."""
    _SIGNATURES = _SIGNATURES

    def search(self, n_scenes, n_goals, max_obstacles, options, d_state4, d_goals, d_obstacle_pos, d_obstacle_radius, d_selected, d_prev_traj,
               d_prev_class, d_prev_count, d_next_class, d_nodes, d_node_count, d_traj_count, d_topology_class, d_status, d_was_reset=None):
        """tmpc_guidance_search: one tick of n_scenes scenes (the header states the arrays and the algorithm)."""
        self._call("tmpc_guidance_search", n_scenes, n_goals, max_obstacles, None if options is None else C.byref(options), d_state4, d_goals,
                   d_obstacle_pos, d_obstacle_radius, d_selected, d_was_reset, d_prev_traj, d_prev_class, d_prev_count, d_next_class, d_nodes,
                   d_node_count, d_traj_count, d_topology_class, d_status)


class GuidanceSearchState:
    """The carried arrays and the outputs of n_scenes searches as torch tensors on a BatchedSolver's device, and the call.  Attributes under
    the header's names without `d_`: prev_traj [Q][P][N + 1][2], prev_class [Q][P], prev_count [Q], next_class [Q] (zero-initialised), nodes
    [Q P][R][3], node_count [Q P], traj_count [Q], topology_class [Q][P], status [Q]."""

    def __init__(self, solver, n_scenes, options):
        import torch
        self.solver, self.entry, self.options, self.Q = solver, GuidanceSearch(solver), options, int(n_scenes)
        dev = torch.device(f"cuda:{solver.device}")
        Q, P, R, S = self.Q, int(options.n_paths), int(options.n_nodes_max), int(solver.dims.N) + 1
        zeros = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        self.prev_traj, self.prev_class = zeros((Q, P, S, 2), torch.float64), zeros((Q, P), torch.int32)
        self.prev_count, self.next_class = zeros((Q,), torch.int32), zeros((Q,), torch.int32)
        self.nodes, self.node_count = zeros((Q * P, R, 3), torch.float64), zeros((Q * P,), torch.int32)
        self.traj_count, self.topology_class, self.status = zeros((Q,), torch.int32), zeros((Q, P), torch.int32), zeros((Q,), torch.int32)
        torch.cuda.synchronize(dev)

    def search(self, n_goals, max_obstacles, d_state4, d_goals, d_obstacle_pos, d_obstacle_radius, d_selected, d_was_reset=None):
        """One tick on the handle's stream from raw device pointers; nothing is read back."""
        self.entry.search(self.Q, n_goals, max_obstacles, self.options, d_state4, d_goals, d_obstacle_pos, d_obstacle_radius, d_selected,
                          self.prev_traj.data_ptr(), self.prev_class.data_ptr(), self.prev_count.data_ptr(), self.next_class.data_ptr(),
                          self.nodes.data_ptr(), self.node_count.data_ptr(), self.traj_count.data_ptr(), self.topology_class.data_ptr(),
                          self.status.data_ptr(), d_was_reset=d_was_reset)
