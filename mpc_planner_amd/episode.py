"""The world of a closed loop on device, include/tmpc_hip_episode.h: the plant step, the obstacles' motion and the episode log.

Every per-tick piece of the planner has a device producer; tmpc_episode_step turns the command guidance_decide wrote into the next tick's
inputs, measures the episode and restarts it, stream-ordered on the handle's stream.  It reads no parameter column and needs no batch, so it
works on any library a BatchedSolver loaded, generated ones included.  One tick of the T-MPC pipeline with the step in front, nothing read
back:

    s = solver.BatchedSolver(dims, Q * P)
    world = EpisodeWorld(s, P, plant0, raw_pos0, raw_vel0, raw_radius, options=episode_options(control_dt=0.05, timeout_ticks=400, ...))
    for tick in range(ticks):
        world.step(d_cmd)                                   # tmpc_episode_step: d_cmd -> world.state4 / state_nx / state_batch, raw_pos, raw_vel
        s.prepare_obstacles(Q, n_slots, M, world.count.data_ptr(), world.state4.data_ptr(), world.raw_pos.data_ptr(), world.raw_radius.data_ptr(),
                            ..., d_raw_vel=world.raw_vel.data_ptr())
        s.guidance_plan(Q, gopt, ..., world.planner_ids.data_ptr(), world.selection.data_ptr(), ...)
        s.warmstart(world.state_batch.data_ptr(), d_mode, d_src)
        s.sample_guidance(...); s.init_with_guidance(...)
        s.set_obstacle_parameters(...); s.linearize_topology_ex(...)
        s.solve(sync=False)
        s.guidance_decide(Q, gopt, ..., world.state_nx.data_ptr(), ..., d_cmd, world.planner_ids.data_ptr(), world.selection.data_ptr())
    s.synchronize(); log = world.log()

mpc_planner_amd.modules.episode_step is the numpy mirror for one scene, bit for bit the device's."""
import ctypes as C

import numpy as np

from ._binding import StackEntries

_int, _i32, _u32, _f64, _vp = C.c_int, C.c_int32, C.c_uint32, C.c_double, C.c_void_p


class TmpcEpisodeOptions(C.Structure):
    """tmpc_episode_options of include/tmpc_hip_episode.h, field for field."""
    _fields_ = [("size", _u32), ("substeps", _i32), ("timeout_ticks", _i32), ("max_episodes", _i32), ("control_dt", _f64),
                ("max_acceleration", _f64), ("max_angular_velocity", _f64), ("robot_radius", _f64), ("goal_x", _f64)]


# The Python side of include/tmpc_hip_episode.h: name -> (restype, argtypes); tests/test_episode_header.py holds it against the header's
# prototype.  Kept apart from the tables of the four older headers.
_SIGNATURES = {
    "tmpc_episode_step": (_int, [_vp, _i32, _i32, _i32, C.POINTER(TmpcEpisodeOptions)] + [_vp] * 21),
}
EXPORTS = list(_SIGNATURES)

# the pointer arguments of tmpc_episode_step, in the header's order
ARRAYS = ("d_cmd", "d_plant", "d_plant0", "d_count", "d_raw_pos", "d_raw_vel", "d_raw_radius", "d_raw_pos0", "d_raw_vel0", "d_box", "d_goal",
          "d_episode", "d_episode_f", "d_log", "d_was_reset", "d_state4", "d_state_nx", "d_state_batch", "d_planner_ids", "d_selection", "d_segment")
OPTIONAL = ("d_box", "d_goal", "d_state_nx", "d_state_batch", "d_planner_ids", "d_selection", "d_segment")


def episode_options(substeps=1, timeout_ticks=0, max_episodes=16, control_dt=0.05, max_acceleration=0.0, max_angular_velocity=2.0,
                    robot_radius=0.325, goal_x=float("inf")):
    """A filled tmpc_episode_options for Episode.step / EpisodeWorld."""
    return TmpcEpisodeOptions(C.sizeof(TmpcEpisodeOptions), int(substeps), int(timeout_ticks), int(max_episodes), float(control_dt),
                              float(max_acceleration), float(max_angular_velocity), float(robot_radius), float(goal_x))


class Episode(StackEntries):
    """The entry point of tmpc_hip_episode.h on a BatchedSolver's library and handle (raw device pointers, like BatchedSolver's own wrappers).
    Enqueued on the handle's stream; a failure raises solver.TmpcError with the library's message."""
    _SIGNATURES = _SIGNATURES

    def step(self, n_scenes, n_slots, P, options, d_cmd, d_plant, d_plant0, d_count, d_raw_pos, d_raw_vel, d_raw_radius, d_raw_pos0, d_raw_vel0,
             d_episode, d_episode_f, d_log, d_was_reset, d_state4, d_box=None, d_goal=None, d_state_nx=None, d_state_batch=None,
             d_planner_ids=None, d_selection=None, d_segment=None):
        """tmpc_episode_step: one control period of n_scenes worlds (the header states the arrays and the seven steps)."""
        self._call("tmpc_episode_step", n_scenes, n_slots, P, None if options is None else C.byref(options), d_cmd, d_plant, d_plant0, d_count,
                   d_raw_pos, d_raw_vel, d_raw_radius, d_raw_pos0, d_raw_vel0, d_box, d_goal, d_episode, d_episode_f, d_log, d_was_reset, d_state4,
                   d_state_nx, d_state_batch, d_planner_ids, d_selection, d_segment)


class EpisodeWorld:
    """The torch tensors of n_scenes worlds on a BatchedSolver's device, from numpy scene descriptions, and their step.

    plant0 [Q][4] = (x, y, psi, v) -- cos / sin of the start heading are evaluated here, once -- or [Q][6] as the device holds it;
    raw_pos0 / raw_vel0 [Q][n_slots][2], raw_radius [Q][n_slots], count [Q] (default: every slot), box [Q][4] and goal [Q][3] optional.
    The tensors are attributes under the names of the header without `d_`: plant, plant0, count, raw_pos, raw_vel, raw_radius, raw_pos0,
    raw_vel0, box, goal, episode, episode_f, log_rows, was_reset, state4, state_nx [Q][nx], state_batch [Q P][nx], planner_ids [Q][P],
    selection [Q][3], segment [Q] -- the cross-tick state of the planner starts as the freshly constructed planner's, like after a reset."""

    def __init__(self, solver, P, plant0, raw_pos0, raw_vel0, raw_radius, options, count=None, box=None, goal=None):
        import torch
        self.solver, self.entry, self.options, self.P = solver, Episode(solver), options, int(P)
        dev = torch.device(f"cuda:{solver.device}")
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        plant0 = np.asarray(plant0, float)
        if plant0.shape[1] == 4:
            plant0 = np.concatenate([plant0, np.cos(plant0[:, 2:3]), np.sin(plant0[:, 2:3])], 1)
        raw_pos0 = np.asarray(raw_pos0, float)
        self.Q, self.n_slots, self.nx = Q, R, nx = len(plant0), raw_pos0.shape[1], int(solver.dims.nx)
        assert plant0.shape == (Q, 6) and raw_pos0.shape == (Q, R, 2) and np.shape(raw_vel0) == (Q, R, 2) and np.shape(raw_radius) == (Q, R)
        self.plant0, self.plant = up(plant0, np.float64), up(plant0, np.float64)
        self.raw_pos0, self.raw_vel0, self.raw_radius = up(raw_pos0, np.float64), up(raw_vel0, np.float64), up(raw_radius, np.float64)
        self.raw_pos, self.raw_vel = self.raw_pos0.clone(), self.raw_vel0.clone()
        self.count = up(np.full(Q, R) if count is None else count, np.int32)
        self.box = None if box is None else up(np.asarray(box, float).reshape(Q, 4), np.float64)
        self.goal = None if goal is None else up(np.asarray(goal, float).reshape(Q, 3), np.float64)
        self.episode = torch.zeros((Q, 4), dtype=torch.int32, device=dev)
        self.episode_f = torch.zeros((Q, 2), dtype=torch.float64, device=dev)
        self.log_rows = torch.zeros((Q, int(options.max_episodes), 4), dtype=torch.float64, device=dev)
        self.was_reset = torch.zeros((Q,), dtype=torch.uint8, device=dev)
        self.state4 = self.plant[:, 0:4].contiguous()
        self.state_nx = torch.zeros((Q, nx), dtype=torch.float64, device=dev)
        self.state_nx[:, 0:4] = self.state4
        self.state_batch = self.state_nx.repeat_interleave(self.P, 0).contiguous()
        self.planner_ids = torch.full((Q, self.P), -1, dtype=torch.int32, device=dev)
        self.selection = up(np.tile(np.array([-1, 0, -1], np.int32), (Q, 1)), np.int32)
        self.segment = torch.full((Q,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)

    def step(self, d_cmd):
        """One control period from the commands d_cmd (f64 [Q][2], a raw device pointer), on the handle's stream; nothing is read back."""
        ptr = lambda t: None if t is None else t.data_ptr()
        self.entry.step(self.Q, self.n_slots, self.P, self.options, d_cmd, ptr(self.plant), ptr(self.plant0), ptr(self.count), ptr(self.raw_pos),
                        ptr(self.raw_vel), ptr(self.raw_radius), ptr(self.raw_pos0), ptr(self.raw_vel0), ptr(self.episode), ptr(self.episode_f),
                        ptr(self.log_rows), ptr(self.was_reset), ptr(self.state4), d_box=ptr(self.box), d_goal=ptr(self.goal),
                        d_state_nx=ptr(self.state_nx), d_state_batch=ptr(self.state_batch), d_planner_ids=ptr(self.planner_ids),
                        d_selection=ptr(self.selection), d_segment=ptr(self.segment))

    def log(self):
        """After a synchronisation of the handle's stream, as numpy: per scene dict(rows [min(finished, max_episodes)][4] = (duration,
        completed, collision ticks, max intrusion) of the finished episodes, finished, ticks, collisions, max_intrusion, intrusion --
        the running counters of the episode under way)."""
        self.solver.synchronize()
        ep, ef, rows = self.episode.cpu().numpy(), self.episode_f.cpu().numpy(), self.log_rows.cpu().numpy()
        return [dict(rows=rows[q, :min(int(ep[q, 2]), rows.shape[1])].copy(), finished=int(ep[q, 2]), ticks=int(ep[q, 0]), collisions=int(ep[q, 1]),
                     max_intrusion=float(ef[q, 0]), intrusion=float(ef[q, 1])) for q in range(self.Q)]
