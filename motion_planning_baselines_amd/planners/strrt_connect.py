"""STRRTConnect: RRT-Connect in (configuration, time) among obstacles whose motion is known, for B independent problems at once on the GPU
(build-defined, DESIGN.md section 10: the reference has nothing like it; the definition is include/mpb.h's).

Time lives on the row grid of a geometry.MovingObstacleField: the caller chooses n_rows = R, row h is the field's time
t_start + h (t_end - t_start) / (R - 1) -- the clock of MovingObstacleField.rows(R) and of ops.DeviceMovingObstacles(robot, field, device,
R).  Every problem starts at (start, row 0) and ends at (goal, row R - 1); a plan is a dense (R, D) trajectory, one configuration per row,
that moves joint k by at most w_k = fp32(dq_max_k * dt_row) per row and is collision-free AT THE ROWS -- the statement
PlanningTask.check_trajs_moving makes.  Obstacle positions are never interpolated between rows: a finer clock is a larger n_rows.  Waiting
(at the goal too) is an ordinary edge with little or no motion.  Every problem (one start / goal pair, or one copy of it) is one
single-wave workgroup of ONE persistent launch of mpb_strrt_run (csrc/mpb_strrt.hip), launched in chunks of `chunk_iters` iterations
between which `max_time` is honoured.

Built on MPPlanner, not on RRTBase: RRTBase's constructor, workspace and launch sequence are those of a planner without a clock (step_size
and n_radius, n_iters + 1 loop bodies, a pre-sample pool kept as a list in LDS and therefore at most 16 384 entries, ops.rrt_init, paths and
lengths as outputs), and it must not change here; what fits is restated below with the same names and meaning -- `chunk_iters`, `max_time`
between launches, copy-major `n_copies` with `problem_offset`, reset()'s top-up of the pre-samples, PATH_TOO_LONG raising.

shortcut(result) -- or shortcut_iters > 0 at construction -- runs the space-time shortcut pass (ops.st_shortcut) over the found plans: a
plan is a chain of random tree vertices joined by straight pieces, and the pass straightens it on the same clock.

The result seeds the optimisers: CHOMP(initial_particle_means=trajs) with a CostCollision(field=moving_field) member at
n_support_points = n_rows sees row h at the same time the plan was checked at.
"""
import time
import types

import numpy as np
import torch

from .. import ops
from .._lib import MPBError
from ..geometry import MovingObstacleField
from .base import MPPlanner, require_cuda


class STRRTConnect(MPPlanner):
    NAME = 'STRRTConnect'

    def __init__(self, task=None, moving_field=None, n_rows=None, start_state_pos=None, goal_state_pos=None, n_iters=None, max_step_rows=8,
                 dq_max=None, n_pre_samples=4096, pre_samples=None, seed=0, chunk_iters=1024, max_nodes=None, max_path_nodes=512,
                 max_time=60., tensor_args=None, shortcut_iters=0, **kwargs):
        assert start_state_pos is not None and goal_state_pos is not None
        super().__init__(name=self.NAME, tensor_args=tensor_args if tensor_args is not None else getattr(task, 'tensor_args', None))
        self.device = require_cuda(self.tensor_args)
        self.task = task
        if getattr(task, 'self_field', None) is not None:       # (the kernel's static predicate knows obstacles only)
            task.require_no_self_field(f'{self.NAME} (the space-time RRT kernel)')
        if getattr(task, 'sdf_field', None) is not None:
            task.require_no_sdf_field(f'{self.NAME} (the space-time RRT kernel)')
        if not isinstance(moving_field, MovingObstacleField):
            raise TypeError('moving_field must be a geometry.MovingObstacleField')
        self.moving_field = moving_field
        self.n_rows = int(n_rows)
        if not ops.STRRT_MIN_ROWS <= self.n_rows <= ops.STRRT_MAX_ROWS:
            raise ValueError(f'n_rows = {self.n_rows} outside {ops.STRRT_MIN_ROWS} .. {ops.STRRT_MAX_ROWS} (MPB_MOVING_MAX_ROWS): the time grid '
                             f'has a start row, rows to sample and a goal row')
        D = task.q_dim
        if dq_max is None:
            dq_max = getattr(task.robot, 'dq_max_np', None)
        if dq_max is None:
            raise ValueError('dq_max: the robot carries no velocity limits (Robot(dq_max=...)) and none were given')
        dq = np.asarray(dq_max.detach().cpu().numpy() if isinstance(dq_max, torch.Tensor) else dq_max, dtype=np.float64).reshape(-1)
        if dq.shape != (D,) or not (np.all(np.isfinite(dq)) and np.all(dq > 0)):
            raise ValueError(f'dq_max must hold {D} finite limits > 0 (got {dq.tolist()})')
        self.dt_row = (moving_field.t_end - moving_field.t_start) / (self.n_rows - 1)        # fp64
        if not self.dt_row > 0:
            raise ValueError('moving_field: t_end must be greater than t_start for a space-time plan')
        self.w_np = (dq * self.dt_row).astype(np.float32)                                    # w_k = fp32(dq_max_k * dt_row)
        if not np.all(self.w_np > 0):
            raise ValueError('dq_max * dt_row underflows fp32')
        self.w = torch.from_numpy(self.w_np).to(self.device)
        self.starts = torch.as_tensor(start_state_pos, dtype=torch.float32).reshape(-1, D).to(self.device).contiguous()
        self.goals = torch.as_tensor(goal_state_pos, dtype=torch.float32).reshape(-1, D).to(self.device).contiguous()
        if self.starts.shape != self.goals.shape:
            raise ValueError('start_state_pos and goal_state_pos must have the same shape, (D,) or (B, D)')
        self.n_iters = self.total_iters = int(n_iters)
        self.max_step_rows = int(max_step_rows)
        if self.max_step_rows < 1:
            raise ValueError('max_step_rows must be at least 1')
        self.n_pre_samples = int(n_pre_samples)
        if not 1 <= self.n_pre_samples <= ops.STRRT_MAX_PRE_SAMPLES:
            raise ValueError(f'n_pre_samples must be in 1 .. {ops.STRRT_MAX_PRE_SAMPLES}')
        self.pre_samples = None if pre_samples is None else torch.as_tensor(pre_samples, dtype=torch.float32).to(self.device)
        self.seed, self.chunk_iters, self.max_time = int(seed), max(1, int(chunk_iters)), float(max_time)
        self.max_nodes = int(max_nodes) if max_nodes is not None else self.total_iters + 1   # a tree gains at most one node per iteration
        self.max_path_nodes = int(max_path_nodes)
        self.shortcut_iters = int(shortcut_iters)            # 0: no shortcut pass, the planner as it is without the argument
        if not 0 <= self.shortcut_iters <= ops.STS_MAX_ITERS:
            raise ValueError(f'shortcut_iters = {self.shortcut_iters} outside 0 .. {ops.STS_MAX_ITERS}')
        self.moving = ops.DeviceMovingObstacles(task.robot, moving_field, self.device, self.n_rows)
        self.workspace = self.status = None
        self.reset()

    def reset(self):
        """Top the pre-samples up to n_pre_samples configurations free of the task's STATIC obstacles (task.random_coll_free_q); nothing is
        ever deleted from them."""
        have = 0 if self.pre_samples is None else self.pre_samples.shape[0]
        if have > self.n_pre_samples:
            raise ValueError(f'pre_samples holds {have} configurations, n_pre_samples is {self.n_pre_samples}')
        fresh = self.task.random_coll_free_q(self.n_pre_samples - have, 1000)
        self.pre_samples = (fresh if self.pre_samples is None else torch.cat((self.pre_samples, fresh), dim=0)).contiguous()

    def optimize_batched(self, n_copies=1, sample_idx=None, sample_row=None, with_log=False, problem_offset=0, **observation):
        """All problems (every start / goal row, n_copies times, copy-major) in one launch sequence.  sample_idx / sample_row: both None
        (device Philox; problem b draws from stream problem_offset + b of `seed`) or both (B, n_iters) int32 recorded draws.  Returns a
        record: trajs (B, R, D) (zero where not found), found (B,) bool, status (B,) int32 (ops.STRRT_*), vertex_q (B, max_path_nodes, D),
        vertex_row (B, max_path_nodes) and n_vertices (B,) int32 -- the plan's tree nodes in ascending rows, from (start, 0) to
        (goal, R - 1) --, log (B, n_iters, ops.STRRT_LOG_WORDS) int32 with with_log, else None.  The trees stay readable through
        ops.strrt_trees(self.workspace).  With shortcut_iters > 0 the found plans then go through shortcut(): trajs are the shortcut
        plans, raw_trajs the plans as joined, shortcut the ops.STShortcut record."""
        n_copies = int(n_copies)
        starts = self.starts.repeat(n_copies, 1) if n_copies > 1 else self.starts
        goals = self.goals.repeat(n_copies, 1) if n_copies > 1 else self.goals
        B, D = starts.shape
        dev, R, T = self.device, self.n_rows, self.total_iters
        ws = ops.STRRTWorkspace(B, self.max_nodes, D, R, dev)
        ops.strrt_init(ws.buf, ws, starts, goals, self.w, self.task.geom, self.moving)
        trajs = torch.zeros(B, R, D, device=dev, dtype=torch.float32)
        vertex_q = torch.zeros(B, self.max_path_nodes, D, device=dev, dtype=torch.float32)
        vertex_row = torch.zeros(B, self.max_path_nodes, device=dev, dtype=torch.int32)
        n_vertices = torch.zeros(B, device=dev, dtype=torch.int32)
        status = torch.zeros(B, device=dev, dtype=torch.int32)
        log = torch.full((B, T, ops.STRRT_LOG_WORDS), ops.STRRT_LOG_NONE, device=dev, dtype=torch.int32) if with_log else None
        if (sample_idx is None) != (sample_row is None):
            raise ValueError('sample_idx and sample_row are given together or not at all')
        draws = [d if d is None else torch.as_tensor(d, dtype=torch.int32).to(dev).reshape(B, T).contiguous() for d in (sample_idx, sample_row)]
        t0 = time.perf_counter()
        it = 0
        while it < T:
            n = min(self.chunk_iters, T - it)
            ops.strrt_run(ws.buf, ws, self.task.geom, self.moving, self.w, self.pre_samples, draws[0], draws[1], trajs, vertex_q, vertex_row,
                          n_vertices, status, it, n, T, self.max_step_rows, seed=self.seed, problem_offset=problem_offset, log=log)
            it += n
            if it < T:
                if not bool((status == ops.STRRT_RUNNING).any().item()):
                    break
                if time.perf_counter() - t0 >= self.max_time:       # chunk granularity
                    break
        self.workspace, self.status = ws, status
        if bool((status == ops.STRRT_PATH_TOO_LONG).any().item()):
            raise MPBError(f'{self.name}: a plan has more than max_path_nodes = {self.max_path_nodes} tree nodes (status PATH_TOO_LONG); '
                           f'construct the planner with a larger max_path_nodes')
        found = status == ops.STRRT_FOUND
        trajs[~found] = 0.                                          # (a discarded join leaves its rows behind)
        result = types.SimpleNamespace(trajs=trajs, found=found, status=status, vertex_q=vertex_q, vertex_row=vertex_row,
                                       n_vertices=n_vertices, log=log)
        if self.shortcut_iters > 0:
            result.raw_trajs = trajs
            result.shortcut = self.shortcut(result, self.shortcut_iters, problem_offset=problem_offset)
            result.trajs = result.shortcut.trajs
        return result

    def shortcut(self, result, n_iters=64, **kw):
        """Shortcut the found trajectories of an optimize_batched record on their own clock (ops.st_shortcut with valid=result.found,
        this planner's static geometry, moving-obstacle buffer and w; the seed defaults to the planner's).  The vertex lists of the record
        describe the plan before the pass.  Returns an ops.STShortcut; rows of problems that were not found pass through (zeros)."""
        kw.setdefault('seed', self.seed)
        return ops.st_shortcut(result.trajs, self.task.geom, self.moving, self.w, n_iters, valid=result.found, **kw)

    def certify(self, result, c_req=0.0, **kw):
        """Certify the found trajectories of an optimize_batched record over the whole continuum of their clock
        (PlanningTask.certify_trajs_moving on this planner's field: the static obstacles and the moving ones between the rows too, the
        required clearance raised by the field's chord deviation; **kw: max_depth, max_intervals, slack).  Only the `found` plans are
        submitted; the others come out with status ops.STC_NOT_VALID and the outputs of a trajectory without a witness (-1, 0, NaN,
        -1, ops.STC_NO_OBSTACLE, 0; n_evals 0, depth_max -1, margin_cert -inf).  Returns an ops.TrajCertificate over all B problems."""
        found = result.found
        B = found.shape[0]
        idx = torch.nonzero(found).flatten()
        part = self.task.certify_trajs_moving(result.trajs[idx].contiguous(), self.moving_field, c_req=c_req, **kw)
        dev = result.trajs.device
        out_i = torch.tensor([ops.STC_NOT_VALID, -1, -1, ops.STC_NO_OBSTACLE, 0, -1], device=dev, dtype=torch.int32).repeat(B, 1)
        out_f = torch.tensor([0.0, 0.0, float('-inf')], device=dev, dtype=torch.float32).repeat(B, 1)
        if idx.numel():
            out_i[idx] = torch.stack([part.status, part.witness_row, part.witness_link, part.witness_obstacle, part.n_evals, part.depth_max], 1)
            out_f[idx] = torch.stack([part.witness_s, part.witness_eta, part.margin_cert], 1)
        return ops.TrajCertificate(out_i, out_f, part.slack, part.c_req, self.moving_field.t_start, self.dt_row, part.chord_deviation)

    def optimize(self, opt_iters=None, **observation):
        """One problem: the (R, D) trajectory or None; several: a list of those."""
        r = self.optimize_batched(**observation)
        out = [r.trajs[b].clone() if f else None for b, f in enumerate(r.found.tolist())]
        return out[0] if len(out) == 1 else out

    def render(self, ax, **kwargs):
        raise NotImplementedError
