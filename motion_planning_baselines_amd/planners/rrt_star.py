"""RRTStar and InfRRTStar with the reference's class surface (mp_baselines/planners/rrt_star.py:84-276 over rrt_base.py),
for B independent problems at once on the GPU.

The reference grows one tree of Python OptimalNode objects per planner, one configuration at a time.  Here every problem
(one start / goal pair, or one copy of it) is one workgroup of ONE persistent launch of mpb_rrt_star_run
(csrc/mpb_rrt_star.hip), which restates the loop body line by line -- the two stopping rules, the goal / sample draw, the
informed rejection, nearest node, extend_path, safe_path, the deletion of a reached pre-sample, goal detection, the
radius neighbourhood, the rewire walk in index order with cost propagation after every rewire, the retrace and
purge_duplicates_from_traj.

Differences from the reference, all documented in DESIGN.md section 10:
  - only the radius neighbourhood is served: n_knn > 0 is refused (torch.topk leaves the order of ties unspecified);
  - `initial_nodes` is refused; n_iters < 2 is refused (the reference divides by n_iters - 1);
  - `max_time` is honoured between launches of `chunk_iters` loop bodies (default 1024), not per iteration; a run cut
    there still returns the best path found so far, as the reference does;
  - an emptied pre-sample pool is not refilled on the device (status POOL_EMPTY, or FOUND with stop_reason POOL_EMPTY);
  - a retrace of more than `max_path_nodes` tree nodes (before duplicates are purged) raises (status PATH_TOO_LONG);
  - the pre-sample pool holds at most 16 384 configurations (the kernel keeps its index list in LDS).
"""
import time

import torch

from .. import ops
from .._lib import MPBError
from .base import MPPlanner, require_cuda
from .rrt_connect import paths_to_list


class RRTStar(MPPlanner):

    def __init__(self, task=None, n_iters=None, start_state_pos=None, n_iters_after_success=None, max_best_cost_iters=1000,
                 cost_eps=1e-2, step_size=0.1, n_radius=1., n_knn=0, max_time=60., goal_prob=.1, goal_state_pos=None,
                 tensor_args=None, n_pre_samples=10000, pre_samples=None, informed=False, seed=0, chunk_iters=1024,
                 max_nodes=None, max_path_nodes=512, **kwargs):
        assert start_state_pos is not None and goal_state_pos is not None
        assert n_knn >= 0, 'knn parameter is < 0'
        if n_knn > 0:
            raise ValueError('RRTStar: n_knn > 0 is not served -- torch.topk leaves the order of tied distances unspecified, so the '
                             'k-nearest neighbourhood has no reproducible reference; use the radius neighbourhood (n_knn = 0, n_radius)')
        if n_iters is None or int(n_iters) < 2:
            raise ValueError('RRTStar: n_iters must be at least 2 (the reference divides by n_iters - 1)')
        super().__init__(name='RRTStar', tensor_args=tensor_args)
        self.device = require_cuda(tensor_args)
        self.task = task
        self.n_iters = int(n_iters)
        self.n_iters_after_success = None if n_iters_after_success is None else int(n_iters_after_success)
        self.max_best_cost_iters = int(max_best_cost_iters) if max_best_cost_iters is not None else self.n_iters
        self.cost_eps = float(cost_eps)
        self.n_knn = 0
        self.goal_prob = float(goal_prob)
        self.informed = bool(informed)
        self.step_size, self.n_radius, self.max_time = float(step_size), float(n_radius), float(max_time)
        self.start_state_pos, self.goal_state_pos = start_state_pos, goal_state_pos
        self.starts = torch.as_tensor(start_state_pos, dtype=torch.float32).reshape(-1, task.q_dim).to(self.device).contiguous()
        self.goals = torch.as_tensor(goal_state_pos, dtype=torch.float32).reshape(-1, task.q_dim).to(self.device).contiguous()
        if self.starts.shape != self.goals.shape:
            raise ValueError('start_state_pos and goal_state_pos must have the same shape, (D,) or (B, D)')
        self.n_pre_samples = int(n_pre_samples)
        if not 1 <= self.n_pre_samples <= ops.RRT_MAX_PRE_SAMPLES:
            raise ValueError(f'n_pre_samples must be in 1 .. {ops.RRT_MAX_PRE_SAMPLES} (the kernel keeps the pool list in LDS)')
        self.pre_samples = None if pre_samples is None else torch.as_tensor(pre_samples, dtype=torch.float32).to(self.device)
        self.seed = int(seed)
        self.chunk_iters = max(1, int(chunk_iters))
        self.total_iters = self.n_iters + 1                        # `while iteration < n_iters: iteration += 1` (rrt_star.py:162-164)
        self.max_nodes = int(max_nodes) if max_nodes is not None else self.total_iters + 1
        self.max_path_nodes = int(max_path_nodes)
        self.workspace = None
        self.status = None
        self.costs = None
        self.reset()

    def reset(self):
        """Top the pool up to n_pre_samples collision-free configurations (rrt_base.py:47-54)."""
        have = 0 if self.pre_samples is None else self.pre_samples.shape[0]
        if have > self.n_pre_samples:
            raise ValueError(f'pre_samples holds {have} configurations, n_pre_samples is {self.n_pre_samples}')
        fresh = self.task.random_coll_free_q(self.n_pre_samples - have, 1000)
        self.pre_samples = (fresh if self.pre_samples is None else torch.cat((self.pre_samples, fresh), dim=0)).contiguous()

    def optimize_batched(self, sample_idx=None, goal_draw=None, n_copies=1, problem_offset=0, **observation):
        """All problems (every start / goal row, n_copies times, copy-major) in one launch sequence.
        sample_idx, goal_draw: both None (device Philox; problem b draws from stream problem_offset + b) or both
        (B, n_iters + 1) int32 recorded draws.  observation: `informed` (default: the constructor's) and `eps` (default
        1e-6) as in the reference; `on_chunk(planner, workspace, costs, lengths, status)` is called after every launch.
        Returns (paths (B, max_path_nodes, D), lengths (B,) int32 -- 0 where no path --, status (B,) int32) as device
        tensors; leaves self.workspace, self.status and self.costs ((B,) goal costs, inf where no path) behind."""
        if observation.get('initial_nodes', None) is not None:
            raise ValueError('RRTStar: initial_nodes is not served (the tree is built on the device from the start state)')
        informed = bool(observation.get('informed', self.informed))
        eps = float(observation.get('eps', 1e-6))
        on_chunk = observation.get('on_chunk', None)
        n_copies = int(n_copies)
        starts = self.starts.repeat(n_copies, 1) if n_copies > 1 else self.starts
        goals = self.goals.repeat(n_copies, 1) if n_copies > 1 else self.goals
        B, D = starts.shape
        ws = ops.RRTStarWorkspace(B, self.max_nodes, self.n_pre_samples, D, self.device)
        geom = self.task.geom
        ops.rrt_star_init(ws.buf, ws, starts, goals, geom)
        paths = torch.zeros(B, self.max_path_nodes, D, device=self.device, dtype=torch.float32)
        lengths = torch.zeros(B, device=self.device, dtype=torch.int32)
        costs = torch.full((B,), float('inf'), device=self.device, dtype=torch.float32)
        status = torch.zeros(B, device=self.device, dtype=torch.int32)
        if (sample_idx is None) != (goal_draw is None):
            raise ValueError('sample_idx and goal_draw are given together or not at all')
        if sample_idx is not None:
            sample_idx = torch.as_tensor(sample_idx, dtype=torch.int32).to(self.device).reshape(B, self.total_iters).contiguous()
            goal_draw = torch.as_tensor(goal_draw, dtype=torch.int32).to(self.device).reshape(B, self.total_iters).contiguous()
        t0 = time.perf_counter()
        it = 0
        while it < self.total_iters:
            n = min(self.chunk_iters, self.total_iters - it)
            ops.rrt_star_run(ws.buf, ws, geom, self.pre_samples, sample_idx, goal_draw, paths, lengths, costs, status, it, n,
                             self.total_iters, self.step_size, self.n_radius, max_best_cost_iters=self.max_best_cost_iters,
                             n_iters_after_success=self.n_iters_after_success, informed=informed, goal_prob=self.goal_prob,
                             cost_eps=self.cost_eps, eps=eps, seed=self.seed, problem_offset=problem_offset)
            it += n
            if on_chunk is not None:
                on_chunk(self, ws, costs, lengths, status)
            if it < self.total_iters:
                if not bool((status == ops.RRT_RUNNING).any().item()):
                    break
                if time.perf_counter() - t0 >= self.max_time:       # chunk granularity
                    break
        self.workspace, self.status, self.costs = ws, status, costs
        if bool((status == ops.RRT_PATH_TOO_LONG).any().item()):
            raise MPBError(f'RRTStar: a path has more than max_path_nodes = {self.max_path_nodes} tree nodes (status '
                           f'PATH_TOO_LONG); construct the planner with a larger max_path_nodes')
        return paths, lengths, status

    def optimize(self, opt_iters=None, **observation):
        """One problem: the (n, D) path or None like the reference; several: a list of those."""
        paths, lengths, status = self.optimize_batched(**observation)
        out = paths_to_list(paths, lengths)
        return out[0] if len(out) == 1 else out

    def render(self, ax, **kwargs):
        raise NotImplementedError


class InfRRTStar(RRTStar):
    """Informed RRT* (rrt_star.py:273-276)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, informed=True, **kwargs)
