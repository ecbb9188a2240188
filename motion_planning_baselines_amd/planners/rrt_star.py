"""RRTStar and InfRRTStar with the reference's class surface (mp_baselines/planners/rrt_star.py:84-276 over rrt_base.py),
for B independent problems at once on the GPU.

The reference grows one tree of Python OptimalNode objects per planner, one configuration at a time.  Here every problem
(one start / goal pair, or one copy of it) is one workgroup of ONE persistent launch of mpb_rrt_star_run
(csrc/mpb_rrt_star.hip), which restates the loop body line by line -- the two stopping rules, the goal / sample draw, the
informed rejection, nearest node, extend_path, safe_path, the deletion of a reached pre-sample, goal detection, the
radius neighbourhood, the rewire walk in index order with cost propagation after every rewire, the retrace and
purge_duplicates_from_traj.

Differences from the reference, besides those every sample-based planner here shares (rrt_base.py):
  - only the radius neighbourhood is served: n_knn > 0 is refused (torch.topk leaves the order of ties unspecified);
  - `initial_nodes` is refused; n_iters < 2 is refused (the reference divides by n_iters - 1);
  - a run cut by `max_time` still returns the best path found so far, as the reference does;
  - an emptied pre-sample pool ends a problem that has a path with FOUND and stop_reason POOL_EMPTY.
"""
import torch

from .. import ops
from .rrt_base import RRTBase


class RRTStar(RRTBase):
    NAME, Workspace = 'RRTStar', ops.RRTStarWorkspace

    def __init__(self, task=None, n_iters=None, start_state_pos=None, n_iters_after_success=None, max_best_cost_iters=1000,
                 cost_eps=1e-2, step_size=0.1, n_radius=1., n_knn=0, max_time=60., goal_prob=.1, goal_state_pos=None,
                 tensor_args=None, n_pre_samples=10000, pre_samples=None, informed=False, seed=0, chunk_iters=1024,
                 max_nodes=None, max_path_nodes=512, **kwargs):
        assert n_knn >= 0, 'knn parameter is < 0'
        if n_knn > 0:
            raise ValueError('RRTStar: n_knn > 0 is not served -- torch.topk leaves the order of tied distances unspecified, so the '
                             'k-nearest neighbourhood has no reproducible reference; use the radius neighbourhood (n_knn = 0, n_radius)')
        if n_iters is None or int(n_iters) < 2:
            raise ValueError('RRTStar: n_iters must be at least 2 (the reference divides by n_iters - 1)')
        self.n_iters_after_success = None if n_iters_after_success is None else int(n_iters_after_success)
        self.max_best_cost_iters = int(max_best_cost_iters) if max_best_cost_iters is not None else int(n_iters)
        self.cost_eps = float(cost_eps)
        self.n_knn = 0
        self.goal_prob = float(goal_prob)
        self.informed = bool(informed)
        self.costs = None
        super().__init__(task, n_iters, start_state_pos, step_size, n_radius, max_time, goal_state_pos, tensor_args, n_pre_samples,
                         pre_samples, seed, chunk_iters, max_nodes, max_path_nodes)

    def optimize_batched(self, sample_idx=None, goal_draw=None, n_copies=1, problem_offset=0, **observation):
        """All problems (every start / goal row, n_copies times, copy-major) in one launch sequence.
        sample_idx, goal_draw: both None (device Philox; problem b draws from stream problem_offset + b) or both
        (B, n_iters + 1) int32 recorded draws.  observation: `informed` (default: the constructor's) and `eps` (default
        1e-6) as in the reference; `on_chunk(planner, workspace, costs, lengths, status)` is called after every launch.
        Returns (paths (B, max_path_nodes, D), lengths (B,) int32 -- 0 where no path --, status (B,) int32) as device
        tensors; leaves self.workspace, self.status and self.costs ((B,) goal costs, inf where no path) behind."""
        if observation.get('initial_nodes', None) is not None:
            raise ValueError('RRTStar: initial_nodes is not served (the tree is built on the device from the start state)')
        out = self._run_batched([sample_idx, goal_draw], n_copies, problem_offset, on_chunk=observation.get('on_chunk', None),
                                informed=bool(observation.get('informed', self.informed)), eps=float(observation.get('eps', 1e-6)))
        return out['paths'], out['lengths'], out['status']

    def _outputs(self, B, D):
        self.costs = torch.full((B,), float('inf'), device=self.device, dtype=torch.float32)
        return dict(super()._outputs(B, D), costs=self.costs)

    def _launch(self, ws, draws, out, it, n, problem_offset, informed, eps):
        ops.rrt_star_run(ws.buf, ws, self.task.geom, self.pre_samples, draws[0], draws[1], out['paths'], out['lengths'], out['costs'],
                         out['status'], it, n, self.total_iters, self.step_size, self.n_radius,
                         max_best_cost_iters=self.max_best_cost_iters, n_iters_after_success=self.n_iters_after_success,
                         informed=informed, goal_prob=self.goal_prob, cost_eps=self.cost_eps, eps=eps, seed=self.seed,
                         problem_offset=problem_offset)


class InfRRTStar(RRTStar):
    """Informed RRT* (rrt_star.py:273-276)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, informed=True, **kwargs)
