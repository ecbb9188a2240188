"""What the batched sample-based planners share (the reference keeps its own in mp_baselines/planners/rrt_base.py): the pool of
pre-samples, the problems' starts and goals, and the driver that runs B problems to completion in launches of `chunk_iters` iterations.
RRTConnect (rrt_connect.py) and RRTStar (rrt_star.py) add their constructor arguments, their workspace kind, the recorded draws they
accept, the launch of one chunk, and what they are launched on (`_scene`): the family refuses a task with a self_field or an sdf_field
by name -- its kernels' predicate knows obstacles only --, RRTConnect alone serves one built with world_predicate=True.

Differences from the reference they share, all documented in DESIGN.md section 10:
  - `max_time` is honoured between launches of `chunk_iters` iterations (default 1024), not per iteration;
  - an emptied pre-sample pool is not refilled on the device: the problem ends with status POOL_EMPTY (cannot happen while
    n_pre_samples > n_iters: an iteration deletes at most one entry);
  - a path of more than `max_path_nodes` tree nodes (before duplicates are purged) raises (status PATH_TOO_LONG);
  - the pre-sample pool holds at most 16 384 configurations (the kernel keeps its index list in LDS).
"""
import time

import torch

from .. import ops
from .._lib import MPBError
from .base import MPPlanner, require_cuda


def paths_to_list(paths, lengths):
    """(paths (B, Lmax, D), lengths (B,)) -> list of (n_b, D) device tensors, None where lengths[b] == 0."""
    return [paths[b, :n].clone() if n > 0 else None for b, n in enumerate(lengths.tolist())]


class RRTBase(MPPlanner):
    # a planner sets NAME (MPPlanner.name) and Workspace (its kind: ops.RRTWorkspace or ops.RRTStarWorkspace) and defines optimize_batched
    # over _run_batched, and _launch(ws, draws, out, it, n, problem_offset, **options): ONE launch of its kernel for iterations
    # it .. it + n - 1 of every problem (draws: the recorded draws, each (B, total_iters) int32 on the device, or all None; out: _outputs())

    def __init__(self, task=None, n_iters=None, start_state_pos=None, step_size=0.1, n_radius=1., max_time=60.,
                 goal_state_pos=None, tensor_args=None, n_pre_samples=10000, pre_samples=None, seed=0, chunk_iters=1024,
                 max_nodes=None, max_path_nodes=512, **kwargs):
        assert start_state_pos is not None and goal_state_pos is not None
        super().__init__(name=self.NAME, tensor_args=tensor_args)
        self.device = require_cuda(tensor_args)
        self.task = task
        self.scene = self._scene(task)
        self.n_iters = int(n_iters)
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
        self.total_iters = self.n_iters + 1                        # `while iteration < n_iters: iteration += 1` (rrt_connect.py:115-116, rrt_star.py:162-164)
        self.max_nodes = int(max_nodes) if max_nodes is not None else self.total_iters + 1
        self.max_path_nodes = int(max_path_nodes)
        self.workspace = self.status = None
        self.reset()

    def _scene(self, task):
        """What the planner's kernels are launched on.  Their in-kernel predicate knows obstacles only: a task with a self_field or
        an sdf_field is refused by name (RRTConnect overrides this: it serves a task built with world_predicate=True)."""
        if getattr(task, 'self_field', None) is not None:
            task.require_no_self_field(f'{self.NAME} (the batched RRT kernels)')
        if getattr(task, 'sdf_field', None) is not None:
            task.require_no_sdf_field(f'{self.NAME} (the batched RRT kernels)')
        return task.geom

    def reset(self):
        """Top the pool up to n_pre_samples collision-free configurations (rrt_base.py:47-54)."""
        have = 0 if self.pre_samples is None else self.pre_samples.shape[0]
        if have > self.n_pre_samples:
            raise ValueError(f'pre_samples holds {have} configurations, n_pre_samples is {self.n_pre_samples}')
        fresh = self.task.random_coll_free_q(self.n_pre_samples - have, 1000)
        self.pre_samples = (fresh if self.pre_samples is None else torch.cat((self.pre_samples, fresh), dim=0)).contiguous()

    def _outputs(self, B, D):
        """The device tensors the launches write, by name."""
        return dict(paths=torch.zeros(B, self.max_path_nodes, D, device=self.device, dtype=torch.float32),
                    lengths=torch.zeros(B, device=self.device, dtype=torch.int32),
                    status=torch.zeros(B, device=self.device, dtype=torch.int32))

    def _run_batched(self, draws, n_copies, problem_offset, on_chunk=None, **options):
        """All problems (every start / goal row, n_copies times, copy-major) in one launch sequence, `max_time` honoured
        between launches; on_chunk(planner, workspace, costs or None, lengths, status) is called after every launch.
        Leaves self.workspace and self.status behind and returns _outputs() as the launches left it: paths
        (B, max_path_nodes, D), lengths (B,) int32 -- 0 where no path --, status (B,) int32, and what the planner adds."""
        n_copies = int(n_copies)
        starts = self.starts.repeat(n_copies, 1) if n_copies > 1 else self.starts
        goals = self.goals.repeat(n_copies, 1) if n_copies > 1 else self.goals
        B, D = starts.shape
        ws = self.Workspace(B, self.max_nodes, self.n_pre_samples, D, self.device)
        ops.rrt_init(ws.buf, ws, starts, goals, self.scene)
        out = self._outputs(B, D)
        status = out['status']
        if any(d is None for d in draws) != all(d is None for d in draws):
            raise ValueError('sample_idx and goal_draw are given together or not at all')
        draws = [d if d is None else torch.as_tensor(d, dtype=torch.int32).to(self.device).reshape(B, self.total_iters).contiguous()
                 for d in draws]
        t0 = time.perf_counter()
        it = 0
        while it < self.total_iters:
            n = min(self.chunk_iters, self.total_iters - it)
            self._launch(ws, draws, out, it, n, problem_offset, **options)
            it += n
            if on_chunk is not None:
                on_chunk(self, ws, out.get('costs'), out['lengths'], status)
            if it < self.total_iters:
                if not bool((status == ops.RRT_RUNNING).any().item()):
                    break
                if time.perf_counter() - t0 >= self.max_time:       # chunk granularity
                    break
        self.workspace, self.status = ws, status
        if bool((status == ops.RRT_PATH_TOO_LONG).any().item()):
            raise MPBError(f'{self.name}: a path has more than max_path_nodes = {self.max_path_nodes} tree nodes (status '
                           f'PATH_TOO_LONG); construct the planner with a larger max_path_nodes')
        return out

    def shortcut(self, paths, lengths, n_iters, check_step=None, **kwargs):
        """Shortcut the (paths, lengths) of optimize_batched on the planner's task (PlanningTask.shortcut_paths): ->
        (paths, lengths, stats).  check_step defaults to step_size, the density the planner's own edges were checked at; path b
        draws from the stream of `seed` (default: the planner's) its problem index names."""
        kwargs.setdefault('seed', self.seed)
        return self.task.shortcut_paths(paths, lengths, n_iters=n_iters, check_step=self.step_size if check_step is None else check_step,
                                        **kwargs)

    def optimize(self, opt_iters=None, **observation):
        """One problem: the (n, D) path or None like the reference; several: a list of those."""
        paths, lengths, status = self.optimize_batched(**observation)
        out = paths_to_list(paths, lengths)
        return out[0] if len(out) == 1 else out

    def render(self, ax, **kwargs):
        raise NotImplementedError
