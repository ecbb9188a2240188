"""HybridPlanner with the reference's class surface (mp_baselines/planners/hybrid_planner.py:10-89).

A sample-based planner proposes position-only paths (one polyline per particle, each with its own number
of waypoints, or None when it found nothing); they are turned into position+velocity support points and
handed to an optimisation-based planner (GPMP2 / StochGPMP of this package) that runs on the GPU.

The reference converts the paths with torch_robotics' ``smoothen_trajectory`` / ``tensor_linspace_v1``
(external, CPU, one path at a time in a Python loop: hybrid_planner.py:44-59).  Here ALL paths are converted
by one launch of mpb_traj_resample (arc-length-uniform linear resampling, average velocity on the interior
points -- build-defined).

The sample-based half is served by this package: RRTConnect, RRTStar / InfRRTStar and MultiSampleBasedPlanner
(planners/rrt_connect.py, planners/rrt_star.py, planners/multi_sample_based_planner.py) grow all trees in one batched
launch sequence on the GPU.  A sample-based planner
that offers ``optimize_batched() -> (paths (N, Lmax, D), lengths (N,), status (N,))`` device tensors is fed straight
into mpb_traj_resample -- no host round trip, no padding loop; a problem without a path gets the straight line
start -> goal, written on the device (hybrid_planner.py:47-51).  Any other sample-based planner stays the caller's
(duck-typed: ``optimize(refill_samples_buffer=True, ...) -> list of (n_i, D) tensors or None``, ``start_state_pos``,
``goal_state_pos``) and takes the list path below.

``shortcut_iters > 0`` puts the shortcut pass every sample-based stack has (pybullet-planning's ``smooth_path``, OMPL's
``PathSimplifier``; the reference did not carry it over) between the two halves: one launch of mpb_path_shortcut over all paths, so
that mpb_traj_resample spends its support points on the shortened polylines and not on the tree's zig-zag.
"""
import torch

from .. import ops
from .base import MPPlanner, require_cuda


class HybridPlanner(MPPlanner):

    def __init__(self, sample_based_planner, opt_based_planner, shortcut_iters=0, shortcut_step=None, **kwargs):
        """shortcut_iters > 0: that many shortcut attempts per path (mpb_path_shortcut) between the sample-based planner and the
        resampling, checked at spacing shortcut_step (None: the sample-based planner's step_size)."""
        super().__init__("HybridSampleAndOptimizationPlanner", **kwargs)
        self.sample_based_planner = sample_based_planner
        self.opt_based_planner = opt_based_planner
        self.device = require_cuda(self.tensor_args)
        self.shortcut_iters, self.shortcut_step = int(shortcut_iters), shortcut_step
        self.shortcut_stats = None                                # (N, 4) of the last optimize() that shortcut

    def render(self, ax, **kwargs):
        raise NotImplementedError

    def paths_to_initial_means(self, traj_l):
        """list of (n_i, D) position paths (or None) -> (1, N, H, 2D) initial particle means
        (hybrid_planner.py:42-66; a missing path becomes the straight line start -> goal, :47-51)."""
        H, dt = self.opt_based_planner.n_support_points, self.opt_based_planner.dt
        paths = []
        for traj in traj_l:
            if traj is None:
                traj = torch.stack((torch.as_tensor(self.sample_based_planner.start_state_pos),
                                    torch.as_tensor(self.sample_based_planner.goal_state_pos)))
            paths.append(torch.as_tensor(traj, dtype=torch.float32).reshape(-1, traj.shape[-1]))
        N, D = len(paths), paths[0].shape[-1]
        Lmax = max(p.shape[0] for p in paths)
        if self.shortcut_iters > 0:
            Lmax += 1                                             # (room for the one node a corner cut adds)
        padded = torch.zeros(N, Lmax, D, dtype=torch.float32)
        for i, p in enumerate(paths):
            padded[i, :p.shape[0]] = p.to('cpu') if not p.is_cuda else p.cpu()
        lengths = torch.tensor([p.shape[0] for p in paths], dtype=torch.int32)
        padded, lengths = padded.to(self.device), lengths.to(self.device)
        if self.shortcut_iters > 0:
            task = getattr(self.opt_based_planner, 'task', None)
            if task is None or not hasattr(task, 'shortcut_paths'):
                raise NotImplementedError('HybridPlanner(shortcut_iters > 0): the sample-based planner hands its paths over as a list '
                                          'and offers no shortcut(), and the optimisation-based planner carries no PlanningTask '
                                          '(`task`) to check shortcuts against')
            step = self.shortcut_step if self.shortcut_step is not None else getattr(self.sample_based_planner, 'step_size', None)
            if step is None:
                raise ValueError('HybridPlanner(shortcut_iters > 0): the sample-based planner has no step_size, give shortcut_step')
            padded, lengths, self.shortcut_stats = task.shortcut_paths(padded, lengths, n_iters=self.shortcut_iters, check_step=step)
        out = ops.traj_resample(padded, lengths, H, dt)
        return out.unsqueeze(0)                                   # 'n h d -> 1 n h d' (:64)

    def batched_paths_to_initial_means(self, paths, lengths):
        """(paths (N, Lmax, D), lengths (N,)) device tensors of optimize_batched -> (1, N, H, 2D) initial particle means;
        lengths[n] == 0 (no path) becomes the straight line start -> goal, on the device."""
        sp = self.sample_based_planner
        N, D = paths.shape[0], paths.shape[-1]
        starts, goals = sp.starts.reshape(-1, D), sp.goals.reshape(-1, D)
        if starts.shape[0] != N:                                  # one start / goal pair for all copies
            starts, goals = starts.expand(N, D), goals.expand(N, D)
        missing = lengths == 0
        paths = paths.clone()
        paths[:, 0] = torch.where(missing[:, None], starts, paths[:, 0])
        paths[:, 1] = torch.where(missing[:, None], goals, paths[:, 1])
        lengths = torch.where(missing, torch.full_like(lengths, 2), lengths)
        H, dt = self.opt_based_planner.n_support_points, self.opt_based_planner.dt
        return ops.traj_resample(paths.contiguous(), lengths.contiguous(), H, dt).unsqueeze(0)

    def optimize(self, debug=False, print_times=False, return_iterations=False, **kwargs):
        if hasattr(self.sample_based_planner, 'optimize_batched'):
            paths, lengths, _ = self.sample_based_planner.optimize_batched(**kwargs)
            if self.shortcut_iters > 0:
                if not hasattr(self.sample_based_planner, 'shortcut'):
                    raise NotImplementedError('HybridPlanner(shortcut_iters > 0): the sample-based planner offers optimize_batched() '
                                              'but no shortcut(paths, lengths, n_iters, check_step)')
                paths, lengths, self.shortcut_stats = self.sample_based_planner.shortcut(paths, lengths, self.shortcut_iters,
                                                                                         check_step=self.shortcut_step)
            means = self.batched_paths_to_initial_means(paths, lengths)
        else:
            traj_l = self.sample_based_planner.optimize(refill_samples_buffer=True, debug=debug, **kwargs)
            means = self.paths_to_initial_means(traj_l)
        self.opt_based_planner.reset(initial_particle_means=means)
        trajs_0 = self.opt_based_planner.get_traj()
        n = self.opt_based_planner.opt_iters
        trajs_iters = torch.empty((n + 1, *trajs_0.shape), device=trajs_0.device, dtype=trajs_0.dtype)
        trajs_iters[0] = trajs_0
        for i in range(n):
            trajs_iters[i + 1] = self.opt_based_planner.optimize(opt_iters=1, debug=debug, **kwargs)
        return trajs_iters if return_iterations else trajs_iters[-1]
