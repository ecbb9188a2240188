"""MultiSampleBasedPlanner with the reference's class surface (mp_baselines/planners/multi_sample_based_planner.py).

The reference copies the planner n_trajectories times and runs the copies in a forkserver process pool.  Independent
copies are batch-parallel: here they are the problems of ONE batched launch sequence of the planner's kernel
(RRTConnect.optimize_batched, RRTStar.optimize_batched), copy c drawing its pool indices from a Philox stream of its own.  The pool keyword
arguments of the reference (`optimize_sequentially`, MultiProcessor's) are accepted and ignored.
"""
from .rrt_base import paths_to_list


class MultiSampleBasedPlanner:

    def __init__(self, planner, n_trajectories=2, optimize_sequentially=False, **kwargs):
        if not hasattr(planner, 'optimize_batched'):
            raise TypeError('MultiSampleBasedPlanner needs a planner with optimize_batched (RRTConnect, RRTStar or InfRRTStar of this package)')
        self.planner = planner
        self.n_trajectories = int(n_trajectories)

    def optimize_batched(self, **kwargs):
        """(paths, lengths, status) of the n_trajectories copies (times the planner's own problems), on the device."""
        return self.planner.optimize_batched(n_copies=self.n_trajectories, **kwargs)

    def shortcut(self, paths, lengths, n_iters, check_step=None, **kwargs):
        """The planner's shortcut() on the (paths, lengths) of optimize_batched."""
        return self.planner.shortcut(paths, lengths, n_iters, check_step=check_step, **kwargs)

    def optimize(self, **kwargs):
        """List of n_trajectories paths ((n, D) tensors) or None."""
        paths, lengths, _ = self.optimize_batched(**kwargs)
        return paths_to_list(paths, lengths)

    @property
    def starts(self):
        return self.planner.starts.repeat(self.n_trajectories, 1)

    @property
    def goals(self):
        return self.planner.goals.repeat(self.n_trajectories, 1)

    @property
    def start_state_pos(self):
        return self.planner.start_state_pos

    @property
    def goal_state_pos(self):
        return self.planner.goal_state_pos
