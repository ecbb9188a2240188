"""RRTConnect with the reference's class surface (mp_baselines/planners/rrt_connect.py:57-192 over rrt_base.py), for B
independent problems at once on the GPU.

The reference grows two trees of Python node objects, one configuration at a time, and MultiSampleBasedPlanner fans
copies of the planner out over a process pool.  Here every problem (one start / goal pair, or one copy of it) is one
workgroup of ONE persistent launch of mpb_rrt_connect_run (csrc/mpb_rrt_connect.hip), which restates the loop body line
by line -- nearest node, extend_path, safe_path, the order-preserving deletion of a reached pre-sample, the tree-name
swap with its `continue` quirk, the retrace and purge_duplicates_from_traj.

Differences from the reference: those every sample-based planner here shares (rrt_base.py), and the loop
runs n_iters + 1 iterations exactly like the reference's `while iteration < n_iters` does.
"""
from .. import ops
from .rrt_base import RRTBase, paths_to_list  # noqa: F401  (paths_to_list: callers outside the package import it from here)


class RRTConnect(RRTBase):
    NAME, Workspace = 'RRTConnect', ops.RRTWorkspace

    def _scene(self, task):
        """task.world on a task built with world_predicate=True (the tree is then grown against obstacles, SDF grid and the robot
        itself: mpb_rrt_connect_*_world), else task.geom after the family's refusals."""
        world = getattr(task, 'world', None)
        return world if world is not None else super()._scene(task)

    def optimize_batched(self, sample_idx=None, n_copies=1, problem_offset=0, **observation):
        """All problems (every start / goal row, n_copies times, copy-major) in one launch sequence.
        sample_idx: None (device Philox; problem b draws from stream problem_offset + b) or (B, n_iters + 1) int32 recorded
        pool indices.  Returns (paths (B, max_path_nodes, D), lengths (B,) int32 -- 0 where no path --, status (B,) int32)
        as device tensors; the trees stay readable through ops.rrt_connect_trees(self.workspace)."""
        out = self._run_batched([sample_idx], n_copies, problem_offset)
        return out['paths'], out['lengths'], out['status']

    def _launch(self, ws, draws, out, it, n, problem_offset):
        ops.rrt_connect_run(ws.buf, ws, self.scene, self.pre_samples, draws[0], out['paths'], out['lengths'], out['status'], it, n,
                            self.total_iters, self.step_size, self.n_radius, seed=self.seed, problem_offset=problem_offset)
