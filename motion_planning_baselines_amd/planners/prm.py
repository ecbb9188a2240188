"""PRM: the roadmap planner (Kavraki et al. 1996) for many start / goal queries against one scene, on the GPU.

The reference has no roadmap planner; the RRT planners here grow one tree per problem and throw it away.  PRM builds ONE graph of
collision-free configurations and answers any number of start / goal pairs against it -- the shape of the work
PlanningTask.inverse_kinematics (many goal configurations per target) and HybridPlanner (one path per particle) hand over.  The
semantics are build-defined (include/mpb.h); three kernels of csrc/mpb_prm.hip do the work:

  build_roadmap()      one mpb_prm_knn launch (every node's k_neighbors nearest nodes) and one mpb_prm_edge_check launch over the
                       M * K candidate edges, each scanned at spacing step_size exactly as the shortcut pass scans a candidate; an
                       edge that is not free, or shorter than ops.PRM_MIN_EDGE, gets the weight +inf.
  optimize_batched()   one mpb_prm_knn launch of the starts and goals against the nodes, one mpb_prm_edge_check launch over the
                       2 * Q * k_connect connection segments and the Q direct ones, one mpb_prm_query launch (one workgroup per
                       query: shortest path over the roadmap, the path walked back from the converged costs).

The roadmap is built once (lazily) and kept: set_queries() swaps the queries.  No launch waits on the host; the planner reads nothing
back.
"""
import torch

from .. import ops
from .base import MPPlanner, require_cuda
from .rrt_base import paths_to_list


class PRM(MPPlanner):
    NAME = 'PRM'

    def __init__(self, task=None, start_state_pos=None, goal_state_pos=None, n_nodes=4096, k_neighbors=16, k_connect=None,
                 step_size=0.1, nodes=None, max_path_nodes=512, tensor_args=None, seed=0, **kwargs):
        assert start_state_pos is not None and goal_state_pos is not None
        super().__init__(name=self.NAME, tensor_args=tensor_args)
        self.device = require_cuda(tensor_args)
        self.task = task
        if getattr(task, 'self_field', None) is not None:       # (the in-kernel predicate knows obstacles only)
            task.require_no_self_field(f'{self.NAME} (mpb_prm_edge_check)')
        if getattr(task, 'sdf_field', None) is not None:
            task.require_no_sdf_field(f'{self.NAME} (mpb_prm_edge_check)')
        self.n_nodes, self.k_neighbors = int(n_nodes), int(k_neighbors)
        self.k_connect = self.k_neighbors if k_connect is None else int(k_connect)
        if not 2 <= self.n_nodes <= ops.PRM_MAX_NODES:
            raise ValueError(f'n_nodes must be in 2 .. {ops.PRM_MAX_NODES} (the query kernel keeps the nodes\' costs in LDS)')
        if not (1 <= self.k_neighbors <= ops.PRM_MAX_K and 1 <= self.k_connect <= ops.PRM_MAX_K):
            raise ValueError(f'k_neighbors and k_connect must be in 1 .. {ops.PRM_MAX_K}')
        self.step_size = float(step_size)
        self.max_path_nodes = int(max_path_nodes)
        self.seed = int(seed)
        self._given_nodes = None if nodes is None else torch.as_tensor(nodes, dtype=torch.float32).reshape(-1, task.q_dim)
        self.nodes = self.nbr = self.w = self.edge_flag = None   # the roadmap (build_roadmap)
        self.costs = self.status = None                          # of the last optimize_batched
        self.set_queries(start_state_pos, goal_state_pos)

    def set_queries(self, start_state_pos, goal_state_pos):
        """Other start / goal pairs, (D,) or (Q, D) each, against the same roadmap."""
        D = self.task.q_dim
        starts = torch.as_tensor(start_state_pos, dtype=torch.float32).reshape(-1, D).to(self.device).contiguous()
        goals = torch.as_tensor(goal_state_pos, dtype=torch.float32).reshape(-1, D).to(self.device).contiguous()
        if starts.shape != goals.shape:
            raise ValueError('start_state_pos and goal_state_pos must have the same shape, (D,) or (Q, D)')
        self.start_state_pos, self.goal_state_pos = start_state_pos, goal_state_pos
        self.starts, self.goals = starts, goals

    def build_roadmap(self):
        """The nodes (given, or n_nodes collision-free draws of the task), their k_neighbors nearest nodes and the weights of
        those edges: two launches.  Lazy and idempotent: a roadmap that exists is returned as it stands.
        -> (nodes (M, D), nbr (M, K) int32, w (M, K): the edge's length, +inf where it is not free or shorter than PRM_MIN_EDGE)."""
        if self.nodes is None:
            nodes = self._given_nodes
            if nodes is None:
                nodes = self.task.random_coll_free_q(self.n_nodes, max(1000, self.n_nodes))
            nodes = nodes.to(self.device).contiguous()
            M = nodes.shape[0]
            if not 2 <= M <= ops.PRM_MAX_NODES:
                raise ValueError(f'nodes holds {M} configurations, a roadmap has 2 .. {ops.PRM_MAX_NODES}')
            K = min(self.k_neighbors, M - 1)
            nbr, dist = ops.prm_knn(nodes, nodes, K, exclude_self=True)
            own = torch.arange(M, device=self.device, dtype=torch.int32).repeat_interleave(K)
            pairs = torch.stack((own, nbr.reshape(-1)), dim=1).contiguous()
            flag, _ = ops.prm_edge_check(nodes, pairs, self.task.geom, self.step_size)
            flag = flag.reshape(M, K)
            keep = (flag == ops.PRM_EDGE_FREE) & (dist >= ops.PRM_MIN_EDGE)
            self.w = torch.where(keep, dist, torch.full_like(dist, float('inf'))).contiguous()
            self.nodes, self.nbr, self.edge_flag = nodes, nbr, flag
        return self.nodes, self.nbr, self.w

    def optimize_batched(self, **observation):
        """Every start / goal row against the roadmap: three launches.  Returns (paths (Q, max_path_nodes, D), lengths (Q,) int32
        -- 0 where no path --, status (Q,) int32 ops.PRM_*) as device tensors; the paths' costs stay in self.costs."""
        nodes, nbr, w = self.build_roadmap()
        M, (Q, D) = nodes.shape[0], self.starts.shape
        Kc = min(self.k_connect, M)
        ends = torch.cat((self.starts, self.goals)).contiguous()
        cidx, cdist = ops.prm_knn(ends, nodes, Kc)
        # the connection segments (end M + r to its near nodes) and the direct ones (start M + q to goal M + Q + q) in ONE edge launch
        pts = torch.cat((nodes, ends)).contiguous()
        end = torch.arange(M, M + 2 * Q, device=self.device, dtype=torch.int32).repeat_interleave(Kc)
        sq = torch.arange(M, M + Q, device=self.device, dtype=torch.int32)
        pairs = torch.cat((torch.stack((end, cidx.reshape(-1)), dim=1), torch.stack((sq, sq + Q), dim=1))).contiguous()
        flag, _ = ops.prm_edge_check(pts, pairs, self.task.geom, self.step_size)
        free = flag == ops.PRM_EDGE_FREE
        inf = torch.full_like(cdist, float('inf'))
        cw = torch.where(free[:2 * Q * Kc].reshape(2 * Q, Kc), cdist, inf).contiguous()
        d2 = torch.zeros(Q, device=self.device, dtype=torch.float32)
        for k in range(D):                                       # (the kernels' distance: the squares summed in index order)
            df = self.starts[:, k] - self.goals[:, k]
            d2 = d2 + df * df
        # (the root through fp64: rounding a double root to fp32 gives the correctly rounded fp32 root, sqrtf's)
        direct = torch.where(free[2 * Q * Kc:], torch.sqrt(d2.double()).float(), inf[:Q, 0]).contiguous()
        paths, lengths, self.costs, self.status = ops.prm_query(nodes, nbr, w, self.starts, self.goals, cidx[:Q].contiguous(), cw[:Q].contiguous(),
                                                                cidx[Q:].contiguous(), cw[Q:].contiguous(), direct, self.max_path_nodes)
        return paths, lengths, self.status

    def shortcut(self, paths, lengths, n_iters, check_step=None, **kwargs):
        """Shortcut the (paths, lengths) of optimize_batched on the planner's task, as RRTBase.shortcut does."""
        kwargs.setdefault('seed', self.seed)
        return self.task.shortcut_paths(paths, lengths, n_iters=n_iters, check_step=self.step_size if check_step is None else check_step,
                                        **kwargs)

    def optimize(self, opt_iters=None, **observation):
        """One query: the (n, D) path or None; several: a list of those."""
        paths, lengths, _ = self.optimize_batched(**observation)
        out = paths_to_list(paths, lengths)
        return out[0] if len(out) == 1 else out

    def render(self, ax, **kwargs):
        raise NotImplementedError
