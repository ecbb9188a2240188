"""Batched PRM (csrc/mpb_prm.hip), Panda + 16 spheres: a roadmap of M = 4 096 nodes with K = 16 neighbours each, edges checked at step
pi/80, and Q = 1 024 random collision-free start / goal pairs answered against it -- next to RRT-Connect (step pi/80, radius pi/4,
n_iters 2000, pool 2000) on the same 1 024 problems.

Timing: warm-up first, HIP events around each launch, 10 repeats, the minimum.  Per launch: the build's knn (M x M) and edge check
(M * K segments), the queries' knn (2 Q x M), edge check (2 Q Kc + Q segments) and query kernel; then the planner's own
optimize_batched (roadmap kept) and RRT-Connect's, and the share of problems each answers.

    python scripts/bench_prm.py [--json OUT]
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from motion_planning_baselines_amd import geometry as G, ops, workloads  # noqa: E402
from motion_planning_baselines_amd.planners import PRM  # noqa: E402
from motion_planning_baselines_amd.planners.rrt_connect import RRTConnect  # noqa: E402
from motion_planning_baselines_amd.robot_field import PlanningTask  # noqa: E402

dev = torch.device('cuda:0')
ta = dict(device=dev, dtype=torch.float32)
robot, field = G.RobotPanda(), G.env_spheres_3d(seed=0)
task = PlanningTask(robot, field, tensor_args=ta, seed=5)
M, K, Q, STEP, REPEATS, WARMUP, LMAX = 4096, 16, 1024, np.pi / 80, 10, 2, 512


def timed(fn):
    """-> (the minimum of REPEATS event-timed calls in ms, the last result)"""
    for _ in range(WARMUP):
        out = fn()
    best = float('inf')
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best, out


q = torch.from_numpy(workloads.collision_free_configs(robot, field, 2 * Q, 91, dev)).to(dev)
starts, goals = q[:Q].contiguous(), q[Q:].contiguous()
prm = PRM(task=task, start_state_pos=starts, goal_state_pos=goals, n_nodes=M, k_neighbors=K, step_size=STEP, max_path_nodes=LMAX, tensor_args=ta)
nodes, nbr, w = prm.build_roadmap()
res = {}
res['build_knn_ms'], (nbr2, dist) = timed(lambda: ops.prm_knn(nodes, nodes, K, exclude_self=True))
pairs = torch.stack((torch.arange(M, device=dev, dtype=torch.int32).repeat_interleave(K), nbr2.reshape(-1)), 1).contiguous()
res['build_edge_ms'], (flag, _) = timed(lambda: ops.prm_edge_check(nodes, pairs, task.geom, STEP))
ends = torch.cat((starts, goals)).contiguous()
res['query_knn_ms'], (cidx, cdist) = timed(lambda: ops.prm_knn(ends, nodes, K))
pts = torch.cat((nodes, ends)).contiguous()
end = torch.arange(M, M + 2 * Q, device=dev, dtype=torch.int32).repeat_interleave(K)
sq = torch.arange(M, M + Q, device=dev, dtype=torch.int32)
cpairs = torch.cat((torch.stack((end, cidx.reshape(-1)), 1), torch.stack((sq, sq + Q), 1))).contiguous()
res['query_edge_ms'], (cflag, _) = timed(lambda: ops.prm_edge_check(pts, cpairs, task.geom, STEP))
inf = torch.full_like(cdist, float('inf'))
cw = torch.where((cflag[:2 * Q * K] == ops.PRM_EDGE_FREE).reshape(2 * Q, K), cdist, inf).contiguous()
no_direct = inf[:Q, 0].contiguous()                           # (the roadmap answers every query: what the kernel costs at its most)
args = (nodes, nbr, w, starts, goals, cidx[:Q].contiguous(), cw[:Q].contiguous(), cidx[Q:].contiguous(), cw[Q:].contiguous())
res['query_ms'], (_, lengths_q, _, status_q) = timed(lambda: ops.prm_query(*args, no_direct, LMAX))
res['query_ok_share_without_direct'] = float((status_q == ops.PRM_OK).float().mean())
res['query_path_rows_mean'] = float(lengths_q[status_q == ops.PRM_OK].float().mean())
res['optimize_batched_ms'], (_, lengths, status) = timed(prm.optimize_batched)
res['prm_ok_share'] = float((status == ops.PRM_OK).float().mean())
res['prm_direct_share'] = float((lengths == 2).float().mean())
res['edges_free_share'] = float((flag == ops.PRM_EDGE_FREE).float().mean())
res['status_counts'] = torch.bincount(status, minlength=6).tolist()

rrt = RRTConnect(task=task, n_iters=2000, start_state_pos=starts, goal_state_pos=goals, step_size=STEP, n_radius=np.pi / 4, tensor_args=ta,
                 n_pre_samples=2000, max_path_nodes=LMAX, seed=7)
REPEATS, WARMUP = 3, 1
res['rrt_connect_ms'], (_, _, rstatus) = timed(rrt.optimize_batched)
res['rrt_connect_found_share'] = float((rstatus == ops.RRT_FOUND).float().mean())
print(f'PRM, Panda + 16 spheres, M {M} K {K} step pi/80, Q {Q}: build knn {res["build_knn_ms"]:.3f} ms, build edge check ({M * K} segments, '
      f'{res["edges_free_share"]:.3f} free) {res["build_edge_ms"]:.3f} ms; queries: knn {res["query_knn_ms"]:.3f} ms, edge check ({len(cpairs)} segments) '
      f'{res["query_edge_ms"]:.3f} ms, query kernel {res["query_ms"]:.3f} ms (no direct segments: {res["query_ok_share_without_direct"]:.3f} OK, '
      f'{res["query_path_rows_mean"]:.1f} rows per path); PRM.optimize_batched {res["optimize_batched_ms"]:.3f} ms, OK {res["prm_ok_share"]:.3f} '
      f'(direct {res["prm_direct_share"]:.3f}), status counts {res["status_counts"]}; RRTConnect.optimize_batched on the same problems '
      f'{res["rrt_connect_ms"]:.1f} ms, found {res["rrt_connect_found_share"]:.3f}')
if '--json' in sys.argv:
    with open(sys.argv[sys.argv.index('--json') + 1], 'w') as fh:
        json.dump(res, fh, indent=1)
