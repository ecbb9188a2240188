"""Checker of an RRT* result (helper of test_rrt_star_goldens_cpu.py, test_gpu_rrt_star.py): structural properties that
hold for ANY correct run, whatever was drawn, evaluated in fp64 on the oracle geometry."""
import numpy as np
import torch

from rrt_checks import hinge_argument, resample


def edge_allowance(ref_robot, q, step_size):
    """How far a point of a free edge may reach into an obstacle.  extend_path checks an edge at points less than step_size
    apart in configuration space (spacing = clamped length / (int(dist / step_size) + 1) < step_size), so every point of
    the edge lies within step_size / 2 of a checked, free configuration, and the hinge argument changes by at most
    Lip * step_size / 2 over that distance: signed distances are 1-Lipschitz in the position of a collision point, and a
    collision point moves by at most Lip |dq|.  Lip = 1 for a point robot (the point IS the configuration); for an arm
    |dx| <= sum_j r_j |dq_j| <= r sqrt(D) |dq| with r_j the distance of the point from joint j's axis, bounded by twice the
    largest distance of any collision point from the base over the configurations q given."""
    q = torch.as_tensor(np.asarray(q), dtype=torch.float64).reshape(-1, ref_robot.q_dim)
    x = ref_robot.fk_map_collision(q)
    D = q.shape[-1]
    if x.shape[-2] == 1 and torch.equal(x[:, 0, :D], q) and not x[:, 0, D:].any():      # a point robot (padded to 3-D)
        lip = 1.0
    else:
        lip = 2.0 * float(x.norm(dim=-1).max()) * np.sqrt(q.shape[-1])
    return lip * step_size / 2.0


def check_rrt_star_result(ref_robot, ref_field, start, goal, nodes, parents, d, cost, goal_idx, path, step_size, n_radius,
                          slack, e_dist, e_cost, atol=1e-5):
    """nodes (n, D), parents (n,) (-1: root), d, cost (n,), goal_idx (-1: none), path (m, D) or None; slack = FACTOR * E_gap,
    e_dist / e_cost = FACTOR * E_dist / E_cost of the scene.  Raises AssertionError naming the first property that fails."""
    start, goal = np.asarray(start, np.float64), np.asarray(goal, np.float64)
    nodes, parents = np.asarray(nodes, np.float64), np.asarray(parents)
    d, cost = np.asarray(d, np.float64), np.asarray(cost, np.float64)
    n = len(nodes)
    assert n >= 1 and len(parents) == n and len(d) == n and len(cost) == n
    assert parents[0] == -1 and np.abs(nodes[0] - start).max() <= atol, 'the root is not the start'
    assert cost[0] == 0.0 and d[0] == 0.0, 'the root has a cost'
    g = hinge_argument(ref_robot, ref_field, nodes)
    assert g.max() <= slack, f'node {int(g.argmax())} is in collision (hinge argument {g.max():.3e} > {slack:.3e})'
    assert (parents[1:] >= 0).all() and (parents[1:] < n).all(), 'a parent index is out of range'
    # acyclic, every node reaches the root: follow the parents at most n steps
    at = np.arange(n)
    for _ in range(n):
        at = np.where(at > 0, parents[np.maximum(at, 0)], at)
        at = np.where(at < 0, 0, at)
        if (at == 0).all():
            break
    assert (at == 0).all(), f'node {int(np.flatnonzero(at != 0)[0])} does not reach the root (a cycle)'
    if n > 1:
        idx = np.arange(1, n)
        elen = np.linalg.norm(nodes[idx] - nodes[parents[idx]], axis=1)
        assert np.abs(d[idx] - elen).max() <= e_dist, f'd differs from the distance to the parent by {np.abs(d[idx] - elen).max():.3e}'
        bad = np.abs(cost[idx] - (cost[parents[idx]] + d[idx]))
        assert bad.max() <= e_cost, f'cost[{int(idx[bad.argmax()])}] differs from cost[parent] + d by {bad.max():.3e}'
        assert elen.max() <= n_radius * (1 + 1e-5), f'edge of length {elen.max():.6f} > n_radius {n_radius}'
        # every edge, re-sampled at extend_path's density, is free up to what that density can miss (the re-sampled points are
        # not the ones the planner checked: a truncated extension was sampled with the spacing of the longer, un-truncated one);
        # duplicate nodes give zero-length edges with nothing to sample
        # (the allowance holds for EVERY point of an edge, so the edges are sampled 8 x denser than the planner's own check)
        pts = [resample(np.stack((nodes[parents[i]], nodes[i])), step_size / 8) for i in idx if elen[i - 1] > 0]
        if pts:
            pts = np.concatenate(pts)
            g = hinge_argument(ref_robot, ref_field, pts)
            allow = slack + edge_allowance(ref_robot, pts, step_size)
            assert g.max() <= allow, f'an edge re-sampled at step_size is in collision (hinge argument {g.max():.3e} > {allow:.3e})'
    if goal_idx is None or goal_idx < 0:
        assert path is None or len(path) == 0, 'a path without a goal node'
        return
    assert 0 < goal_idx < n and np.abs(nodes[goal_idx] - goal).max() <= atol, 'the goal node is not at the goal'
    path = np.asarray(path, np.float64)
    assert path.ndim == 2 and len(path) >= 2
    retrace = []
    j = int(goal_idx)
    while j >= 0:
        retrace.append(nodes[j])
        j = int(parents[j])
    retrace = np.stack(retrace[::-1])
    want = purge_duplicates(retrace)
    assert want.shape == path.shape and np.abs(want - path).max() <= atol, "the path is not the goal node's retrace"
    length = np.linalg.norm(np.diff(path, axis=0), axis=1).sum()
    # (a purged row lies within 1e-6 per coordinate of its successor: leaving it out shortens the polyline by at most twice that norm)
    purged = 4e-6 * np.sqrt(nodes.shape[1]) * (len(retrace) - len(path))
    assert abs(length - cost[goal_idx]) <= e_cost + purged, f'path length {length:.6f} != goal cost {cost[goal_idx]:.6f}'


def purge_duplicates(path, eps=1e-6):
    """purge_duplicates_from_traj (utils.py:33-50) on an (n, D) array."""
    if len(path) <= 2:
        return path
    sel = path[np.flatnonzero((np.abs(np.diff(path, axis=0)) > eps).any(axis=1))]
    if len(sel) == 0:
        sel = path[:1]
    if not np.allclose(sel[0], path[0], rtol=1e-5, atol=1e-8):
        sel = np.concatenate((path[:1], sel))
    if not np.allclose(sel[-1], path[-1], rtol=1e-5, atol=1e-8):
        sel = np.concatenate((sel, path[-1:]))
    return sel


def golden_star_problem(g, k):
    """(start, goal, nodes, parents, d, cost, goal_idx, path) of problem k of an RRT* golden."""
    return (g['starts'][k], g['goals'][k], g[f'p{k}_q'], g[f'p{k}_parent'], g[f'p{k}_d'], g[f'p{k}_cost'], int(g['goal_idx'][k]),
            g[f'p{k}_path'])
