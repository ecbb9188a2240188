"""Checker of an RRT-Connect result (helper of test_rrt_goldens_cpu.py, test_gpu_rrt_connect.py): structural properties
that hold for ANY correct run, whatever indices were drawn, evaluated in fp64 on the oracle geometry."""
import numpy as np
import torch


def hinge_argument(ref_robot, ref_field, q):
    """max_l(margin + r_l - sdf(x_l(q))) per configuration, fp64: positive = in collision."""
    q = torch.as_tensor(np.asarray(q), dtype=torch.float64).reshape(-1, ref_robot.q_dim)
    sd = ref_field.signed_distance(ref_robot.fk_map_collision(q))
    return (ref_field.margin + ref_field.link_radius - sd).max(dim=-1)[0].numpy()


def resample(path, step_size):
    """Every segment of a polyline at extend_path's own density: int(len / step_size) + 2 points, end points included."""
    pts = []
    for a, b in zip(path[:-1], path[1:]):
        n = int(np.linalg.norm(b - a) / step_size) + 2
        pts.append(a + (b - a) * np.linspace(0.0, 1.0, n)[:, None])
    return np.concatenate(pts)


def check_rrt_result(ref_robot, ref_field, start, goal, trees, path, step_size, n_radius, slack, atol=1e-5):
    """trees: ((nodes0 (n0, D), parents0 (n0,)), (nodes1, parents1)), tree 0 rooted at the start, tree 1 at the goal;
    path (n, D) or None; slack = 32 E_gap of the scene.  ref_robot / ref_field: the fp64 oracle geometry.  Raises
    AssertionError naming the first property that does not hold."""
    start, goal = np.asarray(start, np.float64), np.asarray(goal, np.float64)
    edges = set()
    for t, (nodes, parents) in enumerate(trees):
        nodes, parents = np.asarray(nodes, np.float64), np.asarray(parents)
        assert len(nodes) == len(parents) and len(nodes) >= 1
        assert parents[0] == -1 and np.abs(nodes[0] - (start, goal)[t]).max() <= atol, f'tree {t}: root is not the {("start", "goal")[t]}'
        g = hinge_argument(ref_robot, ref_field, nodes)
        assert g.max() <= slack, f'tree {t}: node {int(g.argmax())} is in collision (hinge argument {g.max():.3e} > {slack:.3e})'
        idx = np.arange(1, len(nodes))
        assert (parents[1:] >= 0).all() and (parents[1:] < idx).all(), f'tree {t}: a parent does not precede its child'
        if len(nodes) > 1:
            elen = np.linalg.norm(nodes[1:] - nodes[parents[1:]], axis=1)
            assert elen.max() <= n_radius * (1 + 1e-5), f'tree {t}: edge of length {elen.max():.6f} > n_radius {n_radius}'
        for i in idx:
            a, b = nodes[i].astype(np.float32).tobytes(), nodes[parents[i]].astype(np.float32).tobytes()
            edges.add((a, b))
            edges.add((b, a))
    if path is None:
        return
    path = np.asarray(path, np.float64)
    assert path.ndim == 2 and len(path) >= 2
    fwd = np.abs(path[0] - start).max() <= atol and np.abs(path[-1] - goal).max() <= atol
    bwd = np.abs(path[0] - goal).max() <= atol and np.abs(path[-1] - start).max() <= atol
    assert fwd or bwd, 'the path does not join the start and the goal (in either order, Q15)'
    known = {np.asarray(n, np.float32).tobytes() for nodes, _ in trees for n in np.asarray(nodes)}
    assert all(p.astype(np.float32).tobytes() in known for p in path), 'a path node is not a tree node'
    joins = 0
    for a, b in zip(path[:-1], path[1:]):
        if (a.astype(np.float32).tobytes(), b.astype(np.float32).tobytes()) not in edges:
            joins += 1
            assert np.linalg.norm(b - a) <= n_radius * (1 + 1e-5) + atol, 'the connecting edge is longer than n_radius'
    assert joins <= 1, f'{joins} path segments are neither tree edges nor the one connecting edge'
    g = hinge_argument(ref_robot, ref_field, resample(path, step_size))
    assert g.max() <= slack, f'the path re-sampled at step_size is in collision (hinge argument {g.max():.3e} > {slack:.3e})'


def golden_problem(g, k):
    """(start, goal, trees, path) of problem k of an RRT golden."""
    trees = tuple((g[f'p{k}_tree{t}_q'], g[f'p{k}_tree{t}_parent']) for t in (0, 1))
    return g['starts'][k], g['goals'][k], trees, g[f'p{k}_path']
