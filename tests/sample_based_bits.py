"""The cases of tests/golden/sample_based_bits.npz: what the sample-based kernels leave behind, bit for bit, on small seeded problems.

The fixture is RECORDED from the library of the commit before a change that must not move a bit (tests/golden/make_sample_based_bits.py,
on the GPU) and COMPARED against the library under test (tests/test_gpu_sample_based_bits.py).  Both sides build their inputs here, so a
case is the same launch on both.  One case per instantiation of rrt_connect_kernel and rrt_star_kernel:

    pm2d            D = 2, the geometry and pool of the rrt_pm2d_grid golden                         <2, 0>
    pm3d            D = 3, RobotPointMass(3) among env_spheres_3d          connect <3, 0>,  RRT* <0, 0> (it has no form for D = 3)
    panda_generic   D = 7, the Panda packed with use_model=False                                     <7, 0>
    panda           D = 7, the Panda with its compile-time model                                     <7, Panda>
    arm5            D = 5, the chain of tests/test_gpu_generic_dof.py among env_spheres_3d           <0, 0>

and, at D = 3 -- the one compile-time D the bit-for-bit tests of the roadmap and the shortcut pass have no input set for --, one launch of
prm_knn_kernel<3>, prm_edge_kernel<3, 0> and path_shortcut_kernel<3, 0>.
Shapes: B = 4 problems, a pool of 256, 192 iterations in two launches of 96 (the header words are carried from one to the next), device-
drawn indices (the Philox path), Lmax 256, step = radius / 100; RRT* with n_iters_after_success = 16 but for the informed case (a
problem that goes on for all 192 iterations records 193 nodes, and the fixture is to stay small).  The recorder looks for a (radius, seed) per case at which the recorded
run meets `conditions` -- a tree of more than 64 nodes (the second trip of the nearest scan and of the arg-min), an extension that
walked past its 64th point (the second trip of rrt_first_collision), a FOUND problem, for RRT* a rewire -- and the test asserts them
again from the fixture."""
import numpy as np
import torch

B, N_PRE, ITERS, CHUNK, LMAX = 4, 256, 192, 96, 256
MAX_NODES = ITERS + 2
SCENES = ('pm2d', 'pm3d', 'panda_generic', 'panda', 'arm5')
CASES = tuple((kind, scene) for kind in ('connect', 'star') for scene in SCENES)
INFORMED = ('star', 'pm2d')                                   # the RRT* case that runs with `informed` on
EXTRA = 'd3'                                                  # the D = 3 launches of the roadmap and shortcut kernels
N_AFTER = 16                                                  # the other RRT* cases stop this many iterations after their success
NODE_CAP = 230                                                # nodes a case may record (the fixture stays below 90 KB)


def scene(name, dev):
    """(DeviceGeometry, q_min, q_max, pool (N_PRE, D) float32, the largest radius the recorder tries)."""
    from conftest import load_golden, product_geometry_from_golden
    from motion_planning_baselines_amd import geometry as G, ops
    use_model = True
    if name == 'pm2d':
        g = load_golden('rrt_pm2d_grid')
        robot, field = product_geometry_from_golden(g)
        pool, radius = np.ascontiguousarray(g['pool'][:N_PRE], dtype=np.float32), float(g['n_radius'])
    else:
        if name == 'pm3d':
            robot, field, radius = G.RobotPointMass(3, radius=0.03), G.env_spheres_3d(seed=0), 0.3
        elif name in ('panda', 'panda_generic'):
            robot, field, radius, use_model = G.RobotPanda(), G.env_spheres_3d(seed=0), np.pi / 4, name == 'panda'
        else:
            from test_gpu_generic_dof import make_arm               # (among make_field()'s spheres the 5-joint arm is never free)
            robot, field, radius = make_arm(5), G.env_spheres_3d(seed=0), np.pi / 4
        rng = np.random.RandomState(4000 + robot.q_dim)
        pool = rng.uniform(robot.q_min_np, robot.q_max_np, (N_PRE, robot.q_dim)).astype(np.float32)
    return ops.DeviceGeometry(robot, field, dev, use_model=use_model), robot.q_min_np, robot.q_max_np, pool, radius


def free_configs(geom, q_min, q_max, n, seed, dev):
    """n collision-free configurations by the library's own predicate (the recorder's starts and goals; stored in the fixture)."""
    from motion_planning_baselines_amd import ops
    rng = np.random.RandomState(seed)
    q = torch.from_numpy(rng.uniform(q_min, q_max, (64 * n, len(q_min))).astype(np.float32)).to(dev)
    free = ~ops.collision_check(q, geom).bool()
    q = q[free][:n]
    assert len(q) == n, 'too few free configurations'
    return q.cpu().numpy()


def run(kind, geom, dev, starts, goals, pool, radius, seed, informed=False):
    """One case: {name: integer array} of everything the two launches leave behind (fp32 words as uint32)."""
    from motion_planning_baselines_amd import ops
    starts, goals, pool = (torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev) for x in (starts, goals, pool))
    D = starts.shape[1]
    ws = (ops.RRTWorkspace if kind == 'connect' else ops.RRTStarWorkspace)(B, MAX_NODES, N_PRE, D, dev)
    ops.rrt_init(ws.buf, ws, starts, goals, geom)
    paths = torch.zeros(B, LMAX, D, device=dev)
    lengths = torch.zeros(B, device=dev, dtype=torch.int32)
    status = torch.zeros(B, device=dev, dtype=torch.int32)
    costs = torch.zeros(B, device=dev)
    step = radius / 100.0
    for it in range(0, ITERS, CHUNK):
        if kind == 'connect':
            ops.rrt_connect_run(ws.buf, ws, geom, pool, None, paths, lengths, status, it, CHUNK, ITERS, step, radius, seed=seed)
        else:
            ops.rrt_star_run(ws.buf, ws, geom, pool, None, None, paths, lengths, costs, status, it, CHUNK, ITERS, step, radius,
                             n_iters_after_success=None if informed else N_AFTER, informed=informed, seed=seed)
    torch.cuda.synchronize()
    out = dict(ops.rrt_connect_trees(ws) if kind == 'connect' else ops.rrt_star_tree(ws))
    out.update(paths=paths, lengths=lengths, status_out=status)
    if kind == 'star':
        out['costs'] = costs
    return {k: _bits(v) for k, v in out.items()}


def run_extra(dev, seed=0):
    """prm_knn_kernel<3>, prm_edge_kernel<3, 0> and path_shortcut_kernel<3, 0> on the pm3d scene: M = 64 nodes, K = 4, the E = 64 edges
    node -> its nearest neighbour, N = 4 polylines of 12 pool rows, 32 iterations."""
    from motion_planning_baselines_amd import ops
    geom, q_min, q_max, pool, radius = scene('pm3d', dev)
    nodes = torch.from_numpy(pool[:64]).to(dev)
    idx, dist = ops.prm_knn(nodes, nodes, 4, exclude_self=True)
    pairs = torch.stack([torch.arange(64, device=dev, dtype=torch.int32), idx[:, 0]], 1).contiguous()
    flag, first = ops.prm_edge_check(nodes, pairs, geom, radius / 100.0)
    paths = torch.zeros(4, 16, 3, device=dev)
    paths[:, :12] = torch.from_numpy(pool[64:112].reshape(4, 12, 3)).to(dev)
    lengths = torch.full((4,), 12, device=dev, dtype=torch.int32)
    sp, sl, stats, log = ops.path_shortcut(paths, lengths, geom, 32, radius / 100.0, seed=seed, with_log=True)
    torch.cuda.synchronize()
    return {k: _bits(v) for k, v in dict(knn_idx=idx, knn_dist=dist, edge_flag=flag, edge_first=first, sc_paths=sp, sc_lengths=sl,
                                         sc_stats=stats, sc_log=log).items()}


def _bits(t):
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a.astype(np.int32)


def _f32(a):
    return np.ascontiguousarray(a).view(np.float32)


def conditions(kind, out, radius):
    """{name: bool} of what a recorded case must exercise; also the number of nodes it recorded."""
    from motion_planning_baselines_amd import ops
    if kind == 'connect':
        trees = [(_f32(out['nodes'][b, t]), out['parents'][b, t], int(out['counts'][b, t])) for b in range(B) for t in (0, 1)]
    else:
        trees = [(_f32(out['nodes'][b]), out['parents'][b], int(out['count'][b])) for b in range(B)]
    points = 0.0
    for q, parent, n in trees:
        i = np.arange(1, n)
        i = i[(parent[i] >= 0) & (parent[i] < i)]                 # (a rewired node's parent is younger than the node: not an extension)
        if len(i):
            d = np.linalg.norm(q[i].astype(np.float64) - q[parent[i]].astype(np.float64), axis=1)
            points = max(points, float(d.max()) / (radius / 100.0))   # the index of the extension's point the node is, to rounding
    res = dict(tree_over_64=max(n for _, _, n in trees) > 64, extension_over_64_points=points >= 66.0,
               found=bool((out['status'] == ops.RRT_FOUND).any()))
    if kind == 'star':
        res['rewired'] = bool((out['rewires'] > 0).any())
    return res, sum(n for _, _, n in trees)


def pack(out):
    """The arrays of a case as ONE array of 32-bit words, in the order of their names (an .npz member costs 250 bytes of headers)."""
    return np.concatenate([np.ascontiguousarray(out[k]).view(np.uint32).ravel() for k in sorted(out)])


def unpack(words, like):
    """pack's inverse, with the shapes and types of `like` (the same case run again)."""
    out, o = {}, 0
    for k in sorted(like):
        out[k] = words[o:o + like[k].size].view(like[k].dtype).reshape(like[k].shape)
        o += like[k].size
    assert o == len(words), (o, len(words))
    return out


def pack_inputs(starts, goals, radius, seed):
    return np.concatenate([starts.view(np.uint32).ravel(), goals.view(np.uint32).ravel(), np.array([radius], np.float32).view(np.uint32),
                           np.array([seed], np.uint32)])


def unpack_inputs(words):
    D = (len(words) - 2) // (2 * B)
    q = words[:2 * B * D].view(np.float32).reshape(2, B, D)
    return q[0], q[1], float(words[-2:-1].view(np.float32)[0]), int(words[-1])
