"""The batched PRM on the GPU (csrc/mpb_prm.hip) against the definition restated on the CPU (tests/prm_checks.py): the nearest
neighbours and the queries' answers bit for bit, the edges' flags held to the fp64 oracle wherever fp64 can decide; determinism, the
independence of the queries, and the planner's surface."""
import types

import numpy as np
import pytest
import torch

import prm_checks as C

pytestmark = pytest.mark.gpu
_ROADMAPS = {}


def _geom(p, dev, use_model=True):
    from motion_planning_baselines_amd import ops
    if len(p.fields) == 1:
        return ops.DeviceGeometry(p.robot, p.fields[0], dev, use_model=use_model)
    return ops.DeviceGeometry(p.robot, p.fields, dev, scales=p.scales, use_model=use_model)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).contiguous()


def _knn(dev):
    from motion_planning_baselines_amd import ops

    def knn(queries, nodes, K, exclude_self=False):
        idx, dist = ops.prm_knn(_dev(queries, dev), _dev(nodes, dev), K, exclude_self=exclude_self)
        return idx.cpu().numpy(), dist.cpu().numpy()
    return knn


def _edges(p, geom, dev):
    from motion_planning_baselines_amd import ops

    def edges(pts, pairs):
        flag, first = ops.prm_edge_check(_dev(pts, dev), _dev(pairs, dev), geom, float(p.step))
        return flag.cpu().numpy(), first.cpu().numpy()
    return edges


def _roadmap(name, dev, use_model=True):
    """The kernels' own roadmap and connection tables of the input set (prm_checks.build over the two kernels), computed once."""
    if (name, use_model) not in _ROADMAPS:
        p = C.problem(name)
        _ROADMAPS[name, use_model] = C.build(p, _knn(dev), _edges(p, _geom(p, dev, use_model), dev))
    return _ROADMAPS[name, use_model]


def _query(r, dev, Lmax=C.LMAX, rows=None):
    from motion_planning_baselines_amd import ops
    sel = (lambda a: a) if rows is None else (lambda a: a[rows])
    out = ops.prm_query(_dev(r.nodes, dev), _dev(r.nbr, dev), _dev(r.w, dev), *(_dev(sel(getattr(r, k)), dev) for k in
                        ('starts', 'goals', 'cs', 'ws', 'cg', 'wg', 'direct')), Lmax)
    torch.cuda.synchronize()
    return types.SimpleNamespace(**{k: t.cpu().numpy() for k, t in zip(('paths', 'lengths', 'costs', 'status'), out)})


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b, rows_a=None):
    for k in ('paths', 'lengths', 'costs', 'status'):
        x = getattr(a, k) if rows_a is None else getattr(a, k)[rows_a]
        assert np.array_equal(_bits(x), _bits(getattr(b, k))), k


@pytest.mark.parametrize('name', C.SETS)
def test_knn_equals_the_restatement(gpu_device, name):
    """1. idx equal and dist bit-equal: every node against the nodes (exclude_self), and Q = 11 other rows against the nodes."""
    p, knn = C.problem(name), _knn(gpu_device)
    for queries, K, excl in ((p.nodes, p.K, True), (p.starts, C.KC, False), (p.goals, min(32, p.M), False)):
        idx, dist = knn(queries, p.nodes, K, excl)
        want_idx, want_dist, _ = C.knn32(queries, p.nodes, K, excl)
        assert idx.shape == (len(queries), K) and np.array_equal(idx, want_idx)
        assert np.array_equal(dist.view(np.uint32), want_dist.view(np.uint32))
    assert np.array_equal(_roadmap(name, gpu_device).nbr, C.reference(name).r.nbr)


def test_knn_edges(gpu_device):
    """Duplicated node rows tie by index, M = 2 with K = 1, more than one tile of 64 rows with K = 32, and a NaN row orders as +inf."""
    p, knn = C.problem('panda'), _knn(gpu_device)
    nodes = p.nodes.copy()
    nodes[40], nodes[70] = nodes[3], nodes[3]
    idx, dist = knn(nodes, nodes, 32, True)
    want_idx, want_dist, _ = C.knn32(nodes, nodes, 32, True)
    assert np.array_equal(idx, want_idx) and np.array_equal(dist.view(np.uint32), want_dist.view(np.uint32))
    assert idx[3, :2].tolist() == [40, 70] and idx[70, :2].tolist() == [3, 40] and not dist[[3, 40, 70], :2].any()
    idx, dist = knn(nodes[:1], nodes, 3, False)                     # a query that is no node: the three copies in index order
    assert np.array_equal(idx, C.knn32(nodes[:1], nodes, 3)[0])
    assert knn(nodes[3:4], nodes, 3, False)[0].tolist() == [[3, 40, 70]]
    two = p.nodes[:2]
    idx, dist = knn(two, two, 1, True)
    assert idx.tolist() == [[1], [0]] and dist[0, 0] == dist[1, 0] == C.S.dist32(two[0], two[1])
    nodes = p.nodes[:5].copy()
    nodes[1, 2] = np.nan
    idx, dist = knn(p.starts, nodes, 5, False)
    assert np.array_equal(idx, C.knn32(p.starts, nodes, 5)[0]) and (idx[:, 4] == 1).all() and np.isinf(dist[:, 4]).all()
    assert np.isfinite(dist[:, :4]).all()


@pytest.mark.parametrize('name', C.SETS + ('panda:generic',))
def test_edge_check_against_the_fp64_replay(gpu_device, name):
    """2. Every edge fp64 can decide equals the kernel's flag and first index (the roadmap's M * K edges and the queries' connection and
    direct segments); at most 2 % are undecidable; both flags occur; (a, b) and (b, a) give the same bits."""
    name, _, form = name.partition(':')
    p = C.problem(name)
    r = _roadmap(name, gpu_device, use_model=form != 'generic')
    edges = _edges(p, _geom(p, gpu_device, use_model=form != 'generic'), gpu_device)
    r64 = C.edge_replay64(p, p.nodes, r.pairs, r.flag, r.first)          # (raises on the first decidable edge that differs)
    c64 = C.edge_replay64(p, r.pts, r.cpairs, r.cflag, r.cfirst)
    und = int((~r64.decidable).sum()) + int((~c64.decidable).sum())
    ref = C.reference(name).r
    print(f'{name} {form}: {len(r.pairs)} + {len(r.cpairs)} edges, FREE / BLOCKED {int((r.flag == C.FREE).sum())} / {int((r.flag == C.BLOCKED).sum())}, '
          f'undecidable {und}, longest {int(r64.n_pts.max())} points, first hits past point 63: {int((r.first >= 64).sum())}, flags that differ from '
          f'the fp32 restatement {int((r.flag != ref.flag).sum())}, smallest margin / bar {min(r64.margin_over_bar.min(), c64.margin_over_bar.min()):.1f}')
    assert und <= 0.02 * (len(r.pairs) + len(r.cpairs))
    assert (r.flag == C.FREE).any() and (r.flag == C.BLOCKED).any() and set(np.unique(r.flag)) <= {C.FREE, C.BLOCKED}
    assert ((r.first >= 0) == (r.flag == C.BLOCKED)).all() and (r.first[r.flag == C.FREE] == -1).all()
    flag, first = edges(p.nodes, np.ascontiguousarray(r.pairs[:, ::-1]))
    assert np.array_equal(flag, r.flag) and np.array_equal(first, r.first)


def test_edge_check_edges(gpu_device):
    """a == b checks that one point, an index outside 0 .. P - 1 is BAD_INDEX and never read, a segment of more than 2^20 points is
    TOO_LONG, a hit in the second trip of a long scan, E == 0 -- each also the restatement's answer."""
    from motion_planning_baselines_amd import ops
    p = C.problem('pm2d_grid')
    geom = _geom(p, gpu_device)
    pts = np.concatenate([p.nodes[:4], np.array([[-0.5, -0.5], [-0.66, -0.56], [-0.34, -0.56], [0.9, 1e6]], np.float32)])
    P = len(pts)
    pairs = np.array([[0, 0], [4, 4], [-1, 0], [0, P], [P, -1], [0, 1], [0, 4], [4, 0], [5, 6], [0, 7], [2, 3]], np.int32)
    q = types.SimpleNamespace(**vars(p))
    q.step = np.float32(0.001)                                   # (the line y = -0.56 grazes the circle at (-0.5, -0.5): rows 5 -> 6)
    flag, first = _edges(q, geom, gpu_device)(pts, pairs)
    want_flag, want_first, n_pts = C.edges32(q, pts, pairs)
    assert np.array_equal(flag, want_flag) and np.array_equal(first, want_first)
    assert flag[:5].tolist() == [C.FREE, C.BLOCKED, C.BAD_INDEX, C.BAD_INDEX, C.BAD_INDEX] and first[:5].tolist() == [-1, 0, -1, -1, -1]
    assert flag[6] == flag[7] == C.BLOCKED and first[6] == first[7] > 0
    assert flag[8] == C.BLOCKED and 64 <= first[8] < 128 and n_pts[8] > 300
    assert flag[9] == C.TOO_LONG and first[9] == -1
    C.edge_replay64(q, pts, pairs, flag, first)
    none = ops.prm_edge_check(_dev(pts, gpu_device), torch.zeros(0, 2, device=gpu_device, dtype=torch.int32), geom, 0.01)
    assert none[0].shape == none[1].shape == (0,)
    with pytest.raises(ops._lib.MPBError, match='check_step'):
        ops.prm_edge_check(_dev(pts, gpu_device), _dev(pairs, gpu_device), geom, 0.0)
    with pytest.raises(ValueError):
        ops.prm_edge_check(_dev(pts, gpu_device), _dev(pairs, gpu_device).long(), geom, 0.01)


@pytest.mark.parametrize('name', C.SETS)
def test_query_equals_the_restatement(gpu_device, name):
    """3. The kernel's own roadmap as data: costs, lengths, paths and status bit for bit; every hop of an OK path a finite table entry."""
    p, r = C.problem(name), _roadmap(name, gpu_device)
    got, want = _query(r, gpu_device), C.query32(r)
    print(name, 'status', got.status.tolist(), 'lengths', got.lengths.tolist())
    _same(got, want)
    ei, ej, _ = C.edge_list(r.nbr, r.w)
    entries = set(zip(ei.tolist(), ej.tolist())) | set(zip(ej.tolist(), ei.tolist()))
    for b in np.nonzero(got.status == C.OK)[0]:
        L = int(got.lengths[b])
        assert L >= 2 and np.array_equal(got.paths[b, 0], r.starts[b]) and np.array_equal(got.paths[b, L - 1], r.goals[b])
        ids = [int(np.nonzero((p.nodes == row).all(1))[0][0]) for row in got.paths[b, 1:L - 1]]
        assert all(hop in entries for hop in zip(ids[:-1], ids[1:])), (b, ids)
        if ids:
            assert C.finite(r.ws[b][r.cs[b] == ids[0]]).any() and C.finite(r.wg[b][r.cg[b] == ids[-1]]).any()
    assert (got.status == C.OK).sum() == C.COUNTS[name][7] and (got.lengths > 3).any()
    assert (got.status == C.DISCONNECTED).sum() == C.COUNTS[name][8]


def test_query_edges(gpu_device):
    """A start inside an obstacle: NO_START; a free straight line: the two-node path; Lmax = 3: PATH_TOO_LONG; Q = 0: empty tensors."""
    from motion_planning_baselines_amd import ops
    p = C.problem('pm2d_grid')
    dev = gpu_device
    ref = _roadmap('pm2d_grid', dev)
    zig = C.S.ZIGZAG
    starts = np.stack([np.array([-0.5, -0.5], np.float32), zig[0], p.starts[0], p.starts[0]])
    goals = np.stack([p.goals[0], zig[-1], np.array([0.25, 0.25], np.float32), p.goals[0]])
    r = C.build(p, _knn(dev), _edges(p, _geom(p, dev), dev), starts=starts, goals=goals)
    got = _query(r, dev)
    _same(got, C.query32(r))
    assert got.status.tolist() == [C.NO_START, C.OK, C.NO_GOAL, C.OK] and got.lengths[:3].tolist() == [0, 2, 0]
    assert np.array_equal(got.paths[1, :2], zig[[0, -1]]) and got.costs[1] == C.S.dist32(zig[0], zig[-1]) and not got.paths[1, 2:].any()
    assert np.isinf(got.costs[[0, 2]]).all() and not got.paths[[0, 2]].any()
    full = _query(ref, dev)
    assert np.array_equal(got.paths[3], full.paths[0]) and got.costs[3] == full.costs[0] and got.lengths[3] > 3   # (the batch does not matter)
    for Lmax in (2, 3, int(full.lengths.max()) - 1, int(full.lengths.max())):
        short = _query(ref, dev, Lmax=Lmax)
        _same(short, C.query32(ref, Lmax))
        too = full.lengths > Lmax
        assert (short.status[too] == C.PATH_TOO_LONG).all() and not short.lengths[too].any() and np.isinf(short.costs[too]).all()
        assert np.array_equal(short.lengths[~too], full.lengths[~too]) and too.any() == (Lmax < full.lengths.max())
    none = ops.prm_query(*(_dev(getattr(ref, k), dev) for k in ('nodes', 'nbr', 'w')), *(_dev(getattr(ref, k)[:0], dev) for k in
                         ('starts', 'goals', 'cs', 'ws', 'cg', 'wg', 'direct')), 8)
    assert [tuple(t.shape) for t in none] == [(0, 8, 2), (0,), (0,), (0,)]


def test_the_largest_roadmap(gpu_device):
    """M = 16 384, the limit: the knn launch takes 64 KB of dynamic LDS and the query launch 128 KB, both beyond the default limit the
    launchers raise.  A K = 8 neighbour graph of random points in the plane, every edge kept (no geometry): sampled knn rows and the
    queries' answers equal the restatement bit for bit."""
    from motion_planning_baselines_amd import ops
    dev, M, K = gpu_device, ops.PRM_MAX_NODES, 8
    rng = np.random.RandomState(9)
    nodes = rng.uniform(-1, 1, (M, 2)).astype(np.float32)
    nbr, dist = _knn(dev)(nodes, nodes, K, True)
    rows = np.array([0, 63, 64, 8191, 12289, M - 1])
    key = C.d2_32(nodes[rows], nodes).view(np.uint32).astype(np.uint64)
    key[np.arange(len(rows)), rows] = 0xFFFFFFFF
    order = np.argsort(key, axis=1, kind='stable')[:, :K]
    assert np.array_equal(nbr[rows], order)
    assert np.array_equal(dist[rows].view(np.uint32), np.sqrt(np.take_along_axis(key, order, 1).astype(np.uint32).view(np.float32)).view(np.uint32))
    idx32, dist32, _ = C.knn32(nodes[:3] + np.float32(0.001), nodes, 32)
    idx, d = _knn(dev)(nodes[:3] + np.float32(0.001), nodes, 32, False)
    assert np.array_equal(idx, idx32) and np.array_equal(d.view(np.uint32), dist32.view(np.uint32))
    starts = np.array([[-0.9, -0.9], [0.9, -0.9], [0.0, 0.0]], np.float32)
    goals = np.array([[0.9, 0.9], [-0.9, 0.9], [0.001, 0.0]], np.float32)
    cs, ws = _knn(dev)(starts, nodes, 4, False)
    cg, wg = _knn(dev)(goals, nodes, 4, False)
    r = types.SimpleNamespace(nodes=nodes, nbr=nbr, w=C.weights(dist, np.zeros(dist.shape, np.int32)), starts=starts, goals=goals, cs=cs, ws=ws,
                              cg=cg, wg=wg, direct=np.full(3, np.inf, np.float32))
    got, want = _query(r, dev, Lmax=256), C.query32(r, 256)
    print('lengths', got.lengths.tolist(), 'costs', got.costs.tolist(), 'status', got.status.tolist())
    _same(got, want)
    assert (got.status[:2] == C.OK).all() and (got.lengths[:2] > 40).all() and (got.costs[:2] > 2.5).all()
    _same(got, _query(r, dev, Lmax=256))


@pytest.mark.parametrize('name', ('pm2d_dense', 'panda_chain'))
def test_determinism_and_independence(gpu_device, name):
    """4. Two runs give the same bits (the relaxations race, the fixed point does not); permuting the queries permutes the answers;
    one query alone answers as it does in the batch."""
    p, r = C.problem(name), _roadmap(name, gpu_device)
    a = _query(r, gpu_device)
    for _ in range(3):
        _same(a, _query(r, gpu_device))
    rows = np.random.RandomState(1).permutation(C.Q)
    _same(a, _query(r, gpu_device, rows=rows), rows_a=rows)
    one = [int(np.argmax(a.lengths))]
    _same(a, _query(r, gpu_device, rows=one), rows_a=one)
    again = C.build(p, _knn(gpu_device), _edges(p, _geom(p, gpu_device), gpu_device))
    for k in ('nbr', 'dist', 'flag', 'first', 'w', 'cs', 'ws', 'cg', 'wg', 'direct'):
        assert np.array_equal(_bits(getattr(again, k)), _bits(getattr(r, k))), k


def test_planner_surface(gpu_device):
    """5. PRM.optimize_batched, set_queries on the same roadmap, HybridPlanner(PRM, GPMP2) end to end, and the refusal of an sdf_field."""
    from motion_planning_baselines_amd import geometry as G, ops
    from motion_planning_baselines_amd.planners import PRM
    from motion_planning_baselines_amd.planners.gpmp2 import GPMP2
    from motion_planning_baselines_amd.planners.hybrid_planner import HybridPlanner
    from motion_planning_baselines_amd.robot_field import PlanningTask
    dev = gpu_device
    ta = dict(device=dev, dtype=torch.float32)
    robot, field = G.RobotPointMass(2, radius=0.02), G.env_grid_circles_2d()
    task = PlanningTask(robot, field, tensor_args=ta, seed=3)
    n, H, dt, D = 6, 32, 0.15, 2
    start, goal = torch.tensor([-0.625, -0.625]), torch.tensor([0.625, 0.625])          # (the diagonal runs through the circles' centres)
    prm = PRM(task=task, start_state_pos=start.repeat(n, 1), goal_state_pos=goal.repeat(n, 1), n_nodes=500, k_neighbors=10, step_size=0.01,
              max_path_nodes=64, tensor_args=ta, seed=2)
    assert prm.nodes is None                                     # (lazy)
    paths, lengths, status = prm.optimize_batched()
    assert paths.shape == (n, 64, D) and lengths.shape == status.shape == prm.costs.shape == (n,)
    assert lengths.dtype == status.dtype == torch.int32 and prm.nodes.shape == (500, D) and prm.nbr.shape == prm.w.shape == (500, 10)
    assert (status == ops.PRM_OK).all() and (lengths > 2).all() and torch.isfinite(prm.costs).all(), (status.tolist(), lengths.tolist())
    assert all(torch.equal(paths[b], paths[0]) for b in range(n))
    L = int(lengths[0])
    assert torch.equal(paths[0, 0], start.to(dev)) and torch.equal(paths[0, L - 1], goal.to(dev)) and not paths[0, L:].any()
    assert not task.compute_collision(paths[0, :L]).any()
    seg = torch.linalg.norm((paths[0, 1:L] - paths[0, :L - 1]).double(), dim=-1).sum()
    assert abs(float(seg) - float(prm.costs[0])) <= 1e-5 * float(seg) and float(seg) >= float(torch.linalg.norm((goal - start).double()))
    assert ((prm.edge_flag == ops.PRM_EDGE_FREE) == torch.isfinite(prm.w)).all() and (prm.edge_flag == ops.PRM_EDGE_BLOCKED).any()
    one = prm.optimize()
    assert isinstance(one, list) and len(one) == n and torch.equal(one[0], paths[0, :L])
    sp, sl, stats = prm.shortcut(paths, lengths, 32)
    assert (sl <= lengths + 1).all() and (stats[:, 3] <= stats[:, 2] * (1 + 1e-6)).all()
    # other queries, the same roadmap tensors
    kept = (prm.nodes, prm.nbr, prm.w)
    prm.set_queries(torch.tensor([[0.625, -0.625], [-0.5, -0.5], [-0.64, -0.66]]), torch.tensor([[-0.625, 0.625], [0.625, 0.625], [-0.61, -0.66]]))
    paths2, lengths2, status2 = prm.optimize_batched()
    assert all(x is y for x, y in zip(kept, (prm.nodes, prm.nbr, prm.w))) and all(x is y for x, y in zip(kept, prm.build_roadmap()))
    assert paths2.shape == (3, 64, D) and status2.tolist() == [ops.PRM_OK, ops.PRM_NO_START, ops.PRM_OK] and lengths2[1:].tolist() == [0, 2]
    assert float(prm.costs[2]) == C.S.dist32(np.array([-0.64, -0.66], np.float32), np.array([-0.61, -0.66], np.float32))    # (the kernels' distance)
    assert isinstance(PRM(task=task, start_state_pos=start, goal_state_pos=goal, nodes=prm.nodes, k_neighbors=10, step_size=0.01,
                          tensor_args=ta).optimize(), torch.Tensor)
    # the sample-based half of HybridPlanner, through its optimize_batched branch
    prm.set_queries(start.repeat(n, 1), goal.repeat(n, 1))
    opt = GPMP2(robot=robot, n_dof=D, n_support_points=H, num_particles_per_goal=n, opt_iters=4, dt=dt, start_state=start.to(dev), step_size=1.0,
                multi_goal_states=goal[None].to(dev), initial_particle_means=torch.zeros(n, H, 2 * D, device=dev), collision_fields=[field],
                sigma_start=1e-5, sigma_gp=1e-2, sigma_coll=1e-5, sigma_goal_prior=1e-5,
                solver_params=dict(delta=1e-2, trust_region=True, method='cholesky'), tensor_args=ta)
    iters = HybridPlanner(prm, opt, tensor_args=ta).optimize(return_iterations=True)
    assert iters.shape == (5, n, H, 2 * D) and torch.isfinite(iters).all()
    assert torch.equal(iters[0], ops.traj_resample(paths, lengths, H, dt))                   # the initial means ARE the resampled PRM paths
    assert float((iters[-1][:, 0, :D] - start.to(dev)).abs().max()) < 1e-3 and float((iters[-1][:, -1, :D] - goal.to(dev)).abs().max()) < 1e-3
    # fields the in-kernel predicate does not know
    for kw, word in ((dict(self_field=G.SelfCollisionField(G.RobotPanda())), 'self_field'),
                     (dict(sdf_field=G.GridSDFField.from_field(G.env_spheres_3d(), (-1.2, -1.2, -0.6), (1.2, 1.2, 1.6), 0.05)), 'sdf_field')):
        t = PlanningTask(G.RobotPanda(), G.env_spheres_3d(), tensor_args=ta, **kw)
        with pytest.raises(NotImplementedError, match=word):
            PRM(task=t, start_state_pos=torch.zeros(7), goal_state_pos=torch.ones(7), tensor_args=ta)
