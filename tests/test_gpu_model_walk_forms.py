"""-m gpu: the two forms of the compile-time robot's collision walk in the persistent STOMP kernel (csrc/mpb_geom.h,
waypoint_cost_grid_model<..., UNROLLED>).  A geometry that promises ONE field (geom_flags ONE_FIELD) runs the kernels whose
group loop is unrolled; the same geometry with the bit cleared runs the chained-field kernels, which keep the rolled loop
with one arm per group.  Same calls in the same order, hinges added sphere by sphere: means, samples, costs and weights of
the two must be the same BITS -- on every kernel of the family (d = 14 / 7, exchange / two-batch layout, drawn / injected
noise) and on scenes that reach every path of the walk: group 0 skipped, partly parked and complete (static pruning of
the frame-1 spheres), and grid cells with one, two and three candidates and crowded ones (the exhaustive loop)."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, S, K = 64, 32, 3
SIGMA_COLL = 1e-3
SEED = 5                           # of the means, the injected noise and the clustered scene; chosen on the CPU, see _clustered
SCENES = ('c3', 'clustered', 'base_some', 'base_all')
# (particles, position-only, injected noise): the eight kernels of the family.  P = 0 / -1 stand for the device's CU count and
# one more.  With as many particles as CUs the launcher runs a particle's samples as two batches in one workgroup (asserted);
# with one more it goes back to two workgroups per particle (three rounds of them against two rounds of workgroups that take
# 1.88 times as long: mpb_stomp_api.hip), which then run in rounds -- the layout it reports is asserted against that rule
FORMS = [(P, pos_only, inj) for P in (2, 0, -1) for pos_only in (False, True) for inj in (False, True)]


def _clustered(seed=SEED):
    """About 40 small spheres in five clusters inside the arm's reach: the inflated balls of a cluster overlap, so the compact
    grid has cells with two and three candidates on the fringes and crowded cells (more than four: GRID_OVERFLOW) inside.
    The seed was chosen on the CPU so that the rollouts' look-ups reach all three kinds (asserted before every launch)."""
    from motion_planning_baselines_amd import geometry as G
    rng = np.random.default_rng([seed, 2])
    out = []
    for _ in range(5):
        a, rad, z = rng.uniform(-np.pi, np.pi), rng.uniform(0.35, 0.6), rng.uniform(0.1, 0.8)
        c = np.array([rad * np.cos(a), rad * np.sin(a), z])
        for _ in range(8):
            p = c + rng.normal(0.0, 0.06, 3)
            out.append((p[0], p[1], p[2], rng.uniform(0.02, 0.04)))
    return G.CollisionField(spheres=np.array(out, np.float32), margin=0.05)


def _field(scene):
    from motion_planning_baselines_amd import geometry as G
    if scene == 'clustered':
        return _clustered()
    f = G.env_spheres_3d(seed=0)                                   # C3's 16 spheres: none near the base
    # an obstacle beside the pedestal: near the lowest frame-1 sphere only / near all three of them
    extra = {'c3': [], 'base_some': [(0.2, 0.0, 0.1, 0.1)], 'base_all': [(0.2, 0.0, 0.233, 0.12)]}[scene]
    sph = np.concatenate([f.spheres, np.array(extra, np.float32).reshape(-1, 4)], 0)
    return G.CollisionField(spheres=sph, margin=f.margin)


def _means(P, pos_only):
    """Straight lines between random configurations (particle i is the same whatever P is); they cross the obstacles."""
    from motion_planning_baselines_amd import geometry as G, workloads
    robot = G.RobotPanda()
    lo, hi = robot.q_min_np, robot.q_max_np
    starts = lo + (hi - lo) * np.random.default_rng([SEED, 0]).uniform(size=(P, 7)).astype(np.float32)
    goals = lo + (hi - lo) * np.random.default_rng([SEED, 1]).uniform(size=(P, 7)).astype(np.float32)
    return workloads.straight_line_means(starts, goals, H, 5.0 / H, pos_only, 'cpu')


def _eps(P, d):
    """Injected noise in the reference's draw order (K, S, d, P, H); particle i's is the same whatever P is."""
    e = np.random.default_rng([SEED, 3]).standard_normal((P, K, S, d, H), dtype=np.float32)
    return torch.from_numpy(np.ascontiguousarray(e.transpose(1, 2, 3, 0, 4)))


def _frame1_mask(robot):
    lf = np.asarray(robot.spec()['link_frame'])
    return int(sum(1 << l for l in range(len(lf)) if lf[l] == 1))


def _lookup_kinds(host, robot, samples):
    """How many look-ups of the rollouts `samples` (p, S, H, d) -- the collision spheres of waypoints 1 .. H - 1 that are in
    the link table, placed by the oracle's FK -- land in a grid cell with two candidates, with three, and in a crowded one."""
    from motion_planning_baselines_amd import geometry as G
    from oracle.geometry_ref import RefRobot
    h = G.header(host)
    n_sph, off_grid, n_cells = int(h['n_sph']), int(h['off_grid']), int(h['n_cells'])
    dims = h['grid_dims'].astype(np.int64)
    lo, inv = h['grid_lo'].astype(np.float64), h['grid_inv'].astype(np.float64)
    keep = int(h['keep_mask'])
    ref = RefRobot(robot.spec(), tensor_args=dict(device='cpu', dtype=torch.float64))
    pts = ref.fk_map_collision(samples[..., 1:, :7].double())                    # (p, S, H - 1, links, 3)
    pts = pts[..., [l for l in range(pts.shape[-2]) if (keep >> l) & 1], :].reshape(-1, 3).numpy()
    ix = np.floor((pts - lo) * inv).astype(np.int64)
    ix = ix[((ix >= 0) & (ix < dims)).all(1)]                                     # (outside the box: no candidates)
    words = host.view(np.uint32)[off_grid:off_grid + n_cells][ix[:, 0] + dims[0] * (ix[:, 1] + dims[1] * ix[:, 2])]
    crowded = words == G.GRID_OVERFLOW
    cnt = (G.grid_cell_slots(words) != n_sph).sum(-1)
    cnt[crowded] = -1
    return int((cnt == 2).sum()), int((cnt == 3).sum()), int(crowded.sum())


@pytest.fixture(scope='module')
def shared():
    """What the cases share: geometry per scene, constants, means and injected noise per shape, oracle geometry per scene."""
    d = {}
    yield d
    d.clear()


def _get(shared, key, make):
    if key not in shared:
        shared[key] = make()
    return shared[key]


@pytest.mark.parametrize('P,pos_only,inj', FORMS)
@pytest.mark.parametrize('scene', SCENES)
def test_unrolled_walk_equals_rolled_walk(gpu_device, shared, scene, P, pos_only, inj):
    from motion_planning_baselines_amd import geometry as G, ops
    from motion_planning_baselines_amd.planners.stomp import precision_to_scale_tril, stomp_precision_matrix
    from oracle import planners_ref as O
    from oracle.geometry_ref import make_ref_geometry
    dev = gpu_device
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    if P <= 0:
        P = n_cu - P
    two_batches = P >= n_cu and 188 * ((P + n_cu - 1) // n_cu) < 100 * ((2 * P + n_cu - 1) // n_cu)     # the launcher's rule
    assert two_batches == (P == n_cu)
    d = 7 if pos_only else 14
    robot = _get(shared, 'robot', G.RobotPanda)
    field = _get(shared, ('field', scene), lambda: _field(scene))
    geom = _get(shared, ('geom', scene), lambda: ops.DeviceGeometry(robot, field, dev))
    assert geom.flags & G.GEOM_FLAG_ONE_FIELD
    # group 0 of the walk (the frame-1 spheres, which static pruning may drop): skipped / partly parked / complete
    f1 = _frame1_mask(robot)
    kept1 = int(G.header(geom.host)['keep_mask']) & f1
    assert {'c3': kept1 == 0, 'clustered': True, 'base_some': kept1 not in (0, f1), 'base_all': kept1 == f1}[scene], bin(kept1)

    def consts():
        R = stomp_precision_matrix(H, 5.0 / H, 0.1, dict(device='cpu', dtype=torch.float32))
        return torch.inverse(R).contiguous(), precision_to_scale_tril(R).contiguous()
    Sigma, L = _get(shared, 'consts', consts)
    means0 = _get(shared, ('means', P, pos_only), lambda: _means(P, pos_only))
    eps = _get(shared, ('eps', P, d), lambda: _eps(P, d).to(dev)) if inj else None
    seed, iter0 = 11, 0
    if scene == 'clustered':
        # the first iteration's rollouts of particles 0 and 1, on the host: which kinds of cell do their look-ups meet?
        e0 = eps[0, :, :, :2].cpu() if inj else ops.debug_stomp_normals(
            P, S, d, 1, dev, seed=seed, iter0=iter0, H=H)[0, :2, ..., :H].permute(1, 2, 0, 3).contiguous().cpu()
        two, three, crowded = _lookup_kinds(geom.host, robot, O.stomp_sample(means0[:2], L, e0))
        print(f'look-ups in cells with two candidates {two}, three {three}, crowded {crowded}')
        assert two > 0 and three > 0 and crowded > 0

    ws = ops.stomp_workspace(P, S, H, d, dev)
    assert ops.stomp_run_path(geom, ws, P, S, H, d) == (ops.STOMP_PATH_PERSISTENT if two_batches else ops.STOMP_PATH_PERSISTENT_EXCHANGE)
    chained = copy.copy(geom)                       # the same buffer without the one-field promise: the chained-field kernels
    chained.flags = geom.flags & ~G.GEOM_FLAG_ONE_FIELD
    out = []
    for g in (geom, chained):
        means = means0.to(dev)
        samples = torch.full((P, S, H, d), float('nan'), device=dev)
        costs, weights = torch.full((P, S), float('nan'), device=dev), torch.full((P, S), float('nan'), device=dev)
        ops.stomp_run(means, eps, samples, costs, weights, L.to(dev), Sigma.to(dev), g, S, 7, 1.0 / SIGMA_COLL ** 2, 1.0, 0.1, 1e5,
                      ws, n_iters=K, seed=seed, iter0=iter0)
        torch.cuda.synchronize()
        assert not ops.stomp_run_timed_out(ws)
        out.append((means, samples, costs, weights))
    for name, a, b in zip(('means', 'samples', 'costs', 'weights'), *out):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    means, samples, costs, _ = out[0]
    assert torch.isfinite(means).all() and torch.isfinite(costs).all() and float(costs.max()) > 0
    # the unrolled run's costs against the fp64 oracle on the same samples (a few particles: the first two and the last);
    # the bar is the one the persistent launch's costs are held to against the reference (tests/test_gpu_stomp_fused.py)
    sel = sorted({0, 1, P - 1})
    ref_robot, ref_field = _get(shared, ('ref', scene), lambda: make_ref_geometry(robot, field, dict(device='cpu', dtype=torch.float64)))
    ref = O.collision_cost(samples[sel].cpu().double().flatten(0, 1), ref_robot, ref_field, SIGMA_COLL).reshape(len(sel), S)
    ksig = 1.0 / SIGMA_COLL ** 2
    np.testing.assert_allclose(costs[sel].cpu().numpy(), ref.numpy(), rtol=5e-5, atol=1e-6 * ksig)
