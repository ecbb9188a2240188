"""-m gpu: the generalised persistent STOMP kernel (csrc/mpb_stomp_fused_hx.hip: any H <= 128, d <= 16, S <= 128) --
VERDICT r02 item 4.  Which kernel serves a call is asserted through mpb_stomp_run_path, never inferred from timing.
  * H = 64 shapes FORCED onto it (MPB_STOMP_HX=1) against the two-kernel path: samples and costs bit for bit, weights and
    means to rounding -- the same bars the H = 64 kernel is held to;
  * horizons 32 / 48 / 100 / 128, channel counts 3 / 4 / 6 / 14 (run-time d), S up to 128, ragged last batches, against
    the two-kernel path (whose chunked kernels have their own goldens);
  * n iterations in ONE launch == n launches of one iteration, bit for bit;
  * the reference-generated goldens stomp_panda_h128_s32 (H = 128, S = 32, d = 14) and stomp_panda_h32_s64 reach it
    through mpb_stomp_run (tests/test_gpu_stomp_fused.py parametrises over STOMP_CASES: teacher-forced + free-running)."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_gpu_parity_ops import dev_geom, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture
def force_hx():
    os.environ['MPB_STOMP_HX'] = '1'          # read by the launcher at every call (a test aid)
    yield
    os.environ.pop('MPB_STOMP_HX', None)


def _problem(dev, robot_kind, P, S, H, pos_only, seed=0):
    """(means0, geom, D, d) of a synthetic problem: the Panda among spheres, or a point robot in 2-D / 3-D."""
    from motion_planning_baselines_amd import geometry as G, ops, workloads
    if robot_kind == 'panda':
        wl = workloads.panda_spheres_stomp(P, dev, H=H, S=S, pos_only=pos_only)
        return wl['means0'], ops.DeviceGeometry(wl['robot'], wl['field'], dev), 7, wl['params']['dt']
    D = 2 if robot_kind == 'pm2d' else 3
    robot = G.RobotPointMass(D, radius=0.02)
    gen = torch.Generator().manual_seed(seed)
    if D == 2:
        field = G.env_grid_circles_2d()
    else:
        c = torch.rand(24, 3, generator=gen) * 1.6 - 0.8
        field = G.CollisionField(spheres=np.concatenate([c.numpy(), np.full((24, 1), 0.12)], 1).astype(np.float32), margin=0.03)
    a, b = torch.rand(P, 1, D, generator=gen) * 1.6 - 0.8, torch.rand(P, 1, D, generator=gen) * 1.6 - 0.8
    s = torch.linspace(0, 1, H).reshape(1, H, 1)
    pos = a * (1 - s) + b * s
    dt = 0.04
    means0 = pos if pos_only else torch.cat([pos, ((b - a) / ((H - 1) * dt)).expand(P, H, D)], -1)
    return means0.contiguous().to(dev), ops.DeviceGeometry(robot, field, dev), D, dt


def _constants(H, dt, sigma_spectral, dev):
    from motion_planning_baselines_amd.planners.stomp import precision_to_scale_tril, stomp_precision_matrix
    R = stomp_precision_matrix(H, dt, sigma_spectral, dict(device='cpu', dtype=torch.float32))
    return torch.inverse(R).to(dev).contiguous(), precision_to_scale_tril(R).to(dev).contiguous()


def _compare_with_two_kernel(dev, robot_kind, P, S, H, pos_only, n_iters, costs_exact):
    from motion_planning_baselines_amd import ops
    means0, geom, D, dt = _problem(dev, robot_kind, P, S, H, pos_only)
    d = means0.shape[-1]
    Sigma, L = _constants(H, dt, 0.02, dev)
    mk = lambda: (torch.empty(P, S, H, d, device=dev), torch.empty(P, S, device=dev), torch.empty(P, S, device=dev))
    ws = ops.stomp_workspace(P, S, H, d, dev)
    assert ops.stomp_run_path(geom, ws, P, S, H, d) != ops.STOMP_PATH_TWO_KERNEL
    args = (L, Sigma, geom, S, D, 1e4, 1.0, 0.1, 1e3)
    # (a) one iteration against the two-kernel loop
    mf, (sf, cf, wf) = means0.clone(), mk()
    ops.stomp_run(mf, None, sf, cf, wf, *args, ws, n_iters=1, seed=11)
    mt, (st, ct, wt) = means0.clone(), mk()
    ops.stomp_step(mt, None, st, ct, wt, *args, n_iters=1, seed=11)
    torch.cuda.synchronize()
    assert not ops.stomp_run_timed_out(ws)
    assert torch.isfinite(mf).all() and float(ct.max()) > 0
    assert torch.equal(sf, st)
    if costs_exact:
        assert torch.equal(cf, ct)
    else:       # two horizon chunks: the per-chunk wave sums are added in another order than the two-kernel path's per-lane sums
        np.testing.assert_allclose(cf.cpu().numpy(), ct.cpu().numpy(), rtol=2e-6, atol=1e-7 * float(ct.max()))
    np.testing.assert_allclose(wf.cpu().numpy(), wt.cpu().numpy(), rtol=5e-5, atol=1e-6)
    assert rel_err(mf, mt) < 5e-6
    # (b) n iterations in one launch == n launches of one iteration
    m1, (s1, c1, w1) = means0.clone(), mk()
    ops.stomp_run(m1, None, s1, c1, w1, *args, ws, n_iters=n_iters, seed=11, iter0=5)
    torch.cuda.synchronize()
    assert not ops.stomp_run_timed_out(ws)
    m2, (s2, c2, w2) = means0.clone(), mk()
    for it in range(n_iters):
        ops.stomp_run(m2, None, s2, c2, w2, *args, ws, n_iters=1, seed=11, iter0=5 + it)
    torch.cuda.synchronize()
    assert torch.equal(m1, m2) and torch.equal(s1, s2) and torch.equal(c1, c2) and torch.equal(w1, w2)


@pytest.mark.parametrize('P,S,pos_only,n_iters', [
    (128, 32, False, 3),     # C3's shape: two workgroups per particle
    (8, 16, False, 3),       # one workgroup per particle, one pass
    (8, 64, True, 2),        # four workgroups per particle, d = 7
    (3, 30, False, 2),       # S = 30: a ragged last pass; P not a multiple of 8
    (5, 5, True, 2),
    (300, 32, False, 2),     # more particles than CUs: one workgroup per particle, two passes, no exchange
    (7, 100, False, 2),      # S = 100: 7 passes over 4 workgroups, ragged
    (2, 128, True, 2)])      # S = 128
def test_hx_kernel_h64_equals_two_kernel_path(gpu_device, force_hx, P, S, pos_only, n_iters):
    _compare_with_two_kernel(gpu_device, 'panda', P, S, 64, pos_only, n_iters, costs_exact=True)


@pytest.mark.parametrize('robot_kind,P,S,H,pos_only,n_iters', [
    ('panda', 128, 32, 128, False, 2),    # the h128 bench shape
    ('panda', 4, 32, 128, True, 2),
    ('panda', 3, 20, 100, False, 2),      # a ragged second chunk (36 waypoints), H*d = 1400
    ('panda', 6, 64, 32, True, 2),        # half a chunk
    ('panda', 5, 12, 48, False, 2),
    ('panda', 4, 16, 50, True, 2),        # H d = 350: the last lane row of the weighted sum is cut at 14 lanes (DPP sources 14, 15 beyond it)
    ('panda', 3, 24, 90, True, 2),        # two chunks, H d = 630 = 39 rows + 6 lanes
    ('pm3d', 4, 16, 37, True, 2),         # run-time d = 3, H d = 111 = 6 rows + 15 lanes
    ('pm2d', 9, 24, 128, False, 2),       # run-time d = 4
    ('pm2d', 4, 40, 64, True, 2),         # d = 2 through the run-time-d kernel (forced below is not needed: H = 64 d = 2 is the other kernel's)
    ('pm3d', 5, 16, 96, True, 2),         # d = 3 (odd: scalar stores)
    ('pm3d', 3, 128, 128, False, 2)])     # d = 6, S = 128, H = 128: eight passes over two workgroups
def test_hx_kernel_other_shapes_equal_two_kernel_path(gpu_device, robot_kind, P, S, H, pos_only, n_iters):
    if H == 64:
        os.environ['MPB_STOMP_HX'] = '1'
    try:
        _compare_with_two_kernel(gpu_device, robot_kind, P, S, H, pos_only, n_iters, costs_exact=(H <= 64))
    finally:
        os.environ.pop('MPB_STOMP_HX', None)


@pytest.mark.parametrize('name', ['stomp_panda_h128_s32', 'stomp_panda_h32_s64', 'stomp_pm2d_h48'])
def test_goldens_beyond_h64_reach_the_persistent_kernel(gpu_device, name):
    """The path id of these goldens' shapes (they are run teacher-forced and free-running by test_gpu_stomp_fused.py)."""
    from motion_planning_baselines_amd import ops
    g = load_golden(name)
    dev = gpu_device
    P, S, H, d = int(g['P']), int(g['S']), int(g['H']), g['means0'].shape[-1]
    ws = ops.stomp_workspace(P, S, H, d, dev)
    assert ops.stomp_run_path(dev_geom(g, dev), ws, P, S, H, d) in (ops.STOMP_PATH_PERSISTENT, ops.STOMP_PATH_PERSISTENT_EXCHANGE)


def test_stomp_class_h128_runs_persistent(gpu_device):
    """The planner class at H = 128, S = 32, d = 14, P = 128 (the bench's h128 entry): persistent path, finite, cost falls."""
    from motion_planning_baselines_amd import ops, workloads
    from motion_planning_baselines_amd.planners.costs.cost_functions import CostCollision, CostComposite
    from motion_planning_baselines_amd.planners.stomp import STOMP
    dev = gpu_device
    H = 128
    wl = workloads.panda_spheres_stomp(128, dev, H=H, S=32, pos_only=False)
    ta = dict(device=dev, dtype=torch.float32)
    cost = CostComposite(wl['robot'], H, [CostCollision(wl['robot'], H, field=wl['field'], sigma_coll=wl['sigma_coll'],
                                                        tensor_args=ta)], tensor_args=ta)
    prm = dict(wl['params'])
    prm.update(sigma_spectral=1.0, temperature=0.5)
    pl = STOMP(opt_iters=1, start_state=torch.from_numpy(wl['starts'][0]).to(dev), cost=cost,
               initial_particle_means=wl['means0'], tensor_args=ta, **prm)
    assert pl.run_path() == ops.STOMP_PATH_PERSISTENT_EXCHANGE
    c0 = cost(pl._particle_means).clone()
    out = pl.optimize(opt_iters=40)
    c1 = cost(pl._particle_means)
    torch.cuda.synchronize()
    assert not pl.persistent_timed_out()
    assert torch.isfinite(out).all() and torch.equal(out, pl._particle_means)
    assert float(c1.sum()) < 0.8 * float(c0.sum())


def _sweep_shapes(n, seed):
    """A seeded coarse sample of the generalised kernel's shape space: H in 17 .. 128, d in 1 .. 16 (= D or 2 D of a serial
    chain with D <= 8 joints), S in 1 .. 40, P in 1 .. 12 -- with the residues that decide its code paths covered on purpose:
    H d mod 16 (lane rows of the DPP weighted sum), H mod 64 / H > 64 (one or two horizon chunks), S mod 16 and S mod 8
    (ragged last pass)."""
    rng = np.random.RandomState(seed)
    shapes, seen = [], set()
    while len(shapes) < n:
        # (every eighth shape sits on an edge of the horizon's chunking)
        H = int(rng.randint(17, 129)) if len(shapes) % 8 else int(rng.choice([17, 63, 65, 127, 128, 33, 96, 31]))
        D = int(rng.randint(1, 9))
        pos_only = bool(rng.randint(0, 2))
        d = D if pos_only else 2 * D
        S = int(rng.randint(1, 41))
        P = int(rng.randint(1, 13))
        if H == 64 or (H, d, S) in seen:
            continue
        seen.add((H, d, S))
        shapes.append((P, S, H, D, pos_only))
    return shapes


def test_hx_kernel_shape_space_sweep(gpu_device):
    """VERDICT r05 item 7 (the round-5 bug at H = 37, d = 3 was found by reading, the shapes had been hand-picked): >= 64
    seeded random shapes of stomp_fused_hx_kernel per run against the two-kernel path -- samples bit for bit (costs too
    on one horizon chunk), weights / means to rounding, and K iterations in one launch == K one-iteration launches bit for
    bit -- and, for a handful, the oracle's STOMP iteration on the drawn normals."""
    from motion_planning_baselines_amd import ops
    from test_gpu_generic_dof import make_arm, make_field, trajs
    dev = gpu_device
    shapes = _sweep_shapes(64, seed=20261004)
    residues = {(H * (D if po else 2 * D)) % 16 for _, _, H, D, po in shapes}
    assert len(residues) >= 10 and any(H > 64 for _, _, H, _, _ in shapes) and any(H < 64 for _, _, H, _, _ in shapes)
    field = make_field()
    geoms = {}
    n_oracle = 0
    for i, (P, S, H, D, pos_only) in enumerate(shapes):
        d = D if pos_only else 2 * D
        tag = 'P=%d S=%d H=%d D=%d d=%d' % (P, S, H, D, d)
        if D not in geoms:
            geoms[D] = (make_arm(D), ops.DeviceGeometry(make_arm(D), field, dev))
        robot, geom = geoms[D]
        means0 = trajs(D, P, H, d, seed=i).to(dev)
        Sigma, L = _constants(H, 0.05, 0.05, dev)
        mk = lambda: (torch.empty(P, S, H, d, device=dev), torch.empty(P, S, device=dev), torch.empty(P, S, device=dev))
        ws = ops.stomp_workspace(P, S, H, d, dev)
        assert ops.stomp_run_path(geom, ws, P, S, H, d) != ops.STOMP_PATH_TWO_KERNEL, tag
        args = (L, Sigma, geom, S, D, 25.0, 1.0, 0.3, 2.0)
        mf, (sf, cf, wf) = means0.clone(), mk()
        ops.stomp_run(mf, None, sf, cf, wf, *args, ws, n_iters=1, seed=5, iter0=i)
        mt, (st, ct, wt) = means0.clone(), mk()
        ops.stomp_step(mt, None, st, ct, wt, *args, n_iters=1, seed=5, iter0=i)
        torch.cuda.synchronize()
        assert not ops.stomp_run_timed_out(ws), tag
        assert torch.isfinite(mf).all(), tag
        assert torch.equal(sf, st), tag
        if H <= 64:
            assert torch.equal(cf, ct), tag
        else:
            np.testing.assert_allclose(cf.cpu().numpy(), ct.cpu().numpy(), rtol=2e-6, atol=1e-7 * max(float(ct.max()), 1e-30), err_msg=tag)
        np.testing.assert_allclose(wf.cpu().numpy(), wt.cpu().numpy(), rtol=1e-4, atol=2e-6, err_msg=tag)
        assert rel_err(mf, mt) < 2e-5, (tag, rel_err(mf, mt))      # (soft weights at temperature 2: sums in another order)
        # three iterations in one launch == three launches
        m1, (s1, c1, w1) = means0.clone(), mk()
        ops.stomp_run(m1, None, s1, c1, w1, *args, ws, n_iters=3, seed=5, iter0=7)
        m2, (s2, c2, w2) = means0.clone(), mk()
        for it in range(3):
            ops.stomp_run(m2, None, s2, c2, w2, *args, ws, n_iters=1, seed=5, iter0=7 + it)
        torch.cuda.synchronize()
        assert not ops.stomp_run_timed_out(ws), tag
        assert torch.equal(m1, m2) and torch.equal(s1, s2) and torch.equal(c1, c2) and torch.equal(w1, w2), tag
        if i % 11 == 0:          # the oracle on the normals the kernel drew (stomp.py:150-160), one iteration
            from oracle import planners_ref as O
            from oracle.geometry_ref import make_ref_geometry
            rr, rf = make_ref_geometry(robot, field)
            nrm = ops.debug_stomp_normals(P, S, d, 1, dev, seed=5, iter0=i, particle_offset=0, H=H)
            eps = nrm[0, ..., :H].permute(1, 2, 0, 3).contiguous().cpu()           # (S, d, P, H)
            ref = O.stomp_iteration(means0.cpu(), eps, L.cpu(), Sigma.cpu(), lambda x: O.collision_cost(x, rr, rf, 0.2), 0.3, 2.0)
            assert rel_err(sf, ref['samples']) < 2e-5, tag
            np.testing.assert_allclose(cf.cpu().numpy(), ref['costs'].numpy(), rtol=1e-4, atol=1e-4 * max(float(ref['costs'].max()), 1e-6), err_msg=tag)
            assert rel_err(mf, ref['means']) < 1e-4, (tag, rel_err(mf, ref['means']))
            n_oracle += 1
    assert n_oracle >= 5


def _list_scene(seed=0, n_sph=200, n_box=32, margin=0.04):
    from motion_planning_baselines_amd import geometry as G
    return G.env_spheres_boxes_3d(seed, n_sph, n_box, margin)


@pytest.mark.parametrize('robot_kind,P,S,H,pos_only,use_model', [
    ('panda', 16, 32, 64, False, True),      # C3's shape on a 200-sphere + 32-box scene: the model walk over the list grid
    ('panda', 6, 20, 64, True, False),       # d = 7 through the table-driven walk (run-time d)
    ('arm5', 5, 24, 48, False, False),       # a 5-joint chain, d = 10, H = 48
    ('arm9', 5, 24, 64, True, False),        # a 9-joint chain (MPB_MAX_DOF 12 since round 6), position only: d = 9
    ('panda2', 4, 16, 64, False, True)])     # two chained fields, one of them small: both packed as list grids
def test_list_grid_scene_on_the_persistent_path(gpu_device, robot_kind, P, S, H, pos_only, use_model):
    """Round 6: a scene with 200 obstacle spheres and 32 boxes -- far beyond the compact grid's 63 spheres and
    three candidates per cell, which dropped such scenes to the two-kernel EXHAUSTIVE walk -- stays on the persistent launch: the
    geometry is packed as version 7 (list grid: any number of candidates per cell, boxes culled like spheres) and
    stomp_fused_hx_kernel<..., LIST> keeps its tables in LDS.  Against the two-kernel path (exhaustive evaluator, every obstacle):
    samples and costs bit for bit (conservative candidate sets, same expressions, exact min), weights / means to rounding; three
    iterations in one launch == three launches; injected noise == device noise bits; and the oracle on the drawn normals."""
    from motion_planning_baselines_amd import geometry as G, ops
    from oracle import planners_ref as O
    from oracle.geometry_ref import make_ref_geometry
    from test_gpu_generic_dof import make_arm, trajs
    dev = gpu_device
    field = _list_scene()
    if robot_kind in ('arm5', 'arm9'):
        D = int(robot_kind[3:])
        robot = make_arm(D)
    else:
        robot, D = G.RobotPanda(), 7
    fields = [G.env_spheres_3d(seed=2), field] if robot_kind == 'panda2' else field
    geom = ops.DeviceGeometry(robot, fields, dev, use_model=use_model)
    assert (geom.flags & (G.GEOM_FLAG_ALL_LISTS | G.GEOM_FLAG_ALL_GRIDS)) == G.GEOM_FLAG_ALL_LISTS
    assert bool(geom.flags & G.GEOM_FLAG_MODEL_MASK) == use_model
    d = D if pos_only else 2 * D
    means0 = trajs(D, P, H, d, seed=3).to(dev)
    Sigma, L = _constants(H, 0.05, 0.05, dev)
    mk = lambda: (torch.empty(P, S, H, d, device=dev), torch.empty(P, S, device=dev), torch.empty(P, S, device=dev))
    ws = ops.stomp_workspace(P, S, H, d, dev)
    assert ops.stomp_run_path(geom, ws, P, S, H, d) != ops.STOMP_PATH_TWO_KERNEL
    args = (L, Sigma, geom, S, D, 25.0, 1.0, 0.3, 2.0)
    mf, (sf, cf, wf) = means0.clone(), mk()
    ops.stomp_run(mf, None, sf, cf, wf, *args, ws, n_iters=1, seed=5, iter0=2)
    mt, (st, ct, wt) = means0.clone(), mk()
    ops.stomp_step(mt, None, st, ct, wt, *args, n_iters=1, seed=5, iter0=2)
    torch.cuda.synchronize()
    assert not ops.stomp_run_timed_out(ws)
    assert torch.isfinite(mf).all() and float(ct.max()) > 0 and float((ct > 0).float().mean()) > 0.5
    assert torch.equal(sf, st)
    assert torch.equal(cf, ct), float((cf - ct).abs().max())
    np.testing.assert_allclose(wf.cpu().numpy(), wt.cpu().numpy(), rtol=1e-4, atol=2e-6)
    assert rel_err(mf, mt) < 2e-5
    # three iterations in one launch == three launches; injected normals == the device's own draw
    m1, (s1, c1, w1) = means0.clone(), mk()
    ops.stomp_run(m1, None, s1, c1, w1, *args, ws, n_iters=3, seed=5, iter0=7)
    m2, (s2, c2, w2) = means0.clone(), mk()
    for it in range(3):
        ops.stomp_run(m2, None, s2, c2, w2, *args, ws, n_iters=1, seed=5, iter0=7 + it)
    nrm = ops.debug_stomp_normals(P, S, d, 3, dev, seed=5, iter0=7, particle_offset=0, H=H)
    eps = nrm[..., :H].permute(0, 2, 3, 1, 4).contiguous()
    m3, (s3, c3, w3) = means0.clone(), mk()
    ops.stomp_run(m3, eps, s3, c3, w3, *args, ws, n_iters=3)
    torch.cuda.synchronize()
    assert not ops.stomp_run_timed_out(ws)
    assert torch.equal(m1, m2) and torch.equal(s1, s2) and torch.equal(c1, c2) and torch.equal(w1, w2)
    assert torch.equal(m1, m3) and torch.equal(s1, s3) and torch.equal(c1, c3) and torch.equal(w1, w3)
    # the oracle (stomp.py:150-160) on the normals of the first launch
    nrm = ops.debug_stomp_normals(P, S, d, 1, dev, seed=5, iter0=2, particle_offset=0, H=H)
    e0 = nrm[0, ..., :H].permute(1, 2, 0, 3).contiguous().cpu()
    fl = fields if isinstance(fields, list) else [fields]
    refs = [make_ref_geometry(robot, f) for f in fl]

    def cost_fn(x):
        return sum(O.collision_cost(x, rr, rf, 0.2) for rr, rf in refs)
    ref = O.stomp_iteration(means0.cpu(), e0, L.cpu(), Sigma.cpu(), cost_fn, 0.3, 2.0)
    assert rel_err(sf, ref['samples']) < 2e-5
    np.testing.assert_allclose(cf.cpu().numpy(), ref['costs'].numpy(), rtol=1e-4, atol=1e-4 * float(ref['costs'].max()))
    assert rel_err(mf, ref['means']) < 1e-4
