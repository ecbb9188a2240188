"""Validation of trajectory batches on the GPU (csrc/mpb_traj_validate.hip, ops.traj_collision_stats, the four PlanningTask
methods) against the fp64 oracle at dense points formed in numpy fp32, against the composed route (traj_interpolate ->
collision_check), against itself (strided input, repeated calls), with two chained fields and with the compile-time Panda.

Shapes (N, H, n_interp, short): P = (H-1)(n_interp+1)+1 below one wave (43), waypoints only (3), one segment across a wave
boundary (72: collisions no waypoint sees), more than two waves (129) and more than one 256-thread trip (302)."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden, product_geometry_from_golden, ref_geometry_from_golden
from rrt_checks import hinge_argument

pytestmark = pytest.mark.gpu
SCENES = ('rrt_pm2d_grid', 'rrt_pm2d_dense', 'rrt_panda_spheres')
SHAPES = ((96, 8, 5, 0.15), (96, 3, 0, 0.15), (40, 2, 70, 0.15), (5, 65, 1, 0.3), (3, 2, 300, 0.3))
BETWEEN = (40, 2, 70, 0.15)                                      # the shape whose collisions may lie between the waypoints
CASES = [(s, sh) for s in SCENES for sh in SHAPES]
IDS = [f'{s}-{sh[0]}x{sh[1]}x{sh[2]}' for s, sh in CASES]


def _bounds(g):
    return (-1.0, 1.0) if int(g['robot_kind']) == 0 else (-2.8, 2.8)


def make_trajs(shape, D, lo, hi):
    """(N, H, D) fp32: a short straight line between two uniform draws plus a sine bump, RandomState(11), in the draw order
    a, b, the offset of b, the bump."""
    N, H, _, short = shape
    rng = np.random.RandomState(11)
    a = rng.uniform(lo, hi, (N, 1, D))
    b = rng.uniform(lo, hi, (N, 1, D))
    b = a + short * (hi - lo) * rng.uniform(-1, 1, (N, 1, D))
    t = np.linspace(0, 1, H)[None, :, None]
    w = a + (b - a) * t + 0.05 * (hi - lo) * np.sin(np.pi * t) * rng.uniform(-1, 1, (N, 1, D))
    return w.astype(np.float32)


def dense_points(w, n_interp):
    """The dense points of mpb_traj_interpolate in numpy fp32: x0 + (k / (n+1)) * (x1 - x0), the waypoint itself for k = 0
    and for the last point.  (N, H, D) -> (N, P, D)."""
    N, H, D = w.shape
    n1 = n_interp + 1
    x0, x1 = w[:, :-1, None, :], w[:, 1:, None, :]
    t = (np.arange(n1, dtype=np.float32) / np.float32(n1))[None, None, :, None]
    pts = (x0 + t * (x1 - x0)).astype(np.float32)
    pts[:, :, 0, :] = w[:, :-1]
    return np.concatenate([pts.reshape(N, (H - 1) * n1, D), w[:, -1:]], axis=1)


def oracle_points(rr, rf, pts):
    """(hinge argument max_l(margin + r_l - sdf_l), hinge sum sum_l relu(margin + r_l - sdf_l)) per dense point, fp64."""
    N, P, D = pts.shape
    want = hinge_argument(rr, rf, pts.reshape(-1, D)).reshape(N, P)
    q = torch.as_tensor(pts.reshape(-1, D), dtype=torch.float64)
    sd = rf.signed_distance(rr.fk_map_collision(q))
    gap = torch.relu(rf.margin + rf.link_radius - sd).sum(-1).numpy().reshape(N, P)
    return want, gap


@functools.lru_cache(maxsize=None)
def _scene(name):
    g = load_golden(name)
    rr, rf = ref_geometry_from_golden(g, torch.float64)
    return g, rr, rf


@functools.lru_cache(maxsize=None)
def _task(name, dev):
    from motion_planning_baselines_amd.robot_field import PlanningTask
    robot, field = product_geometry_from_golden(_scene(name)[0])
    return PlanningTask(robot, field, tensor_args=dict(device=dev, dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def _reference(name, shape):
    """The inputs of a case and the oracle's answers, computed once and shared (read only)."""
    g, rr, rf = _scene(name)
    w = make_trajs(shape, int(g['n_dof']), *_bounds(g))
    pts = dense_points(w, shape[2])
    want, gap = oracle_points(rr, rf, pts)
    slack = 32.0 * float(g['E_gap'])
    ref = dict(w=w, pts=pts, want=want, gap=gap, slack=slack, decided=np.abs(want) > slack, L=len(g['link_radius']))
    for k in ('w', 'want', 'gap', 'decided'):
        ref[k].setflags(write=False)
    return ref


def _check_inputs(label, ref, shape):
    """The conditions on the inputs: the undecided share below 1 % (a cap), both answers occur, and in the one-segment shape a
    trajectory is in collision although both of its waypoints are free."""
    want, decided = ref['want'], ref['decided']
    print(f'{label}: {int((~decided).sum())} of {decided.size} dense points within 32 E of the surface (undecided share '
          f'{(~decided).mean():.5f}); in collision {(want > 0).mean():.3f}; trajectories in collision '
          f'{int((want > 0).any(1).sum())} of {len(want)}')
    assert (~decided).mean() < 0.01
    assert 0.02 < (want > 0).mean() < 0.98
    if shape == BETWEEN:
        hidden = (want > 0).any(1) & ~(want[:, 0] > 0) & ~(want[:, -1] > 0)
        print(f'{label}: {int(hidden.sum())} trajectories collide only between their waypoints')
        assert hidden.sum() >= 1


def _call(task, w, n_interp):
    from motion_planning_baselines_amd import ops
    out = ops.traj_collision_stats(torch.from_numpy(w.copy()).to(task.device), task.geom, n_interp=n_interp, with_flags=True)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


@functools.lru_cache(maxsize=None)
def _result(name, shape, dev):
    return _call(_task(name, dev), _reference(name, shape)['w'], shape[2])


def _assert_flags(flags, ref):
    d = ref['decided']
    bad = int((flags[d] != (ref['want'][d] > 0)).sum())
    assert flags.shape == ref['want'].shape and bad == 0, bad


def _first_set(flags):
    return np.where(flags.any(1), flags.argmax(1), -1)


@pytest.mark.parametrize('name,shape', CASES, ids=IDS)
def test_point_flags_against_the_fp64_oracle(gpu_device, name, shape):
    """(1) every decided dense point gets the oracle's answer."""
    ref = _reference(name, shape)
    _check_inputs(f'{name} {shape}', ref, shape)
    _assert_flags(_result(name, shape, gpu_device)[3], ref)


@pytest.mark.parametrize('name,shape', CASES, ids=IDS)
def test_trajectory_outputs(gpu_device, name, shape):
    """(2) count and first index equal the flags' own, exactly, and the oracle's on trajectories without an undecided point;
    max_gap within 32 E_gap L of the fp64 value, and 0 exactly where the oracle says free."""
    ref = _reference(name, shape)
    count, first, gap, flags = _result(name, shape, gpu_device)
    assert count.dtype == np.int32 and first.dtype == np.int32 and gap.dtype == np.float32 and flags.dtype == np.bool_
    assert (count == flags.sum(1)).all()
    assert (first == _first_set(flags)).all()
    whole = ref['decided'].all(1)
    hit = ref['want'] > 0
    print(f'{name} {shape}: {int(whole.sum())} of {len(whole)} trajectories have every point decided')
    assert (count[whole] == hit.sum(1)[whole]).all()
    assert (first[whole] == _first_set(hit)[whole]).all()
    want_gap = ref['gap'].max(1)
    tol = ref['slack'] * ref['L']
    err = np.abs(gap.astype(np.float64) - want_gap)
    print(f'{name} {shape}: max |max_gap - fp64| {err[whole].max():.3e} (tolerance {tol:.3e})')
    assert (err[whole] <= tol).all()
    free = whole & ~hit.any(1)
    assert (gap[free] == 0.0).all() and (gap >= 0.0).all()


@pytest.mark.parametrize('name,shape', CASES, ids=IDS)
def test_strided_states_are_read_in_place(gpu_device, name, shape):
    """(3) the positions as the first D columns of an (N, H, 2D) tensor whose other columns are NaN: the same bits."""
    w = _reference(name, shape)['w']
    wide = np.full(w.shape[:2] + (2 * w.shape[2],), np.nan, np.float32)
    wide[..., :w.shape[2]] = w
    a, b = _result(name, shape, gpu_device), _call(_task(name, gpu_device), wide, shape[2])
    for x, y in zip(a, b):
        assert x.shape == y.shape and (x.view(np.uint8) == y.view(np.uint8)).all()


@pytest.mark.parametrize('name,shape', CASES, ids=IDS)
def test_agrees_with_the_composed_route(gpu_device, name, shape):
    """(4) traj_interpolate -> collision_check gives the same answer on every decided point (all points: printed)."""
    from motion_planning_baselines_amd import ops
    ref, task = _reference(name, shape), _task(name, gpu_device)
    pos = torch.from_numpy(ref['w'].copy()).to(gpu_device)
    D = pos.shape[-1]
    composed = ops.collision_check(ops.traj_interpolate(pos, shape[2]).reshape(-1, D).contiguous(), task.geom).cpu().numpy()
    flags = _result(name, shape, gpu_device)[3]
    composed = composed.reshape(flags.shape)
    print(f'{name} {shape}: fused and composed flags differ at {int((composed != flags).sum())} of {flags.size} points')
    assert (composed[ref['decided']] == flags[ref['decided']]).all()


@pytest.mark.parametrize('name,shape', CASES, ids=IDS)
def test_two_calls_give_the_same_bits(gpu_device, name, shape):
    """(5) no atomics, no order dependence: every output repeats bit for bit."""
    a, b = _result(name, shape, gpu_device), _call(_task(name, gpu_device), _reference(name, shape)['w'], shape[2])
    for x, y in zip(a, b):
        assert (x.view(np.uint8) == y.view(np.uint8)).all()


@pytest.mark.parametrize('shape', (SHAPES[0], SHAPES[4]), ids=('96x8x5', '3x2x300'))
@pytest.mark.parametrize('name', ('rrt_pm2d_grid', 'rrt_panda_spheres'))
def test_two_chained_fields(gpu_device, name, shape):
    """(6) the scene's spheres split into two fields of the same margin: the union is in collision iff a part is, so the flags
    are the single-field oracle's on every point decided for BOTH parts (the restaging of the grids inside the strided loop)."""
    from motion_planning_baselines_amd import geometry as G
    from motion_planning_baselines_amd.robot_field import PlanningTask
    from oracle.geometry_ref import RefCollisionField
    g, rr, rf = _scene(name)
    ref = _reference(name, shape)
    robot, _ = product_geometry_from_golden(g)
    sph, half, margin = g['spheres'], len(g['spheres']) // 2, float(g['margin'])
    assert len(g['boxes']) == 0 and half >= 1
    task = PlanningTask(robot, [G.CollisionField(spheres=sph[:half], margin=margin), G.CollisionField(spheres=sph[half:], margin=margin)],
                        tensor_args=dict(device=gpu_device, dtype=torch.float32))
    ta = dict(device='cpu', dtype=torch.float64)
    D = ref['pts'].shape[-1]
    parts = [hinge_argument(rr, RefCollisionField(dict(spheres=s, boxes=g['boxes'], margin=g['margin']), g['link_radius'], tensor_args=ta),
                            ref['pts'].reshape(-1, D)).reshape(ref['want'].shape) for s in (sph[:half], sph[half:])]
    assert np.array_equal(np.maximum(*parts), ref['want'])       # (the oracle of the union IS the single field's)
    decided = (np.abs(parts[0]) > ref['slack']) & (np.abs(parts[1]) > ref['slack'])
    print(f'{name} {shape}, two fields: undecided share {(~decided).mean():.5f}')
    assert (~decided).mean() < 0.01
    count, first, gap, flags = _call(task, ref['w'], shape[2])
    assert (flags[decided] == (ref['want'][decided] > 0)).all()
    assert (count == flags.sum(1)).all() and (first == _first_set(flags)).all()


def test_compile_time_panda(gpu_device):
    """(7) RobotPanda + env_spheres_3d: the PandaModel::ID instantiation, same assertions as (1)."""
    from motion_planning_baselines_amd import geometry as G
    from motion_planning_baselines_amd.robot_field import PlanningTask
    from oracle.geometry_ref import make_ref_geometry
    robot, field = G.RobotPanda(), G.env_spheres_3d(seed=0)
    task = PlanningTask(robot, field, tensor_args=dict(device=gpu_device, dtype=torch.float32))
    assert (task.geom.flags & G.GEOM_FLAG_MODEL_MASK) == 1 and task.geom.flags & G.GEOM_FLAG_ALL_GRIDS   # what the launcher asks for
    rr, rf = make_ref_geometry(robot, field, dict(device='cpu', dtype=torch.float64))
    shape = SHAPES[0]
    w = make_trajs(shape, 7, -2.8, 2.8)
    pts = dense_points(w, shape[2])
    want, gapsum = oracle_points(rr, rf, pts)
    slack = 32.0 * float(load_golden('rrt_panda_spheres')['E_gap'])
    ref = dict(want=want, decided=np.abs(want) > slack)
    _check_inputs('compile-time Panda', ref, shape)
    count, first, gap, flags = _call(task, w, shape[2])
    _assert_flags(flags, ref)
    assert (count == flags.sum(1)).all() and (first == _first_set(flags)).all()
    whole = ref['decided'].all(1)
    assert (np.abs(gap.astype(np.float64) - gapsum.max(1))[whole] <= slack * len(robot.spec()['link_radius'])).all()


@pytest.mark.parametrize('name', SCENES)
def test_planning_task_methods(gpu_device, name):
    """(8) the four methods on the (96, 8, 5) batch, a (2, 48, H, D) view of it, an all-free and an all-colliding batch."""
    shape = SHAPES[0]
    N, H, n, _ = shape
    g, rr, rf = _scene(name)
    ref, task = _reference(name, shape), _task(name, gpu_device)
    count, first, gap, flags = _result(name, shape, gpu_device)
    P = flags.shape[1]
    trajs = torch.from_numpy(ref['w'].copy()).to(gpu_device)
    free = count == 0
    assert 0 < free.sum() < N
    fraction, intensity = task.compute_fraction_free_trajs(trajs), task.compute_collision_intensity_trajs(trajs)
    assert isinstance(fraction, float) and fraction == free.sum() / N
    assert isinstance(intensity, float) and intensity == flags.sum() / (N * P)
    assert task.compute_success_free_trajs(trajs) == 1
    coll_t, free_t = task.get_trajs_collision_and_free(trajs)
    assert torch.equal(coll_t.cpu(), torch.from_numpy(ref['w'][~free].copy())) and torch.equal(free_t.cpu(), torch.from_numpy(ref['w'][free].copy()))
    coll_t2, coll_i, free_t2, free_i, wic = task.get_trajs_collision_and_free(trajs, return_indices=True)
    assert torch.equal(coll_t2, coll_t) and torch.equal(free_t2, free_t)
    assert (coll_i.cpu().numpy() == np.nonzero(~free)[0]).all() and (free_i.cpu().numpy() == np.nonzero(free)[0]).all()
    assert sorted(coll_i.tolist() + free_i.tolist()) == list(range(N))
    assert wic.dtype == torch.bool and (wic.cpu().numpy() == flags).all()
    # leading dimensions are flattened
    nested = trajs.reshape(2, N // 2, H, -1)
    assert task.compute_fraction_free_trajs(nested) == fraction and task.compute_collision_intensity_trajs(nested) == intensity
    assert task.compute_success_free_trajs(nested) == 1
    nc, nf = task.get_trajs_collision_and_free(nested)
    assert torch.equal(nc, coll_t) and torch.equal(nf, free_t)
    # a state trajectory (positions, velocities): the rows come back whole
    states = torch.cat([trajs, torch.full_like(trajs, float('nan'))], dim=-1)
    sc, sf = task.get_trajs_collision_and_free(states)
    assert sc.shape == (int((~free).sum()), H, 2 * trajs.shape[-1]) and torch.equal(sf[..., :trajs.shape[-1]], free_t)
    # another density: the waypoints alone see fewer collisions, never more
    assert task.compute_collision_intensity_trajs(trajs, num_interpolation=0) == flags[:, ::n + 1].sum() / (N * H)
    # every trajectory free: the golden's first start configuration, free by more than the slack
    q0 = g['starts'][0]
    assert hinge_argument(rr, rf, q0[None])[0] < -ref['slack']
    still = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(q0.astype(np.float32), (N, H, len(q0))))).to(gpu_device)
    c, f = task.get_trajs_collision_and_free(still)
    assert c is None and torch.equal(f, still)
    assert task.compute_fraction_free_trajs(still) == 1.0 and task.compute_collision_intensity_trajs(still) == 0.0
    assert task.compute_success_free_trajs(still) == 1
    # every trajectory in collision: the centre of the scene's first obstacle sphere (point robot), or the configuration whose
    # hinge argument is largest among many draws (arm: a configuration has no "centre of a sphere")
    if int(g['robot_kind']) == 0:
        qc = g['spheres'][0, :len(q0)]
    else:
        draws = np.random.RandomState(0).uniform(-2.5, 2.5, size=(4000, len(q0)))
        qc = draws[hinge_argument(rr, rf, draws).argmax()]
    assert hinge_argument(rr, rf, qc[None].astype(np.float32))[0] > ref['slack']
    stuck = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(qc.astype(np.float32), (N, H, len(q0))))).to(gpu_device)
    c, f = task.get_trajs_collision_and_free(stuck)
    assert f is None and torch.equal(c, stuck)
    assert task.compute_success_free_trajs(stuck) == 0 and task.compute_collision_intensity_trajs(stuck) == 1.0
    assert task.compute_fraction_free_trajs(stuck) == 0.0
