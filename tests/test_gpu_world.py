"""The world predicate on the GPU (csrc/mpb_world.h; ops.DeviceWorld, PlanningTask(world_predicate=True)): one in-kernel predicate over
obstacles, SDF grid and the robot against itself, in the stand-alone op, the trajectory validation, the shortcut pass and RRT-Connect.
Against the three stand-alone predicates bit for bit, against the composed routes, against the old entries with a null world, and
against the fp64 restatements of world_checks.py (which has the scenes and says what is excused)."""
import numpy as np
import pytest
import torch

import path_shortcut_checks as K
import world_checks as W
from rrt_checks import check_rrt_result

pytestmark = pytest.mark.gpu
_SCENES = {}


def _scene(name, dev):
    """(scene, plain task -- three launches per _in_collision --, task with world_predicate=True), built once per scene."""
    from motion_planning_baselines_amd.robot_field import PlanningTask
    if name not in _SCENES:
        sc = W.scene(name)
        kw = dict(self_field=sc.self_field, sdf_field=sc.grid, tensor_args=dict(device=dev, dtype=torch.float32))
        _SCENES[name] = (sc, PlanningTask(sc.robot, sc.field, **kw), PlanningTask(sc.robot, sc.field, world_predicate=True, **kw))
    return _SCENES[name]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _dims_word():
    from motion_planning_baselines_amd import sdf_layout
    return sdf_layout.HEADER_DTYPE.fields['dims'][1] // 4


class _changed_sdf_header:
    """The SDF buffer's nx word edited through the public buffer AFTER the launcher has cached this address's header; restored and
    announced on the way out."""

    def __init__(self, task):
        self.task, self.i = task, _dims_word()

    def __enter__(self):
        words = self.task.sdf_geom.buf.view(torch.int32)
        self.old = int(words[self.i])
        words[self.i] = self.old + 1

    def __exit__(self, *exc):
        from motion_planning_baselines_amd import _lib, ops
        self.task.sdf_geom.buf.view(torch.int32)[self.i] = self.old
        _lib.check(_lib.lib().mpb_sdf_grid_invalidate(ops._ptr(self.task.sdf_geom.buf)), 'mpb_sdf_grid_invalidate')


# ---- 1. the predicate -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', W.SCENES)
def test_predicate(gpu_device, name):
    from motion_planning_baselines_amd import ops
    sc, plain, task = _scene(name, gpu_device)
    world, null = task.world, ops.DeviceWorld(task.geom)
    alone = np.zeros(3, int)
    for label, qn in W.inputs(name).items():
        q = torch.from_numpy(qn).to(gpu_device)
        flag, parts = ops.world_collision_check(q, world, with_parts=True)
        assert torch.equal(flag, ops.world_collision_check(q, world)) and torch.equal(flag, task._in_collision(q))
        assert torch.equal(flag, plain._in_collision(q)), f'{name} {label}: the fused flags differ from the three launches ORed'
        # the three parts: the stand-alone gaps, bit for bit (an absent part: 0)
        gaps = [ops.collision_check(q, plain.geom, with_gap=True)[1], ops.sdf_grid_check(q, plain.sdf_geom, with_gap=True)[1],
                torch.zeros(len(q), device=gpu_device) if plain.self_geom is None else ops.self_collision_check(q, plain.self_geom, with_gap=True)[1]]
        for k, part in enumerate(W.PARTS):
            differ = int((_bits(parts[:, k]) != _bits(gaps[k])).sum())
            assert differ == 0, f'{name} {label}: part {part} differs from its stand-alone gap in {differ} of {len(q)} configurations'
        assert torch.equal(flag, (parts > 0).any(1))
        # a world of the geometry alone: mpb_collision_check's bits
        f0, p0 = ops.world_collision_check(q, null, with_parts=True)
        c0, g0 = ops.collision_check(q, plain.geom, with_gap=True)
        assert torch.equal(f0, c0) and torch.equal(_bits(p0[:, 0]), _bits(g0)) and not p0[:, 1:].any()
        # fp64: the OR of the three restatements wherever no hinge argument lies within its bar of zero
        d = W.decide(sc, qn)
        ok = ~d.excused
        got = flag.cpu().numpy()
        print(f'{name} {label}: n {len(qn)}, in collision {got.mean():.3f}, excused share {d.excused.mean():.4f}, E32 {d.E32.tolist()}')
        assert d.excused.mean() <= W.CAP
        assert (got[ok] == d.flag64[ok]).all(), f'{name} {label}: {int((got[ok] != d.flag64[ok]).sum())} decidable flags differ from fp64'
        pn = parts.cpu().numpy()
        alone += [int(((pn[:, k] > 0) & (np.delete(pn, k, axis=1) <= 0).all(1)).sum()) for k in range(3)]
    for k, part in enumerate(W.PARTS):
        assert sc.parts64[k] is None or alone[k] > 0, f'{name}: no configuration is refused by the {part} part alone'


def test_predicate_refusals_and_a_changed_header(gpu_device):
    from motion_planning_baselines_amd import _lib, ops
    from test_gpu_generic_dof import make_arm
    sc, plain, task = _scene('panda', gpu_device)
    q = torch.from_numpy(W.inputs('panda')['u21']).to(gpu_device)
    flag, parts = ops.world_collision_check(q, task.world, with_parts=True)
    # a buffer packed for another robot width: refused by DeviceWorld, and by the entry itself after it has read the header
    arm = make_arm(12)
    sdf12 = ops.DeviceSDFGrid(arm, W.scene('chain64').grid, gpu_device)
    with pytest.raises(ValueError, match='n_dof = 12'):
        ops.DeviceWorld(task.geom, sdf=sdf12)
    out = torch.empty(len(q), device=gpu_device, dtype=torch.bool)
    h = _lib.lib()
    rc = h.mpb_world_collision_check(ops._ptr(q), ops._ptr(task.geom.buf), int(task.geom.flags), ops._ptr(sdf12.buf), None, ops._ptr(out), None,
                                     len(q), 7, None)
    assert rc == 1 and b'D = 7' in h.mpb_last_error() and b'12 coordinates' in h.mpb_last_error()
    with pytest.raises(TypeError):
        ops.world_collision_check(q, task.geom)
    with pytest.raises(ValueError, match='columns'):
        ops.world_collision_check(q[:, :6].contiguous(), task.world)
    # the header changed under the launcher: every configuration in collision, the part NaN, nothing read through the changed word
    with _changed_sdf_header(task):
        f2, p2 = ops.world_collision_check(q, task.world, with_parts=True)
        assert f2.all() and torch.isnan(p2[:, 1]).all() and torch.equal(_bits(p2[:, [0, 2]]), _bits(parts[:, [0, 2]]))
    f3, p3 = ops.world_collision_check(q, task.world, with_parts=True)
    assert torch.equal(f3, flag) and torch.equal(_bits(p3), _bits(parts))


# ---- 2. validation --------------------------------------------------------------------------------------------------------------------
def _composed(t, n, world, D):
    """traj_interpolate, then world_collision_check on the same points: (count, first, max_gap, flags)."""
    from motion_planning_baselines_amd import ops
    N = t.shape[0]
    dense = ops.traj_interpolate(t, n)
    flag, parts = ops.world_collision_check(dense.reshape(-1, D).contiguous(), world, with_parts=True)
    flag = flag.reshape(N, -1)
    gap = ((parts[:, 0] + parts[:, 1]) + parts[:, 2]).reshape(N, -1).amax(1).clamp_min(0.0)
    P = flag.shape[1]
    first = torch.where(flag, torch.arange(P, device=t.device), P).amin(1)
    return flag.sum(1).to(torch.int32), torch.where(first == P, -1, first).to(torch.int32), gap, flag


@pytest.mark.parametrize('name', W.SCENES)
def test_validation(gpu_device, name):
    from motion_planning_baselines_amd import ops
    sc, plain, task = _scene(name, gpu_device)
    t = torch.from_numpy(W.trajectories(name)).to(gpu_device)
    N, H, D = t.shape
    for tr, n in ((t, 5), (t, 0), (t[:, :2].contiguous(), 0), (t[:, :2].contiguous(), 3)):
        count, first, gap, flags = ops.traj_collision_stats(tr, task.world, n_interp=n, with_flags=True)
        c2, f2, g2, fl2 = _composed(tr, n, task.world, D)
        assert torch.equal(flags, fl2) and torch.equal(count, c2) and torch.equal(first, f2), (name, n)
        assert torch.equal(_bits(gap), _bits(g2)), (name, n, gap.tolist(), g2.tolist())
        # a world of the geometry alone: the old entry's outputs
        old = ops.traj_collision_stats(tr, plain.geom, n_interp=n, with_flags=True)
        new = ops.traj_collision_stats(tr, ops.DeviceWorld(plain.geom), n_interp=n, with_flags=True)
        assert all(torch.equal(_bits(a) if a.dtype == torch.float32 else a, _bits(b) if b.dtype == torch.float32 else b) for a, b in zip(old, new))
    # rows with a velocity half are read in place
    wide = torch.cat([t, torch.randn(N, H, D, device=gpu_device, generator=torch.Generator(device=gpu_device).manual_seed(1))], -1).contiguous()
    assert all(torch.equal(a, b) for a, b in zip(ops.traj_collision_stats(wide, task.world), ops.traj_collision_stats(t, task.world)))
    count, first, gap = ops.traj_collision_stats(t, task.world)
    assert int((count > 0).sum()) > 0
    # the trajectory only the grid refuses, and the one only the self part refuses
    geom_only = ops.traj_collision_stats(t, plain.geom)[0]
    no_grid = ops.traj_collision_stats(t, ops.DeviceWorld(plain.geom, self_collision=plain.self_geom))[0]
    no_self = ops.traj_collision_stats(t, ops.DeviceWorld(plain.geom, sdf=plain.sdf_geom))[0]
    assert count[N - 2] > 0 and geom_only[N - 2] == 0 and no_grid[N - 2] == 0 and no_self[N - 2] == count[N - 2]
    if sc.self_field is not None:
        assert count[N - 1] > 0 and geom_only[N - 1] == 0 and no_self[N - 1] == 0 and no_grid[N - 1] == count[N - 1]
    # the four validation calls of the task
    coll, ci, free, fi, way = task.get_trajs_collision_and_free(t, return_indices=True)
    assert torch.equal(ci, torch.nonzero(count > 0).flatten()) and torch.equal(way, ops.traj_collision_stats(t, task.world, with_flags=True)[3])
    assert task.compute_fraction_free_trajs(t) == int((count == 0).sum()) / N
    assert task.compute_success_free_trajs(t) == int(bool((count == 0).any()))
    assert task.compute_collision_intensity_trajs(t) == int(count.sum()) / (N * ((H - 1) * 6 + 1))
    with pytest.raises(NotImplementedError, match='self_field|sdf_field'):
        plain.get_trajs_collision_and_free(t)


# ---- 3. the shortcut pass -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', W.SCENES)
def test_shortcut(gpu_device, name):
    from motion_planning_baselines_amd import ops
    sc, plain, task = _scene(name, gpu_device)
    p = W.shortcut_problem(name)
    dev = gpu_device
    args = (torch.from_numpy(p.paths).to(dev), torch.from_numpy(p.lengths).to(dev))
    kw = dict(draws=torch.from_numpy(p.draws).to(dev), with_log=True)
    paths, lengths, stats, log = (x.cpu().numpy() for x in ops.path_shortcut(*args, task.world, p.n_iters, float(p.step), **kw))

    def judge(b, it, pts):                                   # the kernel's own predicate on the candidate's dense points (same fp32 bits)
        hit = torch.nonzero(ops.world_collision_check(torch.from_numpy(np.ascontiguousarray(pts)).to(dev), task.world)).flatten()
        return int(hit[0]) if len(hit) else -1
    w_paths, w_len, w_log, w_stats = K._walk(p, judge)
    assert np.array_equal(w_log, log), f'{name}: the walk with the world predicate differs at {np.argwhere(w_log != log)[:5].tolist()}'
    assert np.array_equal(w_len, lengths) and np.array_equal(w_paths.view(np.uint32), paths.view(np.uint32))
    assert np.array_equal(w_stats.view(np.uint32), stats.view(np.uint32))
    r64 = K.replay64(p, log)                                 # every decidable decision against the fp64 OR-predicate
    share = K.undecidable_share(r64.cands)
    codes = np.bincount((log & 0xFF).ravel(), minlength=5)
    print(f'{name}: IDLE / SKIP / REJECT / OVERFLOW / ACCEPT {codes.tolist()}, {len(r64.cands)} candidates, undecidable share {share:.4f}')
    assert share <= W.CAP and codes[K.REJECT] > 0 and codes[K.ACCEPT] > 0
    for b, part in enumerate(p.only):                        # a REJECT the grid alone causes, and one the self part alone causes
        assert (log[b, 0] & 0xFF) == K.REJECT and W.why_rejected(sc, p, b, log) == part, (b, part)
    # through the task, and a world of the geometry alone against the old entry
    via = task.shortcut_paths(*args, n_iters=p.n_iters, check_step=float(p.step), **kw)
    assert np.array_equal(via[3].cpu().numpy(), log) and np.array_equal(via[0].cpu().numpy().view(np.uint32), paths.view(np.uint32))
    old = ops.path_shortcut(*args, plain.geom, p.n_iters, float(p.step), **kw)
    new = ops.path_shortcut(*args, ops.DeviceWorld(plain.geom), p.n_iters, float(p.step), **kw)
    assert all(torch.equal(_bits(a) if a.dtype == torch.float32 else a, _bits(b) if b.dtype == torch.float32 else b) for a, b in zip(old, new))
    assert not np.array_equal(old[3].cpu().numpy(), log)     # (the obstacles alone decide otherwise: the other parts are in the kernel)
    with pytest.raises(NotImplementedError, match='self_field|sdf_field'):
        plain.shortcut_paths(*args, n_iters=4, check_step=0.1)


# ---- 4. RRT-Connect -------------------------------------------------------------------------------------------------------------------
def _rrt(scene_geom, r, dev, rows=None, chunk=None, starts=None, goals=None, pool=None, idx=None, total=None, radius=None, Lmax=256):
    from motion_planning_baselines_amd import ops
    rows = np.arange(r.B) if rows is None else np.asarray(rows)
    starts = torch.from_numpy(np.ascontiguousarray(r.starts[rows] if starts is None else starts)).to(dev)
    goals = torch.from_numpy(np.ascontiguousarray(r.goals[rows] if goals is None else goals)).to(dev)
    pool = torch.from_numpy(np.ascontiguousarray(r.pool if pool is None else pool)).to(dev)
    total = r.total if total is None else total
    idx = torch.from_numpy(np.ascontiguousarray(r.idx[rows, :total] if idx is None else idx)).to(dev)
    B, D = starts.shape
    ws = ops.RRTWorkspace(B, total + 1, pool.shape[0], D, dev)
    ops.rrt_connect_init(ws.buf, ws, starts, goals, scene_geom)
    paths = torch.zeros(B, Lmax, D, device=dev)
    lengths = torch.zeros(B, device=dev, dtype=torch.int32)
    status = torch.zeros(B, device=dev, dtype=torch.int32)
    chunk = chunk or total
    for it in range(0, total, chunk):
        ops.rrt_connect_run(ws.buf, ws, scene_geom, pool, idx, paths, lengths, status, it, min(chunk, total - it), total, r.step,
                            r.radius if radius is None else radius)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in ops.rrt_connect_trees(ws).items()}
    out.update(paths=paths.cpu().numpy(), lengths=lengths.cpu().numpy(), status_out=status.cpu().numpy())
    return out


@pytest.mark.parametrize('name', W.SCENES)
def test_rrt_connect(gpu_device, name):
    from motion_planning_baselines_amd import ops
    from test_gpu_rrt_connect import _same_bits
    sc, plain, task = _scene(name, gpu_device)
    r = W.rrt_problem(name)
    a = _rrt(task.world, r, gpu_device)
    found = a['status'] == ops.RRT_FOUND
    print(f'{name}: statuses {a["status"].tolist()}, nodes {a["counts"].sum(1).tolist()}, path nodes {a["lengths"].tolist()}')
    assert (a['status'] != ops.RRT_RUNNING).all() and (a['status'] == a['status_out']).all()
    assert name != 'panda' or found.any()
    # every tree node and the path re-sampled at step_size are free of each part in turn, within 32 E of that part
    E32 = np.max([W.decide(sc, q).E32 for q in W.inputs(name).values()], axis=0)
    parts = W.fields(sc)
    for part, E in zip(parts, E32):
        for b in range(r.B):
            trees = tuple((a['nodes'][b, t, :a['counts'][b, t]], a['parents'][b, t, :a['counts'][b, t]]) for t in (0, 1))
            path = a['paths'][b, :a['lengths'][b]] if found[b] else None
            check_rrt_result(sc.rr64, part, r.starts[b], r.goals[b], trees, path, r.step, r.radius, 32.0 * float(E))
    # a batch equals one problem at a time; chunked launches equal one launch
    for b in range(r.B):
        _same_bits(a, _rrt(task.world, r, gpu_device, rows=[b]), rows_a=[b], rows_b=[0])
    _same_bits(a, _rrt(task.world, r, gpu_device, chunk=64))
    # a world of the geometry alone: the old entries' workspace and paths
    _same_bits(_rrt(plain.geom, r, gpu_device), _rrt(ops.DeviceWorld(plain.geom), r, gpu_device))
    # the planner on the task
    from motion_planning_baselines_amd.planners.rrt_connect import RRTConnect
    planner = RRTConnect(task=task, n_iters=r.total - 1, start_state_pos=torch.from_numpy(r.starts), goal_state_pos=torch.from_numpy(r.goals),
                         step_size=r.step, n_radius=r.radius, tensor_args=task.tensor_args, n_pre_samples=len(r.pool),
                         pre_samples=torch.from_numpy(r.pool), max_path_nodes=256)
    paths, lengths, status = planner.optimize_batched(sample_idx=r.idx)
    assert np.array_equal(status.cpu().numpy(), a['status']) and np.array_equal(paths.cpu().numpy().view(np.uint32), a['paths'].view(np.uint32))


def test_rrt_connect_statuses(gpu_device):
    from motion_planning_baselines_amd import ops
    sc, plain, task = _scene('panda', gpu_device)
    r = W.rrt_problem('panda')
    folded, in_grid = W.only_line('panda', 'self')[2], W.only_line('panda', 'sdf')[2]
    assert not ops.collision_check(torch.from_numpy(np.stack([folded, in_grid])).to(gpu_device), plain.geom).any()
    bad = ops.RRT_START_OR_GOAL_IN_COLLISION
    starts, goals = r.starts.copy(), r.goals.copy()
    starts[1], goals[3] = folded, in_grid                        # a start in self-collision only, a goal inside a grid-only obstacle
    a = _rrt(task.world, r, gpu_device, starts=starts, goals=goals)
    ref = _rrt(task.world, r, gpu_device)
    assert a['status'][1] == bad and a['status'][3] == bad and a['iters'][[1, 3]].tolist() == [0, 0] and a['counts'][[1, 3]].tolist() == [[1, 1]] * 2
    assert (a['status'][[0, 2, 4]] == ref['status'][[0, 2, 4]]).all()
    assert (_rrt(plain.geom, r, gpu_device, starts=starts, goals=goals)['status'][[1, 3]] != bad).all()     # (the obstacles alone let both pass)
    with _changed_sdf_header(task):                              # every problem: that status, nothing read through the changed word
        c = _rrt(task.world, r, gpu_device)
        assert (c['status'] == bad).all() and (c['iters'] == 0).all() and (c['counts'] == 1).all()
    assert np.array_equal(_rrt(task.world, r, gpu_device)['status'], ref['status'])


def test_the_predicate_is_in_the_tree(gpu_device):
    """The grid-only scene: start and goal see each other through a circle that only the grid holds, and every sample is one of the
    two.  A plain task with `field` alone joins them by the straight line, which the world's validation refuses; the tree grown on the
    world never crosses the circle."""
    from motion_planning_baselines_amd import ops
    from motion_planning_baselines_amd.robot_field import PlanningTask
    sc, plain, task = _scene('pm2d', gpu_device)
    qa, qb, _ = W.only_line('pm2d', 'sdf')
    r = W.rrt_problem('pm2d')
    kw = dict(starts=qa[None], goals=qb[None], pool=np.stack([qb, qa]), idx=np.zeros((1, 33), np.int32), total=33, radius=4.0)
    field_alone = PlanningTask(sc.robot, sc.field, tensor_args=plain.tensor_args)
    a = _rrt(field_alone.geom, r, gpu_device, **kw)
    assert a['status'].tolist() == [ops.RRT_FOUND]
    path = torch.from_numpy(a['paths'][:, :a['lengths'][0]]).to(gpu_device).contiguous()
    assert task.compute_fraction_free_trajs(path, num_interpolation=20) == 0.0
    assert field_alone.compute_fraction_free_trajs(path, num_interpolation=20) == 1.0
    b = _rrt(task.world, r, gpu_device, **kw)
    assert b['status'].tolist() != [ops.RRT_FOUND]
    nodes = np.concatenate([b['nodes'][0, t, :b['counts'][0, t]] for t in (0, 1)])
    assert (W.hinges(sc, nodes) <= 1e-5).all()


# ---- 5. the planners --------------------------------------------------------------------------------------------------------------------
def _free_on_dense_points(plain, trajs, D, n=5):
    from motion_planning_baselines_amd import ops
    dense = ops.traj_interpolate(trajs.contiguous(), n)[..., :D].reshape(-1, D).contiguous()
    return not bool(plain._in_collision(dense).any())


def test_planners(gpu_device):
    from motion_planning_baselines_amd import ops
    from motion_planning_baselines_amd.planners.gpmp2 import GPMP2
    from motion_planning_baselines_amd.planners.hybrid_planner import HybridPlanner
    from motion_planning_baselines_amd.planners.multi_sample_based_planner import MultiSampleBasedPlanner
    from motion_planning_baselines_amd.planners.prm import PRM
    from motion_planning_baselines_amd.planners.rrt_connect import RRTConnect
    from motion_planning_baselines_amd.planners.rrt_star import RRTStar
    from motion_planning_baselines_amd.planners.strrt_connect import STRRTConnect
    sc, plain, task = _scene('panda', gpu_device)
    r, ta, D = W.rrt_problem('panda'), task.tensor_args, sc.D
    kw = dict(n_iters=r.total - 1, step_size=r.step, n_radius=r.radius, tensor_args=ta, n_pre_samples=len(r.pool), pre_samples=torch.from_numpy(r.pool),
              max_path_nodes=256, seed=4)
    planner = RRTConnect(task=task, start_state_pos=torch.from_numpy(r.starts), goal_state_pos=torch.from_numpy(r.goals), **kw)
    assert planner.scene is task.world
    paths, lengths, status = planner.optimize_batched()
    found = status == ops.RRT_FOUND
    assert found.any()
    sp, sl, stats = planner.shortcut(paths, lengths, 16)
    assert float(stats[:, 1].sum()) > 0 and ((sl == 0) == (lengths == 0)).all()
    H = 16
    trajs = ops.traj_resample(sp[found].contiguous(), sl[found].contiguous(), H, 0.1)
    coll, free = task.get_trajs_collision_and_free(trajs)
    print(f'RRTConnect on the world: {int(found.sum())} of {r.B} found, {0 if free is None else len(free)} resampled trajectories free')
    assert (0 if free is None else len(free)) + (0 if coll is None else len(coll)) == int(found.sum())
    assert free is None or _free_on_dense_points(plain, free, D)
    assert coll is None or all(not _free_on_dense_points(plain, c[None], D) for c in coll)
    # the found paths themselves, as polylines: what the tree checked at step_size the validation accepts at 2 points per segment
    k0 = int(torch.nonzero(found)[0])
    poly = paths[k0:k0 + 1, :int(lengths[k0])].contiguous()
    c1, f1 = task.get_trajs_collision_and_free(poly, num_interpolation=2)
    assert (f1 is None) == (not _free_on_dense_points(plain, poly, D, n=2))
    # RRT-Connect, shortcut, GPMP2, "which trajectories are free?": the route end to end at 4 particles
    k = int(torch.nonzero(found)[0])
    start, goal = torch.from_numpy(r.starts[k]), torch.from_numpy(r.goals[k])
    multi = MultiSampleBasedPlanner(RRTConnect(task=task, start_state_pos=start, goal_state_pos=goal, **kw), n_trajectories=4)
    gpmp = GPMP2(robot=sc.robot, n_dof=D, n_support_points=H, num_particles_per_goal=4, opt_iters=2, dt=sc.robot.dt, start_state=start.to(gpu_device),
                 multi_goal_states=goal[None].to(gpu_device), sigma_start=1e-3, sigma_gp=1.0, sigma_coll=1e-2, sigma_goal_prior=1e-3, tensor_args=ta,
                 collision_fields=[sc.field], step_size=0.5, solver_params=dict(delta=1e-2, trust_region=True, method='cholesky'),
                 initial_particle_means=torch.zeros(4, H, 2 * D, device=gpu_device))       # (HybridPlanner resets them to the paths)
    hyb = HybridPlanner(multi, gpmp, shortcut_iters=16, tensor_args=ta)
    out = hyb.optimize()
    assert out.shape[-3:] == (4, H, 2 * D) and bool(torch.isfinite(out).all()) and hyb.shortcut_stats.shape == (4, 4)
    coll, free = task.get_trajs_collision_and_free(out.reshape(-1, H, 2 * D))
    print(f'HybridPlanner on the world: {0 if free is None else len(free)} of 4 trajectories free')
    assert free is None or _free_on_dense_points(plain, free, D)
    assert (0 if free is None else len(free)) + (0 if coll is None else len(coll)) == 4
    # what keeps refusing such a task, by the field's name; and the plain task, which refuses everything it did before
    q2 = dict(start_state_pos=start, goal_state_pos=goal, tensor_args=ta)
    for t in (task, plain):
        for make in (lambda: RRTStar(task=t, n_iters=8, n_pre_samples=len(r.pool), pre_samples=torch.from_numpy(r.pool), **q2),
                     lambda: PRM(task=t, n_nodes=64, **q2),
                     lambda: STRRTConnect(task=t, moving_field=None, n_rows=8, n_iters=8, **q2),
                     lambda: t.certify_trajs(trajs),
                     lambda: t.compute_clearance(trajs[0, :, :D])):
            with pytest.raises(NotImplementedError, match='self_field|sdf_field'):
                make()
    with pytest.raises(NotImplementedError, match='self_field|sdf_field'):
        RRTConnect(task=plain, start_state_pos=start, goal_state_pos=goal, **kw)
    with pytest.raises(NotImplementedError, match='world_predicate=True'):
        plain.shortcut_paths(paths, lengths, n_iters=4, check_step=0.1)
