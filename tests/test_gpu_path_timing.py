"""Path timing among moving obstacles on the GPU (ops.path_time_plan, PlanningTask.time_paths_moving, csrc/mpb_path_timing.hip) against
its restatement (path_timing_checks.py): the free table against the existing moving-obstacle predicate kernel on every decidable cell,
the recurrence bit for bit over the kernel's own table, a gate scene with a known answer, the output against check_trajs_moving and
the velocity bound, each status once, tasks with a self_field / an sdf_field, determinism and the refusals by name."""
import numpy as np
import pytest
import torch

import path_timing_checks as T

pytestmark = pytest.mark.gpu


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope='module')
def runs(gpu_device):
    """name -> (scene, DeviceMovingObstacles, PathTiming with the table, host copies): one launch per scene, shared and left unchanged."""
    from motion_planning_baselines_amd import ops
    cache = {}

    def get(name):
        if name not in cache:
            s = T.scene(name)
            mo = ops.DeviceMovingObstacles(s.robot, s.moving, gpu_device, s.R)
            rec = ops.path_time_plan(_dev(s.P, gpu_device), mo, _dev(s.w, gpu_device), blocked=_dev(s.blocked, gpu_device), with_table=True)
            cache[name] = (s, mo, rec, {k: getattr(rec, k).cpu().numpy() for k in rec._fields})
        return cache[name]
    return get


def _static_field(s):
    """A static scene far from every path: the tasks of these tests are about the moving field."""
    from motion_planning_baselines_amd import geometry as G
    if s.D == 2:
        return G.CollisionField(boxes=np.array([[5.0, 5.0, 0.05, 0.05]], np.float32), margin=0.02)
    return G.CollisionField(spheres=np.array([[5.0, 5.0, 5.0, 0.05]], np.float32), margin=0.02)


def _task(s, dev, **kw):
    from motion_planning_baselines_amd.robot_field import PlanningTask
    return PlanningTask(s.robot, kw.pop('field', None) or _static_field(s), tensor_args=dict(device=dev, dtype=torch.float32), **kw)


@pytest.mark.parametrize('name', T.SHAPES + ('gate',))
def test_free_table_equals_the_existing_predicate_on_decidable_cells(gpu_device, runs, name):
    """free_table[n, j, i] == !(mpb_moving_collision_check of the trajectory that stands on P[n, i] at every row)[j] && !blocked[n, i]
    wherever fp64 decides the cell; the undecidable ones are counted and stay under the cap."""
    from motion_planning_baselines_amd import ops
    s, mo, rec, got = runs(name)
    ref = T.reference(name)
    tiled = _dev(s.P, gpu_device).reshape(s.N * s.S, 1, s.D).expand(-1, s.R, -1).contiguous()
    hit = ops.moving_collision_check(tiled, mo).cpu().numpy().reshape(s.N, s.S, s.R).transpose(0, 2, 1)
    want = ~hit if s.blocked is None else ~hit & ~s.blocked[:, None, :]
    und = np.stack(ref.undecidable)
    differ = got['free_table'] != want
    vs64 = got['free_table'] != np.stack(ref.F)
    print(f'{name}: {und.sum()} of {und.size} cells undecidable, {int(differ.sum())} differ from the existing kernel ({int((differ & ~und).sum())} decidable), '
          f'{int(vs64.sum())} from fp64 ({int((vs64 & ~und).sum())} decidable), free share {got["free_table"].mean():.3f}')
    assert und.mean() <= T.CAP
    assert not (differ & ~und).any(), np.argwhere(differ & ~und)[:5]
    if s.blocked is not None:
        assert not got['free_table'][np.broadcast_to(s.blocked[:, None, :], differ.shape)].any()


@pytest.mark.parametrize('name', T.ALL)
def test_recurrence_equals_the_restatement_over_the_kernels_own_table(runs, name):
    """status, arrival_row, idx and trajs equal the numpy restatement of items 1 - 9 over the kernel's own free table, bit for bit; a
    scene named for a status has it."""
    s, mo, rec, got = runs(name)
    assert np.array_equal(got['found'], got['status'] == T.FOUND)
    for n in range(s.N):
        want = T.restate(s.P[n], s.w, got['free_table'][n])
        assert got['status'][n] == want.status, (name, n, got['status'][n], want.status)
        assert got['arrival_row'][n] == want.arrival, (name, n, got['arrival_row'][n], want.arrival)
        assert np.array_equal(got['idx'][n], want.idx), (name, n, np.argwhere(got['idx'][n] != want.idx)[:5].tolist())
        assert np.array_equal(got['trajs'][n].view(np.uint32), want.traj.view(np.uint32)), (name, n)
    print(f'{name}: statuses {got["status"].tolist()}, arrivals {got["arrival_row"].tolist()}')
    if name in T.STATUS_SCENES:
        assert got['status'][0] == T.STATUS_SCENES[name]
    if name in T.SHAPES:
        assert got['found'].any()
        # the scenes' cells are decidable: the kernel's answer is the fp64 reference's
        ref = T.reference(name)
        if not any(u.any() for u in ref.undecidable):
            assert [t.status for t in ref.timing] == got['status'].tolist() and [t.arrival for t in ref.timing] == got['arrival_row'].tolist()


def test_gate_scene_waits_and_arrives_when_the_restatement_says(runs):
    s, _, _, got = runs('gate')
    _, _, _, away = runs('gate_away')
    ref = T.reference('gate').timing[0]
    assert got['status'][0] == T.FOUND and away['status'][0] == T.FOUND
    idx = got['idx'][0]
    assert got['arrival_row'][0] == ref.arrival == 40 and away['arrival_row'][0] == s.S - 1 < got['arrival_row'][0]
    assert np.array_equal(idx, ref.idx)
    assert (idx[12:21] == 12).all(), idx.tolist()                        # it waits at the gate's edge while the sphere sits in it
    assert (np.diff(idx) >= 0).all() and idx[0] == 0 and (idx[40:] == s.S - 1).all()
    tr = got['trajs'][0]
    assert np.array_equal(tr[0].view(np.uint32), s.P[0, 0].view(np.uint32)) and np.array_equal(tr[-1].view(np.uint32), s.P[0, -1].view(np.uint32))


@pytest.mark.parametrize('name', ('gate', 'pm2_256_1024', 'pm3_33_65', 'panda_65_129', 'panda_256_64', 'arm12_32_64'))
def test_found_trajectories_are_accepted_and_within_the_velocity_bound(gpu_device, runs, name):
    """Every FOUND trajectory is free at every row by task.check_trajs_moving (the existing predicate kernels); every row step moves joint
    k by at most w_k (1 + VEL_SLACK), the STRRT test's slack."""
    s, _, rec, got = runs(name)
    found = got['found']
    assert found.any()
    task = _task(s, gpu_device)
    hit, rows = task.check_trajs_moving(rec.trajs, s.moving)
    rows = rows.cpu().numpy()
    for n in np.nonzero(found)[0]:
        assert not rows[n].any(), (name, n, np.nonzero(rows[n])[0])
        step = np.abs(np.diff(got['trajs'][n].astype(np.float64), axis=0))
        assert (step <= s.w.astype(np.float64) * (1 + T.VEL_SLACK)).all(), (name, n, (step / s.w).max())
        assert (np.diff(got['idx'][n]) >= 0).all()
    print(f'{name}: {int(found.sum())} of {s.N} found, rows refused by check_trajs_moving {int(rows[found].sum())}')
    assert not got['trajs'][~found].any() and (got['idx'][~found] == -1).all() and (got['arrival_row'][~found] == -1).all()


@pytest.mark.parametrize('kind', ('self_field', 'sdf_field'))
def test_tasks_with_a_self_field_or_an_sdf_field_are_served(gpu_device, kind):
    """time_paths_moving runs on a task every other sample-based stage refuses; a sample the task's static predicate refuses is never
    stood on, and the record equals ops.path_time_plan with that predicate as the blocked mask."""
    from motion_planning_baselines_amd import geometry as G, ops
    s = T.scene('panda_65_129')
    field = G.env_spheres_3d(seed=4, n_spheres=5)
    if kind == 'self_field':
        task = _task(s, gpu_device, field=field, self_field=G.SelfCollisionField(s.robot))
    else:
        task = _task(s, gpu_device, field=field, sdf_field=G.GridSDFField.from_field(field, lo=(-1, -1, -1), hi=(1, 1, 1), cell=0.1))
    rng = np.random.RandomState(2)
    P = T._random_paths(s.robot, rng, 8, 33, 0.9, 0.0)
    dq_max = T.make_scene('x', s.robot, s.moving, s.R, T._w_for(P, 3.5), P).dq_max
    rec = task.time_paths_moving(P, s.moving, s.R, dq_max=dq_max)
    blocked = task._in_collision(_dev(P, gpu_device).reshape(-1, s.D)).reshape(8, 33)
    assert blocked.any() and not blocked.all()
    found, idx = rec.found.cpu().numpy(), rec.idx.cpu().numpy()
    b = blocked.cpu().numpy()
    for n in np.nonzero(found)[0]:
        assert not b[n, idx[n]].any()
    st = rec.status.cpu().numpy()
    assert (st[b[:, 0]] == T.START_BLOCKED).all() and (st[~b[:, 0] & b[:, -1]] == T.GOAL_NOT_HOLDABLE).all()
    dt_row = (s.moving.t_end - s.moving.t_start) / (s.R - 1)
    w = torch.from_numpy((dq_max * dt_row).astype(np.float32)).to(gpu_device)
    direct = ops.path_time_plan(_dev(P, gpu_device), task._moving_geom(s.moving, s.R), w, blocked=blocked)
    assert torch.equal(direct.status, rec.status) and torch.equal(direct.idx, rec.idx) and torch.equal(direct.trajs, rec.trajs)
    print(f'{kind}: {int(b.sum())} of {b.size} samples blocked, statuses {st.tolist()}')
    # polylines + lengths: resampled to n_samples first
    lengths = torch.tensor([33, 20, 2, 33, 9, 33, 33, 5], dtype=torch.int32, device=gpu_device)
    rs = task.time_paths_moving(P, s.moving, s.R, lengths=lengths, n_samples=40, dq_max=dq_max)
    assert tuple(rs.trajs.shape) == (8, s.R, s.D) and tuple(rs.idx.shape) == (8, s.R) and int(rs.idx.max()) <= 39


def test_two_runs_give_the_same_bits_and_a_changed_buffer_is_refused(gpu_device, runs):
    from motion_planning_baselines_amd import _lib, ops
    from motion_planning_baselines_amd.moving_layout import MOVING_MAGIC
    s, mo, rec, _ = runs('panda_65_129')
    again = ops.path_time_plan(_dev(s.P, gpu_device), mo, _dev(s.w, gpu_device), blocked=_dev(s.blocked, gpu_device), with_table=True)
    for k in rec._fields:
        assert torch.equal(getattr(rec, k), getattr(again, k)), k
    lean = ops.path_time_plan(_dev(s.P, gpu_device), mo, _dev(s.w, gpu_device))
    assert lean.free_table is None and torch.equal(lean.trajs, rec.trajs) and torch.equal(lean.status, rec.status)
    # the header changes under the launcher (which has the shapes of this address cached): nothing of the buffer is trusted
    own = ops.DeviceMovingObstacles(s.robot, s.moving, gpu_device, s.R)
    ops.path_time_plan(_dev(s.P, gpu_device), own, _dev(s.w, gpu_device))
    words = own.buf.view(torch.int32)
    words[0] = MOVING_MAGIC ^ 1
    bad = ops.path_time_plan(_dev(s.P, gpu_device), own, _dev(s.w, gpu_device), with_table=True)
    assert (bad.status == T.BUFFER_CHANGED).all() and not bad.free_table.any() and not bad.trajs.any() and not bad.found.any()
    words[0] = MOVING_MAGIC
    _lib.check(_lib.lib().mpb_moving_invalidate(ops._ptr(own.buf)), 'mpb_moving_invalidate')
    good = ops.path_time_plan(_dev(s.P, gpu_device), own, _dev(s.w, gpu_device))
    assert torch.equal(good.trajs, rec.trajs)


def test_refusals_by_name(gpu_device):
    from motion_planning_baselines_amd import _lib, geometry as G, ops, path_timing_layout as L
    s = T.scene('gate')
    mo = ops.DeviceMovingObstacles(s.robot, s.moving, gpu_device, s.R)
    P, w = _dev(s.P, gpu_device), _dev(s.w, gpu_device)
    for S in (1, 257):
        with pytest.raises(ValueError, match='n_samples'):
            ops.path_time_plan(torch.zeros(1, S, 2, device=gpu_device), mo, w)
    with pytest.raises(ValueError, match='n_rows'):
        ops.path_time_plan(P, ops.DeviceMovingObstacles(s.robot, s.moving, gpu_device, 1), w)
    with pytest.raises(Exception, match='n_rows|MOVING_MAX_ROWS'):
        ops.path_time_plan(P, ops.DeviceMovingObstacles(s.robot, s.moving, gpu_device, 1025), w)
    with pytest.raises(ValueError, match='float32'):
        ops.path_time_plan(P.double(), mo, w)
    with pytest.raises(ValueError, match='blocked must be bool or uint8'):
        ops.path_time_plan(P, mo, w, blocked=torch.zeros(1, s.S, device=gpu_device))
    with pytest.raises(ValueError, match='D = 3'):
        ops.path_time_plan(torch.zeros(1, s.S, 3, device=gpu_device), mo, w)
    with pytest.raises(TypeError, match='DeviceMovingObstacles'):
        ops.path_time_plan(P, None, w)
    # the LDS need: 49 collision spheres x 256 samples do not fit a workgroup; the wrapper and the library both say so by name
    big = T.scene('arm12_32_64')
    wide = _wide_robot(big.robot)
    mow = ops.DeviceMovingObstacles(wide, big.moving, gpu_device, 1024)
    assert L.lds_bytes(mow.n_links, 256, 1024) > L.PT_MAX_LDS_BYTES
    Pw, ww = torch.zeros(1, 256, 12, device=gpu_device), torch.ones(12, device=gpu_device)
    with pytest.raises(ValueError, match='PT_MAX_LDS_BYTES'):
        ops.path_time_plan(Pw, mow, ww)
    out = torch.zeros(1, 1024, 12, device=gpu_device)
    status = torch.zeros(1, dtype=torch.int32, device=gpu_device)
    rc = _lib.lib().mpb_path_time_plan(ops._ptr(Pw), ops._ptr(mow.buf), ops._ptr(ww), None, ops._ptr(out), None, None, ops._ptr(status), None,
                                       1, 256, 12, 1024, None)
    assert rc == 2 and 'MPB_PT_MAX_LDS_BYTES' in _lib.lib().mpb_last_error().decode()
    rc = _lib.lib().mpb_path_time_plan(ops._ptr(Pw), ops._ptr(mow.buf), ops._ptr(ww), None, ops._ptr(out), None, None, ops._ptr(status), None,
                                       1, 256, 12, 512, None)
    assert rc == 1 and 'n_rows = 512' in _lib.lib().mpb_last_error().decode() and 'n_rows = 1024' in _lib.lib().mpb_last_error().decode()
    # the task's wrapper
    task = _task(s, gpu_device)
    with pytest.raises(TypeError, match='MovingObstacleField'):
        task.time_paths_moving(s.P, _static_field(s), s.R)
    frozen = G.MovingObstacleField([0.0, 1.0], sphere_centers=np.zeros((2, 1, 2)), sphere_radii=[0.1], margin=0.02, t_start=0.5, t_end=0.5)
    with pytest.raises(ValueError, match='t_end'):
        task.time_paths_moving(s.P, frozen, s.R)
    with pytest.raises(ValueError, match='expected \\(N, S, D\\)'):
        task.time_paths_moving(np.zeros((1, s.S, 3), np.float32), s.moving, s.R)
    with pytest.raises(ValueError, match='dq_max'):
        task.time_paths_moving(s.P, s.moving, s.R, dq_max=[1.0])


def _wide_robot(robot):
    """The chain with every collision sphere twice: enough spheres that 256 samples exceed a workgroup's LDS."""
    from motion_planning_baselines_amd import geometry as G
    rs = robot.spec()
    frames = np.repeat(np.asarray(rs['link_frame']), 2)
    return G.RobotSerialChain(np.asarray(rs['joint_tf']), list(frames), np.repeat(np.asarray(rs['link_offset']), 2, axis=0),
                              list(np.repeat(np.asarray(rs['link_radius']), 2)), q_min=robot.q_min_np, q_max=robot.q_max_np)
