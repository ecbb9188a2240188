"""Space-time shortcutting on the GPU (ops.st_shortcut, csrc/mpb_st_shortcut.hip) against its restatement (st_shortcut_checks.py): bit
for bit following the kernel's own log, every decidable decision against fp64, the output against the existing predicate kernels and
the step bound, the draws and launch variants, the pass-through of refused trajectories, a header changed under the launcher, the
planner's shortcut_iters end to end, and the refusals by name."""
import functools

import numpy as np
import pytest
import torch

import st_shortcut_checks as C
import strrt_checks as S

pytestmark = pytest.mark.gpu
CASES = C.SETS + ('panda_16_8:generic',)


def _task(p, dev):
    from motion_planning_baselines_amd.robot_field import PlanningTask
    return PlanningTask(p.robot, p.fields if len(p.fields) > 1 else p.fields[0], tensor_args=dict(device=dev, dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def _scene(name, dev, generic=False):
    """(task, DeviceMovingObstacles, w) of an input set's scene; generic: the Panda packed without its compile-time model."""
    from motion_planning_baselines_amd import ops
    p = C.scene(name)
    task = _task(p, dev)
    if generic:
        task.geom = ops.DeviceGeometry(p.robot, p.fields if len(p.fields) > 1 else p.fields[0], dev, use_model=False)
    return task, ops.DeviceMovingObstacles(p.robot, p.moving, dev, p.R), torch.from_numpy(p.w).to(dev)


def _arrays(rec, s, draws=None, max_span=0):
    """Host copies of a launch's outputs under the names of st_shortcut_checks.run()."""
    out = dict(trajs=rec.trajs.cpu().numpy(), status=rec.status.cpu().numpy(), first_bad=rec.first_bad.cpu().numpy(), stats=rec.stats.cpu().numpy())
    assert np.array_equal(rec.ok.cpu().numpy(), out['status'] == C.OK)
    if rec.log is not None:
        out['log'] = rec.log.cpu().numpy()
        d = C.device_draws(s.seed, s.N, s.n_iters, s.p.R) if draws is None else draws
        out['rows_written'] = C.rows_written(out['log'], d, s.p.R, max_span)
    return out


@functools.lru_cache(maxsize=None)
def _launch(name, dev, generic=False):
    """The input set through ops.st_shortcut once (device draws of its seed, with the log), shared among the tests.  Read-only."""
    from motion_planning_baselines_amd import ops
    s = C.inputs(name)
    task, mo, w = _scene(name, dev, generic)
    rec = ops.st_shortcut(torch.from_numpy(s.trajs).to(dev), task.geom, mo, w, s.n_iters, seed=s.seed, valid=torch.from_numpy(s.valid).to(dev),
                          with_log=True)
    return rec, _arrays(rec, s)


def _same(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b) if x is not None)


@pytest.mark.parametrize('name', CASES)
def test_kernel_equals_restatement_following_its_log(gpu_device, name):
    """The restatement fed the kernel's collision outcomes reproduces trajectories, status, first_bad and stats bit for bit; every decidable
    logged decision and gate scan equals fp64's; undecidable ones stay under the cap.  The STRRT and path-timing inputs come out OK, the
    trajectories made to be refused with their status and row.  On the gate scenes, whose decisions are far from any surface, the
    kernel also equals the free-running fp32 restatement.  `:generic`: the Panda packed without its compile-time model."""
    name, _, form = name.partition(':')
    s = C.inputs(name)
    rec, got = _launch(name, gpu_device, form == 'generic')
    want, seen = C.follow(s.p, s.trajs, got['log'], got['status'], got['first_bad'], audit=True, seed=s.seed, valid=s.valid)
    share = C.undecidable_share(seen)
    ok = got['status'] == C.OK
    print(f'{name}: N {s.N}, R {s.p.R}, D {s.p.D}, {len(seen)} scans audited, {share:.4f} undecidable, statuses {got["status"].tolist()}, accepted '
          f'{int(got["stats"][ok, 1].sum())} of {int(got["stats"][ok, 0].sum())} checked')
    C.same_bits(got, want, name)
    assert len(seen) > 0 and share <= C.CAP
    for n in range(s.N):
        assert (int(got['status'][n]), int(got['first_bad'][n])) == s.expect.get(n, (C.OK, -1)), (name, n, got['status'][n], got['first_bad'][n])
    C.check_guarantee(s.p, s.trajs, got)
    if name in ('gate', 'parity', 'gate129', 'tiny3'):
        C.same_bits(got, C.restated(name).r32, name + ' free-running')


@pytest.mark.parametrize('name', ('gate', 'gate129', 'panda_16_8', 'pandaslow_130_200', 'arm12', 'ptgate'))
def test_ok_outputs_are_free_by_the_existing_kernels_and_within_the_step_bound(gpu_device, name):
    """Every OK output is accepted by PlanningTask.check_trajs_moving -- mpb_collision_check and mpb_moving_collision_check, kernels this
    pass shares no launch with -- and moves joint k by at most w_k (1 + VEL_SLACK) over every step the pass wrote; the task's own route
    (shortcut_trajs_moving, which forms w from dq_max) gives the same bits."""
    s = C.inputs(name)
    task, mo, w = _scene(name, gpu_device)
    rec, got = _launch(name, gpu_device)
    ok = got['status'] == C.OK
    assert ok.any()
    hit, rows = task.check_trajs_moving(rec.trajs, s.p.moving)
    assert not rows.cpu().numpy()[ok].any(), np.argwhere(rows.cpu().numpy()[ok])
    C.check_guarantee(s.p, s.trajs, got)
    via = task.shortcut_trajs_moving(torch.from_numpy(s.trajs).to(gpu_device), s.p.moving, n_iters=s.n_iters, dq_max=s.p.dq_max,
                                     valid=torch.from_numpy(s.valid).to(gpu_device), seed=s.seed, with_log=True)
    assert _same(via, rec)


def test_draws_and_launch_variants(gpu_device):
    """Recorded draws equal the device draws replayed; two launches of halves with problem_offset equal one launch; in place equals out
    of place; two runs give equal bits; max_span clamps as the restatement does."""
    from motion_planning_baselines_amd import ops
    s = C.inputs('gate')
    task, mo, w = _scene('gate', gpu_device)
    rec, got = _launch('gate', gpu_device)
    tr, valid = torch.from_numpy(s.trajs).to(gpu_device), torch.from_numpy(s.valid).to(gpu_device)
    kw = dict(seed=s.seed, with_log=True)
    again = ops.st_shortcut(tr, task.geom, mo, w, s.n_iters, valid=valid, **kw)
    assert _same(again, rec)
    draws = torch.from_numpy(C.device_draws(s.seed, s.N, s.n_iters, s.p.R)).to(gpu_device)
    assert _same(ops.st_shortcut(tr, task.geom, mo, w, s.n_iters, draws=draws, valid=valid, seed=s.seed + 1, with_log=True), rec)
    wild = draws.clone()                                              # out-of-range recorded rows are clamped into 0 .. R - 1
    wild[draws == 0], wild[draws == s.p.R - 1] = -5, s.p.R + 7
    assert _same(ops.st_shortcut(tr, task.geom, mo, w, s.n_iters, draws=wild, valid=valid, with_log=True), rec)
    h = 7
    lo = ops.st_shortcut(tr[:h].contiguous(), task.geom, mo, w, s.n_iters, valid=valid[:h].contiguous(), **kw)
    hi = ops.st_shortcut(tr[h:].contiguous(), task.geom, mo, w, s.n_iters, valid=valid[h:].contiguous(), problem_offset=h, **kw)
    assert _same([torch.cat((a, b)) for a, b in zip(lo, hi)], rec)
    buf = tr.clone()
    inplace = ops.st_shortcut(buf, task.geom, mo, w, s.n_iters, valid=valid, out=buf, **kw)
    assert inplace.trajs is buf and _same(inplace, rec)
    span = ops.st_shortcut(tr, task.geom, mo, w, s.n_iters, valid=valid, max_span=5, **kw)
    got5 = _arrays(span, s, max_span=5)
    want5, _ = C.follow(s.p, s.trajs, got5['log'], got5['status'], got5['first_bad'], audit=False, seed=s.seed, valid=s.valid, max_span=5)
    C.same_bits(got5, want5, 'max_span 5')
    assert not np.array_equal(got5['log'], got['log'])
    none = ops.st_shortcut(tr, task.geom, mo, w, 0, valid=valid, with_log=True)
    assert torch.equal(none.trajs, tr) and none.log.shape == (s.N, 0) and torch.equal(none.status, rec.status)


def test_refused_trajectories_pass_through(gpu_device):
    """valid = 0, a row in a static wall, a row in the moving sphere at its own time only, a step above w (1 + 2^-15): the input's bits,
    the status and first_bad of each, NaN stats, an idle log -- and the trajectories around them are edited all the same."""
    s = C.inputs('gate')
    rec, got = _launch('gate', gpu_device)
    assert s.expect == {12: (C.INPUT_IN_COLLISION, 16), 13: (C.INPUT_IN_COLLISION, 16), 14: (C.INPUT_TOO_FAST, 1), 15: (C.NOT_VALID, -1)}
    for n, (status, bad) in s.expect.items():
        assert got['status'][n] == status and got['first_bad'][n] == bad
        assert np.array_equal(got['trajs'][n].view(np.uint32), s.trajs[n].view(np.uint32)) and np.isnan(got['stats'][n]).all()
        assert (got['log'][n] == C.IDLE).all()
    assert (got['stats'][:12, 1] > 0).all() and (got['trajs'][:12] != s.trajs[:12]).any(axis=(1, 2)).all()


def test_header_changed_under_the_launcher(gpu_device):
    """The buffer's header word edited through the public buffer, as test_gpu_path_timing.py does, after the launcher has cached the
    shapes of this address: BUFFER_CHANGED, untouched rows, NaN stats, nothing of the buffer read; restored and announced, the pass is
    back to its bits."""
    from motion_planning_baselines_amd import _lib, ops
    from motion_planning_baselines_amd.moving_layout import MOVING_MAGIC
    s = C.inputs('ptgate')
    task, _, w = _scene('ptgate', gpu_device)
    rec, _ = _launch('ptgate', gpu_device)
    tr = torch.from_numpy(s.trajs).to(gpu_device)
    own = ops.DeviceMovingObstacles(s.p.robot, s.p.moving, gpu_device, s.p.R)
    assert _same(ops.st_shortcut(tr, task.geom, own, w, s.n_iters, seed=s.seed, with_log=True), rec)
    words = own.buf.view(torch.int32)
    words[0] = MOVING_MAGIC ^ 1
    bad = ops.st_shortcut(tr, task.geom, own, w, s.n_iters, seed=s.seed, with_log=True)
    assert (bad.status == C.BUFFER_CHANGED).all() and not bad.ok.any() and (bad.first_bad == -1).all()
    assert torch.equal(bad.trajs.view(torch.int32), tr.view(torch.int32)) and torch.isnan(bad.stats).all() and (bad.log == C.IDLE).all()
    words[0] = MOVING_MAGIC
    _lib.check(_lib.lib().mpb_moving_invalidate(ops._ptr(own.buf)), 'mpb_moving_invalidate')
    assert _same(ops.st_shortcut(tr, task.geom, own, w, s.n_iters, seed=s.seed, with_log=True), rec)


def test_planner_shortcut_iters_end_to_end(gpu_device):
    """STRRTConnect(..., shortcut_iters=64) on the gate scene returns plans check_trajs_moving accepts, their summed length below the
    unshortcut plans'; shortcut_iters=0 equals the planner without the argument bit for bit; planner.shortcut(result) is the same pass."""
    from test_gpu_strrt import _planner
    p = S.problem('gate')
    task = _task(p, gpu_device)
    plain = _planner(p, gpu_device, task=task).optimize_batched()
    zero = _planner(p, gpu_device, task=task, shortcut_iters=0).optimize_batched()
    for k in ('trajs', 'found', 'status', 'vertex_q', 'vertex_row', 'n_vertices'):
        assert torch.equal(getattr(plain, k), getattr(zero, k)), k
    assert not hasattr(zero, 'shortcut') and plain.found.all()
    planner = _planner(p, gpu_device, task=task, shortcut_iters=64)
    rec = planner.optimize_batched()
    assert torch.equal(rec.found, plain.found) and torch.equal(rec.raw_trajs, plain.trajs) and rec.shortcut.ok.all()
    hit, rows = task.check_trajs_moving(rec.trajs, p.moving)
    assert not hit.any()
    tr = rec.trajs.cpu().numpy()
    assert np.array_equal(tr[:, 0], p.starts) and np.array_equal(tr[:, -1], p.goals)
    step = np.abs(np.diff(tr.astype(np.float64), axis=1))
    assert (step <= p.w.astype(np.float64) * (1 + S.VEL_SLACK)).all()
    before, after = sum(C.length64(t) for t in plain.trajs.cpu().numpy()), sum(C.length64(t) for t in tr)
    print(f'gate: summed length {before:.3f} -> {after:.3f}, accepted {int(rec.shortcut.stats[:, 1].sum())} of {int(rec.shortcut.stats[:, 0].sum())}')
    assert after < before
    by_hand = planner.shortcut(plain, 64)
    assert torch.equal(by_hand.trajs, rec.trajs) and torch.equal(by_hand.stats, rec.shortcut.stats)


def test_refusals_by_name(gpu_device, monkeypatch):
    from motion_planning_baselines_amd import _lib, geometry as G, ops, st_shortcut_layout as L
    from motion_planning_baselines_amd.robot_field import PlanningTask
    s = C.inputs('gate')
    p = s.p
    task, mo, w = _scene('gate', gpu_device)
    tr = torch.from_numpy(s.trajs).to(gpu_device)
    lib = _lib.lib()

    def raw(trajs, mob, N, R, D, n_iters, max_span=0):
        out, st, fb, stats = torch.empty_like(trajs), torch.empty(N, device=gpu_device, dtype=torch.int32), torch.empty(N, device=gpu_device, dtype=torch.int32), torch.empty(N, 4, device=gpu_device)
        rc = lib.mpb_st_shortcut(ops._ptr(trajs), ops._ptr(out), ops._ptr(task.geom.buf), int(task.geom.flags), ops._ptr(mob.buf), ops._ptr(w), None,
                                 None, ops._ptr(st), ops._ptr(fb), ops._ptr(stats), None, N, R, D, n_iters, max_span, 0, 0, None)
        return rc, lib.mpb_last_error().decode()
    # a buffer packed for another row count: the wrapper and the library both name the two numbers
    other = ops.DeviceMovingObstacles(p.robot, p.moving, gpu_device, p.R + 1)
    with pytest.raises(ValueError, match=f'n_rows = {p.R}.*n_rows = {p.R + 1}'):
        ops.st_shortcut(tr, task.geom, other, w, 4)
    rc, msg = raw(tr, other, s.N, p.R, p.D, 4)
    assert rc != 0 and f'n_rows = {p.R}' in msg and f'n_rows = {p.R + 1}' in msg and 'mpb_st_shortcut' in msg
    # D mismatch: a 3-D robot's buffer
    pm3 = C.scene('pm3d')
    mo3 = ops.DeviceMovingObstacles(pm3.robot, pm3.moving, gpu_device, p.R)
    with pytest.raises(ValueError, match='D = 2.*3 degrees'):
        ops.st_shortcut(tr, task.geom, mo3, w, 4)
    rc, msg = raw(tr, mo3, s.N, p.R, p.D, 4)
    assert rc != 0 and 'D = 2' in msg and 'n_dof = 3' in msg
    # n_iters, max_span, n_rows out of range
    for n_iters in (-1, L.STS_MAX_ITERS + 1):
        with pytest.raises(ValueError, match='n_iters'):
            ops.st_shortcut(tr, task.geom, mo, w, n_iters)
        rc, msg = raw(tr, mo, s.N, p.R, p.D, n_iters)
        assert rc != 0 and 'n_iters' in msg and 'MPB_STS_MAX_ITERS' in msg
    with pytest.raises(ValueError, match='max_span'):
        ops.st_shortcut(tr, task.geom, mo, w, 4, max_span=-1)
    assert raw(tr, mo, s.N, p.R, p.D, 4, max_span=-1)[0] != 0
    with pytest.raises(ValueError, match='n_rows = 2'):
        ops.st_shortcut(tr[:, :2].contiguous(), task.geom, ops.DeviceMovingObstacles(p.robot, p.moving, gpu_device, 2), w, 4)
    rc, msg = raw(tr, mo, s.N, 2, p.D, 4)
    assert rc != 0 and 'MPB_STS_MIN_ROWS' in msg
    rc, msg = raw(tr, mo, s.N, 1025, p.D, 4)
    assert rc != 0 and 'MPB_STS_MAX_ROWS' in msg
    with pytest.raises(ValueError, match='draws'):
        ops.st_shortcut(tr, task.geom, mo, w, 4, draws=torch.zeros(s.N, 4, 2, device=gpu_device))
    with pytest.raises(ValueError, match='valid'):
        ops.st_shortcut(tr, task.geom, mo, w, 4, valid=torch.ones(s.N, device=gpu_device))
    # the LDS need above the limit, by name (every served shape fits the 160 KB of a workgroup: the limit is lowered for the call)
    monkeypatch.setattr(L, 'STS_MAX_LDS_BYTES', L.lds_bytes(p.R, p.D) - 1)
    with pytest.raises(ValueError, match='STS_MAX_LDS_BYTES'):
        ops.st_shortcut(tr, task.geom, mo, w, 4)
    monkeypatch.undo()
    # self_field / sdf_field: refused by name, as STRRTConnect refuses them
    panda = C.scene('panda_16_8')
    ta = dict(device=gpu_device, dtype=torch.float32)
    ptr = torch.from_numpy(C.inputs('panda_16_8').trajs).to(gpu_device)
    with pytest.raises(NotImplementedError, match='self_field'):
        PlanningTask(panda.robot, panda.fields[0], self_field=G.SelfCollisionField(panda.robot), tensor_args=ta).shortcut_trajs_moving(ptr, panda.moving)
    sdf = G.GridSDFField.from_field(panda.fields[0], lo=(-1, -1, -1), hi=(1, 1, 1), cell=0.1)
    with pytest.raises(NotImplementedError, match='sdf_field'):
        PlanningTask(panda.robot, panda.fields[0], sdf_field=sdf, tensor_args=ta).shortcut_trajs_moving(ptr, panda.moving)
    with pytest.raises(TypeError, match='MovingObstacleField'):
        task.shortcut_trajs_moving(tr, p.fields[0])
    with pytest.raises(ValueError, match='shortcut_iters'):
        from test_gpu_strrt import _planner
        _planner(S.problem('gate'), gpu_device, task=task, shortcut_iters=-1)
