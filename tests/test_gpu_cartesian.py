"""GPU: Cartesian end-effector moves (csrc/mpb_cartesian.hip) against the fp64 restatement of tests/cartesian_checks.py.
Every bar is collision_kinks.bar(E32) = 4 x max(E32, 2^-23) with E32 the fp32 restatement's own distance from fp64 on the same inputs.
Whether a step is accepted is a threshold: the element-wise comparison holds the problems whose n_ok is the fp64 restatement's (at most
CAP = 2 % may differ, tests/test_cartesian_cpu.py asserts as much of the fp32 restatement), the full run holds what an accepted path must
satisfy, in fp64 from the kernel's output alone."""
import functools

import numpy as np
import pytest
import torch

import cartesian_checks as C

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _geom(name, dev):
    from motion_planning_baselines_amd import geometry as G, ops
    return ops.DeviceGeometry(C.robot_of(name), G.env_spheres_3d(), torch.device(dev))


def _run(inp, dev, K, n_inner, jump_max=C.JUMP_MAX, tol=(C.POS_TOL, C.ROT_TOL), starts=None, goal=None, limits=True):
    from motion_planning_baselines_amd import ops
    f = lambda t: t.to(dev).contiguous()
    out = ops.cartesian_path(f(inp.goal if goal is None else goal), f(inp.starts if starts is None else starts), _geom(inp.name, str(dev)), K,
                             n_inner=n_inner, damping=C.DAMPING, pos_tol=tol[0], rot_tol=tol[1], jump_max=jump_max,
                             position_only=inp.position_only, q_min=f(inp.robot.q_min) if limits else None,
                             q_max=f(inp.robot.q_max) if limits else None)
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


@functools.lru_cache(maxsize=None)
def _full(name, dev):
    """The full run of a set on the device, shared by the tests that read it."""
    return _run(C.inputs(name), torch.device(dev), *C.FULL)


def _agreeing(n_ok, ref, what):
    same = n_ok == ref.r64.n_ok
    differ = float((~same).float().mean())
    print(f'{what}: n_ok differs from fp64 on {int((~same).sum())} of {same.numel()} problems')
    assert differ <= C.CAP
    return same


@pytest.mark.parametrize('name', C.SETS)
def test_elements_against_fp64(gpu_device, name):
    inp = C.inputs(name)
    ref = C.reference(name, *C.ELEMENT, C.JUMP_MAX, C.ELEMENT_TOL)
    q, pe, th, n_ok, status = _run(inp, gpu_device, *C.ELEMENT, tol=C.ELEMENT_TOL)
    assert q.shape == (C.N_TARGETS, C.N_STARTS, 3, inp.robot.q_dim) and pe.shape == th.shape == (C.N_TARGETS, C.N_STARTS, 3)
    assert n_ok.dtype == status.dtype == torch.int32
    assert torch.equal(q[:, :, 0], inp.starts)                            # row 0: q_start's bits
    same = _agreeing(n_ok, ref, name)
    assert torch.equal(status[same], ref.r64.status[same])
    for got, want, E, unit in ((q, ref.r64.q, ref.E32_q, 'rad'), (pe, ref.r64.pos_err, ref.E32_pos, 'm'), (th, ref.r64.rot_err, ref.E32_rot, 'rad')):
        err = float((got.double() - want)[same].abs().max())
        print(f'{name}: error {err:.2e} {unit} (fp32 restatement {E:.2e}), n_ok {torch.bincount(n_ok.flatten(), minlength=3).tolist()}')
        assert err <= C.bar(E)
    assert not bool(pe[:, :, 0].any()) and not bool(th[:, :, 0].any())


@pytest.mark.parametrize('name', C.SETS)
def test_an_accepted_path_is_a_path(gpu_device, name):
    inp, ref = C.inputs(name), C.reference(name, *C.FULL)
    K = C.FULL[0]
    q, pe, th, n_ok, status = _full(name, str(gpu_device))
    N, S, rows, D = q.shape
    tf64 = C.chain(inp.robot, torch.float64)[0]
    pe64, th64, off = (t.reshape(N, S, rows) for t in C.path_errors(tf64, inp.goal.repeat_interleave(S, 0), inp.starts.reshape(-1, D),
                                                                    q.reshape(-1, rows, D), inp.position_only))
    r = torch.arange(rows)[None, None, :]
    acc = r <= n_ok[:, :, None]
    print(f'{name}: accepted rows: fp64 position error at most {float(pe64[acc].max()):.3e} m, rotation error {float(th64[acc].max()):.3e} rad; '
          f'evaluation error of the fp32 restatement {ref.E32_pos_eval:.2e} m, {ref.E32_rot_eval:.2e} rad')
    assert float(pe64[acc].max()) <= C.POS_TOL + C.bar(ref.E32_pos_eval)
    assert float(th64[acc].max()) <= C.ROT_TOL + C.bar(ref.E32_rot_eval)
    step = (q[:, :, 1:] - q[:, :, :-1]).abs().amax(-1)
    assert float(step.max()) <= C.JUMP_MAX
    assert bool(((q >= inp.robot.q_min) & (q <= inp.robot.q_max)).all())
    held = torch.gather(q, 2, n_ok.long()[:, :, None, None].expand(N, S, 1, D))
    assert bool((torch.eq(q, held) | acc[..., None]).all())               # rows beyond n_ok: row n_ok, bit for bit
    assert not bool(pe[r > n_ok[:, :, None] + 1].any()) and not bool(th[r > n_ok[:, :, None] + 1].any())
    assert torch.equal(status == C.OK, n_ok == K) and bool(((status == C.OK) | (status == C.LOST) | (status == C.JUMP) | (status == C.BAD_TARGET)).all())
    share, share64 = float((status == C.OK).float().mean()), float((ref.r64.status == C.OK).float().mean())
    print(f'{name}: complete {share:.3f} (fp64 restatement {share64:.3f})')
    assert share >= share64 - 0.03
    done = status == C.OK
    assert float(off[done].max()) <= C.POS_TOL + C.bar(ref.E32_pos_eval)  # the hand of a complete move stays on the segment
    # and where n_ok agrees, the rows are the fp64 restatement's
    same = _agreeing(n_ok, ref, name)
    err = float((q.double() - ref.r64.q)[same].abs().max())
    print(f'{name}: rows against fp64 {err:.2e} rad (fp32 restatement {ref.E32_q:.2e})')
    assert torch.equal(status[same], ref.r64.status[same])


@pytest.mark.parametrize('name', C.SETS)
def test_jumps_where_the_restatement_jumps(gpu_device, name):
    ref = C.reference(name, *C.FULL, C.JUMP_TIGHT)
    q, pe, th, n_ok, status = _run(C.inputs(name), gpu_device, *C.FULL, jump_max=C.JUMP_TIGHT)
    same = _agreeing(n_ok, ref, name)
    assert torch.equal(status[same], ref.r64.status[same]) and int((status == C.JUMP).sum()) >= 0.1 * status.numel()
    assert float((q[:, :, 1:] - q[:, :, :-1]).abs().max()) <= C.JUMP_TIGHT
    # the rejected step's errors are within the tolerances: it was the jump that stopped it
    jumped = status == C.JUMP
    rej = (n_ok.long() + 1).clamp_max(C.FULL[0])[:, :, None]
    assert float(torch.gather(pe, 2, rej)[..., 0][jumped].max()) <= C.POS_TOL and float(torch.gather(th, 2, rej)[..., 0][jumped].max()) <= C.ROT_TOL


def test_bad_targets(gpu_device):
    inp, ref = C.bad_inputs(), C.reference('bad', *C.FULL)
    q, pe, th, n_ok, status = _run(inp, gpu_device, *C.FULL)
    assert torch.equal(status, ref.r64.status) and bool((status == C.BAD_TARGET).all()) and not bool(n_ok.any())
    assert torch.equal(q, inp.starts[:, :, None, :].expand_as(q)) and not bool(pe.any()) and not bool(th.any())
    # position only ignores the rotation altogether: the same problems are tracked
    po = C.types.SimpleNamespace(name='panda', robot=inp.robot, position_only=True, starts=inp.starts, goal=inp.goal)
    assert not bool((_run(po, gpu_device, *C.FULL)[4] == C.BAD_TARGET).any())


def test_no_inner_iterations(gpu_device):
    """n_inner = 0 steps nowhere: a step is accepted only when its target is already within tolerance of the held pose."""
    from motion_planning_baselines_amd import ops
    inp = C.inputs('panda')
    starts = inp.starts[:5, :1]
    pose = ops.fk_ee_pose(starts[:, 0].to(gpu_device).contiguous(), _geom('panda', str(gpu_device))).cpu()
    q, pe, th, n_ok, status = _run(inp, gpu_device, 1, 0, starts=starts, goal=pose)
    assert bool((status == C.OK).all()) and bool((n_ok == 1).all())
    assert torch.equal(q, starts[:, :, None, :].expand_as(q))
    assert float(pe.max()) <= C.POS_TOL and float(th.max()) <= C.ROT_TOL
    far = pose.clone()
    far[0, :, 3] += torch.tensor([0.2, 0.0, 0.0])
    q, pe, th, n_ok, status = _run(inp, gpu_device, 1, 0, starts=starts, goal=far)
    assert status[:, 0].tolist() == [C.LOST] + [C.OK] * 4 and n_ok[:, 0].tolist() == [0, 1, 1, 1, 1]
    assert torch.equal(q, starts[:, :, None, :].expand_as(q)) and abs(float(pe[0, 0, 1]) - 0.2) < 1e-5
    # with the full run's steps and no iterations nothing moves either
    q, pe, th, n_ok, status = _run(inp, gpu_device, C.FULL[0], 0)
    assert torch.equal(q, inp.starts[:, :, None, :].expand_as(q)) and bool((status[n_ok < C.FULL[0]] == C.LOST).all())


def test_one_step_position_only_is_ik_solves_iteration(gpu_device):
    """K = 1, position only: the step target is t* itself ((1 - 1) t_0 + 1 t*), so an accepted row 1 is mpb_ik_solve's result after the
    same number of iterations, bit for bit -- the iteration written out in ik_solve_kernel and the functions of mpb_ee.h are one."""
    from motion_planning_baselines_amd import ops
    for name in ('panda_pos', 'arm4_pos'):
        inp = C.inputs(name)
        dev = gpu_device
        f = lambda t: t.to(dev).contiguous()
        q, pe, th, n_ok, status = _run(inp, dev, 1, 6, jump_max=float('inf'))
        qi, pei, _, conv, _ = ops.ik_solve(f(inp.goal), f(inp.starts), _geom(name, str(dev)), q_min=f(inp.robot.q_min), q_max=f(inp.robot.q_max),
                                           n_iters=6, damping=C.DAMPING, pos_tol=C.POS_TOL, rot_tol=C.ROT_TOL, position_only=True)
        assert torch.equal(conv.cpu(), status == C.OK) and int(conv.sum()) > 0
        ok = status == C.OK
        assert torch.equal(q[:, :, 1][ok], qi.cpu()[ok]) and torch.equal(pe[:, :, 1], pei.cpu())


def test_layout_independence_and_determinism(gpu_device):
    """A problem solved alone, in the batch of 111, and in a batch of 64 + 1 gives the same bits; two runs give the same bits."""
    inp = C.inputs('panda')
    big = _full('panda', str(gpu_device))
    again = _run(inp, gpu_device, *C.FULL)
    for a, b in zip(big, again):
        assert torch.equal(a, b)
    flat_s, flat_g = inp.starts.reshape(-1, 1, 7), inp.goal.repeat_interleave(C.N_STARTS, 0)
    pick = torch.arange(65) + 40                                          # 64 + 1 problems, one target each
    part = _run(inp, gpu_device, *C.FULL, starts=flat_s[pick], goal=flat_g[pick])
    for n in (0, 64, 110):                                                # (lane 0 of a wave, the first lane of the second, the last)
        alone = _run(inp, gpu_device, *C.FULL, starts=flat_s[n:n + 1], goal=flat_g[n:n + 1])
        for a, b in zip(alone, big):
            assert torch.equal(a[0, 0], b.reshape(-1, *b.shape[2:])[n])
    for a, b in zip(part, big):
        assert torch.equal(a[:, 0], b.reshape(-1, *b.shape[2:])[pick])
    assert len(set(big[4].flatten().tolist())) >= 2


def test_an_address_that_got_another_chain_is_read_again(gpu_device):
    """ONE allocation holds the Panda's geometry (7 joints), then the 12-joint arm's: each call succeeds with the bits of the call on a
    buffer of the robot's own, and a call with the first D afterwards is refused by what the buffer holds now."""
    from motion_planning_baselines_amd import _lib, ops
    h, p = _lib.lib(), ops._ptr
    sets = [C.inputs(name) for name in ('panda', 'arm12')]
    geoms = [_geom(s.name, str(gpu_device)) for s in sets]
    shared = torch.zeros(max(g.host.size for g in geoms), device=gpu_device)
    K, n_inner = 4, 2

    def path(inp):
        N, S, D = inp.starts.shape
        goal, q0 = inp.goal.to(gpu_device).contiguous(), inp.starts.to(gpu_device).contiguous()
        out = [torch.empty(N, S, K + 1, D, device=gpu_device), torch.empty(N, S, K + 1, device=gpu_device), torch.empty(N, S, K + 1, device=gpu_device),
               torch.empty(N, S, device=gpu_device, dtype=torch.int32), torch.empty(N, S, device=gpu_device, dtype=torch.int32)]
        with torch.cuda.device(gpu_device):
            rc = h.mpb_cartesian_path(p(goal), p(q0), p(shared), None, None, *[p(t) for t in out], N, S, D, K, n_inner, C.DAMPING, C.POS_TOL,
                                      C.ROT_TOL, C.JUMP_MAX, 0, ops._stream())
        torch.cuda.synchronize()
        return rc, [t.cpu() for t in out]
    for inp, g in zip(sets, geoms):
        shared[:g.host.size].copy_(torch.from_numpy(g.host))
        torch.cuda.synchronize()
        rc, out = path(inp)
        assert rc == 0, h.mpb_last_error().decode()
        own = _run(types_of(inp, False), gpu_device, K, n_inner, limits=False)
        for a, b in zip(out, own):
            assert torch.equal(a, b)
    rc, _ = path(sets[0])
    assert rc == 1 and 'the chain has 12 joints' in h.mpb_last_error().decode()


def types_of(inp, position_only):
    return C.types.SimpleNamespace(name=inp.name, robot=inp.robot, position_only=position_only, starts=inp.starts, goal=inp.goal)


def test_a_point_robot_and_another_width_are_refused(gpu_device):
    from motion_planning_baselines_amd import _lib, geometry as G, ops
    geom = ops.DeviceGeometry(G.RobotPointMass(3, radius=0.05), G.env_spheres_3d(), gpu_device)
    q = torch.zeros(4, 1, 3, device=gpu_device)
    goal = torch.zeros(4, 3, 4, device=gpu_device)
    with pytest.raises(ValueError, match='point robot'):
        ops.cartesian_path(goal, q, geom, 4)
    with pytest.raises(ValueError, match='degrees of freedom'):
        ops.cartesian_path(goal, q, _geom('panda', str(gpu_device)), 4)
    h, p = _lib.lib(), ops._ptr
    o = [torch.empty(4, 5, 3, device=gpu_device), torch.empty(4, 5, device=gpu_device), torch.empty(4, 5, device=gpu_device),
         torch.empty(4, device=gpu_device, dtype=torch.int32), torch.empty(4, device=gpu_device, dtype=torch.int32)]
    call = lambda g: h.mpb_cartesian_path(p(goal), p(q), p(g.buf), None, None, *[p(t) for t in o], 4, 1, 3, 4, 2, 0.1, 1e-3, 1e-2, 0.5, 0, None)
    assert call(geom) == 2 and 'point robot' in h.mpb_last_error().decode()
    assert call(_geom('panda', str(gpu_device))) == 1 and '7 joints' in h.mpb_last_error().decode()
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _scene(dev):
    """Panda among env_spheres_3d() with the robot's own spheres as a second predicate, plus ONE sphere at the goal of a known straight
    segment: the longest move of the panda set that is complete and free of collisions without that sphere.  Its hand ends inside the
    sphere, so the move is cropped on the way."""
    from motion_planning_baselines_amd import geometry as G
    from motion_planning_baselines_amd.robot_field import PlanningTask
    inp = C.inputs('panda')
    ta = dict(device=torch.device(dev), dtype=torch.float32)
    base = G.env_spheres_3d()
    plain = PlanningTask(inp.robot, base, self_field=G.SelfCollisionField(inp.robot), tensor_args=ta)
    res = plain.cartesian_path(inp.starts, inp.goal, n_steps=C.FULL[0], n_inner=C.FULL[1])
    length = (inp.goal[:, None, :, 3].to(dev) - plain.get_EE_position(inp.starts)).norm(dim=-1)
    assert bool(res.complete.any())
    n, s = divmod(int(torch.where(res.complete, length, torch.zeros_like(length)).argmax()), C.N_STARTS)
    spheres = np.concatenate([np.asarray(base.spheres, dtype=np.float32).reshape(-1, 4), np.asarray([[*inp.goal[n, :, 3].tolist(), 0.04]], dtype=np.float32)])
    task = PlanningTask(inp.robot, G.CollisionField(spheres=spheres, margin=base.margin), self_field=G.SelfCollisionField(inp.robot), tensor_args=ta)
    return inp, task, (n, s)


def test_task_crops_at_the_first_collision(gpu_device):
    from motion_planning_baselines_amd import ops
    inp, task, (n, s) = _scene(str(gpu_device))
    K, n_inner = C.FULL
    kw = dict(n_steps=K, n_inner=n_inner, damping=C.DAMPING, pos_tol=C.POS_TOL, rot_tol=C.ROT_TOL, jump_max=C.JUMP_MAX)
    raw = ops.cartesian_path(inp.goal.to(gpu_device).contiguous(), inp.starts.to(gpu_device).contiguous(), task.geom, K, n_inner=n_inner,
                             damping=C.DAMPING, pos_tol=C.POS_TOL, rot_tol=C.ROT_TOL, jump_max=C.JUMP_MAX, q_min=task.q_min.contiguous(),
                             q_max=task.q_max.contiguous())
    off = task.cartesian_path(inp.starts, inp.goal, collision_free=False, **kw)
    for a, b in zip(raw, (off.q, off.pos_err, off.rot_err, off.n_ok, off.status)):
        assert torch.equal(a, b)                                          # collision_free=False: ops.cartesian_path's output, bit for bit
    assert torch.equal(off.complete, off.status == C.OK) and torch.equal(off.fraction, off.n_ok.float() / K)
    res = task.cartesian_path(inp.starts, inp.goal, **kw)
    N, S, rows, D = res.q.shape
    hit = task.compute_collision(res.q)
    r = torch.arange(rows, device=gpu_device)[None, None, :]
    acc = r <= res.n_ok[:, :, None]
    raw_hit = task.compute_collision(raw[0])
    start_free = ~raw_hit[:, :, 0]
    assert not bool((hit & acc)[start_free].any())                        # every row <= n_ok of every problem is free
    cropped = res.status == C.COLLISION
    print(f'task: {int(cropped.sum())} of {cropped.numel()} problems cropped, {int((cropped & ~start_free).sum())} of them at their start; '
          f'status {torch.bincount(res.status.flatten().cpu(), minlength=5).tolist()}')
    print(f'task: the move to the sphere, problem ({n}, {s}): uncropped n_ok {int(raw[3][n, s])}, cropped to {int(res.n_ok[n, s])}')
    assert bool(cropped[n, s]) and 0 < int(res.n_ok[n, s]) < K            # the sphere on the known segment crops that move on the way
    nxt = (res.n_ok.long() + 1).clamp_max(K)
    at = torch.gather(raw_hit, 2, nxt[:, :, None])[..., 0]
    assert bool(at[cropped & start_free].all())                           # the uncropped row n_ok + 1 collides
    assert bool((res.n_ok[cropped & ~start_free] == 0).all()) and torch.equal(res.q[cropped & ~start_free], raw[0][cropped & ~start_free])
    assert bool((res.n_ok <= raw[3]).all()) and torch.equal(res.status[~cropped], raw[4][~cropped]) and torch.equal(res.q[~cropped], raw[0][~cropped])
    held = torch.gather(res.q, 2, res.n_ok.long()[:, :, None, None].expand(N, S, 1, D))
    assert bool((torch.eq(res.q, held) | acc[..., None])[start_free].all())  # held from the crop on (a start in collision keeps its rows)
    assert torch.equal(torch.where(acc[..., None], res.q, raw[0]), raw[0])  # rows <= n_ok are the tracker's
    # (N, D) starts mean S = 1, and the fields keep those leading dimensions
    one = task.cartesian_path(inp.starts[:, 0], inp.goal, **kw)
    assert one.q.shape == (N, rows, D) and one.n_ok.shape == (N,) and torch.equal(one.q, res.q[:, 0]) and torch.equal(one.status, res.status[:, 0])


def test_ik_then_retreat_then_retime(gpu_device):
    """inverse_kinematics -> select(2) -> a 10 cm retreat along the tool z axis -> retime_trajs of the complete moves."""
    from motion_planning_baselines_amd import geometry as G, ops
    from motion_planning_baselines_amd.robot_field import PlanningTask
    import ik_checks as K
    sc = K.free_scene()
    task = PlanningTask(sc.robot, sc.field, tensor_args=dict(device=gpu_device, dtype=torch.float32))
    grasps, valid = task.inverse_kinematics(sc.target[:8], q_seed=sc.seeds[:8]).select(k=2)
    goal = sc.target[:8].clone().to(gpu_device)
    goal[:, :, 3] -= 0.10 * goal[:, :, 2]                                 # back along the tool's own z axis, the rotation kept
    res = task.cartesian_path(grasps, goal, n_steps=16)
    assert res.q.shape == (8, 2, 17, 7) and res.complete.shape == (8, 2)
    done = res.complete & valid
    print(f'retreat: {int(done.sum())} of {int(valid.sum())} valid grasps retreat completely; status {torch.bincount(res.status.flatten().cpu(), minlength=5).tolist()}')
    assert int(done.sum()) >= 1
    assert not bool(task.compute_collision(res.q[done]).any())
    hand = task.get_EE_pose(res.q[done][:, -1])
    assert float((hand[:, :, 3] - goal[:, None].expand(8, 2, 3, 4)[done][:, :, 3]).norm(dim=-1).max()) <= 1e-3 + 1e-5
    timed = task.retime_trajs(res.q[done], dt=0.01)
    assert bool((timed.status == ops.RETIME_OK).all()) and bool((timed.durations > 0).all())
    assert timed.trajs_dt.shape[0] == int(done.sum()) and timed.trajs_dt.shape[-1] == 14
