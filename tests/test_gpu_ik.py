"""GPU: the end-effector pose op and the batched, collision-free inverse kinematics (csrc/mpb_ik.hip) against the
fp64 restatement of tests/ik_checks.py.  Every bar is collision_kinks.bar(E32) = 4 x max(E32, 2^-23) with E32 the fp32 restatement's own
distance from fp64 on the same inputs; the solver's trajectories are chaotic per problem, so after the full budget the tests hold what
a solution must satisfy (in fp64) and the coverage of the targets, never individual seeds."""
import functools

import numpy as np
import pytest
import torch

import ik_checks as K

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _geom(name, dev):
    from motion_planning_baselines_amd import geometry as G, ops
    return ops.DeviceGeometry(K.robot_of(name), G.env_spheres_3d(), torch.device(dev))


def _solve(name, dev, n_iters=K.N_ITERS, limits=True, target=None, seeds=None):
    from motion_planning_baselines_amd import ops
    inp = K.inputs(name)
    f = lambda t: t.to(dev).contiguous()
    out = ops.ik_solve(f(inp.target if target is None else target), f(inp.seeds if seeds is None else seeds), _geom(name, str(dev)),
                       q_min=f(inp.robot.q_min) if limits else None, q_max=f(inp.robot.q_max) if limits else None, n_iters=n_iters,
                       damping=K.DAMPING, pos_tol=K.POS_TOL, rot_tol=K.ROT_TOL, position_only=inp.position_only)
    return [t.cpu() for t in out]


@functools.lru_cache(maxsize=None)
def _full(name, dev):
    """The full-budget run of a set on the device, shared by the tests that read it."""
    return _solve(name, torch.device(dev))


@pytest.mark.parametrize('name', ['panda', 'arm12', 'arm9', 'arm1'])
def test_pose_and_jacobian_against_fp64(gpu_device, name):
    from motion_planning_baselines_amd import ops
    robot = K.robot_of(name)
    q = K.uniform_q(robot, (257,), 5)                                     # four waves and a tail of one
    p64, J64 = K.pose_jacobian(K.chain(robot, torch.float64)[0], q.double())
    p32, J32 = K.pose_jacobian(K.chain(robot, torch.float32)[0], q)
    E_pose, E_jac = float((p32.double() - p64).abs().max()), float((J32.double() - J64).abs().max())
    pose, jac = ops.fk_ee_pose(q.to(gpu_device), _geom(name, str(gpu_device)), with_jacobian=True)
    e_pose, e_jac = float((pose.cpu().double() - p64).abs().max()), float((jac.cpu().double() - J64).abs().max())
    print(f'{name}: pose error {e_pose:.2e} (fp32 restatement {E_pose:.2e}), Jacobian error {e_jac:.2e} (fp32 restatement {E_jac:.2e})')
    assert pose.shape == (257, 3, 4) and jac.shape == (257, 6, robot.q_dim)
    assert e_pose <= K.bar(E_pose) and e_jac <= K.bar(E_jac)
    assert torch.equal(ops.fk_ee_pose(q.to(gpu_device), _geom(name, str(gpu_device))), pose)           # without the Jacobian: the same bits


def test_position_is_the_tool_frames_collision_sphere_bit_for_bit(gpu_device):
    """A chain with a zero-offset collision sphere on the tool frame: ops.fk_collision_points gives that sphere's centre, the bits of t."""
    from motion_planning_baselines_amd import geometry as G, ops
    panda = K.robot_of('panda')
    s = panda.spec()
    robot = G.RobotSerialChain(s['joint_tf'], list(s['link_frame']) + [panda.q_dim + 1], list(s['link_offset']) + [(0.0, 0.0, 0.0)],
                               list(s['link_radius']) + [0.03], q_min=panda.q_min_np, q_max=panda.q_max_np)
    geom = ops.DeviceGeometry(robot, G.env_spheres_3d(), gpu_device, keep_all_links=True)
    q = K.uniform_q(panda, (257,), 6).to(gpu_device)
    pts = ops.fk_collision_points(q[None], geom)[0]
    assert torch.equal(ops.fk_ee_pose(q, geom)[:, :, 3], pts[:, -1])
    assert torch.equal(ops.fk_ee_pose(q, geom), ops.fk_ee_pose(q, _geom('panda', str(gpu_device))))  # the chain alone decides the pose


@pytest.mark.parametrize('name', ['panda', 'arm12'])
def test_ee_pose_gradient_of_a_linear_functional(gpu_device, name):
    """robot_field.ee_pose's backward (torch, from the kernel's Jacobian) against the fp64 restatement's autograd gradient of a fixed
    random linear functional of the pose; leading dimensions are kept, and the robot's and the task's methods are the same op."""
    from motion_planning_baselines_amd import geometry as G, robot_field
    robot = K.robot_of(name)
    q = K.uniform_q(robot, (3, 43), 7)
    W = torch.as_tensor(np.random.RandomState(8).standard_normal((3, 43, 3, 4)))

    def grad(dtype):
        x = q.to(dtype).reshape(-1, robot.q_dim).requires_grad_(True)
        (K.pose_jacobian(K.chain(robot, dtype)[0], x)[0] * W.to(dtype).reshape(-1, 3, 4)).sum().backward()
        return x.grad.reshape(q.shape)
    g64, g32 = grad(torch.float64), grad(torch.float32)
    E32 = float((g32.double() - g64).abs().max())
    x = q.to(gpu_device).requires_grad_(True)
    pose = robot_field.ee_pose(x, _geom(name, str(gpu_device)))
    assert pose.shape == (3, 43, 3, 4)
    (pose * W.float().to(gpu_device)).sum().backward()
    err = float((x.grad.cpu().double() - g64).abs().max())
    print(f'{name}: gradient error {err:.2e} (fp32 restatement {E32:.2e})')
    assert err <= K.bar(E32)
    task = robot_field.PlanningTask(robot, G.env_spheres_3d(), tensor_args=dict(device=gpu_device, dtype=torch.float32))
    dr, _ = robot_field.device_robot_field(robot, G.env_spheres_3d(), gpu_device)
    assert torch.equal(task.get_EE_pose(q), pose.detach()) and torch.equal(dr.get_EE_pose(q.to(gpu_device)), pose.detach())
    assert torch.equal(task.get_EE_position(q), pose.detach()[..., 3]) and task.get_EE_position(q).shape == (3, 43, 3)
    assert torch.equal(dr.get_EE_position(torch.cat([q, q], -1).to(gpu_device)), pose.detach()[..., 3])       # (states: positions first)


def test_a_point_robot_has_no_end_effector(gpu_device):
    from motion_planning_baselines_amd import _lib, geometry as G, ops
    geom = ops.DeviceGeometry(G.RobotPointMass(3, radius=0.05), G.env_spheres_3d(), gpu_device)
    q = torch.zeros(4, 3, device=gpu_device)
    with pytest.raises(ValueError, match='point robot'):
        ops.fk_ee_pose(q, geom)
    with pytest.raises(ValueError, match='point robot'):
        ops.ik_solve(torch.zeros(4, 3, 4, device=gpu_device), q[:, None].contiguous(), geom)
    # the C-ABI's own refusals that read the header: a point robot is UNSUPPORTED, a chain of another width INVALID
    h, p = _lib.lib(), ops._ptr
    out = torch.empty(4, 12, device=gpu_device)
    assert h.mpb_fk_ee_pose(p(q), p(geom.buf), p(out), None, 4, 3, None) == 2 and 'point robot' in h.mpb_last_error().decode()
    panda = _geom('panda', str(gpu_device))
    assert h.mpb_fk_ee_pose(p(q), p(panda.buf), p(out), None, 4, 3, None) == 1 and '7 joints' in h.mpb_last_error().decode()
    torch.cuda.synchronize()


def test_an_address_that_got_another_chain_is_read_again(gpu_device):
    """The library keeps kind / n_dof of a geometry buffer per address and a geometry buffer has no invalidate: a call whose D disagrees
    with what it kept reads the header again before it refuses.  ONE allocation holds the Panda's geometry (7 joints), then the 12-joint
    arm's: each call succeeds with the bits of the call on a buffer of the robot's own, and a call with the first D afterwards is refused
    by what the buffer holds now."""
    from motion_planning_baselines_amd import _lib, ops
    h, p = _lib.lib(), ops._ptr
    geoms = [_geom(name, str(gpu_device)) for name in ('panda', 'arm12')]
    shared = torch.zeros(max(g.host.size for g in geoms), device=gpu_device)

    def pose(q):
        out = torch.empty(q.shape[0], 3, 4, device=gpu_device)
        with torch.cuda.device(gpu_device):
            return h.mpb_fk_ee_pose(p(q), p(shared), p(out), None, q.shape[0], q.shape[1], ops._stream()), out
    qs = []
    for g in geoms:
        shared[:g.host.size].copy_(torch.from_numpy(g.host))
        torch.cuda.synchronize()
        qs.append(K.uniform_q(g.robot, (65,), 9).to(gpu_device))
        rc, out = pose(qs[-1])
        assert rc == 0, h.mpb_last_error().decode()
        assert torch.equal(out, ops.fk_ee_pose(qs[-1], g))
    rc, _ = pose(qs[0])
    assert rc == 1 and 'the chain has 12 joints' in h.mpb_last_error().decode()
    torch.cuda.synchronize()


@pytest.mark.parametrize('name', K.SETS)
def test_one_step_against_fp64(gpu_device, name):
    inp = K.inputs(name)
    for limits in (True, False):
        ref = K.reference(name, 1, limits)
        q, pe, th, conv, iters = _solve(name, gpu_device, n_iters=1, limits=limits)
        err = float((q.double() - ref.r64.q).abs().max())
        print(f'{name} limits={limits}: one step, q error {err:.2e} rad (fp32 restatement {ref.E32_q:.2e})')
        assert err <= K.bar(ref.E32_q)
        assert bool(((iters == 1) | conv).all())
    ref = K.reference(name, 0)
    q, pe, th, conv, iters = _solve(name, gpu_device, n_iters=0)
    assert torch.equal(q, inp.seeds) and not bool(iters.any())              # no step: the seeds' bits
    e_pos, e_rot = float((pe.double() - ref.r64.pos_err).abs().max()), float((th.double() - ref.r64.rot_err).abs().max())
    print(f'{name}: n_iters = 0, pos_err error {e_pos:.2e} m (fp32 restatement {ref.E32_pos:.2e}), rot_err error {e_rot:.2e} rad ({ref.E32_rot:.2e})')
    assert e_pos <= K.bar(ref.E32_pos) and e_rot <= K.bar(ref.E32_rot)
    assert torch.equal(conv, (ref.r64.pos_err <= K.POS_TOL) & ((ref.r64.rot_err <= K.ROT_TOL) | inp.position_only))     # (none within the bar of a tolerance)


@pytest.mark.parametrize('name', K.SETS)
def test_solutions_are_solutions_and_cover_the_targets(gpu_device, name):
    inp, ref = K.inputs(name), K.reference(name)
    q, pe, th, conv, iters = _full(name, str(gpu_device))
    # what is flagged converged IS a solution, by fp64 forward kinematics
    pe64, th64 = K.fk_error(name, inp.target, q)
    assert float(pe64[conv].max()) <= K.POS_TOL + K.DELTA
    if not inp.position_only:
        assert float(th64[conv].max()) <= K.ROT_TOL + K.DELTA
    assert bool((iters[~conv] == K.N_ITERS).all()) and bool((iters <= K.N_ITERS).all())
    assert bool(((q >= inp.robot.q_min) & (q <= inp.robot.q_max)).all())
    # coverage against the reference, not against the kernel's own claim
    rich = ref.r64.converged.sum(1) >= 3
    share, share64 = float(conv.float().mean()), float(ref.r64.converged.float().mean())
    print(f'{name}: converged share {share:.3f} (fp64 restatement {share64:.3f}); targets with >= 3 converged reference seeds {int(rich.sum())}, '
          f'of which the kernel covers {int((conv.any(1) & rich).sum())}')
    assert bool(conv.any(1)[rich].all())
    assert share >= share64 - 0.03


def test_layout_independence_and_determinism(gpu_device):
    """3 x 37 = 111 problems -- a partial wave, the target changing inside a wave -- return the bits of the same problems of the 64 x 32 run."""
    name = 'panda'
    inp = K.inputs(name)
    big = _full(name, str(gpu_device))
    idx = torch.arange(37) % K.N_SEEDS                                    # (a target has 32 seeds: five problems appear twice)
    small = _solve(name, gpu_device, target=inp.target[:3], seeds=inp.seeds[:3][:, idx])
    again = _solve(name, gpu_device, target=inp.target[:3], seeds=inp.seeds[:3][:, idx])
    for a, b, c in zip(small, big, again):
        assert a.shape[:2] == (3, 37)
        assert torch.equal(a, b[:3][:, idx]) and torch.equal(a, c)
    assert 0 < int(small[3].sum()) < 111


def _check_result(task, res, dev):
    assert torch.equal(res.free, res.converged & ~task.compute_collision(res.q))
    assert res.q.shape == res.converged.shape + (task.q_dim,) and res.iters.dtype == torch.int32


def test_collision_free_goals(gpu_device):
    from motion_planning_baselines_amd import geometry as G
    from motion_planning_baselines_amd.robot_field import PlanningTask
    sc = K.free_scene()
    ta = dict(device=gpu_device, dtype=torch.float32)
    task = PlanningTask(sc.robot, sc.field, tensor_args=ta)
    res = task.inverse_kinematics(sc.target, q_seed=sc.seeds)
    _check_result(task, res, gpu_device)
    rich = sc.free64.sum(1) >= 3
    free = res.free.cpu()
    print(f'free scene: free share {float(free.float().mean()):.3f} (fp64 restatement {float(sc.free64.float().mean()):.3f}); targets with >= 3 free '
          f'reference seeds {int(rich.sum())}, of which the task covers {int((free.any(1) & rich).sum())}')
    assert bool(free.any(1)[rich].all())
    # select: per target the first k free solutions by seed index ...
    q2, valid = res.select(k=2)
    assert q2.shape == (K.N_TARGETS, 2, 7) and valid.shape == (K.N_TARGETS, 2)
    for n in range(K.N_TARGETS):
        first = torch.nonzero(free[n]).flatten()[:2]
        assert valid[n].cpu().tolist() == [True] * len(first) + [False] * (2 - len(first))
        assert torch.equal(q2[n, :len(first)].cpu(), res.q[n].cpu()[first])
    assert not bool(task.compute_collision(q2[valid]).any())
    pe64, th64 = K.fk_error('panda', sc.target, q2.cpu())
    assert float(pe64[valid.cpu()].max()) <= K.POS_TOL + K.DELTA and float(th64[valid.cpu()].max()) <= K.ROT_TOL + K.DELTA
    # ... or, with a q_ref, by distance to it: seed 0 is q_ref, the order is the stable sort's
    q_ref = K.uniform_q(sc.robot, (), 9)
    near = task.inverse_kinematics(sc.target, q_seed=sc.seeds, q_ref=q_ref)
    _check_result(task, near, gpu_device)
    assert torch.equal(near.q[:, 1:], res.q[:, 1:])                       # (the other seeds are the same problems)
    q3, valid3 = near.select(k=3)
    d = torch.linalg.norm(near.q.cpu() - q_ref, dim=-1)
    for n in range(K.N_TARGETS):
        order = torch.argsort(d[n], stable=True)
        first = order[near.free[n].cpu()[order]][:3]
        assert valid3[n].cpu().tolist() == [True] * len(first) + [False] * (3 - len(first))
        assert torch.equal(q3[n, :len(first)].cpu(), near.q[n].cpu()[first])
    # seeds from the task's generator: reproducible per seed, and position-only targets as (N, 3)
    a = PlanningTask(sc.robot, sc.field, tensor_args=ta, seed=5).inverse_kinematics(sc.target[:5], n_seeds=8)
    b = PlanningTask(sc.robot, sc.field, tensor_args=ta, seed=5).inverse_kinematics(sc.target[:5], n_seeds=8)
    assert a.q.shape == (5, 8, 7) and torch.equal(a.q, b.q) and torch.equal(a.free, b.free)
    po = task.inverse_kinematics(sc.target[:5, :, 3], n_seeds=8, position_only=True)
    _check_result(task, po, gpu_device)
    assert float((task.get_EE_position(po.q)[po.converged] - sc.target[:5, None, :, 3].to(gpu_device).expand(5, 8, 3)[po.converged]).norm(dim=-1).max()) <= K.POS_TOL + K.DELTA
    # the same identity with the robot's own spheres and with a precomputed SDF grid ORed in
    for kw in (dict(self_field=G.SelfCollisionField(sc.robot)),
               dict(sdf_field=G.GridSDFField.from_field(sc.field, (-1.2, -1.2, -0.6), (1.2, 1.2, 1.6), 0.05))):
        t2 = PlanningTask(sc.robot, sc.field, tensor_args=ta, **kw)
        r2 = t2.inverse_kinematics(sc.target[:16], q_seed=sc.seeds[:16])
        _check_result(t2, r2, gpu_device)
        assert torch.equal(r2.q, res.q[:16]) and torch.equal(r2.converged, res.converged[:16])
        assert bool((r2.free <= res.free[:16]).all())                     # (one more predicate can only take solutions away)
    off = task.inverse_kinematics(sc.target[:16], q_seed=sc.seeds[:16], collision_free=False)
    assert torch.equal(off.free, off.converged)


def test_planners_take_the_goals(gpu_device):
    """Neither asserts plan quality (the planners' own tests do): the goals IK selects are goals the planners accept."""
    from motion_planning_baselines_amd import ops
    from motion_planning_baselines_amd.planners.gpmp2 import GPMP2
    from motion_planning_baselines_amd.planners.rrt_connect import RRTConnect
    from motion_planning_baselines_amd.robot_field import PlanningTask
    sc = K.free_scene()
    ta = dict(device=gpu_device, dtype=torch.float32)
    task = PlanningTask(sc.robot, sc.field, tensor_args=ta)
    goals, valid = task.inverse_kinematics(sc.target[:2], q_seed=sc.seeds[:2]).select(k=2)
    assert bool(valid.all())
    start = task.random_coll_free_q(1)[0]
    p = RRTConnect(task=task, n_iters=10, start_state_pos=start, goal_state_pos=goals[0, 0], tensor_args=ta, n_pre_samples=64)
    p.optimize()
    assert p.status.tolist() != [ops.RRT_START_OR_GOAL_IN_COLLISION]
    D, H, n = task.q_dim, 8, 2
    pl = GPMP2(robot=sc.robot, n_dof=D, n_support_points=H, num_particles_per_goal=n, opt_iters=2, dt=0.04, start_state=start,
               multi_goal_states=goals.reshape(-1, D), sigma_start_init=1e-3, sigma_goal_init=1e-3, sigma_gp_init=1.0, sigma_start_sample=1e-3,
               sigma_goal_sample=1e-3, collision_fields=[sc.field], sigma_start=1e-3, sigma_gp=1.0, sigma_coll=1e-2, sigma_goal_prior=1e-3,
               step_size=0.5, solver_params=dict(delta=1e-2, trust_region=True, method='cholesky'), tensor_args=ta)
    pl.optimize(opt_iters=2)
    assert pl._particle_means.shape == (4 * n, H, 2 * D) and bool(torch.isfinite(pl._particle_means).all())
