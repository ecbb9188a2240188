"""The planners on a cost that holds a CostEEPose member: CHOMP and STOMP take the planned device path (obstacle kernel, the member's
kernels accumulating, term kernels), MPPI calls the composite on its rollouts, GPMP2 takes it as an extra cost through the dense route.
Small shapes: Panda, H = 16, B = 8."""
import pytest
import torch

import ee_cost_checks as E
import ik_checks as K

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
B, H = 8, 16
DOWN = ((0.0, 0.0, 1.0), (0.0, 0.0, -1.0))         # the tool's z axis pointing down: "keep the cup upright"


def _setup(dev, sigma_obst=0.3):
    from motion_planning_baselines_amd import geometry as G
    from motion_planning_baselines_amd.planners.costs import cost_functions as C
    from test_gpu_edge_cases import _trajs
    ta = dict(device=dev, dtype=torch.float32)
    robot = G.RobotPanda(dt=0.04)
    field = G.env_spheres_3d(0)
    co = C.CostCollision(robot, H, field=field, sigma_coll=sigma_obst, tensor_args=ta)
    sm = C.CostSmoothnessCHOMP(robot, H, tensor_args=ta)
    x0 = _trajs(robot, B, H, robot.q_dim, 11)
    return robot, field, co, sm, x0, ta


def _axis_cost64(robot, x, target, axis):
    """The fp64-restated axis cost sum_{h >= 1} |R a - R* a|^2 of trajectories x (B, H, >= D), per trajectory."""
    tf64, _, _ = K.chain(robot, torch.float64)
    x = x.detach().cpu().double()
    tgt = E.expand_target(target.double(), x.shape[0], x.shape[1], False)
    both = E.trajectory_cost_grad(tf64, x, tgt, 'pos_axis', 1, x.shape[1], axis)[0]
    pos = E.trajectory_cost_grad(tf64, x, tgt, 'pos', 1, x.shape[1], axis)[0]
    return (both - pos).sum(1)


def _chomp(robot, x0, cost, dev, ta, lr, clip):
    from motion_planning_baselines_amd.planners.chomp import CHOMP
    return CHOMP(n_dof=robot.q_dim, n_support_points=H, num_particles_per_goal=B, opt_iters=1, dt=robot.dt, start_state=x0[0, 0].to(dev), cost=cost,
                 weight_prior_cost=1e-8, initial_particle_means=x0.to(dev), step_size=lr, grad_clip=clip, pos_only=True, tensor_args=ta)


def test_chomp_planned_path_against_the_caller_supplied_path(gpu_device):
    """One CHOMP iteration on [obstacles, CostEEPose('path', position + axis), CostSmoothnessCHOMP] through the planned path (obstacle
    gradient kernel, the member's gradient kernel accumulating, terms / apply kernel) against the same composite through CHOMP's
    caller-supplied-cost path, where the member is robot_field.ee_pose + torch + autograd.  The obstacle part of the caller's cost is
    the SAME kernel (its bits agree), the smoothness part fp64 torch.

    The bar, derived: the step is x - lr * clamp(g, +-clip) off the end rows, and the clamp is 1-Lipschitz, so the means differ by at
    most lr * min(2 clip, |dg|) plus one rounding of x.  dg has two parts.  (1) The member: both routes are fp32 evaluations of the same
    closed form at unit k, each within bar(E32) of fp64 in units of S = max(1, largest |element| of the waypoint's fp64 gradient): at most
    w * 2 bar(E32) S.  (2) The sums: the routes add obstacle, member, smoothness and prior gradients in different association and the
    smoothness products are rounded in fp32 in one route only: at most 16 roundings of the largest sum of magnitudes, 16 ULP * Gscale.
    Measured on an MI355X: the means differ by 2.4e-7, the allowance is 9.0e-7 (member E32 4.3e-7), the step 2.3e-1."""
    from motion_planning_baselines_amd.planners.chomp import chomp_precision_matrix
    from motion_planning_baselines_amd.planners.costs import cost_functions as C
    from motion_planning_baselines_amd.robot_field import ee_pose
    dev = gpu_device
    robot, field, co, sm, x0, ta = _setup(dev)
    D = robot.q_dim
    target = E.inputs('panda', B, H).target                                       # one per trajectory: FK of the perturbed last waypoints
    ee = C.CostEEPose(robot, H, target, sigma_pos=1.0, sigma_rot=1.0, axis=E.AXIS, traj_range='path', tensor_args=ta)
    w = [1.0, 0.5, 1e-7]
    comp = C.CostComposite(robot, H, [co, ee, sm], weights_cost_l=w, tensor_args=ta)
    plan = C.device_plan(comp, dev)
    assert [m for m, _ in plan.own] == [ee] and C.fusable_collision(comp) is None and plan[0] is co
    R64 = chomp_precision_matrix(robot.dt, H, dict(device=dev, dtype=torch.float64))
    geom, tgt_d, a = ee.device_geometry(dev), target.to(dev), torch.tensor(E.AXIS, device=dev)

    class Obstacles(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            c, g = co.eval_with_grad(x.contiguous(), weight=w[0])
            ctx.save_for_backward(g)
            return c

        @staticmethod
        def backward(ctx, gc):
            return ctx.saved_tensors[0] * gc[:, None, None]

    def member(x):
        pose = ee_pose(x[..., :D], geom)                                           # (B, H, 3, 4)
        ep = tgt_d[:, None, :, 3] - pose[..., 3]
        du = pose[..., :3] @ a - (tgt_d[:, :, :3] @ a)[:, None]
        return ((ep * ep).sum(-1) + (du * du).sum(-1))[:, 1:].sum(-1)

    def torch_cost(x, **kw):
        x64 = x.double()
        smooth = (x64 * torch.einsum('hk,bkd->bhd', R64, x64)).sum((1, 2))
        return Obstacles.apply(x) + w[1] * member(x) + (w[2] * smooth).float()

    lr, clip = 1e-2, 1e3                                                           # (a clamp that never binds keeps the gradient's size in the step)
    pl, ref = _chomp(robot, x0, comp, dev, ta, lr, clip), _chomp(robot, x0, torch_cost, dev, ta, lr, clip)
    pl.optimize()
    ref.optimize()
    # the bar
    tf64, _, _ = K.chain(robot, torch.float64)
    tf32, _, _ = K.chain(robot, torch.float32)
    full = E.expand_target(target, B, H, False)
    c64, g64, _ = E.trajectory_cost_grad(tf64, x0.double(), full.double(), 'pos_axis', 1, H)
    _, g32, _ = E.trajectory_cost_grad(tf32, x0, full, 'pos_axis', 1, H)
    scale = g64.abs().amax(-1).clamp_min(1.0)
    E32 = float(((g32.double() - g64).abs().amax(-1) / scale).max())
    xd = x0.to(dev)
    _, g_obst = co.eval_with_grad(xd, weight=w[0])
    absRx = torch.einsum('hk,bkd->bhd', R64.abs(), xd.double().abs())
    gscale = float((g_obst.double().abs() + w[1] * g64.abs().to(dev) + 2 * (w[2] + B * 1e-8) * absRx).max())
    dg = w[1] * 2 * E.bar(E32) * float(scale.max()) + 16 * ULP * gscale
    allow = lr * min(2 * clip, dg) + ULP * float(x0.abs().max())
    diff = float((pl._particle_means - ref._particle_means).abs().max())
    moved = float((pl._particle_means.cpu() - x0).abs().max())
    print(f'CHOMP planned against caller-supplied: means differ by {diff:.2e}, allowance {allow:.2e} (member E32 {E32:.2e}, dg <= {dg:.2e}); moved {moved:.2e}')
    assert diff <= allow
    assert moved > 100 * allow                                                     # the step is far above the bar: the comparison sees the gradients
    assert torch.equal(pl._particle_means[:, 0].cpu(), x0[:, 0]) and torch.equal(pl._particle_means[:, -1].cpu(), x0[:, -1])
    # and the member DOES act: without it the result differs by far more than the bar
    pl2 = _chomp(robot, x0, C.CostComposite(robot, H, [co, sm], weights_cost_l=[w[0], w[2]], tensor_args=ta), dev, ta, lr, clip)
    pl2.optimize()
    assert float((pl2._particle_means - ref._particle_means).abs().max()) > 100 * allow


def test_chomp_lowers_the_axis_cost(gpu_device):
    """After 50 iterations with the reference's defaults for the step (step_size 1, grad_clip 0.01) the fp64-restated axis cost of every
    result is strictly below its initial value and strictly below the value of the same run without the member.  Measured on an MI355X:
    the eight costs fall from 11.6 .. 44.2 to 1.3 .. 14.0; without the member they stay at 11.6 .. 43.9."""
    from motion_planning_baselines_amd.planners.costs import cost_functions as C
    dev = gpu_device
    robot, field, co, sm, x0, ta = _setup(dev)
    target = C.CostEEPose.target_for_axis(*DOWN)
    ee = C.CostEEPose(robot, H, target, sigma_rot=0.5, axis=DOWN[0], traj_range='path', tensor_args=ta)
    w = [1.0, 1.0, 1e-7]
    with_m = _chomp(robot, x0, C.CostComposite(robot, H, [co, ee, sm], weights_cost_l=w, tensor_args=ta), dev, ta, 1.0, 0.01)
    without = _chomp(robot, x0, C.CostComposite(robot, H, [co, sm], weights_cost_l=[w[0], w[2]], tensor_args=ta), dev, ta, 1.0, 0.01)
    with_m.optimize(opt_iters=50)
    without.optimize(opt_iters=50)
    c0 = _axis_cost64(robot, x0, target, DOWN[0])
    c1, c2 = _axis_cost64(robot, with_m._particle_means, target, DOWN[0]), _axis_cost64(robot, without._particle_means, target, DOWN[0])
    print(f'CHOMP, 50 iterations: axis cost {c0.tolist()} -> {c1.tolist()} with the member, {c2.tolist()} without')
    assert bool((c1 < c0).all()) and bool((c1 < c2).all())
    assert bool(torch.isfinite(with_m._particle_means).all())


def test_chomp_goal_member_changes_nothing(gpu_device):
    """Quirk Q4: CHOMP zeroes the gradient rows of both endpoints, so a 'goal' member -- whose gradient lives on the last row alone --
    leaves the means bit-identical to the run without it (its cost is still added to planner.costs)."""
    from motion_planning_baselines_amd.planners.costs import cost_functions as C
    dev = gpu_device
    robot, field, co, sm, x0, ta = _setup(dev)
    target = E.inputs('panda', B, H).target
    goal = C.CostEEPose(robot, H, target, sigma_pos=0.1, sigma_rot=0.2, traj_range='goal', tensor_args=ta)
    w = [1.0, 3.0, 1e-7]
    a = _chomp(robot, x0, C.CostComposite(robot, H, [co, goal, sm], weights_cost_l=w, tensor_args=ta), dev, ta, 1e-2, 1e3)
    b = _chomp(robot, x0, C.CostComposite(robot, H, [co, sm], weights_cost_l=[w[0], w[2]], tensor_args=ta), dev, ta, 1e-2, 1e3)
    for _ in range(3):
        a.optimize()
        b.optimize()
    assert torch.equal(a._particle_means, b._particle_means)
    assert float((a._particle_means.cpu() - x0).abs().max()) > 1e-4
    assert bool((a.costs > b.costs).all())


def test_stomp_planned_path_accumulates_the_member(gpu_device):
    """One optimize(opt_iters=1) of two planners with the same seed, with and without the member: the same samples, and planner.costs
    differ by own_eval of the state samples -- one target per particle, its S rollouts reading it (the (p s) order of the flat batch).
    The launches accumulate obstacle, member, terms; every addition is one fp32 rounding of at most half an ulp of its non-negative
    result, and three results enter the difference (o + e, then + t; o + t): 1.5 ULP of the larger total.  Measured on an MI355X: off by at most
    0.55 of that allowance, the member being up to 0.98 of the cost."""
    from motion_planning_baselines_amd import ops
    from motion_planning_baselines_amd.planners.costs import cost_functions as C
    from motion_planning_baselines_amd.planners.stomp import STOMP
    dev = gpu_device
    P, Sn = 4, 16
    robot, field, co, sm, x0, ta = _setup(dev, sigma_obst=0.1)
    D = robot.q_dim
    x0 = x0[:P].to(dev)
    target = E.inputs('panda', B, H).target[:P].contiguous()
    ee = C.CostEEPose(robot, H, target, sigma_pos=0.5, sigma_rot=0.5, traj_range='path', tensor_args=ta)
    w = [1.0, 2.0, 1e-6]

    def planner(cost):
        return STOMP(n_dof=D, n_support_points=H, num_particles_per_goal=P, num_samples=Sn, opt_iters=1, dt=robot.dt, start_state=x0[0, 0],
                     cost=cost, initial_particle_means=x0.clone(), temperature=1.0, step_size=0.1, sigma_spectral=0.05, pos_only=True,
                     tensor_args=ta, seed=9)
    comp = C.CostComposite(robot, H, [co, ee, sm], weights_cost_l=w, tensor_args=ta)
    pl, base = planner(comp), planner(C.CostComposite(robot, H, [co, sm], weights_cost_l=[w[0], w[2]], tensor_args=ta))
    assert C.fusable_collision(comp) is None and C.device_plan(comp, dev).own == [(ee, 2.0)] and pl.run_path() == ops.STOMP_PATH_TWO_KERNEL
    means0 = pl._particle_means.clone()
    pl.optimize(opt_iters=1)
    base.optimize(opt_iters=1)
    torch.cuda.synchronize()
    assert torch.equal(pl.state_particles, base.state_particles)
    flat = pl.state_particles.view(-1, H, D)
    c_ee = ee.own_eval(flat, weight=w[1]).reshape(P, Sn)
    assert float(c_ee.min()) > 0
    err = (pl.costs.double() - base.costs.double() - c_ee.double()).abs()
    allow = 1.5 * ULP * pl.costs.double()
    print(f'STOMP planned path: the member\'s share off by at most {float((err / allow).max()):.2f} of the allowance; its share of the cost '
          f'{float((c_ee.double() / pl.costs.double()).max()):.2f}')
    assert bool((err <= allow).all())
    assert not bool(torch.equal(pl._particle_means, means0)) and not bool(torch.equal(pl._particle_means, base._particle_means))
    assert pl._last_tag == 0                                  # no persistent launch was made for the composite with the member


def test_gpmp2_takes_the_member_through_the_dense_route(gpu_device):
    """One dense step with extra_costs=[CostEEPose] differs from the plain planner's step (by more than 1e-4, the bar of
    test_gpu_self_collision_planners.py's dense-route case) and equals the step solved here in fp64 torch from the composite's own
    get_linear_system: the same (A, b, K) bits, two fp64 Cholesky solves of one SPD system, so the fp32 means agree to two ulp of the
    largest plus what the system's condition number lets two fp64 solves differ by.  Measured on an MI355X: 1.5e-8 (condition number 3.3e4);
    the step differs from the plain one by 5.9e-2."""
    from motion_planning_baselines_amd.planners.costs import cost_functions as C
    from motion_planning_baselines_amd.planners.gpmp2 import GPMP2
    dev = gpu_device
    Hs, n = 8, 2
    robot, field, _, _, _, ta = _setup(dev)
    D = robot.q_dim
    home = torch.tensor([0.0, -0.785, 0.0, -2.356, 0.0, 1.571, 0.785])
    start, goal = home, home + 0.3
    t = torch.linspace(0, 1, Hs).reshape(1, Hs, 1)
    pos = start * (1 - t) + goal * t + 0.02 * torch.randn(n, Hs, D, generator=torch.Generator().manual_seed(2))
    x0 = torch.cat([pos, torch.zeros(n, Hs, D)], -1).to(dev).contiguous()
    target = C.CostEEPose.target_for_axis(*DOWN)
    ee = C.CostEEPose(robot, Hs, target, sigma_rot=0.05, axis=DOWN[0], traj_range='path', tensor_args=ta)
    common = dict(robot=robot, n_dof=D, n_support_points=Hs, num_particles_per_goal=n, opt_iters=1, dt=robot.dt, start_state=start.to(dev),
                  multi_goal_states=goal[None].to(dev), sigma_start=1e-3, sigma_gp=1.0, sigma_coll=1e-2, sigma_goal_prior=1e-3, tensor_args=ta)
    gp_kw = dict(step_size=0.5, solver_params=dict(delta=1e-2, trust_region=True, method='cholesky'))
    opt = GPMP2(collision_fields=[field], extra_costs=[ee], initial_particle_means=x0.clone(), **gp_kw, **common)
    plain = GPMP2(collision_fields=[field], initial_particle_means=x0.clone(), **gp_kw, **common)
    assert opt._dense_extras == [ee]
    A, b, Kd = (m.double() for m in opt.cost.get_linear_system(x0, n_interpolated_points=opt.n_interpolated_points))
    AtK = A.transpose(1, 2) @ Kd
    AtA = AtK @ A
    JtJ = AtA + 1e-2 * AtA.mean(0) * torch.eye(AtA.shape[-1], device=dev, dtype=torch.float64)
    d_theta = torch.cholesky_solve(AtK @ b, torch.linalg.cholesky(JtJ)).reshape(n, Hs, 2 * D)
    want = (x0.double() + 0.5 * d_theta).float()
    cond = float(torch.linalg.cond(JtJ).max())
    opt.optimize(opt_iters=1)
    plain.optimize(opt_iters=1)
    assert bool(torch.isfinite(opt._particle_means).all())
    diff = float((opt._particle_means - want).abs().max())
    acts = float((opt._particle_means - plain._particle_means).abs().max())
    print(f'GPMP2 dense step: off the fp64 solve by {diff:.2e} (condition number {cond:.1e}); differs from the plain step by {acts:.2e}')
    assert acts > 1e-4
    # (two backward-stable fp64 solves of a system of condition number cond agree to ~cond * 2^-52 of the step; then one fp32 rounding each)
    assert diff <= 2 * ULP * float(want.abs().max()) + 0.5 * 8 * cond * 2.0 ** -52 * float(d_theta.abs().max())


def test_mppi_calls_the_composite_on_its_rollouts(gpu_device):
    """MPPI hands a cost it cannot fuse to the cost object on device tensors (ONE scalar, the sum over the rollouts, added to every
    sample's cost): with a composite that holds the member, costs = the kernel's own costs + composite.eval of its samples, summed, and
    the member's eval is part of it.  MPPI's kernel serves up to four controls: a 4-joint chain under velocity control."""
    from motion_planning_baselines_amd.planners.costs import cost_functions as C
    from motion_planning_baselines_amd.planners.mppi import MPPI, PointParticleDynamics
    from test_gpu_generic_dof import make_arm, make_field
    dev = gpu_device
    Tn, Sn = 16, 32
    ta = dict(device=dev, dtype=torch.float32)
    robot = make_arm(4)
    D = robot.q_dim
    co = C.CostCollision(robot, Tn, field=make_field(), sigma_coll=0.3, tensor_args=ta)
    target = C.CostEEPose.target_for_axis(*DOWN, position=(0.3, 0.1, 0.4))
    ee = C.CostEEPose(robot, Tn, target, sigma_pos=0.5, sigma_rot=0.5, axis=DOWN[0], traj_range='path', tensor_args=ta)
    comp = C.CostComposite(robot, Tn, [co, ee], weights_cost_l=[1.0, 2.0], tensor_args=ta)
    start = torch.tensor([0.3, -0.4, 0.5, 0.2])

    def planner():
        system = PointParticleDynamics(rollout_steps=Tn, control_dim=D, state_dim=D, dt=0.05, discount=1., goal_state=torch.zeros(D).to(dev),
                                       ctrl_min=[-2.0] * D, ctrl_max=[2.0] * D,
                                       c_weights={'pos': 1.0, 'vel': 0.0, 'ctrl': 0.1, 'pos_T': 10.0, 'vel_T': 0.}, tensor_args=ta)
        return MPPI(system, num_ctrl_samples=Sn, rollout_steps=Tn, opt_iters=1, control_std=[0.3] * D, temp=1.0, step_size=0.5,
                    cov_prior_type='indep_ctrl', tensor_args=ta, seed=4)
    pl, base = planner(), planner()
    controls, states, costs = pl.sample_and_eval(state=start.to(dev), cost=comp)
    _, states0, costs0 = base.sample_and_eval(state=start.to(dev))
    assert torch.equal(states, states0)
    rollouts = torch.cat((states, controls), dim=-1)
    shift, member = comp.eval(rollouts).sum(-1), ee(rollouts).sum()
    assert float(member) > 0 and float(shift) >= 2.0 * float(member) * (1 - 1e-5)
    want = costs0.double() + shift.double()
    assert float((costs.double() - want).abs().max()) <= ULP * float(want.abs().max())
    pl.optimize(opt_iters=1, state=start.to(dev), cost=comp)                  # and a whole step runs
    assert bool(torch.isfinite(pl.get_mean_controls()).all())
