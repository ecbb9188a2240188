"""The planners on a cost that holds a GridSDFField member: CHOMP and STOMP take the planned device path (obstacle kernel, the member's own
kernel accumulating, term kernels), MPPI calls the composite on its rollouts, GPMP2 takes it as an extra cost through the dense route,
PlanningTask ORs the predicate in; what is not wired yet raises and says so."""
import types

import numpy as np
import pytest
import torch

from conftest import rel_err_waypoint
import sdf_grid_checks as S

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
PANDA_HOME = (0.0, -0.785, 0.0, -2.356, 0.0, 1.571, 0.785)


def _costs(dev, H, sigma_grid=0.2, sigma_obst=0.3):
    from motion_planning_baselines_amd.planners.costs import cost_functions as C
    ta = dict(device=dev, dtype=torch.float32)
    c = S.case('panda')                                  # env_spheres_3d() at cell 0.05, node values supplied
    cg = C.CostCollision(c.robot, H, field=c.grid, sigma_coll=sigma_grid, tensor_args=ta)
    co = C.CostCollision(c.robot, H, field=c.field, sigma_coll=sigma_obst, tensor_args=ta)
    sm = C.CostSmoothnessCHOMP(c.robot, H, tensor_args=ta)
    return c, cg, co, sm, ta


def _conditioned_start(c, B, H):
    """(B, H, D) fp32 straight lines between uniform configurations plus noise: the first seed whose EVERY waypoint is conditioned by the
    fp64 classifier and that has interior waypoints in contact."""
    rr, g, thr = S.data(c, S.F64)
    t = torch.linspace(0, 1, H).reshape(1, H, 1)
    for seed in range(200):
        qa, qb = S.uniform_q(c.robot, B, seed=100 + seed), S.uniform_q(c.robot, B, seed=300 + seed)
        gen = torch.Generator().manual_seed(seed)
        x = (qa[:, None] * (1 - t) + qb[:, None] * t + 0.02 * torch.randn(B, H, c.robot.q_dim, generator=gen)).contiguous()
        cl = S.classify(rr, g, thr, x.double())
        if bool(cl.conditioned.all()) and bool(cl.inside.all()) and int(cl.contact[:, 1:-1].sum()) >= 3:
            return x
    raise AssertionError('no conditioned start found')


def _device_grid_data(sdf, dev):
    """The device buffer's own node tensor and header numbers as the namespace sdf_grid_checks.sample takes, in fp32 on the device."""
    from motion_planning_baselines_amd import sdf_layout as L
    h = L.header(sdf.host)
    to = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float32)).to(dev)
    return types.SimpleNamespace(nodes=sdf.nodes, lo=to(h['lo']), cell=to(h['cell']), inv=to(h['inv_cell']), dims=sdf.dims)


def test_chomp_planned_path_against_its_autograd_path(gpu_device):
    """CHOMP on CostComposite([grid member, smoothness]) -- the grid gradient kernel, then the terms / apply kernel -- against the SAME
    class driven through its autograd path with a torch callable built from DeviceRobot.fk_map_collision and torch trilinear sampling of
    the node tensor.  3 iterations at B = 8, H = 16; the project's parity bar: 1e-4 relative on the final waypoints.  With the grid
    member's weight 0 the result differs by more than 1e-3: the member acts."""
    from motion_planning_baselines_amd.planners.chomp import CHOMP, chomp_precision_matrix
    from motion_planning_baselines_amd.planners.costs import cost_functions as C
    from motion_planning_baselines_amd.robot_field import device_robot_field
    dev = gpu_device
    B, H = 8, 16
    c, cg, co, sm, ta = _costs(dev, H)
    robot, D = c.robot, c.robot.q_dim
    w = [1.0, 1e-7]                          # (R carries 1 / dt^4: the smoothness gradient is then of the collision gradient's size)
    comp = C.CostComposite(robot, H, [cg, sm], weights_cost_l=w, tensor_args=ta)
    x0 = _conditioned_start(c, B, H)
    drobot, _ = device_robot_field(robot, c.field, dev)
    gd = _device_grid_data(cg.device_sdf(dev), dev)
    thr = S.thresholds(robot, np.float32(c.grid.margin), S.F32).to(dev)
    R = chomp_precision_matrix(robot.dt, H, dict(device=dev, dtype=torch.float32))

    def torch_cost(x, **kw):
        pts = drobot.fk_map_collision(x)                                     # (B, H, L, 3), differentiable (its hand-written vjp)
        grid = torch.relu(thr - S.sample(gd, pts)).sum(-1)[:, 1:].sum(-1) * cg.k_sigma
        smooth = (x * torch.einsum('hk,bkd->bhd', R, x)).sum((1, 2))
        return w[0] * grid + w[1] * smooth

    def planner(cost):
        return CHOMP(n_dof=D, n_support_points=H, num_particles_per_goal=B, opt_iters=1, dt=robot.dt, start_state=x0[0, 0].to(dev), cost=cost,
                     weight_prior_cost=1e-8, initial_particle_means=x0.to(dev), step_size=1e-4, grad_clip=1e4, pos_only=True, tensor_args=ta)    # (a clamp that never binds)
    pl, ref = planner(comp), planner(torch_cost)
    plan = C.device_plan(comp, dev)
    assert C.fusable_collision(comp) is None and plan is not None and plan[0] is None and plan.own == [(cg, 1.0)] and plan.selfs == []
    moved = 0.0
    for it in range(3):
        pl.optimize()
        ref.optimize()
        err = rel_err_waypoint(pl._particle_means, ref._particle_means)
        moved = float((pl._particle_means.cpu() - x0).abs().max())
        print(f'iteration {it}: rel err on the waypoints {err:.2e}, moved {moved:.2e}')
        assert err < 1e-4, (it, err)
    assert moved > 1e-3
    pl2 = planner(C.CostComposite(robot, H, [cg, sm], weights_cost_l=[0.0, w[1]], tensor_args=ta))
    for it in range(3):
        pl2.optimize()
    differ = rel_err_waypoint(pl2._particle_means, ref._particle_means)
    print(f'with the grid member at weight 0 the waypoints differ by {differ:.2e}')
    assert differ > 1e-3


def test_stomp_planned_path_accumulates_the_member_costs(gpu_device):
    """After one optimize(opt_iters=1) on CostComposite([obstacle field, grid member, smoothness]), planner.costs = the sample kernel's
    obstacle cost (the same launch repeated on the saved means: same bits) plus sdf_grid_eval plus the terms eval.  The launches
    accumulate in that order, each adding its fresh value onto the buffer in one fp32 rounding of at most half an ulp of the total."""
    from motion_planning_baselines_amd import ops
    from motion_planning_baselines_amd.planners.costs import cost_functions as C
    from motion_planning_baselines_amd.planners.stomp import STOMP
    dev = gpu_device
    P, Sn, H = 3, 16, 32
    c, cg, co, sm, ta = _costs(dev, H, sigma_grid=0.05, sigma_obst=0.1)
    robot, D = c.robot, c.robot.q_dim
    w = [1.0, 2.0, 1e-6]
    comp = C.CostComposite(robot, H, [co, cg, sm], weights_cost_l=w, tensor_args=ta)
    x0 = _conditioned_start(c, P, H).to(dev)
    pl = STOMP(n_dof=D, n_support_points=H, num_particles_per_goal=P, num_samples=Sn, opt_iters=1, dt=robot.dt, start_state=x0[0, 0], cost=comp,
               initial_particle_means=x0.clone(), temperature=1.0, step_size=0.1, sigma_spectral=0.05, pos_only=True, tensor_args=ta, seed=9)
    assert C.fusable_collision(comp) is None and C.device_plan(comp, dev) is not None and pl.run_path() == ops.STOMP_PATH_TWO_KERNEL
    means0, it0 = pl._particle_means.clone(), pl._iter       # (the constructor's reset() has drawn once already)
    pl.optimize(opt_iters=1)
    torch.cuda.synchronize()
    samples = torch.empty_like(pl.state_particles)
    c_obst = torch.empty(P, Sn, device=dev)
    ops.stomp_sample(means0, None, samples, pl.scale_tril, Sn, seed=pl.seed, it=it0, particle_offset=0, geom=co.device_geometry(dev), costs=c_obst,
                     k_sigma=co.k_sigma, weight=w[0])
    assert torch.equal(samples, pl.state_particles)
    flat = pl.state_particles.view(-1, H, D)
    c_grid = ops.sdf_grid_eval(flat, cg.device_sdf(dev), cg.k_sigma, weight=w[1]).reshape(P, Sn)
    c_term = (w[2] * sm(flat)).reshape(P, Sn)
    assert float(c_grid.max()) > 0 and float(c_obst.max()) > 0 and float(c_term.min()) > 0
    want = c_obst.double() + c_grid.double() + c_term.double()
    err = (pl.costs.double() - want).abs()
    allow = 2 * 0.5 * ULP * want + ULP * c_term.double()                   # (+ the product w * smooth formed here rather than in the kernel)
    print(f'STOMP planned path: costs off by at most {float((err / allow).max()):.2f} of the allowance; grid share {float((c_grid.double() / want).max()):.2f}')
    assert bool((err <= allow).all())
    assert not bool(torch.equal(pl._particle_means, means0))
    assert pl._last_tag == 0                                  # no persistent launch was made for the composite with a grid member


def test_mppi_on_a_planar_grid_calls_the_composite_on_its_rollouts(gpu_device):
    """MPPI hands a cost it cannot fuse to the cost object on device tensors (ONE scalar, the sum over the rollouts, added to every
    sample's cost): with a composite that holds a planar grid member under a 2-D point mass, costs = the kernel's own costs +
    composite.eval of its samples, summed -- finite, and equal to the composite called by hand."""
    from motion_planning_baselines_amd.planners.costs import cost_functions as C
    from motion_planning_baselines_amd.planners.mppi import MPPI, PointParticleDynamics
    dev = gpu_device
    Tn, Sn = 16, 32
    ta = dict(device=dev, dtype=torch.float32)
    c = S.case('point2d')
    robot, D = c.robot, 2
    cg = C.CostCollision(robot, Tn, field=c.grid, sigma_coll=0.2, tensor_args=ta)
    comp = C.CostComposite(robot, Tn, [cg], weights_cost_l=[2.0], tensor_args=ta)
    rr, g, thr = S.data(c, S.F64)
    q0 = S.uniform_q(robot, 40, seed=8)
    start = q0[int(torch.nonzero(S.classify(rr, g, thr, q0.double()).contact)[0])]      # a start in contact

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
    shift = comp.eval(torch.cat((states, controls), dim=-1)).sum(-1)
    by_hand = 2.0 * cg.k_sigma * torch.relu(thr.to(dev).float() - S.sample(_device_grid_data(cg.device_sdf(dev), dev),
                                                                           torch.cat((states, torch.zeros_like(states[..., :1])), -1)[..., None, :])).sum(-1)[..., 1:].sum()
    assert float(shift) > 0 and bool(torch.isfinite(costs).all())
    assert abs(float(shift) - float(by_hand)) <= 2 * Tn * Sn * 2.0 ** -24 * float(by_hand)     # (two fp32 sums of Tn * Sn non-negative terms)
    want = costs0.double() + shift.double()
    assert float((costs.double() - want).abs().max()) <= ULP * float(want.abs().max())
    pl.optimize(opt_iters=1, state=start.to(dev), cost=comp)                  # and a whole step runs
    assert bool(torch.isfinite(pl.get_mean_controls()).all())


def test_what_is_not_wired_raises_gpmp2_takes_the_dense_route_and_the_task_ors_the_predicate(gpu_device):
    from motion_planning_baselines_amd import geometry as G, ops
    from motion_planning_baselines_amd.planners.costs import cost_functions as C
    from motion_planning_baselines_amd.planners.gpmp2 import GPMP2
    from motion_planning_baselines_amd.planners.rrt_connect import RRTConnect
    from motion_planning_baselines_amd.planners.stoch_gpmp import StochGPMP
    from motion_planning_baselines_amd.robot_field import PlanningTask
    dev = gpu_device
    H, n = 8, 2
    c, cg, co, sm, ta = _costs(dev, H, sigma_grid=0.05)
    robot, D, field, grid = c.robot, c.robot.q_dim, c.field, c.grid
    start, goal = torch.tensor(PANDA_HOME), torch.tensor(PANDA_HOME) + 0.3
    common = dict(robot=robot, n_dof=D, n_support_points=H, num_particles_per_goal=n, opt_iters=1, dt=robot.dt, start_state=start.to(dev),
                  multi_goal_states=goal[None].to(dev), sigma_start=1e-3, sigma_gp=1.0, sigma_coll=1e-2, sigma_goal_prior=1e-3, tensor_args=ta)
    r = S.reference('panda', H)
    rows = torch.argsort(r.cl.contact[:, 1:].sum(-1), descending=True)[:n]           # the trajectories with the most waypoints in contact
    assert int(r.cl.contact[rows, 1:].sum()) >= 2
    x0 = S.trajs('panda', H, 2 * D)[rows].to(dev).contiguous()
    gp_kw = dict(step_size=0.5, solver_params=dict(delta=1e-2, trust_region=True, method='cholesky'))
    with pytest.raises(NotImplementedError, match='GridSDFField'):
        GPMP2(collision_fields=[field, grid], initial_particle_means=x0.clone(), **gp_kw, **common)
    with pytest.raises(NotImplementedError, match='GridSDFField'):
        StochGPMP(collision_fields=[grid], sigma_start_init=1e-3, sigma_goal_init=1e-3, sigma_gp_init=1.0, sigma_start_sample=1e-3,
                  sigma_goal_sample=1e-3, sigma_gp_sample=1.0, **common)
    # GPMP2 with the grid as an extra cost: the dense route, one step; it differs from the plain planner's step because the grid's rows
    # act (x0 has waypoints in contact)
    opt = GPMP2(collision_fields=[field], extra_costs=[cg], initial_particle_means=x0.clone(), **gp_kw, **common)      # (a planner steps its means in place: each gets its own)
    plain = GPMP2(collision_fields=[field], initial_particle_means=x0.clone(), **gp_kw, **common)
    assert opt._dense_extras == [cg]
    A, b, Kw = cg.get_linear_system(x0)
    _, pw = ops.sdf_grid_eval(x0, cg.device_sdf(dev), 1.0, per_waypoint=True)
    assert A.shape == (n, H - 1, 2 * D * H) and torch.equal(b[..., 0], pw[:, 1:]) and float(b.max()) > 0 and float(A.abs().max()) > 0
    opt.optimize(opt_iters=1)
    plain.optimize(opt_iters=1)
    assert bool(torch.isfinite(opt._particle_means).all())
    assert float((opt._particle_means - plain._particle_means).abs().max()) > 1e-4
    # the task ORs the predicate in; validation and the RRT planners read the obstacle geometry alone
    wide = G.GridSDFField(grid.values, grid.lo, grid.cell, margin=0.15)              # (a wider margin than the obstacle field's: it adds hits)
    task = PlanningTask(robot, field, sdf_field=wide, tensor_args=ta)
    q = S.uniform_q(robot, 512).to(dev)
    obst, by_grid = ops.collision_check(q, task.geom), ops.sdf_grid_check(q, task.sdf_geom)
    assert torch.equal(task.compute_collision(q), obst | by_grid) and int((by_grid & ~obst).sum()) > 0 and int((~by_grid).sum()) > 0
    assert torch.equal(PlanningTask(robot, field, tensor_args=ta).compute_collision(q), obst)
    free = task.random_coll_free_q(16)
    assert free.shape == (16, D) and not bool(ops.sdf_grid_check(free.contiguous(), task.sdf_geom).any())
    trajs = S.trajs('panda', 8, D)[:4].to(dev)
    for call in (lambda: task.get_trajs_collision_and_free(trajs), lambda: task.compute_fraction_free_trajs(trajs),
                 lambda: task.compute_collision_intensity_trajs(trajs), lambda: task.compute_success_free_trajs(trajs),
                 lambda: RRTConnect(task=task, n_iters=10, start_state_pos=start, goal_state_pos=goal, tensor_args=ta, n_pre_samples=64)):
        with pytest.raises(NotImplementedError, match='sdf_field'):
            call()
    # a planar grid under a chain is a ValueError; two coordinates on a 3-D grid are fine (z = 0)
    planar = S.case('point2d').grid
    with pytest.raises(ValueError, match='planar'):
        ops.DeviceSDFGrid(robot, planar, dev)
    p2 = G.RobotPointMass(2)
    sdf3 = ops.DeviceSDFGrid(p2, S.case('point3d').grid, dev)
    q2 = S.uniform_q(p2, 256)
    gap = ops.sdf_grid_check(q2.to(dev), sdf3, with_gap=True)[1].cpu()
    rr, g, _ = S.data(S.case('point3d'), S.F64)
    thr = S.thresholds(p2, np.float32(S.case('point3d').grid.margin), S.F64)
    c64 = S.oracle_cost(S.ref_robot(p2, S.F64), g, thr, q2.double())
    _, g32, _ = S.data(S.case('point3d'), S.F32)
    E32 = float((S.oracle_cost(S.ref_robot(p2, S.F32), g32, thr.float(), q2).double() - c64).abs().max())
    assert float(c64.max()) > 0 and float((gap.double() - c64).abs().max()) <= S.bar(E32)
