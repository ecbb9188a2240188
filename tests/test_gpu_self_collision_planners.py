"""The planners on a cost that holds a SelfCollisionField member: CHOMP and STOMP take the planned device path (obstacle kernel, self
kernel accumulating, term kernels), MPPI calls the composite on its rollouts, GPMP2 takes it as an extra cost through the dense route;
what is not wired yet raises and says so."""
import numpy as np
import pytest
import torch

from conftest import rel_err_waypoint
import collision_kinks as K
import self_collision_checks as S

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23


def _costs(dev, H, sigma_self=0.2, sigma_obst=0.3):
    from motion_planning_baselines_amd import geometry as G
    from motion_planning_baselines_amd.planners.costs import cost_functions as C
    ta = dict(device=dev, dtype=torch.float32)
    robot, sfield = S.case('panda')
    field = G.env_spheres_3d(0)
    co = C.CostCollision(robot, H, field=field, sigma_coll=sigma_obst, tensor_args=ta)
    cs = C.CostCollision(robot, H, field=sfield, sigma_coll=sigma_self, tensor_args=ta)
    sm = C.CostSmoothnessCHOMP(robot, H, tensor_args=ta)
    return robot, field, sfield, co, cs, sm, ta


def _conditioned_start(robot, field, sfield, B, H):
    """(B, H, D) fp32 straight lines between uniform configurations plus noise, the first seed whose EVERY waypoint is conditioned for
    both fields by the fp64 classifiers and that has waypoints in contact with the obstacles and with the robot itself."""
    from oracle.geometry_ref import make_ref_geometry
    rr64, rf64 = make_ref_geometry(robot, field, S.F64)
    a, b, T = S.pair_data(sfield, S.F64)
    t = torch.linspace(0, 1, H).reshape(1, H, 1)
    for seed in range(200):
        qa, qb = S.uniform_q(robot, B, seed=100 + seed), S.uniform_q(robot, B, seed=300 + seed)
        g = torch.Generator().manual_seed(seed)
        x = (qa[:, None] * (1 - t) + qb[:, None] * t + 0.02 * torch.randn(B, H, robot.q_dim, generator=g)).contiguous()
        cs, co = S.classify(rr64, a, b, T, x.double()), K.classify(rr64, rf64, x.double())
        if bool(cs.conditioned.all()) and bool(co.conditioned.all()) and int(cs.contact[:, 1:-1].sum()) >= 3 and int((co.n_active.sum(-1) > 0)[:, 1:-1].sum()) >= 3:
            return x
    raise AssertionError('no conditioned start found')


def test_chomp_planned_path_against_its_autograd_path(gpu_device):
    """CHOMP on CostComposite([obstacle field, self field, smoothness]) -- obstacle gradient kernel, self gradient kernel accumulating
    into the same buffer, terms / apply kernel -- against the SAME class driven through its autograd path with a torch callable built
    from DeviceRobot.fk_map_collision and the pair list (an independent route through kernels that existed before).  3 iterations at
    B = 8, H = 16; the project's parity bar: 1e-4 relative on the final waypoints.  Measured on an MI355X: the waypoints move 2.3e-2 in the
    three iterations and the two routes end on identical fp32 waypoints (their gradients differ by ~1e-6 relative, a step of 1e-4 of that
    is far below half an ulp of a joint angle); without the self member the result differs by more than 1e-3."""
    from motion_planning_baselines_amd.planners.chomp import CHOMP, chomp_precision_matrix
    from motion_planning_baselines_amd.planners.costs import cost_functions as C
    from motion_planning_baselines_amd.robot_field import device_robot_field
    dev = gpu_device
    B, H = 8, 16
    robot, field, sfield, co, cs, sm, ta = _costs(dev, H)
    D = robot.q_dim
    w = [1.0, 2.0, 1e-7]                     # (R carries 1 / dt^4: the smoothness gradient is then of the collision gradients' size)
    comp = C.CostComposite(robot, H, [co, cs, sm], weights_cost_l=w, tensor_args=ta)
    x0 = _conditioned_start(robot, field, sfield, B, H)
    drobot, dfield = device_robot_field(robot, field, dev)
    pa, pb, T = (t.to(dev) for t in S.pair_data(sfield, S.F32))
    R = chomp_precision_matrix(robot.dt, H, dict(device=dev, dtype=torch.float32))

    def torch_cost(x, **kw):
        pts = drobot.fk_map_collision(x)                                     # (B, H, L, 3), differentiable (its hand-written vjp)
        obst = dfield.compute_cost(x, pts)[:, 1:].sum(-1) * co.k_sigma
        n = torch.sqrt(((pts[..., pa, :] - pts[..., pb, :]) ** 2).sum(-1).clamp_min(1e-30))
        selfc = torch.relu(T - n).sum(-1)[:, 1:].sum(-1) * cs.k_sigma
        smooth = (x * torch.einsum('hk,bkd->bhd', R, x)).sum((1, 2))
        return w[0] * obst + w[1] * selfc + w[2] * smooth

    def planner(cost):
        return CHOMP(n_dof=D, n_support_points=H, num_particles_per_goal=B, opt_iters=1, dt=robot.dt, start_state=x0[0, 0].to(dev), cost=cost,
                     weight_prior_cost=1e-8, initial_particle_means=x0.to(dev), step_size=1e-4, grad_clip=1e4, pos_only=True, tensor_args=ta)    # (a clamp that never binds: a clamped step keeps only the gradient's signs)
    pl, ref = planner(comp), planner(torch_cost)
    assert C.fusable_collision(comp) is None and len(C.device_plan(comp, dev).selfs) == 1
    moved = 0.0
    for it in range(3):
        pl.optimize()
        ref.optimize()
        err = rel_err_waypoint(pl._particle_means, ref._particle_means)
        moved = float((pl._particle_means.cpu() - x0).abs().max())
        print(f'iteration {it}: rel err on the waypoints {err:.2e}, moved {moved:.2e}')
        assert err < 1e-4, (it, err)
    assert moved > 1e-3
    # and the self member DOES act: without it the result differs by far more than the bar
    pl2 = planner(C.CostComposite(robot, H, [co, sm], weights_cost_l=[w[0], w[2]], tensor_args=ta))
    for it in range(3):
        pl2.optimize()
    assert rel_err_waypoint(pl2._particle_means, ref._particle_means) > 1e-3


def test_stomp_planned_path_accumulates_the_member_costs(gpu_device):
    """After one optimize(opt_iters=1) on such a composite, planner.costs = the member costs on planner.state_particles: the sample
    kernel's obstacle cost (the same launch repeated on the saved means: same bits), plus the stand-alone self eval, plus the stand-alone
    terms eval.  The launches accumulate in that order, each adding its fresh value onto the buffer: two additions of non-negative
    terms, each one fp32 rounding of at most half an ulp of the total.  A collision-only composite still takes the fused path: the
    persistent launch, seen by its completion tag.  Measured on an MI355X: the costs are off by at most 0.74 of the allowance."""
    from motion_planning_baselines_amd import ops
    from motion_planning_baselines_amd.planners.costs import cost_functions as C
    from motion_planning_baselines_amd.planners.stomp import STOMP
    dev = gpu_device
    P, Sn, H = 3, 16, 32
    robot, field, sfield, co, cs, sm, ta = _costs(dev, H, sigma_self=0.05, sigma_obst=0.1)
    D = robot.q_dim
    w = [1.0, 2.0, 1e-6]
    comp = C.CostComposite(robot, H, [co, cs, sm], weights_cost_l=w, tensor_args=ta)
    x0 = _conditioned_start(robot, field, sfield, P, H).to(dev)

    def planner(cost):
        return STOMP(n_dof=D, n_support_points=H, num_particles_per_goal=P, num_samples=Sn, opt_iters=1, dt=robot.dt, start_state=x0[0, 0],
                     cost=cost, initial_particle_means=x0.clone(), temperature=1.0, step_size=0.1, sigma_spectral=0.05, pos_only=True,
                     tensor_args=ta, seed=9)
    pl = planner(comp)
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
    c_self = ops.self_collision_eval(flat, cs.device_self(dev), cs.k_sigma, weight=w[1]).reshape(P, Sn)
    c_term = (w[2] * sm(flat)).reshape(P, Sn)
    assert float(c_self.max()) > 0 and float(c_obst.max()) > 0 and float(c_term.min()) > 0
    want = c_obst.double() + c_self.double() + c_term.double()
    err = (pl.costs.double() - want).abs()
    allow = 2 * 0.5 * ULP * want + ULP * c_term.double()                   # (+ the product w * smooth formed here rather than in the kernel)
    print(f'STOMP planned path: costs off by at most {float((err / allow).max()):.2f} of the allowance; self share {float((c_self.double() / want).max()):.2f}')
    assert bool((err <= allow).all())
    assert not bool(torch.equal(pl._particle_means, means0))
    assert pl._last_tag == 0                                  # no persistent launch was made for the composite with a self member
    # A collision-only composite still takes the FUSED path: at the headline's form (H = 64, d = 14, S = 32) that is the persistent
    # launch, which run_path() names and which leaves its completion tag behind; the planned path above leaves none.
    P2, S2, H2 = 8, 32, 64
    co2 = C.CostCollision(robot, H2, field=field, sigma_coll=0.1, tensor_args=ta)
    cs2 = C.CostCollision(robot, H2, field=sfield, sigma_coll=0.05, tensor_args=ta)
    t = torch.linspace(0, 1, H2).reshape(1, H2, 1)
    qa, qb = S.uniform_q(robot, P2, seed=21)[:, None], S.uniform_q(robot, P2, seed=22)[:, None]
    m2 = torch.cat([qa * (1 - t) + qb * t, torch.zeros(P2, H2, D)], -1).to(dev).contiguous()

    def planner2(cost):
        return STOMP(n_dof=D, n_support_points=H2, num_particles_per_goal=P2, num_samples=S2, opt_iters=1, dt=robot.dt, start_state=m2[0, 0, :D],
                     cost=cost, initial_particle_means=m2.clone(), temperature=1.0, step_size=0.1, sigma_spectral=0.05, pos_only=False,
                     tensor_args=ta, seed=9)
    fused = planner2(C.CostComposite(robot, H2, [co2], tensor_args=ta))
    assert C.fusable_collision(fused.cost) is not None
    assert fused.run_path() in (ops.STOMP_PATH_PERSISTENT_EXCHANGE, ops.STOMP_PATH_PERSISTENT)
    fused.optimize(opt_iters=1)
    torch.cuda.synchronize()
    assert fused._last_tag != 0 and fused._plan is not None   # the persistent launch ran
    planned = planner2(C.CostComposite(robot, H2, [co2, cs2], tensor_args=ta))
    assert planned.run_path() == ops.STOMP_PATH_TWO_KERNEL
    planned.optimize(opt_iters=1)
    torch.cuda.synchronize()
    assert planned._last_tag == 0 and planned._plan is None and planned._run_ws is None
    assert C.fusable_collision(planner(cs).cost) is None


def test_mppi_calls_the_composite_on_its_rollouts(gpu_device):
    """MPPI hands a cost it cannot fuse to the cost object on device tensors (point.py:191-196: ONE scalar, the sum over the rollouts,
    added to every sample's cost): with a composite that holds a self member, costs = the kernel's own costs + composite.eval of its
    samples, summed.  MPPI's kernel serves up to four controls: a 4-joint chain under velocity control."""
    from motion_planning_baselines_amd.planners.costs import cost_functions as C
    from motion_planning_baselines_amd.planners.mppi import MPPI, PointParticleDynamics
    dev = gpu_device
    from motion_planning_baselines_amd import geometry as G
    from test_gpu_generic_dof import make_arm, make_field
    Tn, Sn = 16, 32
    ta = dict(device=dev, dtype=torch.float32)
    robot = make_arm(4)
    field, sfield = make_field(), G.SelfCollisionField(robot, margin=0.1, min_frame_gap=2)
    co = C.CostCollision(robot, Tn, field=field, sigma_coll=0.3, tensor_args=ta)
    cs = C.CostCollision(robot, Tn, field=sfield, sigma_coll=0.2, tensor_args=ta)
    D = robot.q_dim
    comp = C.CostComposite(robot, Tn, [co, cs], weights_cost_l=[1.0, 2.0], tensor_args=ta)
    q0 = S.uniform_q(robot, 40, seed=8)
    a, b, T = S.pair_data(sfield, S.F64)
    start = q0[int(torch.nonzero(S.classify(S.ref_robot(robot, S.F64), a, b, T, q0.double()).contact)[0])]      # a start in self-contact

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
    assert float(shift) > 0 and float(cs(torch.cat((states, controls), dim=-1)).sum()) > 0
    want = costs0.double() + shift.double()
    assert float((costs.double() - want).abs().max()) <= ULP * float(want.abs().max())
    pl.optimize(opt_iters=1, state=start.to(dev), cost=comp)                  # and a whole step runs
    assert bool(torch.isfinite(pl.get_mean_controls()).all())


def test_what_is_not_wired_raises_and_gpmp2_takes_the_dense_route(gpu_device):
    from motion_planning_baselines_amd import geometry as G
    from motion_planning_baselines_amd.planners.costs import cost_functions as C
    from motion_planning_baselines_amd.planners.gpmp2 import GPMP2
    from motion_planning_baselines_amd.planners.rrt_connect import RRTConnect
    from motion_planning_baselines_amd.planners.stoch_gpmp import StochGPMP
    from motion_planning_baselines_amd.robot_field import PlanningTask
    dev = gpu_device
    H, n = 8, 2
    robot, field, sfield, co, cs, sm, ta = _costs(dev, H, sigma_self=0.05)
    D = robot.q_dim
    start, goal = torch.tensor(S.PANDA_HOME), torch.tensor(S.PANDA_HOME) + 0.3
    common = dict(robot=robot, n_dof=D, n_support_points=H, num_particles_per_goal=n, opt_iters=1, dt=robot.dt, start_state=start.to(dev),
                  multi_goal_states=goal[None].to(dev), sigma_start=1e-3, sigma_gp=1.0, sigma_coll=1e-2, sigma_goal_prior=1e-3, tensor_args=ta)
    r = S.reference('panda', H)
    rows = torch.argsort(r.cl.contact[:, 1:].sum(-1), descending=True)[:n]           # the trajectories with the most waypoints in self-contact
    assert int(r.cl.contact[rows, 1:].sum()) >= 2
    x0 = S.trajs('panda', H, 2 * D)[rows].to(dev).contiguous()
    gp_kw = dict(step_size=0.5, solver_params=dict(delta=1e-2, trust_region=True, method='cholesky'))
    with pytest.raises(NotImplementedError, match='SelfCollisionField'):
        GPMP2(collision_fields=[field, sfield], initial_particle_means=x0.clone(), **gp_kw, **common)
    with pytest.raises(NotImplementedError, match='SelfCollisionField'):
        StochGPMP(collision_fields=[sfield], sigma_start_init=1e-3, sigma_goal_init=1e-3, sigma_gp_init=1.0, sigma_start_sample=1e-3,
                  sigma_goal_sample=1e-3, sigma_gp_sample=1.0, **common)
    # GPMP2 with the self field as an extra cost: the dense route, one step; it differs from the plain planner's step because the self
    # rows act (x0 has waypoints in self-contact)
    opt = GPMP2(collision_fields=[field], extra_costs=[cs], initial_particle_means=x0.clone(), **gp_kw, **common)      # (a planner steps its means in place: each gets its own)
    plain = GPMP2(collision_fields=[field], initial_particle_means=x0.clone(), **gp_kw, **common)
    assert opt._dense_extras == [cs]
    opt.optimize(opt_iters=1)
    plain.optimize(opt_iters=1)
    assert bool(torch.isfinite(opt._particle_means).all())
    assert float((opt._particle_means - plain._particle_means).abs().max()) > 1e-4
    # the task: validation and the RRT planners read the obstacle geometry alone
    task = PlanningTask(robot, field, self_field=sfield, tensor_args=ta)
    trajs = S.trajs('panda', 8, D)[:4].to(dev)
    for call in (lambda: task.get_trajs_collision_and_free(trajs), lambda: task.compute_fraction_free_trajs(trajs),
                 lambda: task.compute_collision_intensity_trajs(trajs), lambda: task.compute_success_free_trajs(trajs),
                 lambda: RRTConnect(task=task, n_iters=10, start_state_pos=start, goal_state_pos=goal, tensor_args=ta, n_pre_samples=64)):
        with pytest.raises(NotImplementedError, match='self_field'):
            call()
    assert PlanningTask(robot, field, tensor_args=ta).compute_fraction_free_trajs(trajs) >= 0.0
