"""GPU: StochGPMP at planner sizes against the oracle's fp64 restatement (oracle/planners_ref.py).

The device path has three stages: a GP-prior sampler (csrc/mpb_prior.hip: the dense MFMA form reads the fp32 means when
scale_tril is given and H <= 128, the chain form reads them widened to fp64), the cost kernel (csrc/mpb_stoch_gpmp.hip)
and mpb_stomp_update with Sigma == NULL.  The goldens of test_gpu_parity_gpmp2_mppi.py run them at H = 16 with one field,
P*S a multiple of 4 and one-hot weights.  The cases here reach what those do not:

  pm2d_h65       D = 2,  H = 65:  the cost kernel's second 64-waypoint chunk holds one row (lane 63 of the first chunk fetches
                                  row 64 by itself); P*S = 21 leaves dead waves in the last block of 4 samples
  panda_goals    D = 7,  H = 64:  compact grid + compile-time Panda model; 2 goals x 2 particles, goal-major goals
  panda_chained  D = 7,  H = 128: a box-only field chained behind the spheres, per-field scales; the dense sampler at its limit
  panda_crowded  D = 7,  H = 64:  200 spheres + 32 boxes, no compact grid: the exhaustive walk
  pm3d_h200      D = 3,  H = 200: the chain sampler (H > 128); four chunks, the last one ragged
  arm12          D = 12, H = 48:  d = 24 in the update
  arm8_h3        D = 8,  H = 3:   the smallest horizon the update takes

Every case runs in two regimes.  'one_hot': the goldens' sampling sigmas (1e-3, 0.5, 1e-3) at T = 1 -- the importance term
puts the costs near 1e6 and the softmax picks one sample.  'soft': sampling sigmas (0.2, 0.3, 0.2), means close to the origin
(the importance term spreads the samples' costs by about sqrt(u^T Sigma^-1 u) T) and a temperature per case, never 1 (a lost
temperature factor is invisible at T = 1): the weights carry information, and they depend on how accurate the costs are.

Bars.  Costs: |c - c_ref| <= 2e-6 |c_ref| + 3e-5 coll_ref + 1e-5 -- the golden test's relative bar (fp64 accumulation of
fp32 inputs, fp32 output) and the collision bars of test_cost_and_grad_vs_oracle (fp32 forward kinematics and SDF).  One-hot:
the argmax per particle, a particle exempt only where the oracle's two best costs lie within 4 fp32 ulps.  Soft: the
weights to rtol 2e-5, atol 1e-7.  Means: 1e-4 per waypoint (conftest.rel_err_waypoint); one-hot, on the particles whose
runner-up weight is below 1e-6 (the samples drawn here are checked to give only such particles)."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import rel_err_waypoint
from test_gpu_generic_dof import make_arm, make_field

pytestmark = pytest.mark.gpu

F64 = dict(device='cpu', dtype=torch.float64)
SIG_COST = (1e-2, 1.0, 1e-2, 1e-1)     # (start, gp, goal prior, collision): the cost sigmas of the StochGPMP goldens
SIG_ONE_HOT = (1e-3, 0.5, 1e-3)        # (start, gp, goal) sampling sigmas of the goldens
SIG_SOFT = (0.2, 0.3, 0.2)
STEP = 0.5
REGIMES = ('one_hot', 'soft')
# name: H, P, S, goals, dt, half width of the box the one-hot regime's ends are drawn from, amplitude of the soft regime's
# excursion from the origin, the soft regime's temperature.  The time steps are exact in fp32 (the C ABI takes dt as a float).
# The temperatures keep the collision part of the costs (fp32 kinematics and SDF, 3e-5 of it allowed) below T: its error
# moves the weights by about that error over T
CASES = {
    'pm2d_h65': (65, 3, 7, 1, 0.09375, 0.9, 0.5, 3000.0),
    'panda_goals': (64, 4, 8, 2, 0.1875, 2.5, 1.2, 12000.0),
    'panda_chained': (128, 2, 6, 1, 0.09375, 1.5, 1.2, 12000.0),
    'panda_crowded': (64, 2, 6, 1, 0.09375, 1.5, 0.5, 12000.0),
    'pm3d_h200': (200, 2, 5, 1, 0.03125, 0.9, 0.5, 8000.0),
    'arm12': (48, 2, 5, 1, 0.125, 1.5, 0.5, 40000.0),
    'arm8_h3': (3, 3, 4, 1, 2.0, 1.5, 0.3, 8000.0),
}


def _box_field(seed, n=16, margin=0.03):
    from motion_planning_baselines_amd import geometry as G
    rng = np.random.RandomState(seed)
    boxes = np.concatenate([rng.uniform(-0.8, 0.8, (n, 3)), rng.uniform(0.05, 0.15, (n, 3))], 1)
    return G.CollisionField(boxes=boxes.astype(np.float32), margin=margin)


def _scene(name):
    """(robot, fields, per-field scales)"""
    from motion_planning_baselines_amd import geometry as G
    if name == 'pm2d_h65':
        return G.RobotPointMass(2, radius=0.01), [G.env_dense_2d(seed=3)], [1.0]
    if name == 'panda_goals':
        return G.RobotPanda(), [G.env_spheres_3d(seed=0)], [1.0]
    if name == 'panda_chained':
        return G.RobotPanda(), [G.env_spheres_3d(seed=0), _box_field(5)], [1.0, 0.6]
    if name == 'panda_crowded':
        return G.RobotPanda(), [G.env_spheres_boxes_3d(seed=0)], [1.0]
    if name == 'pm3d_h200':
        return G.RobotPointMass(3, radius=0.02), [_box_field(7, n=24)], [1.0]
    return make_arm(12 if name == 'arm12' else 8), [make_field()], [1.0]


def _lines(a, b, H, dt):
    """(P,D) ends -> (P,H,2D) straight lines with their constant velocity"""
    tau = torch.linspace(0, 1, H, dtype=torch.float64).reshape(1, H, 1)
    pos = a[:, None] * (1 - tau) + b[:, None] * tau
    return torch.cat([pos, ((b - a) / ((H - 1) * dt))[:, None].expand_as(pos)], -1)


def _bump(amp, H, dt):
    """(P,D) amplitudes -> (P,H,2D): amp sin^2(pi tau) and its time derivative (zero at both ends)"""
    tau = torch.linspace(0, 1, H, dtype=torch.float64).reshape(1, H, 1)
    pos = amp[:, None] * torch.sin(math.pi * tau) ** 2
    return torch.cat([pos, amp[:, None] * math.pi * torch.sin(2 * math.pi * tau) / ((H - 1) * dt)], -1)


@functools.lru_cache(maxsize=None)
def _case(name):
    """Scene, oracle geometry and, per regime: means (P,H,2D), per-particle starts (P,2D), goal-major goals (n_goals,2D),
    sampling sigmas and temperature.  Every number is an fp32 value held in fp64."""
    from oracle.geometry_ref import make_ref_geometry
    H, P, S, n_goals, dt, span, amp, T_soft = CASES[name]
    robot, fields, scales = _scene(name)
    D = robot.q_dim
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    rnd = lambda *shape: 2.0 * torch.rand(*shape, generator=gen, dtype=torch.float64) - 1.0
    f32 = lambda t: t.float().double()
    state = lambda q: torch.cat([q, torch.zeros_like(q)], -1)
    npg = P // n_goals
    regimes = {}
    for regime in REGIMES:
        if regime == 'one_hot':     # straight lines between far-apart ends through the scene, a little noise
            a, g = span * rnd(P, D), span * rnd(n_goals, D)
            m = _lines(a, g.repeat_interleave(npg, 0), H, dt)
            m[:, 1:-1, :D] += 0.02 * torch.randn(P, H - 2, D, generator=gen, dtype=torch.float64)
            sig, T = SIG_ONE_HOT, 1.0
        else:                       # ends near the origin and a smooth excursion: u^T Sigma^-1 u stays of order 1
            a, g = 0.1 * rnd(P, D), 0.1 * rnd(n_goals, D)
            w = rnd(P, D)
            m = _lines(a, g.repeat_interleave(npg, 0), H, dt) + _bump(amp * w / w.norm(dim=1, keepdim=True), H, dt)
            sig, T = SIG_SOFT, T_soft
        regimes[regime] = (f32(m), f32(state(a)), f32(state(g)), sig, T)
    refs = [make_ref_geometry(robot, f, F64) for f in fields]
    return dict(name=name, robot=robot, fields=fields, scales=scales, refs=refs, H=H, P=P, S=S, D=D, dt=dt, npg=npg,
                regimes=regimes)


@functools.lru_cache(maxsize=None)
def _precision(H, dt, D, sig):
    from oracle import planners_ref as O
    return O.gp_prior_precision(H, dt, D, *sig)


@functools.lru_cache(maxsize=None)
def _scale_tril(H, dt, D, sig):
    from oracle import planners_ref as O
    return O.precision_to_scale_tril(_precision(H, dt, D, sig))


def _draw(case, regime, seed):
    """S samples per particle as MultivariateNormal draws them (fp64 normals through the oracle's scale_tril), in fp32"""
    means, _, _, sig, _ = case['regimes'][regime]
    P, H, dim = means.shape
    S = case['S']
    L = _scale_tril(H, case['dt'], case['D'], sig)
    eps = torch.randn(S, P, H * dim, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    x = means.reshape(1, P, H * dim) + (L @ eps.unsqueeze(-1)).squeeze(-1)
    return x.reshape(S, P, H, dim).transpose(0, 1).float().double().contiguous()


def _oracle(case, x, means, starts, goals, sig, T):
    """stoch_gpmp_iteration without its sampling step, for per-particle starts and goal-major goals: x (P,S,H,2D) samples,
    means (P,H,2D) -> costs (P,S), their collision part, weights, the new means (fp64)"""
    from oracle import planners_ref as O
    P, S, H, dim = x.shape
    D, dt = dim // 2, case['dt']
    flat = x.reshape(P * S, H, dim)
    coll = sum(sc * O.collision_cost(flat, rr, rf, SIG_COST[3]) for sc, (rr, rf) in zip(case['scales'], case['refs']))
    comp = (O.cost_gp_eval(flat, starts.repeat_interleave(S, 0), D, dt, SIG_COST[0], SIG_COST[1], F64)
            + O.cost_goal_prior_multi_eval(flat, goals, case['npg'] * S, SIG_COST[2]) + coll)
    Kinv = _precision(H, dt, D, sig)
    V, U = x.reshape(P, S, H * dim), means.reshape(P, 1, H * dim)
    costs = comp.reshape(P, S) + T * (V @ Kinv @ U.transpose(1, 2)).squeeze(2)
    w = torch.softmax(-costs / T, dim=1)
    new = means + STEP * (w.reshape(P, S, 1, 1) * (x - means.unsqueeze(1))).sum(1)
    return dict(costs=costs, coll=coll.reshape(P, S), weights=w, means=new)


def _check(case, regime, costs, weights, means, ref):
    c_ref = ref['costs']
    bar = 2e-6 * c_ref.abs() + 3e-5 * ref['coll'] + 1e-5
    err = (costs.double() - c_ref).abs()
    assert bool((err <= bar).all()), f'cost error up to {float((err / bar).max()):.3g} x its bar'
    keep = torch.ones(c_ref.shape[0], dtype=torch.bool)
    if regime == 'one_hot':
        best = c_ref.topk(2, dim=1, largest=False).values
        b32 = best[:, 0].abs().float()
        ulp = (torch.nextafter(b32, torch.full_like(b32, math.inf)) - b32).double()
        keep = best[:, 1] - best[:, 0] > 4 * ulp
        assert bool((weights.argmax(1) == ref['weights'].argmax(1))[keep].all()), (weights, ref['weights'])
        # the means only where the oracle's softmax is one-hot to 1e-6: at costs near 1e7 an fp32 ulp is 1, and at T = 1 a
        # runner-up weight w2 moves by a factor up to e^(1/2) with the rounding of the fp32 costs alone
        keep &= ref['weights'].topk(2, dim=1).values[:, 1] < 1e-6
        assert bool(keep.any())
    else:
        np.testing.assert_allclose(weights.numpy(), ref['weights'].numpy(), rtol=2e-5, atol=1e-7)
    assert rel_err_waypoint(means[keep], ref['means'][keep], n_pos=case['D']) < 1e-4


def _dev(t, dev, dtype=torch.float32):
    return t.to(device=dev, dtype=dtype).contiguous()


def _geom(case, dev):
    from motion_planning_baselines_amd import ops
    f = case['fields']
    return ops.DeviceGeometry(case['robot'], f if len(f) > 1 else f[0], dev, scales=case['scales'] if len(f) > 1 else None)


def _prior_factor(case, sig, dev, with_tril):
    from motion_planning_baselines_amd.planners.base import gp_prior_factor, gp_prior_scale_tril
    Ud, Uo = gp_prior_factor(case['H'], case['dt'], *sig)
    f64 = lambda a: _dev(torch.as_tensor(a), dev, torch.float64)
    return f64(Ud), f64(Uo), (f64(gp_prior_scale_tril(Ud, Uo)) if with_tril else None)


def _step_bufs(case, means, dev):
    P, S, H, dim = case['P'], case['S'], case['H'], 2 * case['D']
    return dict(means=_dev(means, dev), means64=torch.zeros(P, H, dim, device=dev, dtype=torch.float64),
                samples=torch.zeros(P * S, H, dim, device=dev), costs=torch.zeros(P, S, device=dev),
                weights=torch.zeros(P, S, device=dev))


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('name', list(CASES))
def test_costs_and_update_vs_oracle(gpu_device, name, regime):
    """mpb_stoch_gpmp_costs on samples drawn here, then mpb_stomp_update (Sigma = NULL) on its costs: costs, weights (argmax
    when one-hot) and the new means against the oracle."""
    from motion_planning_baselines_amd import ops
    dev = gpu_device
    case = _case(name)
    means, starts, goals, sig, T = case['regimes'][regime]
    P, S, H, dim = case['P'], case['S'], case['H'], 2 * case['D']
    x = _draw(case, regime, seed=12)
    ref = _oracle(case, x, means, starts, goals, sig, T)
    frac = float((ref['coll'] > 0).double().mean())
    assert frac >= 0.25, f'only {frac:.0%} of the samples touch an obstacle: the collision path is barely tested'
    if regime == 'soft':
        soft = float((ref['weights'].amax(1) < 0.9).double().mean())
        assert soft >= 0.5, f'the largest weight is below 0.9 for only {soft:.0%} of the particles: the case went one-hot'
    else:
        w2 = float(ref['weights'].topk(2, dim=1).values[:, 1].max())
        assert w2 < 1e-6, f'a runner-up weight of {w2:.2g}: the one-hot case is not one-hot'
    m = _dev(means, dev)
    xs = _dev(x, dev)
    costs, w = torch.zeros(P, S, device=dev), torch.zeros(P, S, device=dev)
    ops.stoch_gpmp_costs(xs.reshape(P * S, H, dim), m, _dev(starts, dev), _dev(goals.repeat_interleave(case['npg'], 0), dev),
                         _geom(case, dev), costs, S, SIG_COST, sig, case['dt'], T)
    ops.stomp_update(m, xs, costs, w, None, STEP, T)
    torch.cuda.synchronize()
    _check(case, regime, costs.cpu(), w.cpu(), m.cpu(), ref)


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('name', list(CASES))
def test_step_teacher_forced_vs_oracle(gpu_device, name, regime):
    """One mpb_stoch_gpmp_step (n_iters = 1) draws its own samples (dense sampler with scale_tril at H <= 128, chain sampler at
    H = 200); the oracle takes those samples and the means from before the step."""
    from motion_planning_baselines_amd import ops
    dev = gpu_device
    case = _case(name)
    means, starts, goals, sig, T = case['regimes'][regime]
    P, S, H, dim = case['P'], case['S'], case['H'], 2 * case['D']
    Ud, Uo, tril = _prior_factor(case, sig, dev, with_tril=H <= 128)
    b = _step_bufs(case, means, dev)
    ops.stoch_gpmp_step(b['means'], b['means64'], b['samples'], b['costs'], b['weights'], Ud, Uo, tril, _dev(starts, dev),
                        _dev(goals.repeat_interleave(case['npg'], 0), dev), _geom(case, dev), S, SIG_COST, sig, case['dt'],
                        T, STEP, n_iters=1, seed=23)
    torch.cuda.synchronize()
    x = b['samples'].cpu().double().reshape(P, S, H, dim)
    assert float((x - means.unsqueeze(1)).abs().max()) > 0
    ref = _oracle(case, x, means, starts, goals, sig, T)
    _check(case, regime, b['costs'].cpu(), b['weights'].cpu(), b['means'].cpu(), ref)


@pytest.mark.parametrize('name,sampler', [('panda_goals', 'dense'), ('panda_goals', 'chain'), ('pm3d_h200', 'scale_tril at H > 128')])
def test_step_loop_equals_single_iterations_and_three_calls(gpu_device, name, sampler):
    """mpb_stoch_gpmp_step(n_iters = 3, seed) == three calls with n_iters = 1 and seed + i == three rounds of gp_prior_sample
    (seed + i, means64 refreshed from the current means) -> stoch_gpmp_costs -> stomp_update, bit for bit: a sampler that
    reads stale means (the chain form's means64 not widened again) shows here.  At H = 200 scale_tril is handed over but
    the step's H <= 128 rule sends it to the chain sampler."""
    from motion_planning_baselines_amd import ops
    dev = gpu_device
    case = _case(name)
    means, starts, goals, sig, T = case['regimes']['soft']
    P, S, H, dim, D = case['P'], case['S'], case['H'], 2 * case['D'], case['D']
    Ud, Uo, tril = _prior_factor(case, sig, dev, with_tril=sampler != 'chain')
    st, gl, geom = _dev(starts, dev), _dev(goals.repeat_interleave(case['npg'], 0), dev), _geom(case, dev)
    step = lambda b, n, seed: ops.stoch_gpmp_step(b['means'], b['means64'], b['samples'], b['costs'], b['weights'], Ud, Uo,
                                                  tril, st, gl, geom, S, SIG_COST, sig, case['dt'], T, STEP, n_iters=n, seed=seed)
    seed = 101
    a = _step_bufs(case, means, dev)
    step(a, 3, seed)
    b = _step_bufs(case, means, dev)
    for i in range(3):
        step(b, 1, seed + i)
    c = _step_bufs(case, means, dev)
    for i in range(3):
        c['means64'].copy_(c['means'])
        ops.gp_prior_sample(c['means64'], None, Ud, Uo, S, D, seed=seed + i, scale_tril=tril, out=c['samples'])
        ops.stoch_gpmp_costs(c['samples'], c['means'], st, gl, geom, c['costs'], S, SIG_COST, sig, case['dt'], T)
        ops.stomp_update(c['means'], c['samples'].reshape(P, S, H, dim), c['costs'], c['weights'], None, STEP, T)
    torch.cuda.synchronize()
    assert not torch.equal(a['means'].cpu().double(), means)
    for k in ('means', 'samples', 'costs', 'weights'):
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(a[k], c[k]), k


@pytest.mark.parametrize('noise', ['philox', 'torch_cpu'])
def test_class_at_twelve_joints(gpu_device, noise):
    """StochGPMP on a 12-joint chain (refused by the update before): optimize(5) is finite, equals the sample_and_eval /
    _update_distribution loop bit for bit, and that loop's first iteration matches the oracle."""
    from motion_planning_baselines_amd.planners.stoch_gpmp import StochGPMP
    dev = gpu_device
    case = _case('arm12')
    means, starts, goals, sig, T = case['regimes']['soft']
    P, S, H, D = case['P'], case['S'], case['H'], case['D']
    starts = starts[:1].expand(P, -1)                  # the class has one start state
    kw = dict(robot=case['robot'], n_dof=D, n_support_points=H, num_particles_per_goal=P, opt_iters=5, dt=case['dt'],
              start_state=_dev(starts[0, :D], dev), step_size=STEP, multi_goal_states=_dev(goals[:, :D], dev),
              sigma_start_init=1e-3, sigma_goal_init=1e-3, sigma_gp_init=1.0,
              sigma_start_sample=sig[0], sigma_gp_sample=sig[1], sigma_goal_sample=sig[2], num_samples=S, temperature=T,
              collision_fields=case['fields'], sigma_start=SIG_COST[0], sigma_gp=SIG_COST[1], sigma_goal_prior=SIG_COST[2],
              sigma_coll=SIG_COST[3], tensor_args=dict(device=dev, dtype=torch.float32), noise=noise, seed=5)
    torch.manual_seed(0)
    pa = StochGPMP(initial_particle_means=_dev(means, dev), **kw)     # (each planner updates the tensor it is given)
    traj = pa.optimize(opt_iters=5)
    torch.cuda.synchronize()
    assert traj.shape == (P, H, 2 * D) and bool(torch.isfinite(traj).all())
    torch.manual_seed(0)
    pb = StochGPMP(initial_particle_means=_dev(means, dev), **kw)
    m0 = pb._particle_means.cpu().double()
    for it in range(5):
        costs, samples = pb.sample_and_eval()
        if it == 0:
            c0, x0 = costs.cpu().clone(), samples.cpu().double()
        pb._update_distribution(costs, samples)
        if it == 0:
            ref = _oracle(case, x0, m0, starts, goals, sig, T)
            _check(case, 'soft', c0, pb._weights.reshape(P, S).cpu(), pb._particle_means.cpu(), ref)
    torch.cuda.synchronize()
    assert torch.equal(pa._particle_means, pb._particle_means)
    assert torch.equal(pa.state_samples, pb.state_samples) and torch.equal(pa.costs, pb.costs)
    assert torch.equal(pa._weights, pb._weights)


@pytest.mark.parametrize('H,D', [(16, 13), (2, 4), (257, 4)])
def test_step_refuses_before_any_launch(gpu_device, H, D):
    """D = 13, H = 2 (the update takes H >= 3) and H = 257 are refused before the sampler or the cost kernel is enqueued:
    the output buffers keep their NaN sentinel and the (finite) means their bits."""
    from motion_planning_baselines_amd import geometry as G, ops
    from motion_planning_baselines_amd._lib import MPBError
    from motion_planning_baselines_amd.planners.base import gp_prior_factor, gp_prior_scale_tril
    dev = gpu_device
    P, S, dim = 2, 4, 2 * D
    nan = float('nan')
    means = torch.randn(P, H, dim, generator=torch.Generator().manual_seed(H + D)).to(dev)
    keep = means.clone()
    means64 = torch.full((P, H, dim), nan, device=dev, dtype=torch.float64)
    samples = torch.full((P * S, H, dim), nan, device=dev)
    costs, weights = torch.full((P, S), nan, device=dev), torch.full((P, S), nan, device=dev)
    Ud, Uo = gp_prior_factor(H, 0.1, *SIG_SOFT)
    f64 = lambda a: _dev(torch.as_tensor(a), dev, torch.float64)
    tril = f64(gp_prior_scale_tril(Ud, Uo)) if H <= 128 else None
    geom = ops.DeviceGeometry(G.RobotPointMass(2, radius=0.01), G.env_dense_2d(seed=3), dev)
    zeros = torch.zeros(P, dim, device=dev)
    with pytest.raises(MPBError, match='mpb_stoch_gpmp_step: bad shape'):
        ops.stoch_gpmp_step(means, means64, samples, costs, weights, f64(Ud), f64(Uo), tril, zeros, zeros, geom, S,
                            SIG_COST, SIG_SOFT, 0.1, 2.0, STEP, n_iters=1, seed=0)
    torch.cuda.synchronize()
    assert torch.equal(means, keep)
    for t in (means64, samples, costs, weights):
        assert bool(torch.isnan(t).all())


def test_costs_refuse_thirteen_joints(gpu_device):
    from motion_planning_baselines_amd import geometry as G, ops
    from motion_planning_baselines_amd._lib import MPBError
    dev = gpu_device
    P, S, H, dim = 2, 4, 16, 26
    samples = torch.randn(P * S, H, dim, generator=torch.Generator().manual_seed(1)).to(dev)
    means = samples[::S].clone()
    costs = torch.full((P, S), float('nan'), device=dev)
    geom = ops.DeviceGeometry(G.RobotPointMass(2, radius=0.01), G.env_dense_2d(seed=3), dev)
    zeros = torch.zeros(P, dim, device=dev)
    with pytest.raises(MPBError, match='mpb_stoch_gpmp_costs: bad shape'):
        ops.stoch_gpmp_costs(samples, means, zeros, zeros, geom, costs, S, SIG_COST, SIG_SOFT, 0.1, 2.0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(costs).all())


@pytest.mark.parametrize('H,D,what', [(2, 4, 'n_support_points'), (257, 4, 'n_support_points'), (16, 13, 'n_dof')])
def test_class_refuses_out_of_envelope_shapes(gpu_device, H, D, what):
    """The constructor names the limit before it builds any device state."""
    from motion_planning_baselines_amd import geometry as G
    from motion_planning_baselines_amd.planners.stoch_gpmp import StochGPMP
    dev = gpu_device
    with pytest.raises(ValueError, match=what):
        StochGPMP(robot=G.RobotPointMass(2, radius=0.01), n_dof=D, n_support_points=H, num_particles_per_goal=2, opt_iters=1,
                  dt=0.1, start_state=torch.zeros(D, device=dev), multi_goal_states=torch.ones(1, D, device=dev),
                  sigma_start_init=1e-3, sigma_goal_init=1e-3, sigma_gp_init=1.0, sigma_start_sample=0.2,
                  sigma_gp_sample=0.3, sigma_goal_sample=0.2, num_samples=4, collision_fields=[G.env_dense_2d(seed=3)],
                  tensor_args=dict(device=dev, dtype=torch.float32), noise='philox')
