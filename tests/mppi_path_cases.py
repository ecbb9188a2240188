"""The shapes, inputs and oracle runs that put every launch path of mpb_mppi_step under the oracle (helper module; imported
like collision_kinks.py).  tests/test_host_logic.py pins the launcher's plan of every shape here (CPU, n_cu = 256);
tests/test_gpu_mppi_paths.py asserts the plan again on the device and then runs the shape.

The inputs keep the softmax SPREAD: at temp 300 (costs of a few hundred, differences of tens to hundreds) the effective sample
size 1 / sum(w^2) stays above 2.5, so that a wrong weight on any sample, or a sample missing from the update's sums, moves
the mean -- tests/test_gpu_edge_cases.py::test_mppi_shapes_vs_oracle runs at temp 0.7, where one sample holds all the weight.
Nothing here looks at the code under test: the conditions on the inputs are asserted on the oracle alone (check_conditions)."""
import collections
import functools
import types

import torch

NOISE_GLOBAL, NOISE_LDS, NOISE_MATRIX = 0, 1, 2
MODE_NAME = {NOISE_GLOBAL: 'GLOBAL', NOISE_LDS: 'LDS', NOISE_MATRIX: 'MATRIX'}
Case = collections.namedtuple('Case', 'NP S T c scene mode waves grid_words lds_bytes what')
Plan = collections.namedtuple('Plan', 'mode waves grid_words lds_bytes')

# mpb_mppi_plan at n_cu = 256 (noise mode, waves, grid words, LDS bytes).  A retuned launcher fails test_host_logic's plan table, and
# with it says which of the cases below no longer reaches the path it is here for.
CASES = {
    'a': Case(2, 12, 65, 1, None, NOISE_LDS, 12, 0, 24264, 'one lane in chunk 2, remainder loop (kend 65), c = 1, waves = S'),
    'b': Case(2, 9, 67, 4, None, NOISE_LDS, 9, 0, 93808, 'c = 4, T % 4 = 3, waves = 9'),
    'c': Case(2, 37, 72, 3, 'spheres3d', NOISE_LDS, 16, 4096, 128480, '3-D point on the grid (z_on), S % 16 != 0, collision in chunk 2'),
    'c2': Case(2, 37, 72, 3, 'spheres3d_80', NOISE_LDS, 16, 0, 111056, '3-D point, exhaustive walk (80 spheres: no compact grid), chunk 2'),
    'd': Case(2, 20, 96, 2, 'circles2d', NOISE_LDS, 16, 1089, 109136, 'grid staged behind the transposed factor, chunk 2'),
    'e': Case(1, 20, 200, 2, 'circles2d', NOISE_GLOBAL, 16, 1089, 67024, 'grid with nothing in front of it, four chunks'),
    'f': Case(2, 120, 64, 2, 'dense2d', NOISE_LDS, 16, 1677, 114800, 'T = 64 on the per-lane product, S > 64 block softmax, boxes'),
    'g': Case(2, 130, 48, 2, None, NOISE_LDS, 16, 0, 79184, 'T < 64 on the per-lane product: ragged lanes, S > 64'),
    'h': Case(2, 18, 50, 3, None, NOISE_MATRIX, 16, 0, 88072, 'device draw: G4 = 13 (g4 >= G4 guard), T % 4 = 2, S % 16 = 2'),
    'i1': Case(3, 5, 48, 2, 'dense2d', NOISE_MATRIX, 5, 1677, 52368, 'device draw, S < 16, T < 64'),
    'i2': Case(2, 33, 64, 2, 'dense2d', NOISE_MATRIX, 16, 1677, 85792, 'device draw, S % 16 = 1'),
}

# the shapes the suite ran before this module, with the path each takes (tests/test_gpu_edge_cases.py::test_mppi_shapes_vs_oracle,
# _MPPI_WAVES_CHILD, the goldens and bench.py's `mppi` entry): NP, S, T, c, scene -> plan
EARLIER = [
    ((3, 5, 48, 2, 'dense2d'), Plan(NOISE_MATRIX, 5, 1677, 52368)),
    ((2, 33, 64, 2, 'dense2d'), Plan(NOISE_MATRIX, 16, 1677, 85792)),
    ((2, 100, 100, 3, None), Plan(NOISE_GLOBAL, 16, 0, 144656)),
    ((1, 20, 200, 2, None), Plan(NOISE_GLOBAL, 16, 0, 61616)),
    ((4, 16, 64, 1, None), Plan(NOISE_MATRIX, 16, 0, 26064)),
    ((2, 24, 96, 4, None), Plan(NOISE_GLOBAL, 16, 0, 65440)),
    ((2, 1, 64, 2, 'dense2d'), Plan(NOISE_MATRIX, 1, 1677, 51104)),
    ((3, 2, 64, 2, 'dense2d'), Plan(NOISE_MATRIX, 2, 1677, 51632)),
    ((3, 40, 64, 2, 'circles2d_r01'), Plan(NOISE_MATRIX, 16, 1089, 87184)),       # _MPPI_WAVES_CHILD
    ((1, 32, 64, 2, 'circles2d_r01'), Plan(NOISE_MATRIX, 16, 1089, 74160)),       # the goldens (one problem)
    ((64, 32, 64, 2, 'circles2d_r01'), Plan(NOISE_MATRIX, 16, 1089, 74160)),      # test_mppi_device_noise_is_the_injected_path
    ((1024, 32, 64, 2, 'circles2d_r01'), Plan(NOISE_MATRIX, 8, 1089, 74160)),     # bench.py's `mppi` entry: two workgroups per CU
]

DT, TEMP, STEP, K_SIGMA, WEIGHT = 0.05, 300.0, 0.1, 4.0, 1.5
CW = dict(pos=1.0, vel=0.5, ctrl=0.1, pos_T=20.0)
N_IT = 2
SEED, ITER0 = 11, 5                  # of the device draw
F32 = dict(device='cpu', dtype=torch.float32)
F64 = dict(device='cpu', dtype=torch.float64)
ULP = 2.0 ** -23
FLOOR_ULPS = 4.0                     # "a few fp32 ulps of the quantity's largest magnitude in that problem"
FACTOR = 4.0                         # tests/collision_kinks.py's, for its reasons: association (MFMA tiles / DPP trees against a
#                                      sequential chain), v_exp / v_rcp at 1-2 ulp; and a factor two above that
MIN_ESS = 2.5


def scene(name):
    """name -> (product robot, product CollisionField) or (None, None)"""
    from motion_planning_baselines_amd import geometry as G
    if name is None:
        return None, None
    # (3-D: a robot radius that bridges the gaps of the sphere cloud -- with 0.05 the rollouts, which drift up to 2 m in 72 steps,
    # meet nothing beyond step 64; 80 spheres are beyond the compact broad-phase grid's 63: the launcher walks them all)
    if name == 'spheres3d':
        return G.RobotPointMass(3, radius=0.5), G.env_spheres_3d(seed=2)
    if name == 'spheres3d_80':
        return G.RobotPointMass(3, radius=0.5), G.env_spheres_3d(seed=2, n_spheres=80)
    if name == 'circles2d':
        return G.RobotPointMass(2, radius=0.02), G.env_grid_circles_2d()
    if name == 'circles2d_r01':
        return G.RobotPointMass(2, radius=0.01), G.env_grid_circles_2d()
    if name == 'dense2d':
        return G.RobotPointMass(2, radius=0.02), G.env_dense_2d()
    raise KeyError(name)


def scene_flags(name):
    """(mpb_geom_flags of the packed scene, has_geom): what mpb_mppi_plan takes, without a device"""
    from motion_planning_baselines_amd import _lib, geometry as G
    robot, field = scene(name)
    return (0, False) if robot is None else (_lib.geom_flags(G.pack_geometry(robot, field)), True)


@functools.lru_cache(maxsize=None)
def problem(name, NP=None):
    """The fp32 inputs of a case (NP: another number of problems of the same shape -- drawn from the same generator, so the
    first problems are NOT the case's own).  Treat as read-only."""
    from oracle import planners_ref as O
    from oracle.geometry_ref import make_ref_geometry
    cs = CASES[name]
    NP = cs.NP if NP is None else NP
    S, T, c = cs.S, cs.T, cs.c
    gen = torch.Generator().manual_seed(NP * 1000 + S + T + c)
    Cov = O.mppi_covariance([0.3 + 0.05 * i for i in range(c)], T, c, 'const_ctrl', F32) + 0.2 * torch.eye(T).unsqueeze(-1)
    tril = torch.stack([torch.linalg.cholesky(Cov[..., i]) for i in range(c)]).contiguous()
    cinv = torch.stack([torch.inverse(Cov[..., i]) for i in range(c)]).contiguous()
    mean0 = 0.02 * torch.randn(NP, T, c, generator=gen)
    if cs.c == 3 and cs.scene is not None:      # start and goal inside the sphere cloud
        state0 = 0.3 * torch.randn(NP, c, generator=gen)
        goal = 0.3 * torch.randn(NP, c, generator=gen)
    else:
        state0 = 0.5 * torch.randn(NP, c, generator=gen)
        goal = 0.5 * torch.randn(NP, c, generator=gen)
    robot, field = scene(cs.scene)
    geo = {}
    if robot is not None:
        geo = {torch.float32: make_ref_geometry(robot, field, F32), torch.float64: make_ref_geometry(robot, field, F64)}
    return types.SimpleNamespace(name=name, NP=NP, S=S, T=T, c=c, tril=tril, cinv=cinv, mean0=mean0, state0=state0, goal=goal,
                                 cmin=torch.full((c,), -0.6), cmax=torch.full((c,), 0.5),
                                 disc=0.99 ** torch.arange(T, dtype=torch.float32), robot=robot, field=field, geo=geo)


def oracle_run(pr, eps, dtype, n_it=N_IT):
    """oracle.planners_ref.mppi_iteration over n_it iterations of every problem in `dtype`, the Q6 shift formed as
    test_mppi_shapes_vs_oracle forms it.  eps (n_it, NP, c, S, T).  Per problem a namespace: the last iteration's controls,
    states, costs (S), weights (S); mean after n_it; per iteration ess, weights, late (collision cost summed over steps
    t >= 64 of all samples); best_cost, best_states as MPPI._save_best keeps them."""
    from oracle import planners_ref as O
    f = lambda t: t.to(dtype)
    tril, cinv, cmin, cmax, disc = f(pr.tril), f(pr.cinv), f(pr.cmin), f(pr.cmax), f(pr.disc)
    out = []
    for p in range(pr.NP):
        m, s0, gl = f(pr.mean0[p]), f(pr.state0[p]), f(pr.goal[p])
        r = types.SimpleNamespace(ess=[], weights_it=[], late=[], best_cost=float('inf'), best_states=None)
        for it in range(n_it):
            e = f(eps[it, p])
            shift = 0.0
            if pr.geo:
                rr, rf = pr.geo[dtype]
                pre = O.mppi_iteration(m, e, tril, cinv, s0, gl, DT, cmin, cmax, CW, disc, TEMP, STEP, pr.c)
                q = pre['states'][:, 1:, :pr.c]
                per_step = rf.compute_cost(q, rr.fk_map_collision(q))            # (S, T - 1): steps 1 .. T - 1
                shift = WEIGHT * K_SIGMA * float(per_step.sum())
                r.late.append(float(per_step[:, 63:].sum()))
            o = O.mppi_iteration(m, e, tril, cinv, s0, gl, DT, cmin, cmax, CW, disc, TEMP, STEP, pr.c, shift_cost=shift)
            m = o['mean']
            w = o['weights'].reshape(-1)
            r.ess.append(1.0 / float((w.double() ** 2).sum()))
            r.weights_it.append(w)
            cst = o['costs'].reshape(-1)
            if float(cst.min()) < r.best_cost:
                r.best_cost, r.best_states = float(cst.min()), o['states'][int(cst.argmin())]
        r.controls, r.states, r.costs, r.weights, r.mean = o['controls'], o['states'], cst, w, m
        out.append(r)
    return out


def check_conditions(name, pr, ref64):
    """The conditions on the inputs, on the fp64 oracle alone."""
    cs = CASES[name]
    for p, r in enumerate(ref64):
        tag = (name, p)
        if cs.S >= 5:
            assert min(r.ess) >= MIN_ESS, (tag, 'effective sample size', r.ess)
        if cs.S > 64:       # some sample the S > 64 softmax / update could lose carries weight
            for w in r.weights_it:
                assert float(w[64:].max()) >= 1e-3 * float(w.max()), (tag, 'no weight beyond sample 64')
        if cs.scene is not None and cs.T > 64:
            assert min(r.late) > 0.0, (tag, 'no collision cost beyond the first 64 steps', r.late)
        u = r.controls
        outside = (u < pr.cmin.double()) | (u > pr.cmax.double())
        assert bool(outside.any()) and not bool(outside.all()), (tag, 'clamping not active')


QUANTITIES = ('controls', 'states', 'costs', 'weights', 'mean')


def bars(ref32, ref64):
    """Per problem {quantity: (E32, bar)}: E32 the fp32 oracle's own deviation from the fp64 oracle (max abs over the problem),
    the floor FLOOR_ULPS fp32 ulps of the quantity's largest magnitude in the problem, bar = FACTOR * max(E32, floor)."""
    out = []
    for a, b in zip(ref32, ref64):
        d = {}
        for k in QUANTITIES:
            x32, x64 = getattr(a, k).double(), getattr(b, k)
            e32 = float((x32 - x64).abs().max())
            floor = FLOOR_ULPS * ULP * float(x64.abs().max())
            d[k] = (e32, FACTOR * max(e32, floor))
        out.append(d)
    return out


# ------------------------------------------------------------------------------------------------
# the device side (tests/test_gpu_mppi_paths.py and its child processes)
# ------------------------------------------------------------------------------------------------
OUTPUTS = ('mean', 'controls', 'states', 'costs', 'weights', 'best_cost', 'best_states')


def device_geometry(pr, dev):
    from motion_planning_baselines_amd import ops
    return None if pr.robot is None else ops.DeviceGeometry(pr.robot, pr.field, dev)


def device_plan(name, pr, geom, has_eps):
    """mpb_mppi_plan for the device the test runs on, held to the case's pinned path; returns the line a test prints"""
    from motion_planning_baselines_amd import ops
    cs = CASES[name]
    pl = ops.mppi_plan(geom, pr.NP, pr.S, pr.T, pr.c, has_eps=has_eps)
    assert (pl.noise_mode, pl.grid_words) == (cs.mode, cs.grid_words), (name, 'takes another path on this device', pl)
    assert pl.waves == cs.waves or pr.NP != cs.NP, (name, pl)
    return 'case %s NP=%d S=%d T=%d c=%d scene=%s: plan %s, %d waves, grid_words %d, LDS %d B, %s normals' % (
        name, pr.NP, pr.S, pr.T, pr.c, cs.scene, MODE_NAME[pl.noise_mode], pl.waves, pl.grid_words, pl.lds_bytes,
        'injected' if has_eps else 'drawn')


def launch(pr, geom, dev, eps, n_iters=N_IT, iter0=ITER0, mean=None, best=None, problems=None):
    """One mppi_step launch on the inputs of `pr` (problems: a slice of them) tracking the best sample; eps (n_iters, NP, c, S, T) on
    the device, or None: drawn with SEED.  mean / best = (best_cost, best_states): carried over from an earlier launch.
    Returns {name: tensor} of OUTPUTS after a synchronize."""
    from motion_planning_baselines_amd import ops
    sl = slice(0, pr.NP) if problems is None else problems
    f = lambda t: t.contiguous().to(dev)
    NP = len(range(*sl.indices(pr.NP)))
    o = dict(mean=f(pr.mean0[sl]) if mean is None else mean.clone(),
             controls=torch.empty(NP, pr.S, pr.T, pr.c, device=dev), states=torch.empty(NP, pr.S, pr.T, pr.c, device=dev),
             costs=torch.empty(NP, pr.S, device=dev), weights=torch.empty(NP, pr.S, device=dev),
             best_cost=torch.full((NP,), 3.0e38, device=dev) if best is None else best[0].clone(),
             best_states=torch.zeros(NP, pr.T, pr.c, device=dev) if best is None else best[1].clone())
    ops.mppi_step(o['mean'], eps, f(pr.tril), f(pr.cinv), f(pr.state0[sl]), f(pr.goal[sl]), f(pr.cmin), f(pr.cmax), f(pr.disc),
                  f(torch.tensor([CW['pos'], CW['vel'], CW['ctrl'], CW['pos_T']])), geom, o['controls'], o['states'], o['costs'],
                  o['weights'], DT, k_sigma=K_SIGMA, weight=WEIGHT, temp=TEMP, step_size=STEP, n_iters=n_iters, seed=SEED, iter0=iter0,
                  best_cost=o['best_cost'], best_states=o['best_states'])
    torch.cuda.synchronize()
    return o
