"""GPU: ONE CHOMP step of every kernel and loop form of csrc/mpb_chomp.hip against the fp64 oracle, element by element.

The CHOMP tests on the fused kernels compare iterates by a global relative error at the reference's parameters, where the clamp hides
most elements' magnitude.  Here tests/chomp_step_checks.py decides from the oracle ALONE what every element of one step owes:

    e = |x1 - x1_fp64| / unit   <=   4 * max(E32, 2^-23)          (K.bar; unit and E32: the helper's docstring)

on every interior element of every conditioned waypoint, none left out; an element whose unit is 0 (rows 0 and H-1, the velocity
channels of a collision-only step) keeps the bits of x0; a decided clamped element is  x0 -+ lr * clip  bit for bit; costs_out is the
scaled collision cost of the iterate BEFORE the last update (include/mpb.h).  Iterates are compared, never a gradient recovered by
dividing a difference; one iteration per comparison; lr = 2^-3.

One case per kernel path, asserted from geom_flags and the packed header (C.kernel_of): chomp_point4_kernel (partially filled quad
slots, 3-D, the largest block), chomp_lean_kernel, chomp_kernel<0> modes 0 / 1 / 2, chomp_kernel<Panda> modes 1 / 2; then the clamp, a
shard (B_global = 3 B), three fused iterations against three single ones, the quad's tie conventions, and the composite route
cost_terms_grad(apply=True), which runs the same prior, clamp, mask and step.  tests/test_chomp_step_cpu.py holds the conditions
(exclusion share, undecided share, E32) on the CPU."""
import types

import numpy as np
import pytest
import torch

import chomp_step_checks as C
import collision_kinks as K

pytestmark = pytest.mark.gpu
NAN = float('nan')


def _geom(case, dev):
    """The case's DeviceGeometry, on the kernel path the case names."""
    from motion_planning_baselines_amd import geometry as G
    from test_gpu_collision_grad_elements import make_geom
    _, name, kw, H, _, path, clear_small = C.CASE[case]
    bs = C.base(name, H)
    geom = make_geom(bs, dev, **kw)
    if clear_small:
        assert geom.flags & G.GEOM_FLAG_POINT_SMALL
        geom.flags &= ~G.GEOM_FLAG_POINT_SMALL
    assert C.kernel_of(geom, H, bs.robot.q_dim) == path, C.kernel_of(geom, H, bs.robot.q_dim)
    return geom


def _step(ref, geom, dev, x=None, n_iters=1):
    """ops.chomp_step on a copy of x (default: the case's x0) -> (means, costs_out), both on the CPU."""
    from motion_planning_baselines_amd import ops
    m = (ref.x0 if x is None else x).to(dev).clone()
    costs = torch.full((K.B,), NAN, device=dev)
    ops.chomp_step(m, ref.R.to(dev), geom, ref.D, C.K_SIGMA, ref.weight, ref.w_prior, C.LR, ref.grad_clip, n_iters=n_iters,
                   B_global=ref.B_global, costs_out=costs)
    torch.cuda.synchronize()
    return m.cpu(), costs.cpu()


def _judge(tag, ref, x1):
    e = C.error(ref, x1)
    worst = float(e[ref.judged].max())
    share = getattr(getattr(ref, 'base', None), 'share', 0.0)
    print(f'{tag}: judged {int(ref.judged.sum())} of {int(ref.interior.sum())} interior elements ({share * 100:.2f} % of the waypoints '
          f'in contact excluded, {ref.undecided_share * 100:.3f} % of the elements undecided), worst e {worst:.3e} against E32 '
          f'{ref.E32:.3e} (bar {K.bar(ref.E32):.3e})')
    assert x1.shape == ref.x0.shape and torch.isfinite(x1).all()
    assert int(ref.zero.sum()) > 0 and C.same_bits(x1[ref.zero], ref.x0[ref.zero])         # incl. rows 0 and H-1
    assert C.same_bits(x1[:, 0], ref.x0[:, 0]) and C.same_bits(x1[:, -1], ref.x0[:, -1])
    if ref.clamped is not None:
        n_bad = int((x1[ref.clamped].view(torch.int32) != ref.want_clamped[ref.clamped].view(torch.int32)).sum())
        print(f'    {int(ref.clamped.sum())} decided clamped elements, {n_bad} of them not x0 -+ lr * clip')
        assert int(ref.clamped.sum()) > 100 and n_bad == 0
    assert int(ref.judged.sum()) > 100
    assert worst <= K.bar(ref.E32), (worst, ref.E32)
    return worst


def _judge_costs(tag, ref, costs):
    assert torch.isfinite(costs).all()
    if ref.weight == 0.0:
        assert bool((costs == 0).all())
        return
    n_ok = int(ref.cost_ok.sum())
    worst = float(((costs.double() - ref.c64).abs() / ref.cost_den)[ref.cost_ok].max())
    print(f'    costs_out: {n_ok} of {K.B} particles judged, worst e {worst:.3e} against E32 {ref.cost_E32:.3e} (bar {K.bar(ref.cost_E32):.3e})')
    assert n_ok >= 5 and float(ref.c64[ref.cost_ok].max()) > 0
    assert worst <= K.bar(ref.cost_E32), (worst, ref.cost_E32)


# ------------------------------------------------------------------------------------------------
# 1 + 4a.  one unclipped step per kernel path: collision only, prior only, both; costs_out against the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', C.FAMILIES)
@pytest.mark.parametrize('case', [c[0] for c in C.STEP_CASES])
def test_one_step_every_element(gpu_device, case, family):
    from motion_planning_baselines_amd import geometry as G
    _, name, kw, H, dmul, path, _ = C.CASE[case]
    ref = C.reference(name, H, dmul, family)
    geom = _geom(case, gpu_device)
    x1, costs = _step(ref, geom, gpu_device)
    tag = f'chomp step {case} {kw} H={H} d={ref.d} {family} [{path}]'
    _judge(tag, ref, x1)
    _judge_costs(tag, ref, costs)
    assert not torch.equal(x1[:, 1:-1, :ref.D], ref.x0[:, 1:-1, :ref.D])
    if name in C.NEW_SCENES:        # the quad kernel == the one-lane kernel, with partially filled slots and in 3-D
        assert geom.flags & G.GEOM_FLAG_POINT_SMALL
        geom.flags &= ~G.GEOM_FLAG_POINT_SMALL
        assert C.kernel_of(geom, H, ref.D) == 'lean'
        y1, costs_lean = _step(ref, geom, gpu_device)
        assert C.same_bits(x1, y1) and C.same_bits(costs, costs_lean)


# ------------------------------------------------------------------------------------------------
# 2.  the clamp: decided clamped elements exact, decided unclamped ones to the bar
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', C.CLIPPED)
def test_clipped_step(gpu_device, case):
    _, name, kw, H, dmul, path, _ = C.CASE[case]
    clip = C.pick_clip(name, H, dmul)
    ref = C.reference(name, H, dmul, 'both', clip)
    assert ref.undecided_share <= C.UNDECIDED_CAP
    x1, costs = _step(ref, _geom(case, gpu_device), gpu_device)
    tag = f'chomp clipped step {case} H={H} d={ref.d} clip={clip} ({ref.clamped_share * 100:.1f} % clamped) [{path}]'
    _judge(tag, ref, x1)
    _judge_costs(tag, ref, costs)
    # no element, judged or not, moves further than the clamp allows (x1 is rounded once: half an ulp of it)
    assert bool(((x1.double() - ref.x0.double()).abs() <= C.LR * clip + 2.0 ** -24 * x1.double().abs()).all())


# ------------------------------------------------------------------------------------------------
# 3.  a shard: B_global = 3 B scales the prior alone
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', C.SHARDED)
def test_shard_step(gpu_device, case):
    _, name, kw, H, dmul, path, _ = C.CASE[case]
    ref = C.reference(name, H, dmul, 'both', None, C.SHARD)
    assert ref.B_global == C.SHARD * K.B
    x1, costs = _step(ref, _geom(case, gpu_device), gpu_device)
    tag = f'chomp shard step {case} H={H} d={ref.d} B_global={ref.B_global} [{path}]'
    _judge(tag, ref, x1)
    _judge_costs(tag, ref, costs)


# ------------------------------------------------------------------------------------------------
# 4b.  three fused iterations == three single ones; costs_out is the third one's: the iterate before the last update
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', C.FUSED)
def test_fused_three_equals_three_steps(gpu_device, case):
    _, name, kw, H, dmul, path, _ = C.CASE[case]
    ref = types.SimpleNamespace(**vars(C.reference(name, H, dmul, 'both')))
    ref.grad_clip = 1.0                  # no element moves more than lr per step: four steps stay inside the joint range
    geom = _geom(case, gpu_device)
    fused, costs_fused = _step(ref, geom, gpu_device, n_iters=3)
    x, costs = ref.x0, []
    for _ in range(4):
        x_prev = x
        x, c = _step(ref, geom, gpu_device, x=x)
        costs.append(c)
    assert torch.isfinite(fused).all() and torch.isfinite(costs_fused).all()
    assert C.same_bits(fused, x_prev)
    assert C.same_bits(costs_fused, costs[2])
    assert not torch.equal(costs[2], costs[1]) and not torch.equal(costs[2], costs[3])      # neither one update early nor one late


# ------------------------------------------------------------------------------------------------
# 5.  the quad kernel's tie conventions: lowest obstacle index wins, in a lane, between neighbouring lanes, across both exchanges
# ------------------------------------------------------------------------------------------------
def _tie_cases():
    from test_gpu_collision_grad_elements import CONVENTIONS, _fillers
    out = dict(CONVENTIONS)
    for i, j in ((0, 1), (0, 4), (1, 6), (3, 4)):          # lanes (0, 1): first exchange; (0, 0): one lane; (1, 2), (3, 0): second
        for sign in (-1.0, 1.0):                           # the lower index sits at sign * 0.5: d cost / d x points at it
            sph = _fillers(j + 1)
            sph[i] = [sign * 0.5, 0, 0, 0.25]
            sph[j] = [-sign * 0.5, 0, 0, 0.25]
            out[f'pair_{i}_{j}_{"neg" if sign < 0 else "pos"}'] = (sph.tolist(), None, [[0, 0, 0], [0, 0.125, 0]], [[sign, 0, 0], None])
    return out


TIES = _tie_cases()


@pytest.mark.parametrize('case', list(TIES))
def test_quad_tie_conventions(gpu_device, case):
    from motion_planning_baselines_amd import geometry as G, ops
    from oracle.geometry_ref import make_ref_geometry
    spheres, boxes, points, expect = TIES[case]
    robot = G.RobotPointMass(3, radius=0.25, q_limits=(-1.0, 1.0))
    field = G.CollisionField(spheres=None if spheres is None else np.asarray(spheres, np.float32),
                             boxes=None if boxes is None else np.asarray(boxes, np.float32), margin=0.25)
    geom = ops.DeviceGeometry(robot, field, gpu_device)
    P = len(points)
    H = P + 2
    assert C.kernel_of(geom, H, 3) == 'point4'
    x0 = torch.tensor([[[0.875, 0.875, 0.875]] + points + [[0.875, 0.875, 0.875]]], dtype=torch.float32)      # (1, H, 3)
    rr, rf = make_ref_geometry(robot, field)
    xg = x0.clone().requires_grad_(True)
    cost = rf.compute_cost(xg, rr.fk_map_collision(xg))
    want, = torch.autograd.grad(cost.sum(), xg)
    assert bool((cost[0, 1:-1] > 0).all())
    runs = []
    for lean in (False, True):
        if lean:
            geom.flags &= ~G.GEOM_FLAG_POINT_SMALL
            assert C.kernel_of(geom, H, 3) == 'lean'
        m = x0.to(gpu_device).clone()
        ops.chomp_step(m, C.precision(H).to(gpu_device), geom, 3, 1.0, 1.0, 0.0, C.LR, C.NO_CLIP, n_iters=1)
        torch.cuda.synchronize()
        runs.append(m.cpu())
    x1 = runs[0]
    step = (x1 - x0)[0, 1:-1]                                            # exact: both are small multiples of a power of two, or close
    print(f'{case}: step / -lr {(step / -C.LR).tolist()} oracle {want[0, 1:-1].tolist()}')
    assert torch.isfinite(x1).all() and C.same_bits(x1[:, 0], x0[:, 0]) and C.same_bits(x1[:, -1], x0[:, -1])
    for p, e in enumerate(expect):
        if e is not None:               # decided by the convention alone: exact, on both sides
            assert step[p].tolist() == [-C.LR * float(v) for v in e], (case, p, step[p])
            assert want[0, p + 1].tolist() == [float(v) for v in e], (case, p, want[0, p + 1])
        else:                           # a generic direction on the chosen obstacle: the gradient to rounding, x1 (< 0.25) rounded once
            assert float((step[p] + C.LR * want[0, p + 1]).abs().max()) <= C.LR * K.FACTOR * K.ULP + 2.0 ** -27, (case, p, step[p])
            assert float(step[p, 0]) * float(want[0, p + 1, 0]) < 0
    assert C.same_bits(runs[0], runs[1])


# ------------------------------------------------------------------------------------------------
# 6.  the composite route: cost_terms_grad(apply=True) with a given incoming gradient and no cost term
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,dmul,clipped', C.COMPOSITE_CASES)
def test_composite_apply(gpu_device, H, dmul, clipped):
    from motion_planning_baselines_amd import ops
    ref = C.composite_reference(H, dmul, clipped)
    assert ref.undecided_share <= C.UNDECIDED_CAP
    x = ref.x0.to(gpu_device).clone()
    ops.cost_terms_grad(x, ref.D, grad_in=ref.grad_in.to(gpu_device), apply=True, R=ref.R.to(gpu_device), prior_bw=ref.prior_bw,
                        lr=C.LR, grad_clip=ref.grad_clip, terms=())
    torch.cuda.synchronize()
    _judge(f'cost_terms_grad apply H={H} d={ref.d} clip={ref.grad_clip}', ref, x.cpu())
