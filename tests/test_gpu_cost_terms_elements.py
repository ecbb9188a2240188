"""GPU: mpb_cost_terms_eval / mpb_cost_terms_grad and the trajectory utilities of csrc/mpb_costs.hip against the fp64 oracle, element
by element (tests/cost_terms_checks.py holds the cases, the closed form, the units and the bars; tests/test_cost_terms_cpu.py their
conditions).

    gradient   |g - g64| <= 2^-24 |g64| + 2^-44 unit  [+ the fp32 V tile's term under VEL_FD]  [+ ulp32(grad_in) / 2]
               on EVERY element, each term alone and together, H = 2 .. 256 (one and several lane trips, the wave boundary), ragged
               and single-wave blocks, a shard's jl_scale; a zero unit is an exact zero; the aliased call and a second call repeat
               the bits
    step       cost_terms_grad(apply=True) with the terms ON, judged like tests/test_gpu_chomp_step_elements.py
    eval       per trajectory with the same form of bar; jl_total; broadcast_jlim; accumulate
    LDS        the largest accepted shapes meet the bars, one row more is refused with nothing written
    utilities  traj_interpolate, traj_finite_difference, gp_factor_error, traj_resample per element, each streaming kernel also on
               a second trip of its grid-stride loop; resample with NaN padding and clamped lengths

Every test prints the worst element over its bar."""
import numpy as np
import pytest
import torch

import chomp_step_checks as C
import collision_kinks as K
import cost_terms_checks as T

pytestmark = pytest.mark.gpu
NAN = float('nan')


def _grad(ref, dev, grad_in=None, aliased=False):
    """ops.cost_terms_grad(apply=False) -> the gradient on the CPU; trajs must keep its bits."""
    from motion_planning_baselines_amd import ops
    p = ref.p
    x = ref.x.to(dev)
    gi = None if grad_in is None else grad_in.to(dev).clone()
    out = gi if aliased else torch.full(ref.x.shape, NAN, device=dev)
    got = ops.cost_terms_grad(x, p.D, grad_in=gi, grad_out=out, jl_scale=ref.jl_scale, **p.spec(ref.terms, ref.fd, dev))
    torch.cuda.synchronize()
    assert got is out and T.same_bits(x.cpu(), ref.x)
    if gi is not None and not aliased:
        assert T.same_bits(gi.cpu(), grad_in)
    return got.cpu()


def _judge_grad(tag, ref, got, grad_in=None):
    want, bar = T.grad_bar(ref, grad_in)
    r = T.ratio(got, want, bar)
    worst = float(r.max())
    at = tuple(int(i) for i in np.unravel_index(int(r.argmax()), r.shape))
    print(f'{tag}: {got.numel()} elements judged ({int(ref.zero.sum())} exact), worst error / bar {worst:.3f} at (b, h, c) = {at}')
    assert got.shape == ref.x.shape and torch.isfinite(got).all()
    if grad_in is None:
        assert bool((got[ref.zero] == 0).all())
    else:
        assert T.same_bits(got[ref.zero], grad_in[ref.zero])
    assert worst <= 1.0, (tag, worst, at)
    return worst


# ------------------------------------------------------------------------------------------------
# 1.  the gradient, per element
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', T.CASES, ids=T.case_id)
def test_gradient_every_element(gpu_device, case):
    p = T.problem(*case)
    worst = {False: 0.0, True: 0.0}
    for name, (terms, fd, dmul) in T.CONFIGS.items():
        for jl_mul in ((1, T.SHARD) if 'jlim' in terms else (1,)):
            ref = T.reference(p, name, jl_mul)
            gin = T.grad_in_for(ref)
            for grad_in in (None, gin):
                tag = f'grad {T.case_id(case)} {name} jl_scale={ref.jl_scale:g} grad_in={"no" if grad_in is None else "yes"}'
                worst[fd] = max(worst[fd], _judge_grad(tag, ref, _grad(ref, gpu_device, grad_in), grad_in))
    print(f'grad {T.case_id(case)}: worst error / bar {worst[False]:.3f} with stored velocities, {worst[True]:.3f} under VEL_FD')


@pytest.mark.parametrize('name', ['all', 'gp+smooth+jlim-fd'])
@pytest.mark.parametrize('case', [(21, 3, 7), (21, 65, 7), (21, 256, 7), (5, 65, 7)], ids=T.case_id)
def test_gradient_aliased_and_repeated(gpu_device, case, name):
    """grad_out is grad_in (what planners/chomp.py passes against __restrict__ pointers) returns the bits of the call with separate
    buffers, and so does a second call."""
    ref = T.reference(T.problem(*case), name)
    gin = T.grad_in_for(ref)
    a = _grad(ref, gpu_device, gin)
    assert T.same_bits(a, _grad(ref, gpu_device, gin))
    assert T.same_bits(a, _grad(ref, gpu_device, gin, aliased=True))
    assert not torch.equal(a, gin)
    b = _grad(ref, gpu_device)
    assert T.same_bits(b, _grad(ref, gpu_device))


# ------------------------------------------------------------------------------------------------
# 2.  the step with the terms on: the composite's last group
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,dmul,clipped', C.COMPOSITE_TERM_CASES)
def test_step_with_terms(gpu_device, H, dmul, clipped):
    from motion_planning_baselines_amd import ops
    from test_gpu_chomp_step_elements import _judge
    ref = C.composite_reference(H, dmul, clipped, C.COMPOSITE_TERMS[dmul])
    tref = ref.tref
    assert ref.undecided_share <= C.UNDECIDED_CAP
    dev = gpu_device
    x = ref.x0.to(dev).clone()
    gi = ref.grad_in.to(dev)
    ops.cost_terms_grad(x, ref.D, grad_in=gi, apply=True, R=ref.R.to(dev), prior_bw=ref.prior_bw, lr=C.LR, grad_clip=ref.grad_clip,
                        jl_scale=tref.jl_scale, **tref.p.spec(tref.terms, tref.fd, dev))
    torch.cuda.synchronize()
    x1 = x.cpu()
    assert T.same_bits(gi.cpu(), ref.grad_in)
    tag = f'cost_terms_grad apply + {C.COMPOSITE_TERMS[dmul]} H={H} d={ref.d} clip={ref.grad_clip}'
    _judge(tag, ref, x1)
    # The same elements against the contract itself, in absolute terms: the fp64 sum grad_in + terms is rounded once (2^-24 |g64|, plus
    # the V tile's term), the prior is three fp32 fmas and one product (4 * 2^-24 of its unit), the new iterate is rounded once.
    prior_unit = C.unit_of(C.base(C.COMPOSITE_SCENE, H), ref.x0, 0.0, C.W_PRIOR, K.B)
    bar = (C.LR * (2.0 ** -24 * ref.g64.abs() + tref.vterm + 2.0 ** -44 * tref.unit) + 4.0 * 2.0 ** -24 * prior_unit
           + 2.0 ** -24 * ref.x64.abs()) * (1.0 + 2.0 ** -20)
    r = ((x1.double() - ref.x64).abs() / bar)[ref.judged]
    print(f'    against the contract: worst error / bar {float(r.max()):.3f} on {int(ref.judged.sum())} elements')
    assert float(r.max()) <= 1.0


# ------------------------------------------------------------------------------------------------
# 3.  eval, per trajectory
# ------------------------------------------------------------------------------------------------
def _eval(ref, dev, out=None, **kw):
    from motion_planning_baselines_amd import ops
    p = ref.p
    x = ref.x.to(dev)
    buf = torch.full((p.B,), NAN, device=dev) if out is None else out.to(dev).clone()
    got, jl = ops.cost_terms_eval(x, p.D, out=buf, **kw, **p.spec(ref.terms, ref.fd, dev))
    torch.cuda.synchronize()
    assert got is buf and T.same_bits(x.cpu(), ref.x)
    return got.cpu(), (None if jl is None else float(jl.cpu()))


def _judge_eval(tag, ref, got, jl):
    bar = T.cost_bar(ref)
    r = T.ratio(got, ref.c64, bar)
    line = f'{tag}: {got.numel()} trajectories, worst error / bar {float(r.max()):.3f}'
    assert torch.isfinite(got).all() and bool((got[bar == 0] == 0).all())
    rj = 0.0
    if ref.jl64 is not None:
        rj = abs(jl - ref.jl64) / ref.jl_bar
        line += f'; jl_total error / bar {rj:.3f}'
    else:
        assert jl is None
    print(line)
    assert float(r.max()) <= 1.0 and rj <= 1.0
    return max(float(r.max()), rj)


@pytest.mark.parametrize('case', T.CASES, ids=T.case_id)
def test_eval_every_trajectory(gpu_device, case):
    p = T.problem(*case)
    worst = 0.0
    for name, (terms, fd, dmul) in T.CONFIGS.items():
        ref = T.reference(p, name)
        off, jl = _eval(ref, gpu_device, broadcast_jlim=False)                  # no out[b] carries the joint-limit scalar
        worst = max(worst, _judge_eval(f'eval {T.case_id(case)} {name}', ref, off, jl))
        gen = torch.Generator().manual_seed(3)
        base = (float(ref.c64.abs().max()) + 1.0) * torch.randn(p.B, generator=gen)
        acc, jl_acc = _eval(ref, gpu_device, out=base, accumulate=True, broadcast_jlim=False)
        assert T.same_bits(acc, base + off)                                     # out + fresh in fp32, bit for bit
        if ref.jl64 is not None:
            on, jl_on = _eval(ref, gpu_device, broadcast_jlim=True)             # every out[b] carries it
            assert abs(jl_on - ref.jl64) <= ref.jl_bar and abs(jl_acc - ref.jl64) <= ref.jl_bar
            assert T.same_bits(on, off + torch.tensor(jl_on, dtype=torch.float64).float())
            if not set(terms) - {'jlim'}:                                       # nothing else in out: the scalar itself, rounded once
                assert bool((off == 0).all()) and bool((on == torch.tensor(jl_on, dtype=torch.float64).float()).all()) and float(on[0]) > 0
            both, jl_b = _eval(ref, gpu_device, out=base, accumulate=True, broadcast_jlim=True)
            assert T.same_bits(both, (base + off) + torch.tensor(jl_b, dtype=torch.float64).float())
    print(f'eval {T.case_id(case)}: worst error / bar {worst:.3f}')


# ------------------------------------------------------------------------------------------------
# 4.  the LDS limits: 4 waves x H x (d | 1) x 4 bytes <= 150 KiB for eval, twice that for grad
# ------------------------------------------------------------------------------------------------
def test_lds_largest_shapes_and_refusals(gpu_device):
    from motion_planning_baselines_amd import ops
    from motion_planning_baselines_amd._lib import MPBError
    dev = gpu_device
    # grad: H (d | 1) = 192 * 25 = 4 800 is the largest product accepted
    ref = T.reference(T.problem(5, 192, 12), 'all')
    assert ref.d == 24 and 4 * 2 * 192 * 25 * 4 == 150 * 1024
    _judge_grad('grad at the LDS limit B5-H192-d24 all', ref, _grad(ref, dev))
    gin = T.grad_in_for(ref)
    _judge_grad('grad at the LDS limit B5-H192-d24 all grad_in=yes', ref, _grad(ref, dev, gin), gin)
    # one row more is refused before anything is written
    ref = T.reference(T.problem(5, 193, 12), 'all')
    x, out = ref.x.to(dev), torch.full(ref.x.shape, NAN, device=dev)
    for apply in (False, True):
        with pytest.raises(MPBError, match='too large for the LDS tiles'):
            ops.cost_terms_grad(x, 12, grad_out=out, apply=apply, lr=0.5, grad_clip=1.0, jl_scale=5.0, **ref.p.spec(ref.terms, ref.fd, dev))
    torch.cuda.synchronize()
    assert T.same_bits(x.cpu(), ref.x) and bool(torch.isnan(out).all())
    # eval: H (d | 1) = 9 600 is out of reach under H <= 256 and d <= 24; the largest shape there is
    ref = T.reference(T.problem(5, 256, 12), 'all')
    _judge_eval('eval at its largest shape B5-H256-d24 all', ref, *_eval(ref, dev, broadcast_jlim=False))
    # Today's behaviour at H = 256 with 12 joints: the position-only gradient (d = 12: 256 * 13 = 3 328) is accepted, the one with stored
    # velocities (d = 24: 256 * 25 = 6 400 > 4 800) is refused -- a 12-joint composite CHOMP at H = 256 needs position-only trajectories.
    pos = T.reference(T.problem(5, 256, 12), 'gp+smooth+jlim-fd')
    _judge_grad('grad B5-H256-d12 gp+smooth+jlim-fd', pos, _grad(pos, dev))
    with pytest.raises(MPBError, match='too large for the LDS tiles'):
        _grad(ref, dev)


# ------------------------------------------------------------------------------------------------
# 5.  the utilities, per element
# ------------------------------------------------------------------------------------------------
def _lines(B, H, d, seed):
    """Straight lines plus noise through the origin's neighbourhood (both signs), fp32 (B, H, d)."""
    gen = torch.Generator().manual_seed(seed)
    a, b = 3.0 * torch.rand(B, 1, d, generator=gen) - 1.5, 3.0 * torch.rand(B, 1, d, generator=gen) - 1.5
    return (a + torch.linspace(0.0, 1.0, H).reshape(1, H, 1) * (b - a) + 0.05 * torch.randn(B, H, d, generator=gen)).float().contiguous()


def _report(tag, got, want, bar):
    r = T.ratio(got, want, bar)
    print(f'{tag}: {got.numel()} elements judged, worst error / bar {float(r.max()):.3f}')
    assert torch.isfinite(got).all() and bool((got.double()[bar == 0] == want[bar == 0]).all())
    assert float(r.max()) <= 1.0, tag


# the last shape of each list: the output exceeds the 16 384 x 256 threads of the capped grid by less than 1 % -- a second trip
@pytest.mark.parametrize('B,H,d,n', [(3, 5, 7, 0), (3, 5, 7, 1), (3, 5, 7, 7), (3, 2, 3, 64), (5, 66, 14, 64), (64, 129, 64, 7)])
def test_traj_interpolate_every_element(gpu_device, B, H, d, n):
    from motion_planning_baselines_amd import ops
    from oracle import planners_ref as O
    x = _lines(B, H, d, 1)
    got = ops.traj_interpolate(x.to(gpu_device), n).cpu()
    want = O.interpolate_trajs(x.double(), n)
    assert got.shape == want.shape == (B, (H - 1) * (n + 1) + 1, d)
    if (B, H, d, n) == (64, 129, 64, 7):
        assert 4194304 < got.numel() < 1.01 * 4194304
    ax = x.double().abs()
    seg = (ax[:, :-1] + ax[:, 1:])[:, :, None].expand(-1, -1, n + 1, -1).flatten(1, 2)
    bar = 2.0 ** -23 * torch.cat((seg, 2.0 * ax[:, -1:]), 1)
    _report(f'traj_interpolate B={B} H={H} d={d} n={n}', got, want, bar)
    assert T.same_bits(got[:, ::n + 1], x)                                       # support points keep their bits


@pytest.mark.parametrize('B,H,D', [(3, 2, 7), (3, 3, 7), (5, 65, 1), (21, 129, 7), (64, 257, 128)])
def test_traj_finite_difference_every_element(gpu_device, B, H, D):
    from motion_planning_baselines_amd import ops
    from oracle import planners_ref as O
    x = _lines(B, H, D, 2)
    got = ops.traj_finite_difference(x.to(gpu_device), T.DT).cpu()
    assert got.shape == (B, H, 2 * D)
    if D == 128:
        assert 4194304 < got.numel() < 1.01 * 4194304
    want = O.finite_difference_central(x.double(), T.DT)
    bar = torch.zeros_like(want)
    bar[:, 1:-1] = 2.0 ** -23 * (x[:, 2:].double().abs() + x[:, :-2].double().abs()) / (2.0 * T.DT)
    _report(f'traj_finite_difference B={B} H={H} D={D}', got[..., D:], want, bar)
    assert T.same_bits(got[..., :D], x)                                          # positions keep their bits
    assert bool((got[:, 0, D:] == 0).all()) and bool((got[:, -1, D:] == 0).all())
    if H > 2:
        assert float(got[:, 1:-1, D:].abs().max()) > 0


@pytest.mark.parametrize('B,H,D', [(3, 2, 7), (3, 3, 1), (21, 65, 7), (5, 129, 12), (64, 258, 128)])
def test_gp_factor_error_every_element(gpu_device, B, H, D):
    from motion_planning_baselines_amd import ops
    from oracle import planners_ref as O
    x = _lines(B, H, 2 * D, 3)
    got = ops.gp_factor_error(x.to(gpu_device), D, T.DT).cpu()
    assert got.shape == (B, H - 1, 2 * D)
    if D == 128:
        assert 4194304 < got.numel() < 1.01 * 4194304
    want = O.gp_error(x.double(), O.gp_phi(D, T.DT, T.F64))
    ax = x.double().abs()
    bar = 2.0 ** -23 * (ax[:, 1:] + ax[:, :-1])
    bar[..., :D] += 2.0 ** -23 * T.DT * ax[:, :-1, D:]
    _report(f'gp_factor_error B={B} H={H} D={D}', got, want, bar)


RESAMPLE_L = (1, 2, 3, 64, 65, 128, 129, 200)


def _paths():
    """One padded batch (N, 200, 3): random walks of the lengths RESAMPLE_L (the scan's carry at 64 | 65 and 128 | 129), one of them
    with repeated waypoints, then a path of five identical points and a walk that stands still for a while; padding rows are NaN."""
    gen = torch.Generator().manual_seed(9)
    D, Lmax = 3, max(RESAMPLE_L)
    lengths = list(RESAMPLE_L) + [5, 70]
    paths = torch.full((len(lengths), Lmax, D), NAN)
    for n, L in enumerate(lengths):
        paths[n, :L] = torch.rand(D, generator=gen) - 0.5 + torch.cumsum(0.1 * torch.randn(L, D, generator=gen), 0)
    paths[6, 10:13] = paths[6, 9]                        # L = 129: repeated waypoints inside ...
    paths[6, 0:2] = paths[6, 2]                          # ... and at the start
    paths[8, :5] = paths[8, 0]                           # identical points: zero arc length
    paths[9, 30:50] = paths[9, 29]
    return paths.float().contiguous(), torch.tensor(lengths, dtype=torch.int32)


@pytest.mark.parametrize('H', [2, 3, 64, 65, 200])
def test_traj_resample_every_element(gpu_device, H):
    from motion_planning_baselines_amd import ops
    from oracle import planners_ref as O
    dev = gpu_device
    paths, lengths = _paths()
    N, Lmax, D = paths.shape
    got = ops.traj_resample(paths.to(dev), lengths.to(dev), H, T.DT).cpu()
    assert got.shape == (N, H, 2 * D) and not bool(torch.isnan(got).any())      # no padding row was read
    worst_p = worst_v = 0.0
    for n, L in enumerate(lengths.tolist()):
        P = paths[n, :L]
        want = O.resample_path(P.double().numpy(), H, T.DT)
        ep = (got[n, :, :D].double() - want[:, :D]).abs() / (2.0 ** -23 * float(P.abs().max()))
        bar_v = 2.0 ** -23 * want[:, D:].abs()
        rv = T.ratio(got[n, :, D:], want[:, D:], bar_v)
        assert bool((got[n, :, D:].double()[bar_v == 0] == 0).all())             # rest at both ends, and a path that ends where it starts
        worst_p, worst_v = max(worst_p, float(ep.max())), max(worst_v, float(rv.max()))
        assert T.same_bits(got[n, 0, :D], P[0]) and T.same_bits(got[n, -1, :D], P[-1])
        # every path equals its unpadded single call bit for bit
        alone = ops.traj_resample(P.unsqueeze(0).contiguous().to(dev), torch.tensor([L], dtype=torch.int32, device=dev), H, T.DT).cpu()
        assert T.same_bits(alone[0], got[n]), (n, L)
    print(f'traj_resample H={H}: {got.numel()} elements of {N} paths judged, worst error / bar {worst_p:.3f} on positions, '
          f'{worst_v:.3f} on velocities')
    assert worst_p <= 1.0 and worst_v <= 1.0
    assert bool((got[8, :, :D] == paths[8, 0]).all())


def test_traj_resample_clamps_lengths(gpu_device):
    """lengths outside 1 .. Lmax are clamped into it (include/mpb.h): 0 reads one row, Lmax + 5 reads Lmax rows and no further."""
    from motion_planning_baselines_amd import ops
    dev = gpu_device
    gen = torch.Generator().manual_seed(4)
    Lmax, D, H = 70, 3, 33
    paths = torch.cumsum(0.1 * torch.randn(3, Lmax, D, generator=gen), 1).contiguous()      # the last path ends the allocation's data
    odd = ops.traj_resample(paths.to(dev), torch.tensor([0, Lmax + 5, Lmax + 5], dtype=torch.int32, device=dev), H, T.DT).cpu()
    ok = ops.traj_resample(paths.to(dev), torch.tensor([1, Lmax, Lmax], dtype=torch.int32, device=dev), H, T.DT).cpu()
    assert torch.isfinite(odd).all() and T.same_bits(odd, ok)
    assert bool((odd[0, :, :D] == paths[0, 0]).all()) and bool((odd[0, :, D:] == 0).all())
    assert T.same_bits(odd[1, -1, :D], paths[1, -1])
