"""-m gpu: the STOMP sample and update kernels, the two-kernel step and the persistent launches, element by element against the
fp64 oracle (helper and criterion: tests/stomp_kernels_checks.py; conditions on the inputs and planted faults:
tests/test_stomp_kernels_cpu.py).  Every element of every output is judged: e = |got - ref64| / unit <= 4 max(E32, 2^-23), E32 the
fp32 restatement's worst e on the same inputs; an element whose unit is 0 carries the bits of the means; a weight whose fp64 value
is below fp32's smallest normal comes out below 2^-125.  Each test prints E32, the kernel's worst e and the bar ("STOMP-ELEM").

1. ops.stomp_sample, injected eps, geom = None: the H = 64 kernel at its six channel counts with P S = 5 and 9; the chunked kernel
   at H = 64 with the other channel counts and at M = 1, 2, 4 chunks (a one-row last chunk, three of four chunks, vector and scalar
   stores, d = 16, S in {1, 3}); three L each (rows over four decades, STOMP's own, identity with bf16 eps: fp32(mean + eps) bit for
   bit); drawn noise (ops.debug_stomp_normals, particle_offset != 0) for one case per kernel.
2. ops.stomp_update: weights against stomp_weights, means against the fp64 update from the RETURNED weights, with Sigma (rows over
   four decades; STOMP's own on two shapes) and without; the dispatch path of every case asserted from its shape.
3. ops.stomp_step, n_iters = 3 == three rounds of stomp_sample(geom, costs) -> stomp_update, bit for bit, outputs the third's.
4. ops.stomp_run, one teacher-forced iteration on each persistent layout at the smallest P >= 2 that reaches it, the kernel's own
   costs as the softmax's input and PERSISTENT_EXTRA more roundings of a logit in the weight's unit (counted in the helper)."""
import pytest
import torch

import stomp_kernels_checks as C

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------
# 1. samples
# ------------------------------------------------------------------------------------------------
def _run_sample(dev, pr, eps=True, **kw):
    from motion_planning_baselines_amd import ops
    out = torch.full((pr.P, pr.S, pr.H, pr.d), float('nan'), device=dev)
    ops.stomp_sample(pr.means.to(dev), pr.eps.to(dev) if eps else None, out, pr.L.to(dev), pr.S, **kw)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize('P,S,H,d', C.SAMPLE_H64 + C.SAMPLE_HX)
def test_samples_per_element(gpu_device, P, S, H, d):
    kernel = C.sample_kernel_of(H, d)
    assert kernel == ('h64' if (P, S, H, d) in C.SAMPLE_H64 else 'hx')
    for family in C.L_FAMILIES:
        pr = C.sample_problem(P, S, H, d, family)
        ref = C.sample_reference(pr.means, pr.L, pr.eps)
        got = _run_sample(gpu_device, pr)
        C.check_samples(f'sample/{kernel} {(P, S, H, d)} L={family}', got, ref)
        if family == 'identity':
            assert C.same_bits(got, ref.x32), 'L = I, bf16 eps: a sample is fp32(mean + eps)'


@pytest.mark.parametrize('P,S,H,d', C.SAMPLE_DRAWN)
def test_drawn_samples_per_element(gpu_device, P, S, H, d):
    """eps = None: the kernel's own normals (fetched with the same seed, iteration and particle offset) through the same product."""
    from motion_planning_baselines_amd import ops
    seed, it, off = 77, 3, 5
    kernel = C.sample_kernel_of(H, d)
    for family in ('dense', 'stomp'):
        pr = C.sample_problem(P, S, H, d, family)
        nrm = ops.debug_stomp_normals(P, S, d, 1, gpu_device, seed=seed, iter0=it, particle_offset=off, H=H)
        torch.cuda.synchronize()
        eps = nrm[0, :, :, :, :H].permute(1, 2, 0, 3).contiguous().cpu()                     # (P, S, d, Hp) -> (S, d, P, H)
        assert bool(torch.isfinite(eps).all()) and 0.5 < float(eps.std()) < 1.5
        ref = C.sample_reference(pr.means, pr.L, eps)
        got = _run_sample(gpu_device, pr, eps=False, seed=seed, it=it, particle_offset=off)
        C.check_samples(f'sample/{kernel} drawn {(P, S, H, d)} L={family}', got, ref)
        other = _run_sample(gpu_device, pr, eps=False, seed=seed, it=it, particle_offset=off + 1)
        assert not torch.equal(other, got)


# ------------------------------------------------------------------------------------------------
# 2. update
# ------------------------------------------------------------------------------------------------
def _check_update(label, pr, w, m):
    wr = C.weights_reference(pr.costs, pr.temperature)
    C.check_weights(label, w, wr)
    mr = C.mean_reference(pr.means, pr.samples, w, pr.Sigma, pr.lr)
    C.check_means(label, m, mr, pr.means)
    return wr, mr


def _run_update(dev, pr):
    from motion_planning_baselines_amd import ops
    m = pr.means.clone().to(dev)
    w = torch.full((pr.P, pr.S), float('nan'), device=dev)
    ops.stomp_update(m, pr.samples.to(dev), pr.costs.to(dev), w, None if pr.Sigma is None else pr.Sigma.to(dev), pr.lr, pr.temperature)
    torch.cuda.synchronize()
    return w.cpu(), m.cpu()


@pytest.mark.parametrize('S,H,d', C.UPDATE_V4 + C.UPDATE_GENERIC)
def test_update_per_element(gpu_device, S, H, d):
    shape = (S, H, d)
    assert (C.update_kernel_of(*shape) == 'v4') == (shape in C.UPDATE_V4)
    P = C.update_P(shape)
    kinds = ('spd', None) + (('stomp',) if shape in C.UPDATE_ALL_FAMILIES else ())
    for family in C.update_families(shape):
        for kind in kinds:
            pr = C.update_problem(P, S, H, d, family, kind)
            w, m = _run_update(gpu_device, pr)
            label = f'update/{C.update_kernel_of(S, H, d, kind is not None)} {shape} costs={family} Sigma={kind}'
            wr, mr = _check_update(label, pr, w, m)
            if family == 'equal':
                # every weight the same bits; the means move by lr Sigma mean(delta) within the bar
                assert bool((w.view(torch.int32) == w.view(torch.int32)[0, 0]).all())
                flat64 = C._update(pr.means.double(), pr.samples.double(), torch.full((P, S), 1.0 / S, dtype=torch.float64),
                                   None if pr.Sigma is None else pr.Sigma.double(), pr.lr)
                _, _, bad = C.judge(label + ' means vs mean(delta)', m, flat64, mr.unit, mr.E32)
                assert len(bad) == 0
            if family == 'onehot':
                assert bool(((w == 1.0).sum(1) == 1).all()) and bool(((w == 0.0).sum(1) == S - 1).all())
            if family == 'tied':
                top = w.topk(2, dim=1)[0]
                assert C.same_bits(top[:, 0], top[:, 1]) and bool((top[:, 0] > 0.25).all())


def test_update_beyond_the_lds_budget_is_refused_untouched(gpu_device):
    from motion_planning_baselines_amd import ops
    from motion_planning_baselines_amd._lib import MPBError
    S, H, d = C.UPDATE_REFUSED
    assert C.update_kernel_of(S, H, d) is None
    P = 2
    m0 = torch.randn(P, H, d)
    m, w = m0.clone().to(gpu_device), torch.full((P, S), 7.0, device=gpu_device)
    samples, costs = torch.empty(P, S, H, d, device=gpu_device), torch.zeros(P, S, device=gpu_device)
    Sigma = C.covariance(H, 'spd').to(gpu_device)
    for sg in (Sigma, None):
        with pytest.raises(MPBError, match='too large for LDS'):
            ops.stomp_update(m, samples, costs, w, sg, C.LR, 0.7)
    torch.cuda.synchronize()
    assert C.same_bits(m.cpu(), m0) and bool((w == 7.0).all())


# ------------------------------------------------------------------------------------------------
# 3. the two-kernel step
# ------------------------------------------------------------------------------------------------
def _point_scene(dev, P, H):
    """A 3-D point robot on straight lines, a sphere of radius 0.25 on the middle of every line and twelve more: every rollout is in
    contact.  (means0 (P, H, 3), geometry, D)"""
    import numpy as np
    from motion_planning_baselines_amd import geometry as G, ops
    gen = torch.Generator().manual_seed(4)
    a, b = torch.rand(P, 1, 3, generator=gen) * 1.6 - 0.8, torch.rand(P, 1, 3, generator=gen) * 1.6 - 0.8
    t = torch.linspace(0, 1, H).reshape(1, H, 1)
    means0 = (a * (1 - t) + b * t).contiguous()
    centres = torch.cat([means0[:, H // 2], torch.rand(12, 3, generator=gen) * 1.6 - 0.8])
    sph = np.concatenate([centres.numpy(), np.full((len(centres), 1), 0.25)], 1).astype(np.float32)
    return means0.to(dev), ops.DeviceGeometry(G.RobotPointMass(3, radius=0.02), G.CollisionField(spheres=sph, margin=0.03), dev), 3


@pytest.mark.parametrize('kind,P,S,H,drawn', [('pm3d', 3, 5, 65, False), ('panda', 2, 33, 64, True)])
def test_step_equals_three_rounds_of_sample_and_update(gpu_device, kind, P, S, H, drawn):
    from motion_planning_baselines_amd import ops
    from test_gpu_stomp_fused_hx import _problem
    dev = gpu_device
    means0, geom, D = _point_scene(dev, P, H) if kind == 'pm3d' else _problem(dev, kind, P, S, H, pos_only=False)[:3]
    d = means0.shape[-1]
    assert (P, S, H, d) in ((3, 5, 65, 3), (2, 33, 64, 14))
    # (STOMP's own constants at sigma_spectral = 64 * 0.02: a noise of a few centimetres keeps the rollouts in the scene)
    L, Sigma = C.stomp_constants(H)[0].to(dev) / 64.0, C.stomp_constants(H)[1].to(dev) / 4096.0
    ksig, weight, lr, temp, n, seed, it0 = 1.0e4, 1.0, 0.1, 1.0e3, 3, 5, 2
    eps = None if drawn else torch.randn(n, S, d, P, H, generator=torch.Generator().manual_seed(9)).to(dev)
    mk = lambda: (torch.empty(P, S, H, d, device=dev), torch.empty(P, S, device=dev), torch.empty(P, S, device=dev))
    m1, (s1, c1, w1) = means0.clone(), mk()
    ops.stomp_step(m1, eps, s1, c1, w1, L, Sigma, geom, S, D, ksig, weight, lr, temp, n_iters=n, seed=seed, iter0=it0)
    m2, (s2, c2, w2) = means0.clone(), mk()
    rounds = []
    for it in range(n):
        ops.stomp_sample(m2, None if drawn else eps[it].clone(), s2, L, S, seed=seed, it=it0 + it, geom=geom, costs=c2, k_sigma=ksig, weight=weight)
        ops.stomp_update(m2, s2, c2, w2, Sigma, lr, temp)
        rounds.append((s2.clone(), c2.clone(), w2.clone(), m2.clone()))
    torch.cuda.synchronize()
    assert float(c1.max()) > 0 and bool(torch.isfinite(m1).all())
    for name, a, b in (('samples', s1, s2), ('costs', c1, c2), ('weights', w1, w2), ('means', m1, m2)):
        assert C.same_bits(a, b), name
    # ... and they are the third iteration's, not the second's
    assert not torch.equal(s1, rounds[1][0]) and not torch.equal(c1, rounds[1][1]) and not torch.equal(w1, rounds[1][2])
    assert not torch.equal(m1, rounds[1][3])


# ------------------------------------------------------------------------------------------------
# 4. the persistent launches
# ------------------------------------------------------------------------------------------------
def _smallest_P(ops, geom, want, S, H, d, dev):
    """The smallest P >= 2 whose path is `want`, and its workspace (the path depends on the geometry's flags, not on its particles)."""
    for P in range(2, 513):
        ws = ops.stomp_workspace(P, S, H, d, dev)
        if ops.stomp_run_path(geom, ws, P, S, H, d) == want:
            return P, ws
    raise AssertionError('no P up to 512 reaches the path')


@pytest.mark.parametrize('layout,S,H,pos_only', [
    ('exchange', 32, 64, False),          # H = 64 kernel, two workgroups per particle exchanging their partials
    ('two-batch', 24, 64, True),          # H = 64 kernel, one workgroup per particle, two batches of 16 (the second partial)
    ('generalised', 12, 48, False),       # csrc/mpb_stomp_fused_hx.hip
    ('generalised', 32, 128, True)])
def test_persistent_iteration_per_element(gpu_device, layout, S, H, pos_only):
    from motion_planning_baselines_amd import ops
    from test_gpu_stomp_fused_hx import _problem
    dev = gpu_device
    d = 7 if pos_only else 14
    want = ops.STOMP_PATH_PERSISTENT if layout == 'two-batch' else None
    if layout == 'exchange':
        want = ops.STOMP_PATH_PERSISTENT_EXCHANGE
    geom = _problem(dev, 'panda', 2, S, H, pos_only)[1]
    if want is None:                      # whichever persistent form the generalised kernel takes at P = 2
        P, ws = 2, ops.stomp_workspace(2, S, H, d, dev)
        assert ops.stomp_run_path(geom, ws, P, S, H, d) in (ops.STOMP_PATH_PERSISTENT, ops.STOMP_PATH_PERSISTENT_EXCHANGE)
    else:
        P, ws = _smallest_P(ops, geom, want, S, H, d, dev)
        # (S in 17 .. 32 at H = 64 is two chunks of 16: without the exchange they are the two batches of one workgroup)
        assert layout != 'two-batch' or (16 < S <= 32 and P > 2)
    means0, geom, D, _ = _problem(dev, 'panda', P, S, H, pos_only)
    assert ops.stomp_run_path(geom, ws, P, S, H, d) != ops.STOMP_PATH_TWO_KERNEL and (want is None or ops.stomp_run_path(geom, ws, P, S, H, d) == want)
    assert means0.shape == (P, H, d)
    L, Sigma = C.stomp_constants(H)
    ksig, weight, lr, temp = 1.0e4, 1.0, 0.1, 1.0e3
    eps = torch.randn(1, S, d, P, H, generator=torch.Generator().manual_seed(31 + H + S))
    m = means0.clone()
    samples = torch.full((P, S, H, d), float('nan'), device=dev)
    costs, w = torch.full((P, S), float('nan'), device=dev), torch.full((P, S), float('nan'), device=dev)
    status = ops.StompRunStatus()
    tag = ops.stomp_run(m, eps.to(dev), samples, costs, w, L.to(dev), Sigma.to(dev), geom, S, D, ksig, weight, lr, temp, ws,
                        n_iters=1, status=status)
    torch.cuda.synchronize()
    assert tag != 0 and status.lost() is None and not ops.stomp_run_timed_out(ws)
    label = f'persistent/{layout} {(P, S, H, d)}'
    means0, samples, costs, w, m = means0.cpu(), samples.cpu(), costs.cpu(), w.cpu(), m.cpu()
    C.check_samples(label, samples, C.sample_reference(means0, L, eps[0]))
    assert bool(torch.isfinite(costs).all()) and float(costs.min()) >= 0 and float(costs.max()) > 0
    wr = C.weights_reference(costs, temp, C.PERSISTENT_EXTRA)
    assert int((wr.w64 > 1e-3).sum(1).max()) >= 2                      # the softmax has something to decide
    C.check_weights(label, w, wr)
    C.check_means(label, m, C.mean_reference(means0, samples, w, Sigma, lr), means0)
