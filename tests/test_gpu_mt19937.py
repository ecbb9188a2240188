"""-m gpu: noise='mt19937' -- torch's CPU generator run on the device (csrc/mpb_mt19937.hip, ops.torch_cpu_normal_) against
the CPU generator itself: uniforms bit for bit (the debug export), normals within 4 ULP (or 2^-22 near zero), the generator
state byte for byte; the planners with noise='mt19937' against the reference goldens and against noise='torch_cpu'."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from test_gpu_planners import T, make_cost, rel_err

pytestmark = pytest.mark.gpu

C3 = (32, 14, 128, 64)                       # the headline's (S, d, P, H) block: 3 670 016 normals an iteration


def _state_bytes(gen=None):
    return bytes((gen.get_state() if gen is not None else torch.get_rng_state()).numpy().tobytes())


def _ulp_report(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    ulp = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    ok = (ulp <= 4) | (np.abs(a.astype(np.float64) - b) <= 2.0 ** -22)
    return bool(ok.all()), float((ulp == 0).mean()), int(ulp[np.abs(b) > 2.0 ** -22].max(initial=0))


@pytest.mark.parametrize('block,n_calls', [((17,), 1), ((17,), 5), ((5, 20), 3), (C3, 1), (C3, 2)])
def test_device_uniforms_bit_for_bit(gpu_device, block, n_calls):
    from motion_planning_baselines_amd import ops
    n = int(np.prod(block))
    torch.manual_seed(1234)
    torch.empty(321).uniform_()                                  # a start state in the middle of the array
    out, after = ops.debug_mt19937_uniforms(n, n_calls, gpu_device)
    ref = torch.stack([torch.empty(n).uniform_() for _ in range(n_calls)])
    assert torch.equal(out.cpu().view(torch.int32), ref.view(torch.int32))
    assert after.to_bytes() == _state_bytes()


@pytest.mark.parametrize('block,n_calls,pre', [((17,), 1, 0), ((17,), 3, 50), ((100,), 5, 623), ((7, 33), 4, 10), (C3, 1, 0), (C3, 2, 77)])
def test_device_normals_and_state(gpu_device, block, n_calls, pre):
    from motion_planning_baselines_amd import ops
    torch.manual_seed(42)
    if pre:
        torch.empty(pre).uniform_()
    s0 = torch.get_rng_state()
    out = torch.empty(n_calls, *block, device=gpu_device)
    ops.torch_cpu_normal_(out, n_calls)
    dev_state = _state_bytes()
    torch.set_rng_state(s0)
    ref = torch.stack([torch.empty(*block).normal_() for _ in range(n_calls)])
    assert dev_state == _state_bytes()                          # the generator advanced exactly as by the CPU draws
    ok, exact, worst = _ulp_report(out.cpu().numpy(), ref.numpy())
    print('block %s x %d: %.1f %% of the normals bit-exact, worst %d ULP' % (block, n_calls, 100 * exact, worst))
    assert ok
    assert exact > 0.5


def test_explicit_generator_and_later_draws_continue(gpu_device):
    from motion_planning_baselines_amd import ops
    g, h = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    out = torch.empty(2, 3000, device=gpu_device)
    before = _state_bytes()
    ops.torch_cpu_normal_(out, 2, generator=g)
    assert _state_bytes() == before                              # the global generator is untouched
    ref = torch.stack([torch.empty(3000).normal_(generator=h) for _ in range(2)])
    assert _ulp_report(out.cpu().numpy(), ref.numpy())[0]
    assert torch.equal(torch.empty(1000).uniform_(generator=g), torch.empty(1000).uniform_(generator=h))


def test_refusals(gpu_device):
    from motion_planning_baselines_amd import ops
    from motion_planning_baselines_amd._lib import MPBError
    with pytest.raises(MPBError, match='float32'):
        ops.torch_cpu_normal_(torch.empty(1, 64, device=gpu_device, dtype=torch.float64), 1)
    with pytest.raises(MPBError, match='16'):
        ops.torch_cpu_normal_(torch.empty(2, 15, device=gpu_device), 2)
    with pytest.raises(MPBError, match='contiguous'):
        ops.torch_cpu_normal_(torch.empty(64, 2, device=gpu_device).t(), 2)
    with pytest.raises(MPBError, match='GPU'):
        ops.torch_cpu_normal_(torch.empty(1, 64), 1)
    with pytest.raises(MPBError, match='shape'):
        ops.torch_cpu_normal_(torch.empty(3, 64, device=gpu_device), 2)


def _stomp(g, dev, cost, opt_iters, noise):
    from motion_planning_baselines_amd.planners.stomp import STOMP
    return STOMP(n_dof=int(g['D']), n_support_points=int(g['H']), num_particles_per_goal=int(g['P']),
                 num_samples=int(g['S']), opt_iters=opt_iters, dt=float(g['dt']), start_state=T(g['start']).to(dev), cost=cost,
                 initial_particle_means=T(g['means0']).to(dev), multi_goal_states=T(g['goal']).unsqueeze(0).to(dev),
                 temperature=float(g['temperature']), step_size=float(g['lr']), sigma_spectral=float(g['sigma_spectral']),
                 pos_only=bool(g['pos_only']), tensor_args=dict(device=dev, dtype=torch.float32), noise=noise)


@pytest.mark.parametrize('name', ['stomp_pm2d_c1', 'stomp_panda_t1', 'stomp_pm2d_benign'])
def test_stomp_mt19937_same_seed_as_reference(gpu_device, name):
    """test_stomp_class_same_seed_as_reference's bars with the draws made on the device, opt_iters=1 and opt_iters=n."""
    g = load_golden(name)
    dev = gpu_device
    cost, _, _ = make_cost(g, dev)
    n = g['eps'].shape[0]
    errs = {}
    for noise in ('torch_cpu', 'mt19937'):
        torch.manual_seed(int(g['seed']))
        pl = _stomp(g, dev, cost, 1, noise)
        pl.Sigma = T(g['Sigma']).to(dev).contiguous()                   # the golden's constants (see that test)
        pl.scale_tril = T(g['L']).to(dev).contiguous()
        for _ in range(n):
            pl.optimize()
        torch.cuda.synchronize()
        errs[noise] = (rel_err(pl.state_particles, T(g['samples'][-1])), rel_err(pl._particle_means, T(g['means'][-1])),
                       _state_bytes())
        torch.manual_seed(int(g['seed']))
        pl2 = _stomp(g, dev, cost, n, noise)
        pl2.Sigma, pl2.scale_tril = pl.Sigma, pl.scale_tril
        pl2.optimize()
        torch.cuda.synchronize()
        errs[noise + ' n'] = rel_err(pl2._particle_means, T(g['means'][-1]))
    print(name, errs['torch_cpu'][:2], errs['torch_cpu n'], 'mt19937:', errs['mt19937'][:2], errs['mt19937 n'])
    assert errs['mt19937'][0] < 1e-4 and errs['mt19937'][1] < 1e-4 and errs['mt19937 n'] < 1e-4
    assert errs['mt19937'][2] == errs['torch_cpu'][2]                  # the generator is left where the CPU draws leave it


@pytest.mark.parametrize('fused', [False, True])
def test_mppi_mt19937_vs_golden(gpu_device, fused):
    """test_mppi_any_cost_object_vs_golden's checks with noise='mt19937', through the caller's cost object and the fused cost."""
    from test_gpu_api_holes import _mppi
    from motion_planning_baselines_amd.planners.costs.cost_functions import fusable_collision
    g = load_golden('mppi_pm2d_indep_cost')
    dev = gpu_device
    inner, _, _ = make_cost(g, dev)
    Tn, S = int(g['T']), int(g['S'])

    class CallersCost:
        def eval(self, trajs, **kw):
            return inner.eval(trajs, **kw)

    cost = inner if fused else CallersCost()
    assert (fusable_collision(cost) is not None) == fused
    torch.manual_seed(1)
    pl = _mppi(g, dev, noise='mt19937')
    obs = dict(state=T(g['start']).to(dev), goal_state=T(g['goal']).to(dev), cost=cost)
    for it in range(g['eps'].shape[0]):
        U, X, c = pl.optimize(**obs)
        assert U.shape == (S, Tn, 2) and X.shape == (S, Tn, 2) and c.shape == (S, 1)
        np.testing.assert_allclose(c.cpu().numpy(), g['costs'][it], rtol=5e-5)
        assert rel_err(pl.get_mean_controls(), T(g['mean'][it])) < 1e-4, it
        flat = np.stack([g['costs'][k].reshape(-1) for k in range(it + 1)])
        it_b, s_b = np.unravel_index(np.argmin(flat), flat.shape)
        np.testing.assert_allclose(float(pl.best_cost), flat[it_b, s_b], rtol=5e-5)
        np.testing.assert_allclose(pl.best_traj.cpu().numpy(), g['states'][it_b][s_b], rtol=1e-4, atol=1e-5)


def test_stomp_c3_mt19937_vs_torch_cpu(gpu_device):
    """Full C3 (P = 128, S = 32: B = 4096), 2 iterations from the same seed with noise='mt19937' and noise='torch_cpu'.  Bar on the
    final means: 1e-4 relative over all particles.  The generator must end in the same state byte for byte."""
    from motion_planning_baselines_amd import workloads
    from motion_planning_baselines_amd.planners.stomp import STOMP
    from motion_planning_baselines_amd.planners.costs.cost_functions import CostCollision, CostComposite
    dev = gpu_device
    wl = workloads.panda_spheres_stomp(128, dev, H=64, S=32, pos_only=False)
    prm = wl['params']
    ta = dict(device=dev, dtype=torch.float32)
    cost = CostComposite(wl['robot'], 64, [CostCollision(wl['robot'], 64, field=wl['field'], sigma_coll=wl['sigma_coll'],
                                                         tensor_args=ta)], tensor_args=ta)
    res = {}
    for noise in ('torch_cpu', 'mt19937'):
        torch.manual_seed(3)
        pl = STOMP(opt_iters=2, start_state=torch.from_numpy(wl['starts'][0]).to(dev), cost=cost, initial_particle_means=wl['means0'],
                   tensor_args=ta, noise=noise, seed=0, check='sync', **prm)
        pl.optimize()
        torch.cuda.synchronize()
        res[noise] = (pl._particle_means.cpu(), _state_bytes())
    err = rel_err(res['mt19937'][0], res['torch_cpu'][0])
    print('C3 2 iterations: means rel err mt19937 vs torch_cpu %.2e' % err)
    assert res['mt19937'][1] == res['torch_cpu'][1]
    assert err < 1e-4, err


def test_stomp_mt19937_on_device_without_index(gpu_device):
    """tensor_args device 'cuda' (no index: the reference examples' get_torch_device() spelling) with noise='mt19937', on the
    persistent path and through sample(): same means and same generator state as noise='torch_cpu' on the same spelling."""
    g = load_golden('stomp_panda_t1')
    dev = torch.device('cuda')
    with torch.cuda.device(gpu_device):
        cost, _, _ = make_cost(g, dev)
        res = {}
        for noise in ('torch_cpu', 'mt19937'):
            torch.manual_seed(int(g['seed']))
            pl = _stomp(g, dev, cost, 3, noise)
            pl.optimize()
            pl.sample()
            torch.cuda.synchronize()
            res[noise] = (pl._particle_means.cpu(), pl.state_particles.cpu(), _state_bytes())
    assert res['mt19937'][2] == res['torch_cpu'][2]
    assert rel_err(res['mt19937'][0], res['torch_cpu'][0]) < 1e-4
    assert rel_err(res['mt19937'][1], res['torch_cpu'][1]) < 1e-4
    from motion_planning_baselines_amd import ops
    out = torch.empty(2, 100, device=dev)
    torch.manual_seed(8)
    ops.torch_cpu_normal_(out, 2)
    torch.manual_seed(8)
    assert _ulp_report(out.cpu().numpy(), torch.stack([torch.empty(100).normal_() for _ in range(2)]).numpy())[0]


def test_generator_advanced_when_a_launch_raises(gpu_device, monkeypatch):
    """optimize(20) draws in chunks of 16 + 4; when the launch after the first chunk raises, the CPU generator has still
    advanced by the draws made (as with noise='torch_cpu', which draws on the host)."""
    from motion_planning_baselines_amd import ops
    from motion_planning_baselines_amd._lib import MPBError
    g = load_golden('stomp_pm2d_c1')
    dev = gpu_device
    cost, _, _ = make_cost(g, dev)
    torch.manual_seed(4)
    pl = _stomp(g, dev, cost, 20, 'mt19937')
    s0 = torch.get_rng_state()

    def refuse(*a, **k):
        raise MPBError('refused on purpose by the test')
    monkeypatch.setattr(ops, 'stomp_run', refuse)
    with pytest.raises(MPBError, match='on purpose'):
        pl.optimize()
    after = _state_bytes()
    torch.set_rng_state(s0)
    S, d, P, H = pl.num_samples, pl.d_state_opt, pl.num_particles, pl.n_support_points
    for _ in range(16):
        torch.empty(S, d, P, H).normal_()
    assert after == _state_bytes()


_TWO_STREAMS = r"""
import sys
import torch
from motion_planning_baselines_amd import ops
from motion_planning_baselines_amd.mt19937 import MTState
dev = torch.device(sys.argv[1])
ga, gb = torch.Generator().manual_seed(1), torch.Generator().manual_seed(2)
ra, rb = torch.Generator().manual_seed(1), torch.Generator().manual_seed(2)
sa, sb = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
oa, ob = torch.empty(4, 50000, device=dev), torch.empty(4, 50000, device=dev)
torch.cuda.synchronize()
with torch.cuda.stream(sa):
    a = ops.TorchCpuGeneratorOnDevice(dev, ga)
    a.normal_(oa, 4)
with torch.cuda.stream(sb):
    b = ops.TorchCpuGeneratorOnDevice(dev, gb)
    b.normal_(ob, 4)
with torch.cuda.stream(sa):
    a.store()
with torch.cuda.stream(sb):
    b.store()
torch.cuda.synchronize()
for out, ref in ((oa, ra), (ob, rb)):
    want = torch.stack([torch.empty(50000).normal_(generator=ref) for _ in range(4)])
    assert (out.cpu() - want).abs().max().item() < 2e-6
assert torch.equal(ga.get_state(), ra.get_state()) and torch.equal(gb.get_state(), rb.get_state())
print('two streams ok')
"""


def test_draws_on_two_streams(gpu_device):
    """Two generators of the same draw shape on two streams at once: each stream has its own scratch, both draws are right.
    (In a child process: the streams it creates would shift which hardware queue later tests' side streams land on.)"""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-c', _TWO_STREAMS, str(gpu_device)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and 'two streams ok' in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
