"""-m gpu: a persistent STOMP launch writes samples, costs and weights for its LAST iteration only (include/mpb.h).

The H = 64 kernel (csrc/mpb_stomp_fused.hip) stores them once, behind its iteration loop, from what the last iteration left in
the waves' LDS tiles and registers; its two-batch layout and the generalised kernel (csrc/mpb_stomp_fused_hx.hip) store from
inside the loop under a test on the last iteration.  Checked per layout, with device-drawn and with injected noise:
  A. one launch of K = 5 iterations == five launches of one iteration (iter0 advancing): means, samples, costs, weights, bit for bit;
  B. outputs pre-filled with NaN, one launch of K = 3: every element of all three is finite and equals three single launches
     -- a wave, a batch or a chunk whose final store was lost shows as a NaN;
  C. the NaN poison of a forged model tag / one-field flag still reaches `costs` with K > 1.
The bars are equality of bits: the stores moved, the arithmetic did not.
MPB_STOMP_BATCHES is read once per process, so the forced two-batch layout runs this file as a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

# name -> (P, S, H, pos_only, scene, environment of the process, expected path: 'exchange' | 'single' | None = any persistent)
CASES = {
    'exchange_c3_shape': (16, 32, 64, False, 'spheres', {}, 'exchange'),        # C3's shape with P reduced: two workgroups per particle
    'exchange_s24_idle_waves': (5, 24, 64, False, 'spheres', {}, 'exchange'),   # second chunk: 8 of 16 waves live
    'exchange_s30': (3, 30, 64, False, 'spheres', {}, 'exchange'),              # the reference example's S
    'single_chunk_s12': (6, 12, 64, False, 'spheres', {}, 'single'),            # S <= 16: one workgroup per particle, four idle waves
    'two_batches_forced': (6, 32, 64, False, 'spheres', {'MPB_STOMP_BATCHES': '2'}, 'single'),
    'two_batches_forced_s24': (5, 24, 64, False, 'spheres', {'MPB_STOMP_BATCHES': '2'}, 'single'),   # a partial second batch
    'paired_draw_d7': (8, 32, 64, True, 'spheres', {}, 'exchange'),             # d = 7: waves 0-7 draw for two rollouts each
    'paired_draw_d7_two_batches': (5, 24, 64, True, 'spheres', {'MPB_STOMP_BATCHES': '2'}, 'single'),
    'hx_h128': (4, 32, 128, False, 'spheres', {}, None),                        # the generalised kernel, two horizon chunks
    'hx_h48': (5, 12, 48, False, 'spheres', {}, None),                          # ... one chunk, not full
    'hx_h48_several_passes': (3, 40, 48, True, 'spheres', {}, None),            # ... several passes per workgroup
    'list_scene': (6, 32, 64, False, 'list', {}, None),                         # 200 spheres + 32 boxes: the LIST instantiation
}
NOISES = ('device', 'injected')


def _setup(name, dev):
    from motion_planning_baselines_amd import geometry as G, ops, workloads
    from motion_planning_baselines_amd.planners.stomp import precision_to_scale_tril, stomp_precision_matrix
    P, S, H, pos_only, scene, _, path = CASES[name]
    wl = workloads.panda_spheres_stomp(P, dev, H=H, S=S, pos_only=pos_only)
    if scene == 'list':
        geom = ops.DeviceGeometry(wl['robot'], G.env_spheres_boxes_3d(0, 200, 32, 0.04), dev)
        assert (geom.flags & (G.GEOM_FLAG_ALL_LISTS | G.GEOM_FLAG_ALL_GRIDS)) == G.GEOM_FLAG_ALL_LISTS
        scal = (25.0, 1.0, 0.3, 2.0)              # k_sigma, weight, lr, temperature
    else:
        geom = ops.DeviceGeometry(wl['robot'], wl['field'], dev)
        scal = (1e4, 1.0, 0.1, 1e3)
    means0 = wl['means0']
    d = means0.shape[-1]
    R = stomp_precision_matrix(H, wl['params']['dt'], 0.02, dict(device='cpu', dtype=torch.float32))
    Sigma, L = torch.inverse(R).to(dev).contiguous(), precision_to_scale_tril(R).to(dev).contiguous()
    ws = ops.stomp_workspace(P, S, H, d, dev)
    got = ops.stomp_run_path(geom, ws, P, S, H, d)
    assert got != ops.STOMP_PATH_TWO_KERNEL
    if path is not None:
        assert got == (ops.STOMP_PATH_PERSISTENT_EXCHANGE if path == 'exchange' else ops.STOMP_PATH_PERSISTENT), (name, got)
    return dict(P=P, S=S, H=H, d=d, means0=means0, geom=geom, L=L, Sigma=Sigma, ws=ws, scal=scal, dev=dev)


def _bufs(c, fill=None):
    P, S, H, d, dev = c['P'], c['S'], c['H'], c['d'], c['dev']
    mk = (lambda *s: torch.empty(*s, device=dev)) if fill is None else (lambda *s: torch.full(s, fill, device=dev))
    return mk(P, S, H, d), mk(P, S), mk(P, S)


def _one_launch_and_k_launches(c, noise, K, fill=None, seed=11, iter0=5):
    """([means, samples, costs, weights] of ONE launch of K iterations -- outputs pre-filled with `fill` --, the same of K launches
    of one iteration each)."""
    from motion_planning_baselines_amd import ops
    dev = c['dev']
    eps = None
    if noise == 'injected':
        eps = torch.randn(K, c['S'], c['d'], c['P'], c['H'], generator=torch.Generator().manual_seed(4)).to(dev).contiguous()
    tail = (c['L'], c['Sigma'], c['geom'], c['S'], 7, *c['scal'], c['ws'])
    m1, out1 = c['means0'].clone(), _bufs(c, fill)
    ops.stomp_run(m1, eps, *out1, *tail, n_iters=K, seed=seed, iter0=iter0)
    torch.cuda.synchronize()
    assert not ops.stomp_run_timed_out(c['ws'])
    m2, out2 = c['means0'].clone(), _bufs(c)
    for it in range(K):
        ops.stomp_run(m2, None if eps is None else eps[it:it + 1].contiguous(), *out2, *tail, n_iters=1, seed=seed, iter0=iter0 + it)
    torch.cuda.synchronize()
    assert not ops.stomp_run_timed_out(c['ws'])
    return [m1, *out1], [m2, *out2]


_NAMES = ('means', 'samples', 'costs', 'weights')


def check_one_launch_equals_k_launches(name, noise, dev):
    c = _setup(name, dev)
    one, many = _one_launch_and_k_launches(c, noise, 5)
    for k, a, b in zip(_NAMES, one, many):
        assert torch.equal(a, b), (name, noise, k, int((a != b).sum()))
    assert torch.isfinite(one[0]).all() and float(one[2].max()) > 0
    w = one[3].double().sum(dim=1)
    assert float((w - 1).abs().max()) < 1e-4          # (the weights of a particle are a softmax)


def check_outputs_fully_written(name, noise, dev):
    c = _setup(name, dev)
    one, many = _one_launch_and_k_launches(c, noise, 3, fill=float('nan'))
    for k, a, b in zip(_NAMES[1:], one[1:], many[1:]):
        bad = ~torch.isfinite(a)
        assert not bool(bad.any()), (name, noise, k, 'elements left unwritten:', int(bad.sum()))
        assert torch.equal(a, b), (name, noise, k, int((a != b).sum()))
    assert torch.equal(one[0], many[0])


def check_poison(name, noise, dev):
    """K = 3 on the two forged-flag paths: a buffer without the model tag under flags that claim it, and (H = 64) a buffer that
    chains two fields under flags that claim one.  Every cost must be the NaN poison; the honest buffers give finite costs."""
    from motion_planning_baselines_amd import geometry as G, ops
    from motion_planning_baselines_amd.planners.stomp import precision_to_scale_tril, stomp_precision_matrix
    P, S, H, pos_only, _, _, _ = CASES[name]
    robot = G.RobotPanda()
    D = robot.q_dim
    d = D if pos_only else 2 * D
    tagged = ops.DeviceGeometry(robot, [G.env_spheres_3d()], dev)
    big = G.CollisionField(spheres=np.array([[0.5, 0.5, 0.5, 0.9], [-0.6, 0.2, 0.4, 0.1]], np.float32), margin=0.05)
    plain = ops.DeviceGeometry(robot, [big], dev)
    assert tagged.flags & G.GEOM_FLAG_MODEL_MASK and not plain.flags & G.GEOM_FLAG_MODEL_MASK and plain.flags & G.GEOM_FLAG_ALL_GRIDS
    two = ops.DeviceGeometry(robot, [G.env_spheres_3d(), G.env_spheres_3d(seed=2)], dev)
    assert tagged.flags & G.GEOM_FLAG_ONE_FIELD and not two.flags & G.GEOM_FLAG_ONE_FIELD

    class ForgedModel:
        buf, flags = plain.buf, tagged.flags

    class ForgedOneField:
        buf, flags = two.buf, tagged.flags
    R = stomp_precision_matrix(H, 0.05, 1.0, dict(device='cpu', dtype=torch.float32))
    Sigma, L = torch.inverse(R).contiguous().to(dev), precision_to_scale_tril(R).contiguous().to(dev)
    gen = torch.Generator().manual_seed(4)
    a, b = torch.rand(P, 1, D, generator=gen) * 2 - 1, torch.rand(P, 1, D, generator=gen) * 2 - 1
    s = torch.linspace(0, 1, H).reshape(1, H, 1)
    pos = a * (1 - s) + b * s
    means0 = (pos if pos_only else torch.cat([pos, torch.zeros_like(pos)], -1)).contiguous().to(dev)
    K = 3
    eps = torch.randn(K, S, d, P, H, generator=gen).to(dev).contiguous() if noise == 'injected' else None
    forged = [('model', plain, ForgedModel)] + ([('one_field', two, ForgedOneField)] if H == 64 else [])
    for kind, honest, forge in forged:
        got = {}
        for tag, gm in (('honest', honest), ('forged', forge)):
            means = means0.clone()
            samples, weights = torch.empty(P, S, H, d, device=dev), torch.empty(P, S, device=dev)
            costs = torch.zeros(P, S, device=dev)
            ws = ops.stomp_workspace(P, S, H, d, dev)
            assert ops.stomp_run_path(gm, ws, P, S, H, d) != ops.STOMP_PATH_TWO_KERNEL
            ops.stomp_run(means, eps, samples, costs, weights, L, Sigma, gm, S, D, 6.25, 1.0, 0.2, 0.7, ws, n_iters=K, seed=3)
            torch.cuda.synchronize()
            assert not ops.stomp_run_timed_out(ws)
            got[tag] = costs.cpu()
        assert torch.isfinite(got['honest']).all() and float(got['honest'].max()) > 0, (name, kind)
        assert torch.isnan(got['forged']).all(), (name, noise, kind, got['forged'])


CHECKS = {'a': check_one_launch_equals_k_launches, 'b': check_outputs_fully_written, 'c': check_poison}


def _run(check, name, noise, dev):
    env = CASES[name][5]
    if not env:
        return CHECKS[check](name, noise, dev)
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''), **env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), check, name, noise], cwd=ROOT, env=e, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize('noise', NOISES)
@pytest.mark.parametrize('name', list(CASES))
def test_one_launch_of_k_equals_k_launches_of_one(gpu_device, name, noise):
    _run('a', name, noise, gpu_device)


@pytest.mark.parametrize('noise', NOISES)
@pytest.mark.parametrize('name', list(CASES))
def test_last_iteration_outputs_are_fully_written(gpu_device, name, noise):
    _run('b', name, noise, gpu_device)


@pytest.mark.parametrize('noise', NOISES)
@pytest.mark.parametrize('name', ['single_chunk_s12', 'exchange_c3_shape', 'two_batches_forced', 'paired_draw_d7', 'hx_h128', 'hx_h48'])
def test_poison_reaches_costs_with_several_iterations(gpu_device, name, noise):
    _run('c', name, noise, gpu_device)


if __name__ == '__main__':
    assert torch.cuda.is_available(), 'needs a GPU'
    CHECKS[sys.argv[1]](sys.argv[2], sys.argv[3], torch.device('cuda:0'))
