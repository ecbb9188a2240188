"""-m gpu: every launch path of mpb_mppi_step under the fp64 oracle, on inputs with a SPREAD softmax.

mpb_mppi_step has three noise products (MATRIX: all samples on the matrix pipe, T <= 64; LDS: per lane against the transposed
factor in LDS; GLOBAL: the same against global memory), two noise sources (drawn / injected), a grid and an exhaustive
collision walk, one or more 64-step chunks and two softmax forms (S <= 64 on one wave, beyond that block-wide).  Until this
file the suite ran MATRIX and GLOBAL only, the device draw at one full-tile shape, no collision beyond the first chunk, and
all of it at a temperature where one sample holds all the weight (tests/mppi_path_cases.py has the shapes, the inputs and the
conditions asserted on the oracle alone; tests/test_host_logic.py pins the plans).  Every test asserts the path it is here for
through ops.mppi_plan -- the launcher's own decision -- and prints it.

Case c's scene (3-D point, 16 spheres) is grid-backed -- its plan says so -- so c is the 3-D point on the grid (z_on) beyond the first
chunk; the exhaustive walk there is case c2 (80 spheres: beyond the compact grid) and the MPB_MPPI_NO_GRID child of case c.

Bars (test_path_vs_oracle): per problem and quantity, 4 x max(E32, 4 fp32 ulps of the quantity's largest magnitude), E32 the fp32
CPU oracle's own deviation from the fp64 oracle on the same inputs; and never looser than test_mppi_shapes_vs_oracle's bars,
which are asserted beside them.

Measured on an MI355X (per case the problem that takes the largest share of its bar: kernel error against the fp64 oracle / E32 / bar, absolute):

  case  controls                          states                            costs                             weights                           mean
  a     7.58e-07 / 6.48e-07 / 9.07e-06    2.49e-07 / 1.15e-06 / 4.61e-06    1.25e-04 / 2.62e-04 / 1.05e-03    2.85e-08 / 3.43e-08 / 2.69e-07    3.66e-08 / 7.27e-08 / 3.28e-07
  b     1.93e-06 / 1.93e-06 / 1.60e-05    3.56e-07 / 1.63e-06 / 6.54e-06    3.02e-04 / 4.85e-04 / 1.94e-03    9.98e-08 / 8.61e-08 / 5.73e-07    8.89e-08 / 1.46e-07 / 5.82e-07
  c     2.61e-06 / 1.35e-06 / 1.73e-05    8.55e-07 / 1.45e-06 / 5.81e-06    4.41e-04 / 7.18e-04 / 3.93e-03    4.53e-08 / 1.30e-07 / 5.20e-07    5.76e-08 / 5.68e-08 / 4.18e-07
  c2    2.61e-06 / 1.57e-06 / 1.73e-05    8.55e-07 / 1.45e-06 / 5.81e-06    4.73e-04 / 2.14e-03 / 8.57e-03    5.62e-08 / 8.53e-08 / 3.41e-07    7.19e-08 / 1.02e-07 / 4.18e-07
  d     2.49e-06 / 2.01e-06 / 1.89e-05    7.99e-07 / 2.65e-06 / 1.06e-05    3.91e-04 / 2.89e-04 / 1.16e-03    9.64e-08 / 5.23e-08 / 2.29e-07    1.70e-07 / 6.95e-08 / 2.78e-07
  e     4.55e-06 / 4.05e-06 / 1.99e-05    1.45e-06 / 1.05e-05 / 4.20e-05    1.89e-03 / 1.63e-03 / 6.52e-03    2.39e-07 / 1.82e-07 / 7.27e-07    4.41e-07 / 7.99e-07 / 3.20e-06
  f     2.63e-06 / 2.15e-06 / 1.87e-05    3.81e-07 / 1.50e-06 / 5.99e-06    2.46e-04 / 3.73e-04 / 1.65e-03    8.72e-09 / 9.25e-09 / 4.14e-08    5.75e-08 / 3.63e-08 / 2.93e-07
  g     1.63e-06 / 1.63e-06 / 1.53e-05    2.61e-07 / 1.11e-06 / 4.43e-06    1.42e-04 / 1.57e-04 / 7.32e-04    3.99e-09 / 3.94e-09 / 3.40e-08    2.47e-08 / 2.95e-08 / 1.18e-07
  h     1.45e-06 / 1.21e-06 / 1.45e-05    2.22e-07 / 1.31e-06 / 5.22e-06    1.71e-04 / 1.52e-04 / 9.71e-04    3.19e-08 / 5.75e-08 / 2.79e-07    9.22e-08 / 5.44e-08 / 2.47e-07
  i1    1.04e-06 / 1.43e-06 / 9.61e-06    2.99e-07 / 1.15e-06 / 4.59e-06    1.63e-04 / 1.56e-04 / 6.26e-04    4.80e-08 / 6.02e-08 / 5.19e-07    4.22e-08 / 6.09e-08 / 2.58e-07
  i2    2.59e-06 / 2.11e-06 / 1.89e-05    2.85e-07 / 1.45e-06 / 5.81e-06    3.08e-04 / 2.55e-04 / 1.15e-03    4.87e-08 / 3.06e-08 / 1.22e-07    8.10e-08 / 6.62e-08 / 4.14e-07

The largest share of its bar any quantity takes: 0.61 (case d, mean).  No quantity needs a factor above 4.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mppi_path_cases as M
from conftest import ROOT

pytestmark = pytest.mark.gpu


def _same_bits(a, b, what):
    for k in M.OUTPUTS:
        assert torch.equal(a[k], b[k]), (what, k, float((a[k] - b[k]).abs().max()))


@pytest.mark.parametrize('name', list(M.CASES))
def test_path_vs_oracle(gpu_device, name):
    """Two iterations in one launch with the best sample tracked: drawn == injected bit for bit, and the kernel against the fp64
    oracle on the normals it drew, per problem, at 4 x max(E32, floor)."""
    from motion_planning_baselines_amd import ops
    dev = gpu_device
    pr = M.problem(name)
    geom = M.device_geometry(pr, dev)
    print(M.device_plan(name, pr, geom, False))
    print(M.device_plan(name, pr, geom, True))
    nrm = ops.debug_mppi_normals(pr.NP, pr.S, pr.T, pr.c, M.N_IT, dev, seed=M.SEED, iter0=M.ITER0)
    torch.cuda.synchronize()
    assert torch.isfinite(nrm).all() and float(nrm.abs().max()) <= 5.66
    eps = nrm.cpu()
    ref64, ref32 = M.oracle_run(pr, eps, torch.float64), M.oracle_run(pr, eps, torch.float32)
    M.check_conditions(name, pr, ref64)                     # (the oracle alone, before anything of the kernel's is looked at)
    drawn, injected = M.launch(pr, geom, dev, None), M.launch(pr, geom, dev, nrm)
    _same_bits(drawn, injected, (name, 'drawn != injected'))
    bars = M.bars(ref32, ref64)
    got = {k: v.cpu().double() for k, v in drawn.items()}
    failed = []
    for p in range(pr.NP):
        r = ref64[p]
        want = dict(controls=r.controls, states=r.states, costs=r.costs, weights=r.weights, mean=r.mean)
        for k in M.QUANTITIES:
            err = float((got[k][p] - want[k]).abs().max())
            e32, bar = bars[p][k]
            print('case %s problem %d %-8s err %.2e  E32 %.2e  bar %.2e  (%.2f of the bar)  min ESS %.1f' % (
                name, p, k, err, e32, bar, err / bar, min(r.ess)))
            if not err <= bar:
                failed.append((name, p, k, err, e32, bar))
    assert not failed, ('(case, problem, quantity, error, E32, bar)', failed)
    for p in range(pr.NP):       # ... and test_mppi_shapes_vs_oracle's own bars, so that none of the above is looser
        r = ref64[p]
        want = dict(controls=r.controls, states=r.states, mean=r.mean)
        rel = lambda k: float((got[k][p] - want[k]).abs().max() / want[k].abs().max())
        assert rel('controls') < 1e-4 and rel('states') < 1e-4 and rel('mean') < 2e-4, (name, p)
        np.testing.assert_allclose(got['costs'][p].numpy(), r.costs.numpy(), rtol=2e-4)
        np.testing.assert_allclose(got['weights'][p].numpy(), r.weights.numpy(), rtol=5e-2, atol=1e-5)
        np.testing.assert_allclose(float(got['best_cost'][p]), r.best_cost, rtol=2e-4)


@pytest.mark.parametrize('name', ['c', 'f', 'h'])
def test_best_is_the_first_cheapest_sample_bit_for_bit(gpu_device, name):
    """After ONE iteration from a fresh best_cost: best_cost is costs.min() and best_states the states of the first argmin, bit
    for bit -- save-best redoes the winner's rollout from its controls in LDS with the arithmetic of the first one."""
    dev = gpu_device
    pr = M.problem(name)
    geom = M.device_geometry(pr, dev)
    print(M.device_plan(name, pr, geom, False))
    o = M.launch(pr, geom, dev, None, n_iters=1)
    assert pr.S > 2
    for p in range(pr.NP):
        win = int(o['costs'][p].argmin())                    # (first index on ties, like the kernel)
        assert float(o['best_cost'][p]) == float(o['costs'][p].min()), (name, p)
        assert torch.equal(o['best_states'][p], o['states'][p, win]), (name, p, win,
                                                                      float((o['best_states'][p] - o['states'][p, win]).abs().max()))


_CHILD = r"""
import sys, numpy as np, torch
import mppi_path_cases as M
from motion_planning_baselines_amd import ops
name, out = sys.argv[1], sys.argv[2]
dev = torch.device('cuda:0')
pr = M.problem(name)
geom = M.device_geometry(pr, dev)
pl = ops.mppi_plan(geom, pr.NP, pr.S, pr.T, pr.c)
o = M.launch(pr, geom, dev, None)
np.savez(out, plan=np.array(tuple(pl)), **{k: v.cpu().numpy() for k, v in o.items()})
"""


def test_lds_product_equals_global_product_and_grid_equals_exhaustive(gpu_device, tmp_path):
    """Case c (T = 72: two chunks, collision in the second, 3-D point on the grid) in fresh child processes under MPB_MPPI_NOISE=1
    (LDS) and =0 (GLOBAL) -- both accumulate fmaf in ascending k up to the same kend -- and under MPB_MPPI_NO_GRID=1 (the
    exhaustive walk at base > 0; the grid only culls).  The variables are read once per process.  The parent's own natural run
    (LDS, grid) equals all three bit for bit."""
    dev = gpu_device
    name = 'c'
    pr = M.problem(name)
    geom = M.device_geometry(pr, dev)
    print(M.device_plan(name, pr, geom, False))
    mine = {k: v.cpu().numpy() for k, v in M.launch(pr, geom, dev, None).items()}
    cs = M.CASES[name]
    for var, val, mode, grid in (('MPB_MPPI_NOISE', '1', M.NOISE_LDS, cs.grid_words), ('MPB_MPPI_NOISE', '0', M.NOISE_GLOBAL, cs.grid_words),
                                 ('MPB_MPPI_NO_GRID', '1', M.NOISE_LDS, 0)):
        out = str(tmp_path / ('%s_%s.npz' % (var, val)))
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, 'tests'), os.environ.get('PYTHONPATH', '')]))
        env[var] = val
        r = subprocess.run([sys.executable, '-c', _CHILD, name, out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        res = np.load(out)
        print('child %s=%s: plan %s, grid_words %d' % (var, val, M.MODE_NAME[int(res['plan'][0])], int(res['plan'][2])))
        assert (int(res['plan'][0]), int(res['plan'][2])) == (mode, grid), (var, val, res['plan'])
        for k in M.OUTPUTS:
            assert res[k].tobytes() == mine[k].tobytes(), (var, val, k)
    assert float(mine['best_cost'].max()) < 1e30 and np.isfinite(mine['mean']).all()


@pytest.mark.parametrize('name', ['d', 'h'])
def test_one_launch_equals_one_launch_per_iteration(gpu_device, name):
    """n_iters = 3 in one launch == three launches of one iteration with iter0 = 0, 1, 2 (device noise): mean and the last
    iteration's outputs, and best_cost / best_states -- what carries over between calls -- bit for bit."""
    dev = gpu_device
    pr = M.problem(name)
    geom = M.device_geometry(pr, dev)
    print(M.device_plan(name, pr, geom, False))
    one = M.launch(pr, geom, dev, None, n_iters=3, iter0=0)
    o = None
    for it in range(3):
        o = M.launch(pr, geom, dev, None, n_iters=1, iter0=it, mean=None if o is None else o['mean'],
                     best=None if o is None else (o['best_cost'], o['best_states']))
    _same_bits(one, o, (name, 'one launch != three'))
    assert float(one['best_cost'].max()) < 1e30


@pytest.mark.parametrize('name', ['a', 'h'])
def test_a_problems_bits_do_not_depend_on_np(gpu_device, name):
    """include/mpb.h: a problem's outputs are the same bits whatever NP is.  Three problems in one launch (injected normals) equal
    each problem launched alone."""
    dev = gpu_device
    pr = M.problem(name, NP=3)
    geom = M.device_geometry(pr, dev)
    print(M.device_plan(name, pr, geom, True))
    eps = torch.randn(M.N_IT, pr.NP, pr.c, pr.S, pr.T, generator=torch.Generator().manual_seed(17)).to(dev)
    batch = M.launch(pr, geom, dev, eps)
    for p in range(pr.NP):
        alone = M.launch(pr, geom, dev, eps[:, p:p + 1].contiguous(), problems=slice(p, p + 1))
        for k in M.OUTPUTS:
            assert torch.equal(batch[k][p:p + 1], alone[k]), (name, p, k)
    assert float(batch['best_cost'].max()) < 1e30
