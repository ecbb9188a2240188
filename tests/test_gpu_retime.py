"""mpb_traj_retime / mpb_traj_retime_sample on the GPU, every element of every output held to the fp64 restatement of the definition
(tests/retime_checks.py).  The bar of each element-wise check is collision_kinks.bar (factor 4, floor 2^-23) of the fp32 restatement's own
worst error on the same inputs, relative to the quantity's largest magnitude in the set: the kernel may differ from the fp32 restatement
by fma contraction only, since a minimum is exact in any order.  The restatements are computed once per set and shared."""
import ctypes
import functools
import math
import types

import numpy as np
import pytest
import torch

import retime_checks as K
from collision_kinks import bar

pytestmark = pytest.mark.gpu
DT = 1e-3                                                        # the control period of the sampling checks
DEV = 'cuda:0'


def _gpu(inp):
    return (torch.from_numpy(inp.trajs).to(DEV), torch.from_numpy(inp.v_max).to(DEV), torch.from_numpy(inp.a_max).to(DEV))


def _np(timing):
    return types.SimpleNamespace(**{k: getattr(timing, k).cpu().numpy() for k in timing._fields})


@functools.lru_cache(maxsize=None)
def _timing(name):
    """(the op's TrajTiming on the device, the same as numpy arrays) of a set: one launch, shared by the tests."""
    from motion_planning_baselines_amd import ops
    inp = K.inputs(name)
    trajs, v, a = _gpu(inp)
    tm = ops.traj_retime(trajs, v, a, sdot_max=inp.sdot_max, t_max=inp.t_max)
    torch.cuda.synchronize()
    return trajs, tm, _np(tm)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.int32)


@pytest.mark.parametrize('name', K.SETS)
def test_timing_held_to_fp64(name, gpu_device):
    inp, r64, r32 = K.reference(name)
    _, _, k = _timing(name)
    assert k.x.shape == (inp.N, inp.H) and k.u.shape == (inp.N, inp.H - 1) and k.t.shape == (inp.N, inp.H) and k.qd.shape == (inp.N, inp.H, inp.D)
    assert not k.status.any() and np.array_equal(k.duration, k.t[:, -1])
    M = float(r64.x.max())
    E32 = float(np.abs(r32.x - r64.x).max()) / M
    ex, eu = float(np.abs(k.x - r64.x).max()) / M, float(np.abs(k.u - r64.u).max()) / M
    same = float((_bits(k.x) == _bits(r32.x)).mean()), float((_bits(k.u) == _bits(r32.u)).mean())
    # qd = p_i sqrt(x_i): the same rule on its own scale
    Mq = float(np.abs(r64.qd).max())
    E32q, eq = float(np.abs(r32.qd - r64.qd).max()) / Mq, float(np.abs(k.qd - r64.qd).max()) / Mq
    # t: the first-order propagation of the bar on x through 2 / (sqrt(x_i) + sqrt(x_{i+1})), summed, plus 4 H 2^-23 t (derived)
    tb = K.time_bar(r64.x, bar(E32) * M, r64.t, inp.H)
    et = np.abs(k.t - r64.t)
    print(f'{name}: M {M:.4g}  E32 {E32:.2e}  bar {bar(E32):.2e}  kernel x {ex:.2e} u {eu:.2e}  (bits equal to the fp32 restatement: x {same[0]:.4f} '
          f'u {same[1]:.4f})  qd: E32 {E32q:.2e} kernel {eq:.2e}  t: worst error {et.max():.2e} s at a bar of {tb.reshape(-1)[et.argmax()]:.2e}, '
          f'worst error / bar {np.max(et[:, 1:] / tb[:, 1:]):.3f}, T off by at most {et[:, -1].max():.2e} s')
    assert ex <= bar(E32) and eu <= bar(E32), (ex, eu, bar(E32))
    assert eq <= bar(E32q), (eq, bar(E32q))
    assert np.all(et <= tb), float(np.max(et[:, 1:] / tb[:, 1:]))


@pytest.mark.parametrize('name', K.SETS)
def test_limits_hold_at_the_waypoints(name, gpu_device):
    """Independently of the restatement: from the kernel's own x, u, in fp64, the speeds against v and the accelerations at both ends of
    every interval against a.  The overstep, in units of 2^-23 (|p u| + |c x| + a), is at most four times the fp32 restatement's own."""
    inp, _, r32 = K.reference(name)
    _, _, k = _timing(name)
    over_v, over_a = K.overstep(inp, k.x, k.u)
    ref_v, ref_a = K.overstep(inp, r32.x, r32.u)
    print(f'{name}: overstep in rounding units: velocity {over_v:.2f} (fp32 restatement {ref_v:.2f}), acceleration {over_a:.2f} ({ref_a:.2f})')
    assert over_v <= 4.0 * max(ref_v, 1.0) and over_a <= 4.0 * max(ref_a, 1.0)
    assert not _bits(k.x[:, 0]).any() and not _bits(k.x[:, -1]).any()                      # rest to rest, exactly
    assert not k.qd[:, 0].any() and not k.qd[:, -1].any() and not _bits(k.t[:, 0]).any()   # (p_i * 0: a zero of either sign)
    assert np.all(k.x >= 0) and np.all(np.diff(k.t, axis=1) > 0)


@pytest.mark.parametrize('name', K.SETS)
def test_sampling_held_to_fp64(name, gpu_device):
    """The sampler is fed the retime kernel's own x, u, t bits; the fp64 and fp32 restatements of the sampler are fed the same."""
    from motion_planning_baselines_amd import ops
    inp = K.inputs(name)
    trajs, tm, k = _timing(name)
    want_rows = np.array([math.ceil(float(T) / float(np.float32(DT))) + 1 for T in k.duration])
    T_rows = int(want_rows.max()) + 3
    out, rows, st = (v.cpu().numpy() for v in ops.traj_retime_sample(trajs, tm, DT, n_rows=T_rows))
    assert out.shape == (inp.N, T_rows, 2 * inp.D) and not st.any()
    assert np.array_equal(rows, want_rows)                                                 # ceil(fl32(T) / dt) + 1, exactly
    o64, rows64, _ = K.sample(inp, k.x, k.u, k.t, k.status, DT, T_rows, np.float64)
    o32, _, _ = K.sample(inp, k.x, k.u, k.t, k.status, DT, T_rows, np.float32)
    assert np.array_equal(rows64, want_rows)
    D = inp.D
    for what, sl in (('position', slice(0, D)), ('velocity', slice(D, 2 * D))):
        M = float(np.abs(o64[..., sl]).max())
        E32 = float(np.abs(o32[..., sl] - o64[..., sl]).max()) / M
        e = float(np.abs(out[..., sl] - o64[..., sl]).max()) / M
        print(f'{name}: {T_rows} rows at dt = {DT}: {what}: M {M:.4g}  E32 {E32:.2e}  bar {bar(E32):.2e}  kernel {e:.2e}')
        assert e <= bar(E32), (what, e, bar(E32))
    last = inp.trajs[:, -1, :D]
    for n in range(inp.N):                                       # rows at and past n_rows hold the last waypoint at rest
        tail = out[n, rows[n]:]
        assert np.array_equal(_bits(tail[:, :D]), _bits(np.broadcast_to(last[n], tail[:, :D].shape))) and not _bits(tail[:, D:]).any()
    assert np.array_equal(_bits(out[:, 0, :D]), _bits(inp.trajs[:, 0, :D])) and not out[:, 0, D:].any()      # (p_0 * 0: a zero of either sign)
    # one row short of the longest: TOO_LONG for those that do not fit, the rows that fit unchanged; n_rows=None sizes to the longest
    short = int(want_rows.max()) - 1
    out_s, rows_s, st_s = (v.cpu().numpy() for v in ops.traj_retime_sample(trajs, tm, DT, n_rows=short))
    assert np.array_equal(st_s, np.where(want_rows > short, K.TOO_LONG, K.OK)) and st_s.any() and np.array_equal(rows_s, want_rows)
    assert np.array_equal(_bits(out_s), _bits(out[:, :short]))
    out_n, _, st_n = ops.traj_retime_sample(trajs, tm, DT)
    assert out_n.shape[1] == int(want_rows.max()) and not st_n.any() and np.array_equal(_bits(out_n.cpu().numpy()), _bits(out[:, :out_n.shape[1]]))


def test_stalled_and_stationary_trajectories(gpu_device):
    from motion_planning_baselines_amd import ops
    d = K.duplicates()
    trajs, v, a = _gpu(d)
    tm = ops.traj_retime(trajs, v, a)
    k = _np(tm)
    assert k.status.tolist() == [K.STALLED] and not np.isnan(k.x).any() and not np.isnan(k.u).any() and not np.isnan(k.t).any()
    assert np.isposinf(k.t[0, -1]) and not k.x[0, -2:].any()                               # two adjacent zeros: the last step takes forever
    out, rows, st = (t.cpu().numpy() for t in ops.traj_retime_sample(trajs, tm, 1e-2, n_rows=16))
    assert rows.tolist() == [0] and st.tolist() == [K.STALLED] and not np.isnan(out).any()
    assert not out[0, :, 0].any() and not out[0, :, 1].any()                               # every row holds the first waypoint (0) at rest
    out, rows, st = ops.traj_retime_sample(trajs, tm, 1e-2)                                # sized by the longest OK duration: none, one row
    assert out.shape == (1, 1, 2) and st.tolist() == [K.STALLED]
    # a trajectory that does not move: nothing binds but sdot_max
    q = torch.full((3, 8, 7), 0.25, device=DEV)
    tm = ops.traj_retime(q, torch.from_numpy(K.PANDA_V).float(), torch.from_numpy(K.PANDA_A).float(), sdot_max=1e3)
    k = _np(tm)
    assert not k.status.any() and np.isfinite(k.t).all() and np.all(k.x[:, 1:-1] == np.float32(1e6)) and not k.x[:, [0, -1]].any() and not k.qd.any()
    np.testing.assert_allclose(k.duration, 2 * 2e-3 + 5 * 1e-3, rtol=1e-6)
    # a trajectory slower than t_max is STALLED, with its finite timing written
    tm = ops.traj_retime(_gpu(K.inputs('panda_h16'))[0], K.PANDA_V, K.PANDA_A, t_max=1.3)
    k = _np(tm)
    assert np.array_equal(k.status, np.where(k.duration > np.float32(1.3), K.STALLED, K.OK)) and 0 < k.status.sum() < len(k.status)


def test_limits_the_python_side_would_refuse_stall_in_the_kernel(gpu_device):
    """v_max / a_max are device memory: the C side cannot see them.  A limit that is not finite and > 0 gives STALLED and zeros."""
    from motion_planning_baselines_amd import _lib, ops
    inp = K.inputs('dof2_h4')
    trajs, v, a = _gpu(inp)
    N, H, D = inp.N, inp.H, inp.D
    with pytest.raises(ValueError, match='a_max'):
        ops.traj_retime(trajs, v, torch.tensor([1.0, 0.0]))
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        for which in (0, 1):
            lim = [v.clone(), a.clone()]
            lim[which][1] = bad
            x, t = torch.full((N, H), 7.0, device=DEV), torch.full((N, H), 7.0, device=DEV)
            u, qd = torch.full((N, H - 1), 7.0, device=DEV), torch.full((N, H, D), 7.0, device=DEV)
            status = torch.full((N,), -1, device=DEV, dtype=torch.int32)
            p = lambda z: ctypes.c_void_p(z.data_ptr())
            _lib.check(_lib.lib().mpb_traj_retime(p(trajs), inp.W, p(lim[0]), p(lim[1]), p(x), p(u), p(t), p(qd), p(status), N, H, D, 1e3, 1e4,
                                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'mpb_traj_retime')
            torch.cuda.synchronize()
            assert status.tolist() == [K.STALLED] * N and not x.any() and not u.any() and not t.any() and not qd.any(), (bad, which)


def test_rows_are_read_in_place_and_runs_repeat(gpu_device):
    from motion_planning_baselines_amd import ops
    inp = K.inputs('panda_h64_w2d')
    trajs, tm, k = _timing('panda_h64_w2d')
    D = inp.D
    assert inp.W == 2 * D
    narrow = trajs[:, :, :D].contiguous()
    poisoned = trajs.clone()
    poisoned[:, :, D:] = float('nan')
    v, a = torch.from_numpy(inp.v_max), torch.from_numpy(inp.a_max)
    base = ops.traj_retime_sample(trajs, tm, DT, n_rows=2000)
    for other in (narrow, poisoned, trajs):                      # W = D, W = 2D with poisoned velocity columns, and a second run: same bits
        tm2 = ops.traj_retime(other, v, a)
        for f in tm._fields:
            assert torch.equal(getattr(tm2, f).view(torch.int32), getattr(tm, f).view(torch.int32)), f
        for one, two in zip(ops.traj_retime_sample(other, tm2, DT, n_rows=2000), base):
            assert torch.equal(one.view(torch.int32), two.view(torch.int32))
    # N = 1 (the last trajectory alone gives its own bits) and N = 0
    tm1 = ops.traj_retime(trajs[-1:].contiguous(), v, a)
    for f in tm._fields:
        assert torch.equal(getattr(tm1, f).view(torch.int32), getattr(tm, f)[-1:].view(torch.int32)), f
    one = ops.traj_retime_sample(trajs[-1:].contiguous(), tm1, DT, n_rows=2000)
    assert torch.equal(one[0].view(torch.int32), base[0][-1:].view(torch.int32)) and torch.equal(one[1], base[1][-1:])
    tm0 = ops.traj_retime(trajs[:0].contiguous(), v, a)
    assert tm0.x.shape == (0, 64) and tm0.u.shape == (0, 63) and tm0.qd.shape == (0, 64, 7) and tm0.duration.shape == (0,)
    out0, rows0, st0 = ops.traj_retime_sample(trajs[:0].contiguous(), tm0, DT)
    assert out0.shape == (0, 1, 14) and rows0.shape == (0,) and st0.shape == (0,)


def test_planning_task_retimes_a_batch_with_leading_dimensions(gpu_device):
    from motion_planning_baselines_amd import geometry as G, ops
    from motion_planning_baselines_amd.robot_field import PlanningTask
    inp = K.inputs('panda_h64_w2d')
    task = PlanningTask(G.RobotPanda(), G.env_spheres_3d(), tensor_args=dict(device=gpu_device, dtype=torch.float32))
    trajs = torch.from_numpy(inp.trajs[:10]).to(gpu_device).reshape(2, 5, inp.H, inp.W)
    res = task.retime_trajs(trajs)
    tm = ops.traj_retime(trajs.reshape(10, inp.H, inp.W), task.robot.dq_max, task.robot.ddq_max)
    assert res.durations.shape == (2, 5) and res.status.shape == (2, 5) and res.trajs_dt is None and res.n_rows is None
    assert torch.equal(res.durations.reshape(-1), tm.duration) and not res.status.any()
    assert torch.equal(res.durations, _timing('panda_h64_w2d')[1].duration[:10].reshape(2, 5))      # the Panda's limits are the set's
    slow = task.retime_trajs(trajs, scale=0.5)
    assert bool((slow.durations > res.durations).all())
    print('durations at scale 0.5 over scale 1:', (slow.durations / res.durations).reshape(-1).tolist())
    res = task.retime_trajs(trajs, dt=DT, v_max=[1.0] * 7)
    n = int(res.n_rows.max())
    assert res.trajs_dt.shape == (2, 5, n, 14) and res.n_rows.shape == (2, 5) and not res.sample_status.any()
    assert float(res.trajs_dt[..., 7:].abs().max()) <= 1.0 * 1.25                         # the cubic between waypoints: not a guarantee, a sanity bound
