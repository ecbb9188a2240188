"""mpb_path_blend / mpb_path_blend_sample without a device: the definition as tests/path_blend_checks.py restates it against its three
guarantees, the sampler against the integrals of its own derivatives, convergence in fp32, the layout header, the
symbols and their binding, the host-side refusals in the order include/mpb.h gives them, what the compiler made of the two kernels, and
the argument errors of the Python surface."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import path_blend_checks as K
from conftest import ROOT

INVALID, UNSUPPORTED = 1, 2
NAMES = ('mpb_path_blend', 'mpb_path_blend_sample')
CASES = [(name, delta) for name in K.SETS for delta in K.DELTAS]


# ---- the definition ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,delta', CASES)
def test_restatement_keeps_its_guarantees_and_fp32_converges(name, delta):
    """Guarantees 1 and 2 of restate(fp64) from its own T and tb, to 1e-12 relative: the velocity limit on every segment, the
    acceleration limit in every blend, blends that do not overlap, the deviation below the cap.  restate(fp32) converges within the
    default sweep limit: every path of every set is OK in both precisions."""
    inp, r64, r32 = K.reference(name, delta)
    assert not r64.status.any() and not r32.status.any() and r32.sweeps.max() <= K.MAX_SWEEPS
    v, dv, a = K.kinematics(inp, r64.T, r64.tb, np.float64)
    vm, am = inp.v_max.astype(np.float64), inp.a_max.astype(np.float64)
    assert np.all(np.abs(v) <= vm * (1 + 1e-12)) and np.all(np.abs(a) <= am * (1 + 1e-12))
    for n in range(inp.N):
        L = int(inp.lengths[n])
        T, tb = r64.T[n, :L - 1], r64.tb[n, :L]
        assert np.all(T > 0) and np.all(tb[:-1] <= T * (1 + 1e-12)) and np.all(tb[1:] <= T * (1 + 1e-12))
        assert np.all(r64.T[n, L - 1:] == 0) and np.all(r64.tb[n, L:] == 0) and np.all(r64.tw[n, L:] == 0) and np.all(r64.dev[n, L:] == 0)
        assert r64.tw[n, 0] == tb[0] / 2 and r64.duration[n] == r64.tw[n, L - 1] + tb[-1] / 2
    dev_k = np.abs(dv) * r64.tb[:, :, None] / 8.0
    np.testing.assert_allclose(dev_k.max(2), r64.dev, rtol=1e-12, atol=0)
    if np.isfinite(delta):
        assert np.all(dev_k <= delta * (1 + 1e-12))


@pytest.mark.parametrize('name', ['panda_h16', 'lengths_h16', 'dof2_h4', 'panda_h3', 'panda_h2', 'collinear_h5'])
def test_sampled_restatement_integrates_and_stays_within_dev_of_the_polyline(name):
    """restate(fp64) sampled at 4 001 evenly spaced times of three paths: positions are the integral of the velocities and velocities the
    integral of the accelerations, by the trapezoid rule within its error bound -- qd is piecewise linear and qdd piecewise constant
    with at most 2L kinks / jumps (the window boundaries), a step of width h without one is integrated exactly, a step with a kink of
    qd (slope change at most 2 a_k) is off by at most 2 a_k h^2 / 8, a step with a jump of qdd (at most 2 a_k) by at most a_k h: the bound
    at time tau is those times the number of window boundaries up to tau, plus 1e-9 for the sums' rounding.  The trajectory starts and
    ends on the end waypoints at rest, and every sample is within dev_ik of the polyline point guarantee 2 names, per joint."""
    inp, r64, _ = K.reference(name, 0.05)
    D, M = inp.D, 4001
    am = inp.a_max.astype(np.float64)
    v, dv, a = K.kinematics(inp, r64.T, r64.tb, np.float64)
    dev_k = np.abs(dv) * r64.tb[:, :, None] / 8.0
    for n in (0, 1, inp.N - 1):
        L = int(inp.lengths[n])
        one = K.types.SimpleNamespace(**{**vars(inp), 'paths': inp.paths[n:n + 1], 'lengths': inp.lengths[n:n + 1], 'N': 1})
        tau = np.linspace(0.0, float(r64.duration[n]), M)
        h = tau[1] - tau[0]
        out, _, st = K.sample(one, r64.T[n:n + 1], r64.tb[n:n + 1], r64.tw[n:n + 1], r64.duration[n:n + 1], r64.status[n:n + 1], 1e-3, M, np.float64, tau=tau)
        q, qd, qdd = out[0, :, :D], out[0, :, D:2 * D], out[0, :, 2 * D:]
        q0, q1 = inp.paths[n, 0, :D].astype(np.float64), inp.paths[n, L - 1, :D].astype(np.float64)
        assert np.array_equal(q[0], q0) and np.array_equal(q[-1], q1) and not qd[0].any() and not qd[-1].any()
        assert np.all(np.abs(qd) <= inp.v_max * (1 + 1e-12)) and np.all(np.abs(qdd) <= am * (1 + 1e-12))
        tw, tb = r64.tw[n, :L], r64.tb[n, :L]
        kinks = np.searchsorted(np.sort(np.concatenate([tw - tb / 2, tw + tb / 2])), tau, side='right')[:, None]
        int_qd = np.concatenate([np.zeros((1, D)), np.cumsum((qd[1:] + qd[:-1]) * (h / 2), 0)])
        int_qdd = np.concatenate([np.zeros((1, D)), np.cumsum((qdd[1:] + qdd[:-1]) * (h / 2), 0)])
        assert np.all(np.abs(q - q0 - int_qd) <= kinks * (2 * am * h * h / 8) + 1e-9)
        assert np.all(np.abs(qd - int_qdd) <= kinks * (am * h) + 1e-9)
        # guarantee 2: the polyline point at the same tau on the side of the window tau is on
        p = K.polyline_at(inp, n, r64.tw, tau)
        inside = np.abs(tau[:, None] - tw[None, :]) <= tb[None, :] / 2                       # (4001, L): windows do not overlap
        bound = np.where(inside.any(1)[:, None], dev_k[n, inside.argmax(1)], 0.0)
        assert np.all(np.abs(q - p) <= bound * (1 + 1e-9) + 1e-12), float((np.abs(q - p) - bound).max())


def test_guarantee_3_spheres_stay_within_the_reach_weighted_deviation():
    """Every collision sphere of the Panda on the blended trajectory is within sum_k rho_kl dev_ik of where it is on the polyline point
    of guarantee 2 (fp64 forward kinematics of tests/certify_checks.py, the reach table of the certifier)."""
    import certify_checks as C
    from motion_planning_baselines_amd import blend_layout as BL
    sc = C.scene('panda')
    inp, r64, _ = K.reference('panda_h16', np.inf)
    dev_k = BL.joint_deviation(inp.paths[:, :, :7], r64.T, r64.tb)
    assert np.allclose(dev_k.max(2), r64.dev, rtol=1e-12, atol=0)
    dev_w = BL.workspace_deviation(sc.rho, dev_k)
    for n in (0, 5, 36):
        tau = np.linspace(0.0, float(r64.duration[n]), 801)
        one = K.types.SimpleNamespace(**{**vars(inp), 'paths': inp.paths[n:n + 1], 'lengths': inp.lengths[n:n + 1], 'N': 1})
        out, _, _ = K.sample(one, r64.T[n:n + 1], r64.tb[n:n + 1], r64.tw[n:n + 1], r64.duration[n:n + 1], r64.status[n:n + 1], 1e-3, 801, np.float64, tau=tau)
        moved = np.linalg.norm(C.centres(sc, out[0, :, :7]) - C.centres(sc, K.polyline_at(inp, n, r64.tw, tau)), axis=-1)     # (801, links)
        tw, tb = r64.tw[n], r64.tb[n]
        inside = np.abs(tau[:, None] - tw[None, :]) <= tb[None, :] / 2
        bound = np.where(inside.any(1)[:, None], dev_k[n, inside.argmax(1)] @ sc.rho.astype(np.float64), 0.0)
        assert np.all(moved <= bound * (1 + 1e-9) + 1e-12) and moved.max() <= dev_w[n] and moved.max() > 0.01 * dev_w[n]


def test_statuses_of_the_restatement():
    for dtype in (np.float64, np.float32):
        r = K.restate(K.inputs('duplicate'), dtype)
        assert r.status.tolist() == [K.OK, K.DEGENERATE_SEGMENT, K.OK] and r.first_bad.tolist() == [-1, 4, -1]
        assert not r.T[1].any() and not r.tb[1].any() and not r.tw[1].any() and not r.dev[1].any() and r.duration[1] == 0
        r = K.restate(K.inputs('bad_input'), dtype)
        assert r.status.tolist() == [K.BAD_INPUT, K.OK, K.BAD_INPUT, K.BAD_INPUT, K.BAD_INPUT, K.OK] and (r.first_bad == -1).all()
        inp = K.inputs('collinear_h5')
        r = K.restate(inp, dtype)
        assert not r.status.any() and np.all(r.tb[:, 2] == 0) and np.all(r.dev[:, 2] == 0) and np.all(r.tb[:, 1] > 0)
        assert not K.kinematics(inp, r.T, r.tb, dtype)[2][:, 2].any()                       # a == 0 there
    r32 = K.restate(K.inputs('needs_sweeps'), np.float32)
    assert not r32.status.any() and r32.sweeps.tolist() == [1, 2, 1, 2]
    one = K.restate(K.inputs('needs_sweeps'), np.float32, max_sweeps=1)
    assert one.status.tolist() == [K.OK, K.NOT_CONVERGED, K.OK, K.NOT_CONVERGED] and one.sweeps.tolist() == [1, 1, 1, 1]
    assert not one.T[1].any() and one.duration[1] == 0 and np.array_equal(one.T[0], r32.T[0])


def test_hand_off_paths_are_what_the_prototype_says():
    """The paths of the certificate hand-off (path_blend_checks.handoff) on the CPU prototype: the fp64 certifier finds every path FREE, and
    with restate(fp64) at least one path is certified at delta = 0.01 that is not at delta = inf, and some never are."""
    import certify_checks as C
    from motion_planning_baselines_amd import blend_layout as BL, certify_layout as CL
    sc, inp = K.handoff()
    certs = [C.certify_ref(sc, q, CL.CERT_DEFAULT_SLACK) for q in inp.paths]
    assert inp.N == 10 and all(c['status'] == C.FREE for c in certs)
    margin = np.array([c['margin_cert'] for c in certs])
    certified = {}
    for delta in K.DELTAS:
        r = K.restate(inp, np.float64, delta)
        dev_w = BL.workspace_deviation(sc.rho, BL.joint_deviation(inp.paths, r.T, r.tb))
        certified[delta] = (r.status == K.OK) & (dev_w < margin)
        print(f'delta {delta}: deviation_workspace {np.round(dev_w, 4).tolist()} margin_cert {np.round(margin, 4).tolist()}')
        if np.isfinite(delta):                                       # a point robot's bound: delta times the largest column sum of rho
            assert np.all(dev_w <= delta * sc.rho.astype(np.float64).sum(0).max() * (1 + 1e-12))
    assert (certified[0.01] & ~certified[np.inf]).any() and certified[np.inf].any() and not certified[0.01].all()
    assert certified[np.inf].tolist() == [1, 0, 1, 1, 1, 1, 0, 1, 0, 1] and certified[0.01].tolist() == [1, 0, 1, 1, 1, 1, 0, 1, 1, 1]
    # far from a tie: the device's fp32 margin_cert and T, tb decide every path the same way
    for delta in K.DELTAS:
        r = K.restate(inp, np.float64, delta)
        dev_w = BL.workspace_deviation(sc.rho, BL.joint_deviation(inp.paths, r.T, r.tb))
        assert np.all(np.abs(dev_w - margin) > 1e-3)


def test_measured_constants_are_what_the_checks_module_measures():
    """E32 and the overstep of restate(fp32) recorded in path_blend_checks (and DESIGN.md 10) bound what measure() finds now."""
    worst, over = K.measure()
    assert all(worst[k] <= K.E32_MEASURED[k] for k in worst), worst
    assert max(over) <= K.OVERSTEP_MEASURED, over


# ---- the layout and the library ------------------------------------------------------------------------------------------------------
def test_layout_header_is_generated_and_listed():
    from motion_planning_baselines_amd import blend_layout as BL, build, model_gen
    assert open(model_gen.BLEND_LAYOUT_HEADER).read() == model_gen.blend_layout_header_text()
    assert not model_gen.stale_headers()
    assert 'mpb_blend_layout.h' in open(build.__file__).read() and 'mpb_path_blend.hip' in build.SOURCES
    hdr = open(os.path.join(ROOT, 'include', 'mpb.h')).read()
    assert '#include "mpb_blend_layout.h"' in hdr
    lay = open(model_gen.BLEND_LAYOUT_HEADER).read()
    for i, code in enumerate(BL.STATUS):
        assert f'#define MPB_BLEND_{code} {i}\n' in lay and getattr(K, code) == i
    assert f'#define MPB_BLEND_DEFAULT_MAX_SWEEPS {BL.BLEND_DEFAULT_MAX_SWEEPS}\n' in lay


def test_symbols_are_exported_and_bound_and_the_abi_version_stays():
    from motion_planning_baselines_amd import _lib, ops
    h = _lib.lib()
    for name, n_args in zip(NAMES, (19, 17)):
        assert name in _lib.SIGNATURES and hasattr(h, name) and len(_lib.SIGNATURES[name]) == n_args
    hdr = open(os.path.join(ROOT, 'include', 'mpb.h')).read()
    assert re.search(r'int mpb_path_blend\(const float \*paths, size_t row_stride, const int \*lengths, const float \*v_max, const float \*a_max,', hdr)
    assert re.search(r'int mpb_path_blend_sample\(const float \*paths, size_t row_stride, const int \*lengths, const float \*T, const float \*tb,', hdr)
    assert (h.mpb_version() & 0xFFFF) == _lib.ABI_VERSION == 7                                  # additive: the ABI version stays
    for i, code in enumerate(ops.BLEND_STATUS):
        assert getattr(ops, 'BLEND_' + code) == i == getattr(K, code)
    f, i, p, z = ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert _lib.SIGNATURES[NAMES[0]] == [p, z, p, p, p, f, i, p, p, p, p, p, p, p, p, i, i, i, p]
    assert _lib.SIGNATURES[NAMES[1]] == [p, z, p, p, p, p, p, p, p, p, p, i, i, i, f, i, p]


def _blend(h, **kw):
    p = ctypes.c_void_p
    a = dict(paths=4096, row_stride=14, lengths=4096, v_max=4096, a_max=4096, max_deviation=0.05, max_sweeps=64, T=4096, tb=4096, tw=4096,
             dev=4096, duration=4096, sweeps=4096, status=4096, first_bad=4096, N=3, H=8, D=7)
    a.update(kw)
    rc = h.mpb_path_blend(p(a['paths']), a['row_stride'], p(a['lengths']), p(a['v_max']), p(a['a_max']), a['max_deviation'], a['max_sweeps'],
                          p(a['T']), p(a['tb']), p(a['tw']), p(a['dev']), p(a['duration']), p(a['sweeps']), p(a['status']), p(a['first_bad']),
                          a['N'], a['H'], a['D'], p(0))
    return rc, h.mpb_last_error().decode()


def _sample(h, **kw):
    p = ctypes.c_void_p
    a = dict(paths=4096, row_stride=14, lengths=4096, T=4096, tb=4096, tw=4096, duration=4096, blend_status=4096, out=4096, n_rows=4096,
             status=4096, N=3, H=8, D=7, dt=1e-3, T_rows=100)
    a.update(kw)
    rc = h.mpb_path_blend_sample(p(a['paths']), a['row_stride'], p(a['lengths']), p(a['T']), p(a['tb']), p(a['tw']), p(a['duration']),
                                 p(a['blend_status']), p(a['out']), p(a['n_rows']), p(a['status']), a['N'], a['H'], a['D'], a['dt'], a['T_rows'], p(0))
    return rc, h.mpb_last_error().decode()


def _ladder(call, name, ladder):
    """Each refusal alone and together with every later one: the earlier check answers."""
    from motion_planning_baselines_amd import _lib
    h = _lib.lib()
    for i, (bad, code, word) in enumerate(ladder):
        rc, msg = call(h, **bad)
        assert rc == code and msg.startswith(name + ':') and word in msg, (bad, rc, msg)
        later = {}
        for other, _, _ in ladder[i + 1:]:
            later.update(other)
            rc, msg = call(h, **{**later, **bad})
            assert rc == code and word in msg, (bad, later, rc, msg)
    return h


def test_refusals_that_need_no_device_in_the_stated_order():
    """Nothing is launched by any of these calls: every pointer is null or a host address that is never dereferenced."""
    nan, inf = float('nan'), float('inf')
    h = _ladder(_blend, NAMES[0], [(dict(D=13), UNSUPPORTED, 'MPB_MAX_DOF'), (dict(H=257), UNSUPPORTED, 'MPB_MAX_H'),
                                   (dict(N=-1), INVALID, 'bad shape'), (dict(max_deviation=0.0), INVALID, 'max_deviation'),
                                   (dict(max_sweeps=0), INVALID, 'max_sweeps'), (dict(first_bad=0), INVALID, 'null pointer')])
    for bad in (dict(H=1), dict(D=0), dict(row_stride=6)):
        rc, msg = _blend(h, **bad)
        assert rc == INVALID and 'bad shape' in msg, (bad, msg)
    assert 'null pointer' in _blend(h, H=256, D=12, row_stride=12, T=0)[1] and 'null pointer' in _blend(h, H=2, T=0)[1]
    for v in (0.0, -0.0, -1.0, nan, -inf):
        assert 'max_deviation' in _blend(h, max_deviation=v)[1], v
    assert 'null pointer' in _blend(h, max_deviation=inf, T=0)[1]                        # +inf is "no cap", not a refusal
    for ptr in ('paths', 'v_max', 'a_max', 'T', 'tb', 'tw', 'dev', 'duration', 'sweeps', 'status', 'first_bad'):
        rc, msg = _blend(h, **{ptr: 0})
        assert rc == INVALID and 'null pointer' in msg, ptr
    assert _blend(h, N=0)[0] == 0 and _blend(h, N=0, lengths=0, max_deviation=inf)[0] == 0     # an empty batch: MPB_OK, nothing launched ...
    assert _blend(h, N=0, status=0)[0] == INVALID and _blend(h, N=0, H=1)[0] == INVALID       # ... but only after every check above

    h = _ladder(_sample, NAMES[1], [(dict(D=13), UNSUPPORTED, 'MPB_MAX_DOF'), (dict(H=257), UNSUPPORTED, 'MPB_MAX_H'),
                                    (dict(H=1), INVALID, 'bad shape'), (dict(dt=nan), INVALID, 'dt'), (dict(T_rows=0), INVALID, 'T_rows'),
                                    (dict(out=0), INVALID, 'null pointer')])
    for bad in (dict(N=-1), dict(D=0), dict(row_stride=6)):
        rc, msg = _sample(h, **bad)
        assert rc == INVALID and 'bad shape' in msg, (bad, msg)
    for v in (0.0, -0.0, -1e-3, inf, -inf):
        assert 'dt' in _sample(h, dt=v)[1], v
    rc, msg = _sample(h, N=2 ** 20, T_rows=2 ** 30)
    assert rc == INVALID and 'blocks' in msg
    for ptr in ('paths', 'T', 'tb', 'tw', 'duration', 'blend_status', 'out', 'n_rows', 'status'):
        rc, msg = _sample(h, **{ptr: 0})
        assert rc == INVALID and 'null pointer' in msg, ptr
    assert _sample(h, N=0)[0] == 0 and _sample(h, N=0, lengths=0)[0] == 0 and _sample(h, N=0, status=0)[0] == INVALID


def test_the_kernels_keep_out_of_scratch():
    """build() records what the compiler made of every kernel (csrc/kernel_resources.json): neither new kernel spills, and the blend
    kernel's LDS is dynamic alone (sized to the path)."""
    from motion_planning_baselines_amd import build
    build.build(verbose=False)
    res = json.load(open(build.RESOURCES))
    new = {k: v for k, v in res.items() if 'path_blend' in k}
    assert sorted(new) == ['_Z17path_blend_kernel6PbArgs', '_Z24path_blend_sample_kernel12PbSampleArgs'], sorted(new)
    for name, r in new.items():
        print(name, r)
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0 and r['lds'] == 0 and r['occupancy'] == 8, (name, r)


# ---- the Python surface ----------------------------------------------------------------------------------------------------------------
def _task(robot):
    from motion_planning_baselines_amd.robot_field import PlanningTask
    task = PlanningTask.__new__(PlanningTask)                    # (the constructor needs a device; these errors do not)
    task.robot, task.q_dim, task.device = robot, robot.q_dim, torch.device('cpu')
    return task


def test_blend_paths_argument_errors_that_need_no_device():
    from motion_planning_baselines_amd import geometry as G, ops
    from motion_planning_baselines_amd._lib import MPBError
    paths = torch.zeros(4, 8, 2)
    with pytest.raises(ValueError, match='no v_max given and the robot carries no dq_max'):
        _task(G.RobotPointMass(2)).blend_paths(paths)
    with pytest.raises(ValueError, match='no a_max given and the robot carries no ddq_max'):
        _task(G.RobotPointMass(2)).blend_paths(paths, v_max=[1.0, 1.0])
    task = _task(G.RobotPointMass(2, dq_max=[1.0, 1.0], ddq_max=[2.0, 2.0]))
    with pytest.raises(ValueError, match='a_max has 3 entries'):
        task.blend_paths(paths, a_max=[1.0, 1.0, 1.0])
    for scale in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='scale'):
            task.blend_paths(paths, scale=scale)
    with pytest.raises(ValueError, match='expected \\(..., H, W\\)'):
        task.blend_paths(torch.zeros(4, 8, 1))
    with pytest.raises(MPBError, match='no CPU fallback'):                                # the op itself refuses CPU tensors
        task.blend_paths(paths)
    with pytest.raises(MPBError, match='no CPU fallback'):
        ops.path_blend(paths, [1.0, 1.0], [1.0, 1.0])
    timing = ops.BlendTiming(*[torch.zeros(1)] * 8, None, float('inf'), 2)
    with pytest.raises(MPBError, match='no CPU fallback'):
        ops.path_blend_sample(paths, timing, 1e-3)


def test_host_deviation_helpers_agree_with_the_restatement():
    from motion_planning_baselines_amd import blend_layout as BL
    inp, r64, _ = K.reference('lengths_h16', 0.05)
    dev_k = BL.joint_deviation(inp.paths[:, :, :7], r64.T, r64.tb, inp.lengths)
    assert np.isfinite(dev_k).all() and np.allclose(dev_k.max(2), r64.dev, rtol=1e-12, atol=0)
    rho = np.arange(1, 7 * 3 + 1, dtype=np.float64).reshape(7, 3)
    w = BL.workspace_deviation(rho, dev_k)
    assert w.shape == (inp.N,) and np.allclose(w, np.einsum('nik,kl->nil', dev_k, rho).max((1, 2)))
