"""CPU: the end-effector pose cost (csrc/mpb_ee_cost.hip, CostEEPose) as far as no device is needed -- the two symbols and their bindings,
what the compiler made of the kernels, the launchers' refusals, the class's argument errors, its dense linear system on the fp64
restatement -- and the conditions on the input sets that tests/test_gpu_ee_cost.py relies on, asserted on tests/ee_cost_checks.py alone."""
import ctypes
import json
import math
import os
import re

import pytest
import torch

import ee_cost_checks as E
import ik_checks as K

INVALID, UNSUPPORTED = 1, 2          # include/mpb.h MPB_E_INVALID, MPB_E_UNSUPPORTED
NAMES = ('mpb_ee_cost_eval', 'mpb_ee_cost_grad')


def test_header_and_binding_agree_on_the_new_signatures():
    from motion_planning_baselines_amd import _lib
    h = _lib.lib()
    text = open(os.path.join(__import__('conftest').ROOT, 'include', 'mpb.h')).read()
    kinds = {'int': ctypes.c_int, 'float': ctypes.c_float}
    for name in NAMES:
        assert hasattr(h, name) and name in _lib.SIGNATURES
        m = re.search(r'^int %s\((.*?)\);' % name, text, re.S | re.M)
        assert m, name
        params = [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]
        want = [ctypes.c_void_p if '*' in p else kinds[p.split()[0]] for p in params]
        assert want == _lib.SIGNATURES[name], (name, params)
        assert len(want) == 23
    assert (h.mpb_version() & 0xFFFF) == _lib.ABI_VERSION == 7                                 # additive: the ABI version stays


def test_kernels_keep_their_state_in_registers_and_the_ik_kernels_are_unchanged():
    """csrc/kernel_resources.json: the twelve new kernels (wave / lane form x three term sets x cost / gradient) have no scratch, no
    spills of either register file and no LDS; the pose and IK kernels, whose shared pieces moved into csrc/mpb_ee.h, keep the figures
    they had before the move (recorded from the parent commit's build)."""
    from motion_planning_baselines_amd import build
    build.build(verbose=False)
    res = json.load(open(build.RESOURCES))
    new = {k: v for k, v in res.items() if 'ee_cost_wave_kernel' in k or 'ee_cost_lane_kernel' in k}
    assert len(new) == 12, sorted(new)
    for name, r in new.items():
        print(name, r)
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0 and r['lds'] == 0, (name, r)
    before = {'_Z17fk_ee_pose_kernelPKfS0_PfS1_ii': dict(sgprs=70, vgprs=100, scratch=0, sgpr_spill=0, vgpr_spill=0),
              '_Z15ik_solve_kernelILb1EEvPKfS1_S1_S1_S1_PfS2_S2_PhPiiiiifff': dict(sgprs=106, vgprs=133, scratch=0, sgpr_spill=0, vgpr_spill=0),
              '_Z15ik_solve_kernelILb0EEvPKfS1_S1_S1_S1_PfS2_S2_PhPiiiiifff': dict(sgprs=106, vgprs=179, scratch=0, sgpr_spill=2, vgpr_spill=0)}
    for name, want in before.items():
        assert {k: res[name][k] for k in want} == want, (name, res[name])


def test_refusals_that_need_no_device_in_the_stated_order():
    from motion_planning_baselines_amd import _lib
    h = _lib.lib()
    null, p, odd = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 8)      # (never dereferenced on these paths)
    err = lambda: h.mpb_last_error().decode()

    def call(fn, ptr=p, geom=p, B=4, H=8, d=7, D=7, h_begin=1, h_end=8, group=4, sg=0, sh=0, k_pos=1.0, k_rot=1.0, use_axis=0,
             axis=(0.0, 0.0, 1.0), weight=1.0, acc=0):
        return getattr(h, fn)(ptr, geom, ptr, ptr, ptr, B, H, d, D, h_begin, h_end, group, sg, sh, k_pos, k_rot, use_axis, *axis, weight, acc, null)

    for fn in NAMES:
        # beyond MPB_MAX_DOF: UNSUPPORTED, before anything else
        assert call(fn, ptr=null, geom=null, B=-1, D=13, d=13) == UNSUPPORTED and 'MPB_MAX_DOF' in err()
        assert call(fn, ptr=null, geom=null, d=25) == UNSUPPORTED and 'MPB_MAX_DOF' in err()
        # shapes, the range, the group, the terms, the axis: INVALID, before B == 0 and before the pointers
        for kw in (dict(B=-1), dict(H=0), dict(D=0, d=0), dict(d=6), dict(h_begin=-1), dict(h_begin=8), dict(h_begin=3, h_end=3), dict(h_end=9),
                   dict(group=0), dict(group=3), dict(sg=-1), dict(sh=-1), dict(k_pos=-1.0), dict(k_rot=float('nan')), dict(k_pos=float('inf')),
                   dict(k_pos=0.0, k_rot=0.0), dict(use_axis=1, axis=(0.0, 0.0, 1.01)), dict(use_axis=1, axis=(0.0, 0.0, 0.0)),
                   dict(use_axis=1, axis=(float('nan'), 0.0, 1.0)), dict(use_axis=1, k_rot=0.0)):
            assert call(fn, ptr=null, geom=null, **kw) == INVALID, (fn, kw)
            if 'B' not in kw and 'group' not in kw:
                assert call(fn, ptr=null, geom=null, **{**kw, 'B': 0}) == INVALID, (fn, kw)
        assert call(fn, ptr=null, geom=null, d=6) == INVALID and 'narrower' in err()
        assert call(fn, ptr=null, geom=null, group=3) == INVALID and 'divide' in err()
        assert call(fn, ptr=null, geom=null, k_pos=0.0, k_rot=0.0) == INVALID and 'both terms' in err()
        assert call(fn, ptr=null, geom=null, use_axis=1, axis=(0.6, 0.0, 0.9)) == INVALID and 'unit' in err()
        # nothing to do: OK whatever the pointers; an axis within 1e-3 of unit length is accepted
        assert call(fn, ptr=null, geom=null, B=0) == 0
        assert call(fn, ptr=null, geom=null, B=0, use_axis=1, axis=(0.0, 0.6, 0.8005)) == 0
        # pointers
        assert call(fn, ptr=null) == INVALID and 'null' in err()
        assert call(fn, geom=null) == INVALID and 'null' in err()
        assert call(fn, geom=odd) == INVALID and 'aligned' in err()


def test_python_wrappers_and_the_class_refuse_on_the_host():
    from motion_planning_baselines_amd import geometry as G, ops
    from motion_planning_baselines_amd.planners.costs import cost_functions as C
    with pytest.raises(ValueError, match='GPU'):
        ops.ee_cost_eval(torch.zeros(3, 5, 7), None, torch.zeros(3, 4), k_pos=1.0)
    with pytest.raises(ValueError, match='expected'):
        ops.ee_cost_grad(torch.zeros(3, 7), None, torch.zeros(3, 4), k_pos=1.0)
    robot = K.robot_of('panda')
    H, T = 16, torch.eye(3, 4)
    ok = C.CostEEPose(robot, H, T, sigma_pos=0.1, sigma_rot=0.2, axis=(0.0, 0.0, 1.0), traj_range='path')
    assert ok.own_kernels and not ok.is_self and ok.range_of(H) == (1, H) and ok.num_goals == 1
    assert C.CostEEPose(robot, H, T, sigma_pos=0.1).range_of(H) == (H - 1, H)
    assert C.CostEEPose(robot, H, T.expand(H, 3, 4), sigma_pos=0.1, target_per_waypoint=True, traj_range=(3, 9)).range_of(H) == (3, 9)
    assert C.CostEEPose(robot, H, T.expand(5, H, 3, 4), sigma_rot=0.1, target_per_waypoint=True).num_goals == 5
    with pytest.raises(ValueError, match='sigma'):
        C.CostEEPose(robot, H, T)
    with pytest.raises(ValueError, match='unit'):
        C.CostEEPose(robot, H, T, sigma_rot=0.1, axis=(0.0, 0.0, 1.1))
    with pytest.raises(ValueError, match='sigma_rot'):
        C.CostEEPose(robot, H, T, sigma_pos=0.1, axis=(0.0, 0.0, 1.0))
    for bad in (torch.zeros(4, 4), torch.zeros(3, 4, 1), torch.zeros(2, 2, 3, 4)):
        with pytest.raises(ValueError, match='target has shape'):
            C.CostEEPose(robot, H, bad, sigma_pos=0.1)
    with pytest.raises(ValueError, match='target has shape'):
        C.CostEEPose(robot, H, torch.zeros(H + 1, 3, 4), sigma_pos=0.1, target_per_waypoint=True)
    with pytest.raises(ValueError, match='range'):
        C.CostEEPose(robot, H, T, sigma_pos=0.1, traj_range=(9, 3))
    with pytest.raises(ValueError, match='point robot'):
        C.CostEEPose(G.RobotPointMass(2), H, T, sigma_pos=0.1)
    # the composite: the member is one with kernels of its own, never an obstacle member, never fused
    sm = C.CostGPTrajectory(robot, H, dt=0.1, sigma_gp=1.0)
    co = C.CostCollision(robot, H, field=G.env_spheres_3d(0), sigma_coll=0.3)
    comp = C.CostComposite(robot, H, [co, ok, sm])
    assert comp.own_terms() == [(ok, 1.0)] and comp.collision_terms() == [(co, 1.0)] and comp.self_terms() == []
    assert comp.single_collision_term() is None and C.fusable_collision(comp) is None and C.fusable_collision(ok) is None
    # B % G != 0, before anything is launched
    three = C.CostEEPose(robot, H, T.expand(3, 3, 4).contiguous(), sigma_pos=0.1)
    with pytest.raises(ValueError, match='GPU|divide'):
        three.eval(torch.zeros(4, H, 7))
    # the helper: R* a = d, a proper rotation, the opposite direction included
    for a, d in (((0.0, 0.0, 1.0), (0.0, 0.0, 1.0)), ((0.0, 0.0, 1.0), (0.0, 0.0, -1.0)), (E.AXIS, (0.3, -0.4, 0.2)), ((1.0, 0.0, 0.0), (-1.0, 1e-9, 0.0))):
        Ts = C.CostEEPose.target_for_axis(a, d, position=(0.1, 0.2, 0.3)).double()
        R, dn = Ts[:, :3], torch.tensor(d, dtype=torch.float64) / torch.tensor(d, dtype=torch.float64).norm()
        assert float((R @ torch.tensor(a, dtype=torch.float64) - dn).abs().max()) < 1e-6
        assert float((R @ R.T - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-6 and abs(float(torch.linalg.det(R)) - 1.0) < 1e-6
        assert Ts[:, 3].tolist() == pytest.approx([0.1, 0.2, 0.3])


def _autograd_gap(robot_name, terms, rounded):
    """Largest |closed form - autograd| of the restated cost in fp64 over the path set's kept waypoints, unit k."""
    ref = E.reference(robot_name, 48, 37, terms, 1, 37)
    inp = ref.inp
    tf64, _, _ = K.chain(inp.robot, torch.float64)
    B, H, D = 48, 37, inp.D
    if rounded:
        tgt = inp.target.double()
    else:                                   # the targets before their rounding to fp32: fp64 FK of the same perturbed configurations
        import numpy as np
        qt = inp.trajs[:, -1, :D].double() + torch.as_tensor(np.random.RandomState(3).uniform(-0.6, 0.6, (B, D)))
        tgt = K.pose_jacobian(tf64, qt)[0]
    q = inp.trajs[:, :, :D].double().reshape(-1, D).requires_grad_(True)
    c, g, th = E.waypoint_cost_grad(tf64, q, E.expand_target(tgt, B, H, False).reshape(-1, 3, 4), terms)
    ga, = torch.autograd.grad(c.sum(), q)
    keep = (torch.arange(H) >= 1).repeat(B)
    if terms == 'pos_rot':
        keep = keep & (th.detach() < math.pi - E.MARGIN)
    return float((g.detach() - ga)[keep].abs().max())


@pytest.mark.parametrize('robot_name', E.ROBOTS)
def test_closed_form_gradient_is_the_derivative_of_the_restated_cost(robot_name):
    """fp64, against autograd of the restated cost: the position and axis forms are exact derivatives on every robot (1e-10); the
    rotation form is the exact derivative of theta^2 when R and R* are orthonormal -- the two test arms with unrounded targets, theta <
    pi - 0.05 (1e-10).  With fp32-rounded targets, or the Panda's fp32 joint transforms, E = R* R^T leaves SO(3) by ~1e-7 and autograd of
    the stated function differs from the closed form at the 1e-6 level: recorded, not barred (the tests' reference is the closed form)."""
    for terms in ('pos', 'pos_axis'):
        gap = _autograd_gap(robot_name, terms, rounded=True)
        print(f'{robot_name} {terms}: closed form vs autograd {gap:.2e}')
        assert gap < 1e-10
    exact, rounded = _autograd_gap(robot_name, 'pos_rot', rounded=False), _autograd_gap(robot_name, 'pos_rot', rounded=True)
    print(f'{robot_name} pos_rot: closed form vs autograd {exact:.2e} with fp64 targets, {rounded:.2e} with fp32-rounded targets')
    if robot_name != 'panda':
        assert exact < 1e-10


@pytest.mark.parametrize('case', sorted(E.CASES))
def test_reference_alone_keeps_the_conditions_the_gpu_tests_rely_on(case):
    """Per input set: at most CAP of the waypoints in range are left out of the full-rotation checks (none for the other terms), and E32
    is of rounding size."""
    ref = E.reference(*E.CASES[case])
    print(f'{case}: left out {ref.left_out:.3f}; E32 cost {ref.E32_c:.2e} gradient {ref.E32_g:.2e}; bars {E.bar(ref.E32_c):.2e} {E.bar(ref.E32_g):.2e}')
    assert ref.left_out <= E.CAP
    if E.CASES[case][3] != 'pos_rot':
        assert ref.left_out == 0.0
    assert ref.E32_c < 1e-5 and ref.E32_g < 1e-5
    assert int(ref.keep.sum()) > 0


def test_wave_sum_restatement_adds_everything_once():
    import numpy as np
    v = np.random.RandomState(0).randint(0, 1000, 64).astype(np.float32)        # (integers: every order gives the exact sum)
    assert float(E.wave_sum_f32(v)) == float(v.sum())
    assert float(E.ordered_sum_f32(np.arange(70, dtype=np.float32))) == 69 * 70 / 2


@pytest.mark.parametrize('mode', ['pos_rot', 'pos_axis', 'rot', 'per_waypoint'])
def test_linear_system_shapes_and_normal_equations(mode, monkeypatch):
    """CostEEPose.get_linear_system with the pose op replaced by the fp64 restatement (everything else is the class's own torch code):
    one block of rows per waypoint of the range at that waypoint's position columns, K diagonal, and A^T K b = -grad / 2 of the restated
    closed-form gradient to 1e-10."""
    from motion_planning_baselines_amd import ops
    from motion_planning_baselines_amd.planners.costs import cost_functions as C
    robot = K.robot_of('arm9')
    tf64, _, _ = K.chain(robot, torch.float64)
    B, H, D = 6, 12, robot.q_dim
    per_wp = mode == 'per_waypoint'
    inp = E.inputs('arm9', B, H, True, 3, per_wp)
    trajs = torch.nan_to_num(inp.trajs, nan=0.25).double()
    monkeypatch.setattr(ops, 'fk_ee_pose', lambda q, geom, with_jacobian=False: K.pose_jacobian(tf64, q.double()))
    monkeypatch.setattr(C.CostEEPose, 'device_geometry', lambda self, device: None)
    s_pos, s_rot = (None if mode == 'rot' else 0.5), 0.7
    axis = E.AXIS if mode == 'pos_axis' else None
    rng = (2, 7) if mode != 'rot' else 'goal'
    cost = C.CostEEPose(robot, H, inp.target, sigma_pos=s_pos, sigma_rot=s_rot, axis=axis, traj_range=rng, target_per_waypoint=per_wp)
    h0, h1 = cost.range_of(H)
    A, b, Kd = cost.get_linear_system(trajs)
    m = 3 if mode == 'rot' else 6
    n = (h1 - h0) * m
    assert A.shape == (B, n, 2 * D * H) and b.shape == (B, n, 1) and Kd.shape == (B, n, n) and A.dtype == torch.float64
    want_k = torch.tensor(([1 / 0.25] * 3 if s_pos else []) + [1 / 0.49] * 3, dtype=torch.float64).repeat(h1 - h0)
    assert torch.allclose(Kd, torch.diag(want_k).expand(B, n, n), rtol=1e-12, atol=0)
    cols = torch.zeros(2 * D * H, dtype=torch.bool)
    for h in range(h0, h1):
        cols[h * 2 * D:h * 2 * D + D] = True
    assert float(A[:, :, ~cols].abs().max()) == 0.0 and float(A.abs().max()) > 0
    tgt = E.expand_target(inp.target.double(), B, H, per_wp)
    g_all = lambda terms: E.trajectory_cost_grad(tf64, trajs, tgt, terms, h0, h1)[1]
    g_pos = g_all('pos')
    g_rot = g_all('pos_axis' if axis else 'pos_rot') - g_pos
    want = (cost.k_pos * g_pos if s_pos else 0.0) + cost.k_rot * g_rot                  # (B, H, D)
    got = (A.transpose(1, 2) @ Kd @ b).reshape(B, H, 2 * D)[:, :, :D]
    gap = float((got + 0.5 * want).abs().max())
    print(f'{mode}: |A^T K b + grad / 2| = {gap:.2e}, largest |grad| {float(want.abs().max()):.2e}')
    assert gap < 1e-10 * max(1.0, float(want.abs().max()))
    # and the composite stacks it like any member with a linear system
    comp = C.CostComposite(robot, H, [cost, cost])
    A2, b2, K2 = comp.get_linear_system(trajs)
    assert A2.shape == (B, 2 * n, 2 * D * H) and K2.shape == (B, 2 * n, 2 * n) and torch.equal(A2[:, n:], A)
