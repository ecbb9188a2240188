"""CPU: the end-effector pose op and the batched inverse kinematics (csrc/mpb_ik.hip) as far as no device is needed -- the two symbols
and their bindings, what the compiler made of the kernels, the launchers' refusals in the order include/mpb.h states -- and the
conditions on the input sets that tests/test_gpu_ik.py relies on, asserted on the restatement of tests/ik_checks.py alone."""
import ctypes
import json

import pytest
import torch

import ik_checks as K

INVALID, UNSUPPORTED = 1, 2          # include/mpb.h MPB_E_INVALID, MPB_E_UNSUPPORTED


def test_library_exports_the_two_symbols():
    from motion_planning_baselines_amd import _lib
    h = _lib.lib()
    for name in ('mpb_fk_ee_pose', 'mpb_ik_solve'):
        assert hasattr(h, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['mpb_fk_ee_pose']) == 7 and len(_lib.SIGNATURES['mpb_ik_solve']) == 19
    assert (h.mpb_version() & 0xFFFF) == _lib.ABI_VERSION == 7                                 # additive: the ABI version stays
    from motion_planning_baselines_amd import ops
    text = open(__import__('os').path.join(__import__('conftest').ROOT, 'include', 'mpb.h')).read()
    assert f'#define MPB_IK_MAX_ITERS {ops.IK_MAX_ITERS}\n' in text and '#define MPB_IK_MIN_DAMPING 1e-2f\n' in text and ops.IK_MIN_DAMPING == 1e-2


def test_kernels_keep_their_state_in_registers():
    """build() records what the compiler made of every kernel (csrc/kernel_resources.json): one lane holds a whole problem -- the chain's
    joint axes and origins, the 6 x 6 system -- in registers; nothing may go to scratch memory, and the kernels use no LDS."""
    from motion_planning_baselines_amd import build
    build.build(verbose=False)
    res = json.load(open(build.RESOURCES))
    hits = {k: v for k, v in res.items() if k.startswith(('_Z17fk_ee_pose_kernel', '_Z15ik_solve_kernelILb0EE', '_Z15ik_solve_kernelILb1EE'))}
    assert len(hits) == 3, list(hits)
    assert sum('ik_solve_kernel' in k or 'fk_ee_pose_kernel' in k for k in res) == 3
    for name, r in hits.items():
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0, (name, r)
        assert r['lds'] == 0, (name, r)


def test_refusals_that_need_no_device_in_the_stated_order():
    from motion_planning_baselines_amd import _lib
    h = _lib.lib()
    null, p, odd = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 8)      # (never dereferenced on these paths)
    err = lambda: h.mpb_last_error().decode()

    def solve(N=4, S=8, D=7, n_iters=64, damping=0.1, pos_tol=1e-3, rot_tol=1e-2, ptr=p, geom=p, q_min=null, q_max=null):
        return h.mpb_ik_solve(ptr, ptr, geom, q_min, q_max, ptr, ptr, ptr, ptr, ptr, N, S, D, n_iters, damping, pos_tol, rot_tol, 0, null)

    # 1. beyond MPB_MAX_DOF: UNSUPPORTED, before anything else (sizes, null pointers)
    assert h.mpb_fk_ee_pose(null, null, null, null, -1, 13, null) == UNSUPPORTED and 'MPB_MAX_DOF' in err()
    assert solve(N=-1, D=13, n_iters=-1, ptr=null, geom=null) == UNSUPPORTED and 'MPB_MAX_DOF' in err()
    # 2. sizes and settings: INVALID, before N == 0 and before the pointers
    assert h.mpb_fk_ee_pose(null, null, null, null, -1, 7, null) == INVALID
    assert h.mpb_fk_ee_pose(null, null, null, null, 0, 0, null) == INVALID
    for kw in (dict(N=-1), dict(S=-1), dict(D=0), dict(N=1 << 16, S=1 << 15), dict(n_iters=-1), dict(n_iters=1025), dict(damping=9.9e-3),
               dict(damping=-0.1), dict(damping=float('nan')), dict(pos_tol=-1e-9), dict(rot_tol=-1e-9), dict(pos_tol=float('nan'))):
        assert solve(ptr=null, geom=null, **kw) == INVALID, kw
        if 'N' not in kw:
            assert solve(N=0, ptr=null, geom=null, **kw) == INVALID, kw
    assert solve(n_iters=1025, ptr=null, geom=null) == INVALID and 'n_iters' in err()
    assert solve(damping=1e-3, ptr=null, geom=null) == INVALID and 'damping' in err()
    # 3. nothing to do: OK whatever the pointers
    assert h.mpb_fk_ee_pose(null, null, null, null, 0, 7, null) == 0
    assert solve(N=0, ptr=null, geom=null) == 0 and solve(S=0, ptr=null, geom=null) == 0
    assert solve(N=0, n_iters=0, damping=1e-2, pos_tol=0.0, rot_tol=0.0, ptr=null, geom=null) == 0          # the bounds themselves are accepted
    assert solve(N=0, n_iters=1024, ptr=null, geom=null) == 0
    # 4. pointers: a null required one, one limit without the other, a misaligned geometry buffer
    assert h.mpb_fk_ee_pose(null, p, p, null, 3, 7, null) == INVALID and 'null' in err()
    assert h.mpb_fk_ee_pose(p, null, p, null, 3, 7, null) == INVALID and h.mpb_fk_ee_pose(p, p, null, null, 3, 7, null) == INVALID
    assert h.mpb_fk_ee_pose(p, odd, p, null, 3, 7, null) == INVALID and 'aligned' in err()
    assert solve(ptr=null) == INVALID and 'null' in err()
    assert solve(geom=null) == INVALID and 'null' in err()
    assert solve(q_min=p) == INVALID and 'both or neither' in err()
    assert solve(q_max=p) == INVALID and 'both or neither' in err()
    assert solve(geom=odd) == INVALID and 'aligned' in err()
    assert solve(geom=odd, q_min=p, q_max=p) == INVALID and 'aligned' in err()


def test_python_wrappers_refuse_on_the_host():
    """ops.fk_ee_pose / ops.ik_solve check device, dtype, shape and the settings before any launch (CPU tensors: nothing is launched)."""
    from motion_planning_baselines_amd import ops
    with pytest.raises(ValueError, match='GPU'):
        ops.fk_ee_pose(torch.zeros(3, 7), None)
    with pytest.raises(ValueError, match='expected'):
        ops.fk_ee_pose(torch.zeros(3, 2, 7), None)
    with pytest.raises(ValueError, match='expected'):
        ops.ik_solve(torch.zeros(3, 3, 4), torch.zeros(3, 7), None)
    with pytest.raises(ValueError, match='GPU'):
        ops.ik_solve(torch.zeros(3, 3, 4), torch.zeros(3, 2, 7), None)
    # the task keeps everything it had next to the new methods, and the result object is a class of its own
    from motion_planning_baselines_amd.robot_field import IKResult, PlanningTask
    for m in ('compute_collision', 'random_q', 'random_coll_free_q', 'distance_q', 'get_trajs_collision_and_free', 'compute_fraction_free_trajs',
              'compute_collision_intensity_trajs', 'compute_success_free_trajs', 'get_EE_pose', 'get_EE_position', 'inverse_kinematics'):
        assert callable(getattr(PlanningTask, m)) and not hasattr(IKResult, m), m
    assert callable(IKResult.select)


@pytest.mark.parametrize('name', K.SETS)
def test_reference_alone_keeps_the_conditions_the_gpu_tests_rely_on(name):
    """Per input set: at least 90 % of the targets have three or more converged seeds in fp64 (test_gpu_ik.py asks the kernel for at least
    one on those), and after ONE step -- of up to five radians -- the fp32 restatement stays below 1e-3 rad of the fp64 one."""
    ref = K.reference(name)
    per = ref.r64.converged.sum(1)
    share64, share32 = float(ref.r64.converged.float().mean()), float(ref.r32.converged.float().mean())
    one = {lim: K.reference(name, 1, lim) for lim in (True, False)}
    step = float((one[False].r64.q - K.inputs(name).seeds.double()).abs().max())
    print(f'{name}: converged share fp64 {share64:.3f} fp32 {share32:.3f}; targets with >= 3 converged seeds {int((per >= 3).sum())} of '
          f'{len(per)}, minimum {int(per.min())}; one step: E32 {one[True].E32_q:.2e} rad with limits, {one[False].E32_q:.2e} without, '
          f'longest step {step:.2f} rad')
    assert float((per >= 3).float().mean()) >= 0.9
    assert abs(share64 - share32) <= 0.03 / 5                     # (the kernel is given five times this)
    assert one[True].E32_q < 1e-3 and one[False].E32_q < 1e-3
    # the restatement keeps its own promises: unconverged problems used the whole budget, converged ones meet the tolerances in fp64
    assert bool((ref.r64.iters[~ref.r64.converged] == K.N_ITERS).all())
    assert float(ref.r64.pos_err[ref.r64.converged].max()) <= K.POS_TOL
    if not K.inputs(name).position_only:
        assert float(ref.r64.rot_err[ref.r64.converged].max()) <= K.ROT_TOL
    tf, lo, hi = K.chain(K.inputs(name).robot, torch.float64)
    assert bool(((ref.r64.q >= lo) & (ref.r64.q <= hi)).all())


def test_restated_jacobian_is_the_derivative_of_the_restated_pose():
    """J of ik_checks against autograd through ik_checks.fk, fp64: rows 0-2 d t / d q, rows 3-5 the axis of d R / d q = [w]x R."""
    robot = K.robot_of('panda')
    tf, _, _ = K.chain(robot, torch.float64)
    q = K.uniform_q(robot, (5,), 11).double().requires_grad_(True)
    pose, J = K.pose_jacobian(tf, q)
    for a in range(3):
        g, = torch.autograd.grad(pose[:, a, 3].sum(), q, retain_graph=True)
        assert float((g - J[:, a].detach()).abs().max()) < 1e-12
    R = pose[:, :, :3].detach()
    for j in range(robot.q_dim):
        dR = torch.stack([torch.stack([torch.autograd.grad(pose[:, a, b].sum(), q, retain_graph=True)[0][:, j] for b in range(3)], -1)
                          for a in range(3)], -2)
        W = dR @ R.transpose(1, 2)                                                            # [z_j]x
        w = torch.stack([W[:, 2, 1], W[:, 0, 2], W[:, 1, 0]], -1)
        assert float((w - J[:, 3:, j].detach()).abs().max()) < 1e-6     # (the chain's fp32 transforms are orthonormal to ~1e-7 only)


def test_collision_free_goals_exist_in_the_reference():
    """The scene of test_gpu_ik.py's collision-free check, by the restatement and the oracle's collision cost alone: Panda among
    env_spheres_3d(), targets = FK of the first 64 collision-free of 4 000 uniform configurations; at least 90 % of them have three or
    more converged, collision-free seeds."""
    sc = K.free_scene()
    per = sc.free64.sum(1)
    print(f'free scene: targets with >= 3 free converged seeds {int((per >= 3).sum())} of {len(per)}, free share {float(sc.free64.float().mean()):.3f}')
    assert float((per >= 3).float().mean()) >= 0.9
