"""CPU: Cartesian end-effector moves (csrc/mpb_cartesian.hip) as far as no device is needed -- the symbol and its binding, what the
compiler made of the kernel, the launcher's refusals in the order include/mpb.h states, the wrappers' host-side checks -- and the
conditions on the input sets that tests/test_gpu_cartesian.py relies on, asserted on the restatement of tests/cartesian_checks.py alone."""
import ctypes
import json
import math
import os
import re

import pytest
import torch

import cartesian_checks as C

INVALID, UNSUPPORTED = 1, 2          # include/mpb.h MPB_E_INVALID, MPB_E_UNSUPPORTED


def test_library_exports_the_symbol_and_the_constants_agree():
    from motion_planning_baselines_amd import _lib, ops
    h = _lib.lib()
    assert hasattr(h, 'mpb_cartesian_path') and len(_lib.SIGNATURES['mpb_cartesian_path']) == 21
    assert (h.mpb_version() & 0xFFFF) == _lib.ABI_VERSION == 7                                 # additive: the ABI version stays
    text = open(os.path.join(__import__('conftest').ROOT, 'include', 'mpb.h')).read()
    proto = re.search(r'int mpb_cartesian_path\(([^;]*?)\);', text, flags=re.S).group(1)
    assert len(proto.split(',')) == 21
    define = lambda name: re.search(rf'#define {name} (\S+)', text).group(1)
    for name in ('OK', 'LOST', 'JUMP', 'BAD_TARGET', 'COLLISION', 'MAX_STEPS', 'MAX_WORK'):
        assert int(define('MPB_CART_' + name)) == getattr(ops, 'CART_' + name), name
    assert (ops.CART_OK, ops.CART_LOST, ops.CART_JUMP, ops.CART_BAD_TARGET, ops.CART_COLLISION) == (C.OK, C.LOST, C.JUMP, C.BAD_TARGET, C.COLLISION)
    assert ops.CART_MAX_STEPS == 4096 and ops.CART_MAX_WORK == 65536
    turn = float(define('MPB_CART_MAX_TURN').rstrip('f'))
    assert turn == ops.CART_MAX_TURN and abs(turn - (math.pi - 0.1)) < 1e-7 and abs(C.MAX_TURN - turn) < 1e-7


def test_kernel_keeps_its_state_in_registers():
    """csrc/kernel_resources.json: exactly two instantiations (full pose, position only); one lane holds a whole problem -- the chain's
    joint axes and origins, the 6 x 6 system, the two end poses, the iterate and the last accepted configuration -- in registers."""
    from motion_planning_baselines_amd import build
    build.build(verbose=False)
    res = json.load(open(build.RESOURCES))
    hits = {k: v for k, v in res.items() if 'cart_path_kernel' in k}
    assert len(hits) == 2 and sorted('ILb0E' in k for k in hits) == [False, True], list(hits)
    for name, r in hits.items():
        print(name, r)
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['lds'] == 0, (name, r)


def test_refusals_that_need_no_device_in_the_stated_order():
    from motion_planning_baselines_amd import _lib
    h = _lib.lib()
    null, p, odd = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 8)      # (never dereferenced on these paths)
    err = lambda: h.mpb_last_error().decode()

    def path(N=4, S=3, D=7, K=32, n_inner=8, damping=0.1, pos_tol=1e-3, rot_tol=1e-2, jump_max=0.5, ptr=p, geom=p, q_min=null, q_max=null):
        return h.mpb_cartesian_path(ptr, ptr, geom, q_min, q_max, ptr, ptr, ptr, ptr, ptr, N, S, D, K, n_inner, damping, pos_tol, rot_tol,
                                    jump_max, 0, null)

    # 1. beyond MPB_MAX_DOF: UNSUPPORTED, before anything else (sizes, settings, null pointers)
    assert path(N=-1, D=13, K=0, n_inner=-1, jump_max=0.0, ptr=null, geom=null) == UNSUPPORTED and 'MPB_MAX_DOF' in err()
    # 2. sizes and settings: INVALID, before N == 0 and before the pointers
    for kw in (dict(N=-1), dict(S=-1), dict(D=0), dict(N=1 << 16, S=1 << 15), dict(K=0), dict(K=-1), dict(K=4097), dict(n_inner=-1),
               dict(n_inner=1025), dict(K=65, n_inner=1024), dict(K=4096, n_inner=17), dict(damping=9.9e-3), dict(damping=-0.1),
               dict(damping=float('nan')), dict(pos_tol=-1e-9), dict(rot_tol=-1e-9), dict(pos_tol=float('nan')), dict(rot_tol=float('nan')),
               dict(jump_max=0.0), dict(jump_max=-1.0), dict(jump_max=float('nan'))):
        assert path(ptr=null, geom=null, **kw) == INVALID, kw
        if 'N' not in kw:
            assert path(N=0, ptr=null, geom=null, **kw) == INVALID, kw
    assert path(K=4097, ptr=null, geom=null) == INVALID and 'K = 4097' in err()
    assert path(n_inner=1025, ptr=null, geom=null) == INVALID and 'n_inner' in err()
    assert path(K=4096, n_inner=17, ptr=null, geom=null) == INVALID and 'K * n_inner' in err()
    assert path(damping=1e-3, ptr=null, geom=null) == INVALID and 'damping' in err()
    assert path(jump_max=0.0, ptr=null, geom=null) == INVALID and 'jump_max' in err()
    # 3. nothing to do: OK whatever the pointers; the bounds themselves are accepted
    assert path(N=0, ptr=null, geom=null) == 0 and path(S=0, ptr=null, geom=null) == 0
    assert path(N=0, K=1, n_inner=0, damping=1e-2, pos_tol=0.0, rot_tol=0.0, jump_max=float('inf'), ptr=null, geom=null) == 0
    assert path(N=0, K=4096, n_inner=16, ptr=null, geom=null) == 0 and path(N=0, K=64, n_inner=1024, ptr=null, geom=null) == 0
    # 4. pointers: a null required one, one limit without the other, a misaligned geometry buffer
    assert path(ptr=null) == INVALID and 'null' in err()
    assert path(geom=null) == INVALID and 'null' in err()
    assert path(q_min=p) == INVALID and 'both or neither' in err()
    assert path(q_max=p) == INVALID and 'both or neither' in err()
    assert path(geom=odd) == INVALID and 'aligned' in err()
    assert path(geom=odd, q_min=p, q_max=p) == INVALID and 'aligned' in err()


def test_python_wrappers_refuse_on_the_host():
    """ops.cartesian_path / PlanningTask.cartesian_path check device, dtype, shape and the settings before any launch."""
    from motion_planning_baselines_amd import ops
    from motion_planning_baselines_amd.robot_field import CartesianPathResult, PlanningTask
    with pytest.raises(ValueError, match='expected'):
        ops.cartesian_path(torch.zeros(3, 3, 4), torch.zeros(3, 7), None, 8)
    with pytest.raises(ValueError, match='GPU'):
        ops.cartesian_path(torch.zeros(3, 3, 4), torch.zeros(3, 2, 7), None, 8)
    assert callable(PlanningTask.cartesian_path) and not hasattr(CartesianPathResult, 'cartesian_path')

    class _Task:          # (the method's own shape checks come before it touches the geometry)
        device, q_dim = torch.device('cpu'), 7
    for q0, goal, kw in ((torch.zeros(3, 2, 6), torch.zeros(3, 3, 4), {}), (torch.zeros(7), torch.zeros(1, 3, 4), {}),
                         (torch.zeros(3, 2, 7), torch.zeros(2, 3, 4), {}), (torch.zeros(3, 7), torch.zeros(3, 3), {}),
                         (torch.zeros(3, 7), torch.zeros(3, 4), dict(position_only=True))):
        with pytest.raises(ValueError, match='expected'):
            PlanningTask.cartesian_path(_Task(), q0, goal, **kw)


@pytest.mark.parametrize('name', C.SETS)
def test_reference_alone_keeps_the_conditions_the_gpu_tests_rely_on(name):
    K = C.FULL[0]
    ref, el, jp = C.reference(name, *C.FULL), C.reference(name, *C.ELEMENT, C.JUMP_MAX, C.ELEMENT_TOL), C.reference(name, *C.FULL, C.JUMP_TIGHT)
    complete64, early64 = float((ref.r64.status == C.OK).float().mean()), float((ref.r64.n_ok < K).float().mean())
    differ = {k: float((~r.same).float().mean()) for k, r in (('full', ref), ('element', el), ('jump', jp))}
    jump64 = float((jp.r64.status == C.JUMP).float().mean())
    E_el = max(el.E32_q, el.E32_pos, el.E32_rot)
    print(f'{name}: complete {complete64:.3f} (fp32 {float((ref.r32.status == C.OK).float().mean()):.3f}), stopped early {early64:.3f}, n_ok differs '
          f'{differ}, E32 full run q {ref.E32_q:.2e} pos {ref.E32_pos:.2e} rot {ref.E32_rot:.2e}, K = 2 run {E_el:.2e}, n_ok of the K = 2 run '
          f'{torch.bincount(el.r64.n_ok.flatten(), minlength=3).tolist()}, JUMP share at jump_max {C.JUMP_TIGHT}: {jump64:.3f}')
    assert complete64 >= 0.30 and early64 >= 0.10
    assert max(differ.values()) <= C.CAP
    assert E_el < 1e-4
    assert jump64 >= 0.10
    # the restatement keeps its own promises
    inp = C.inputs(name)
    r = ref.r64
    rows = torch.arange(K + 1)[None, None, :]
    acc = rows <= r.n_ok[:, :, None]
    assert bool(((r.status == C.OK) == (r.n_ok == K)).all())
    assert torch.equal(r.q[:, :, 0], inp.starts.double())
    assert float(r.pos_err[acc].max()) <= C.POS_TOL and float(r.rot_err[acc].max()) <= C.ROT_TOL
    held = torch.gather(r.q, 2, r.n_ok.long()[:, :, None, None].expand(*r.n_ok.shape, 1, r.q.shape[-1]))
    assert bool(((r.q == held) | acc[..., None]).all())
    assert bool((r.pos_err[rows > r.n_ok[:, :, None] + 1] == 0).all())
    lost = r.status == C.LOST
    rej = torch.gather(r.pos_err, 2, (r.n_ok.long() + 1).clamp_max(K)[:, :, None])[..., 0]
    rej_rot = torch.gather(r.rot_err, 2, (r.n_ok.long() + 1).clamp_max(K)[:, :, None])[..., 0]
    assert bool(((rej > C.POS_TOL) | (rej_rot > C.ROT_TOL))[lost].all())
    tf, lo, hi = C.chain(inp.robot, torch.float64)
    assert bool(((r.q >= lo) & (r.q <= hi)).all())


def test_bad_targets_in_the_reference():
    ref = C.reference('bad', *C.FULL)
    for r in (ref.r64, ref.r32):
        assert bool((r.status == C.BAD_TARGET).all()) and not bool(r.n_ok.any())
        assert torch.equal(r.q, C.bad_inputs().starts.to(r.q.dtype)[:, :, None, :].expand_as(r.q)) and not bool(r.pos_err.any())


@pytest.mark.parametrize('name', ['panda', 'arm12'])
def test_restated_geodesic_ends_at_the_goal(name):
    """fp64: t_K is t* exactly (the convex form), R_K is R* within 1e-6 (the goal is an fp32 rounding of a rotation and the chain's fp32
    transforms are orthonormal to about 1e-7 only), the angle grows linearly and the steps stay rotations."""
    inp = C.inputs(name)
    tf, _, _ = C.chain(inp.robot, torch.float64)
    q0, goal = inp.starts.double().reshape(-1, inp.robot.q_dim), inp.goal.double().repeat_interleave(C.N_STARTS, 0)
    R0, t0, theta, a, bad = C.start_and_turn(tf, goal, q0, False)
    assert not bool(bad.any()) and float(theta.max()) > 0.3
    for K in (1, 7, 32):
        end = C.step_target(R0, t0, goal, theta, a, K, K, False)
        assert torch.equal(end[:, :, 3], goal[:, :, 3])
        assert float((end[:, :, :3] - goal[:, :, :3]).abs().max()) <= 1e-6
        start = C.step_target(R0, t0, goal, theta, a, 0, K, False)
        assert torch.equal(start[:, :, 3], t0) and float((start[:, :, :3] - R0).abs().max()) <= 1e-15
    half = C.step_target(R0, t0, goal, theta, a, 16, 32, False)
    th_half, _, _ = C.turn(R0, half[:, :, :3])
    assert float((th_half - 0.5 * theta).abs().max()) <= 1e-6
    assert float((half[:, :, :3] @ half[:, :, :3].transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-6
    assert float((half[:, :, 3] - 0.5 * (t0 + goal[:, :, 3])).abs().max()) <= 1e-15
