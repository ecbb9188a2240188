"""GPU: the end-effector pose cost kernels (mpb_ee_cost_eval / _grad through ops.ee_cost_eval / _grad) against the fp64 restatement of
tests/ee_cost_checks.py: every in-range, non-excluded waypoint's cost and every element of its gradient within bar(E32), at unit k; the
sums, the accumulate form, the rows outside the range, run-to-run bits and the header guard.  Measured on an MI355X (DESIGN section 10 has
the table): cost errors 0.8e-7 to 5.7e-7 against E32 of 0.5e-7 to 4.8e-7, gradient errors 1.2e-7 to 2.1e-6 against E32 of 1.2e-7 to 2.8e-6;
every `out` is bit for bit `weight` times the per-waypoint costs summed in the kernels' order."""
import numpy as np
import pytest
import torch

import ee_cost_checks as E

pytestmark = pytest.mark.gpu


def _device_case(case, dev):
    from motion_planning_baselines_amd.planners.costs import cost_functions as C
    robot_name, B, H, terms, h0, h1 = E.CASES[case][:6]
    wide, groups, per_wp = (tuple(E.CASES[case][6:]) + (False, None, False)[len(E.CASES[case]) - 6:])
    ref = E.reference(*E.CASES[case])
    inp = ref.inp
    # (sigma = 1: unit k, the units of the bars)
    cost = C.CostEEPose(inp.robot, H, inp.target, sigma_pos=1.0, sigma_rot=None if terms == 'pos' else 1.0,
                        axis=E.AXIS if terms == 'pos_axis' else None, traj_range=(h0, h1), target_per_waypoint=per_wp)
    return ref, cost, inp.trajs.to(dev)


@pytest.mark.parametrize('case', sorted(E.CASES))
def test_every_waypoint_and_gradient_element_against_fp64(gpu_device, case):
    dev = gpu_device
    ref, cost, x = _device_case(case, dev)
    B, H, d = x.shape
    D = ref.inp.D
    weight = 1.75
    out, pw = cost.own_eval(x, weight=weight, per_waypoint=True)
    out_g, grad = cost.own_grad(x, weight=weight)
    torch.cuda.synchronize()
    pw, grad_c, out_c, out_gc = pw.cpu(), grad.cpu(), out.cpu(), out_g.cpu()
    assert bool(torch.isfinite(pw).all()) and bool(torch.isfinite(grad_c).all())
    e_c, e_g = E.cost_error(ref, pw), E.grad_error(ref, grad_c[:, :, :D] / weight)
    bar_c, bar_g = E.bar(ref.E32_c), E.bar(ref.E32_g)
    print(f'{case}: cost error {e_c:.2e} (E32 {ref.E32_c:.2e}, bar {bar_c:.2e}); gradient error {e_g:.2e} (E32 {ref.E32_g:.2e}, bar {bar_g:.2e}); '
          f'left out {ref.left_out:.3f}')
    assert e_c <= bar_c and e_g <= bar_g
    # outside the range: exactly 0, and so are the velocity channels (whose inputs are NaN)
    assert float(pw[~ref.live].abs().max() if (~ref.live).any() else 0.0) == 0.0
    assert float(grad_c[~ref.live].abs().max()) == 0.0
    if d > D:
        assert float(grad_c[:, :, D:].abs().max()) == 0.0
    # out = weight * the sum of the per-waypoint costs in the kernel's order, and the gradient launch returns the same cost
    want = np.array([np.float32(weight) * E.ordered_sum_f32(pw[b].numpy()) for b in range(B)], np.float32)
    tot64 = weight * pw.double().sum(1)
    e_out = float(((out_c.double() - torch.from_numpy(want).double()).abs() / tot64.clamp_min(1.0)).max())
    print(f'{case}: out against the fp32-ordered sum {e_out:.2e}; bit-equal {bool(np.array_equal(out_c.numpy(), want))}')
    assert e_out <= bar_c
    assert float(((out_gc.double() - out_c.double()).abs() / tot64.clamp_min(1.0)).max()) <= bar_c
    # the same bits on a second run
    out2, pw2 = cost.own_eval(x, weight=weight, per_waypoint=True)
    out_g2, grad2 = cost.own_grad(x, weight=weight)
    assert torch.equal(out2, out) and torch.equal(pw2.cpu(), pw) and torch.equal(grad2, grad) and torch.equal(out_g2, out_g)


@pytest.mark.parametrize('case', ['panda-pos_rot-path', 'panda-pos_axis-range-3-9', 'arm12-pos_axis-goal-130', 'panda-pos_axis-wide',
                                  'arm9-pos_rot-goal-130-wide'])
def test_accumulate_adds_the_fresh_value_in_one_rounding_and_touches_nothing_else(gpu_device, case):
    dev = gpu_device
    ref, cost, x = _device_case(case, dev)
    B, H, d = x.shape
    D = ref.inp.D
    g = torch.Generator().manual_seed(5)
    out0, grad0 = (3.0 * torch.randn(B, generator=g)).to(dev), (3.0 * torch.randn(B, H, d, generator=g)).to(dev)
    fresh_out, fresh_grad = cost.own_grad(x, weight=0.5)
    out, grad = out0.clone(), grad0.clone()
    r_out, r_grad = cost.own_grad(x, weight=0.5, out=out, grad=grad, accumulate=True)
    assert r_out.data_ptr() == out.data_ptr() and r_grad.data_ptr() == grad.data_ptr()
    live = ref.live.to(dev)
    assert torch.equal(out, out0 + fresh_out)                                                  # (one fp32 addition: the same bits)
    assert torch.equal(grad[:, :, :D][live], (grad0[:, :, :D] + fresh_grad[:, :, :D])[live])
    assert torch.equal(grad[~live], grad0[~live])                                              # rows outside the range: untouched
    if d > D:
        assert torch.equal(grad[:, :, D:], grad0[:, :, D:])                                    # velocity channels: untouched
    # the cost launch: out accumulates, per_waypoint is written
    out_e = out0.clone()
    _, pw = cost.own_eval(x, weight=0.5, out=out_e, accumulate=True, per_waypoint=True)
    fresh_e, pw_f = cost.own_eval(x, weight=0.5, per_waypoint=True)
    assert torch.equal(out_e, out0 + fresh_e) and torch.equal(pw, pw_f) and float(pw[~live].abs().max()) == 0.0


def test_sigmas_weight_and_the_class_conventions(gpu_device):
    """k = 1 / sigma^2 per term against the unit-k restatement (cost = k_pos c_p + k_rot c_a), eval / eval_with_grad / __call__, a
    4-D batch, the composite accumulating the member onto its total, and the 'goal' / 'path' names of the range."""
    from motion_planning_baselines_amd.planners.costs import cost_functions as C
    dev = gpu_device
    ref_p, ref_a = E.reference(*E.CASES['panda-pos-path']), E.reference(*E.CASES['panda-pos_axis-path'])
    inp = ref_a.inp
    B, H, D = 48, 37, inp.D
    x = inp.trajs.to(dev)
    s_pos, s_rot = 0.5, 0.25
    cost = C.CostEEPose(inp.robot, H, inp.target, sigma_pos=s_pos, sigma_rot=s_rot, axis=E.AXIS, traj_range='path')
    want_c = (ref_p.c64 / s_pos ** 2 + (ref_a.c64 - ref_p.c64) / s_rot ** 2).sum(1)
    want_g = ref_p.g64 / s_pos ** 2 + (ref_a.g64 - ref_p.g64) / s_rot ** 2
    c, g = cost.eval_with_grad(x, weight=2.0)
    rel = lambda a, b: float((a.cpu().double() - b).abs().max() / b.abs().max())
    print(f'sigmas: cost {rel(c, 2.0 * want_c):.2e}, gradient {rel(g, 2.0 * want_g):.2e} of the largest')
    assert rel(c, 2.0 * want_c) < 1e-5 and rel(g, 2.0 * want_g) < 1e-5
    assert torch.equal(cost(x), cost.eval(x)) and rel(cost(x), want_c) < 1e-5
    assert torch.equal(cost.eval(x.reshape(6, 8, H, D)), cost.eval(x))
    # rotation term alone (sigma_pos None) = the difference of the two restatements
    rot_only = C.CostEEPose(inp.robot, H, inp.target, sigma_rot=s_rot, axis=E.AXIS, traj_range='path')
    assert rel(rot_only.eval(x), ((ref_a.c64 - ref_p.c64) / s_rot ** 2).sum(1)) < 1e-5
    # 'goal' is the last waypoint
    goal = C.CostEEPose(inp.robot, H, inp.target, sigma_pos=s_pos, traj_range='goal')
    _, pw = goal.own_eval(x, per_waypoint=True)
    assert float(pw[:, :-1].abs().max()) == 0.0 and float(pw[:, -1].min()) > 0.0
    # the composite adds the member onto what came before it, weight and all
    sm = C.CostGPTrajectory(inp.robot, H, dt=0.1, sigma_gp=3.0)
    comp = C.CostComposite(inp.robot, H, [cost, sm, goal], weights_cost_l=[0.5, 1.0, 2.0])
    xw = torch.cat([x, 0.1 * torch.randn(B, H, D, generator=torch.Generator().manual_seed(1)).to(dev)], -1).contiguous()
    total = comp.eval(xw)
    want = 0.5 * cost.eval(xw).double() + sm.eval(xw).double() + 2.0 * goal.eval(xw).double()
    assert float(((total.double() - want).abs() / want).max()) < 1e-6
    plan = C.device_plan(comp, dev)
    assert [m for m, _ in plan.own] == [cost, goal] and [w for _, w in plan.own] == [0.5, 2.0] and plan[0] is None and plan.selfs == []
    bare = C.device_plan(cost, dev)
    assert bare.own == [(cost, 1.0)] and bare[0] is None and bare[2] == []
    with pytest.raises(ValueError, match='divide'):
        C.CostEEPose(inp.robot, H, inp.target[:5].contiguous(), sigma_pos=1.0).eval(x)


def test_a_header_changed_after_the_first_call_gives_nan_and_writes_nothing_else(gpu_device):
    """The launcher keeps what it read of a buffer's header; the kernels compare the header with the D they were launched with.  A buffer
    whose n_dof word is changed after the first call answers NaN in out and on the range's rows, and writes nothing else: the rows
    outside the range and the velocity channels stay 0 (or, accumulating, untouched), and nothing past the outputs is written."""
    from motion_planning_baselines_amd import geometry as G, ops
    dev = gpu_device
    ref = E.reference(*E.CASES['panda-pos_axis-wide'])
    inp = ref.inp
    B, H, D = 48, 37, inp.D
    x, target = inp.trajs.to(dev), inp.target.to(dev)
    far = G.CollisionField(spheres=np.array([[1.0e6, 1.0e6, 1.0e6, 1.0]], np.float32))
    geom = ops.DeviceGeometry(inp.robot, far, dev)
    kw = dict(k_pos=1.0, k_rot=1.0, axis=E.AXIS)
    for rng in ((1, H), (H - 1, H)):                                                   # the wave form and the lane form
        good, _ = ops.ee_cost_grad(x, geom, target, h_begin=rng[0], h_end=rng[1], **kw)
        assert bool(torch.isfinite(good).all())
    bits = geom.buf.view(torch.int32)
    saved = bits.clone()
    off = G.HEADER_DTYPE.fields['n_dof'][1] // 4
    assert int(bits[off]) == D
    bits[off] = D - 1                                                                  # "another robot" at the same address
    for rng in ((1, H), (H - 1, H)):
        live = torch.zeros(H, dtype=torch.bool, device=dev)
        live[rng[0]:rng[1]] = True
        pad = torch.full((B * H * 2 * D + 64,), 7.0, device=dev)
        grad = pad[:B * H * 2 * D].view(B, H, 2 * D)
        out, _ = ops.ee_cost_grad(x, geom, target, h_begin=rng[0], h_end=rng[1], grad=grad, **kw)
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(grad[:, live, :D]).all())
        assert float(grad[:, ~live].abs().max()) == 0.0 and float(grad[:, :, D:].abs().max()) == 0.0
        assert bool((pad[B * H * 2 * D:] == 7.0).all())
        out_e, pw = ops.ee_cost_eval(x, geom, target, h_begin=rng[0], h_end=rng[1], per_waypoint=True, **kw)
        assert bool(torch.isnan(out_e).all()) and bool(torch.isnan(pw[:, live]).all()) and float(pw[:, ~live].abs().max()) == 0.0
    bits.copy_(saved)
    again, _ = ops.ee_cost_grad(x, geom, target, h_begin=1, h_end=H, **kw)
    assert torch.equal(again, ops.ee_cost_grad(x, geom, target, h_begin=1, h_end=H, **kw)[0]) and bool(torch.isfinite(again).all())


def test_device_refusals(gpu_device):
    """What only the buffer's header tells: a point robot is MPB_E_UNSUPPORTED, a D that is not the chain's MPB_E_INVALID."""
    import ctypes
    from motion_planning_baselines_amd import _lib, geometry as G, ops
    dev = gpu_device
    point = ops.DeviceGeometry(G.RobotPointMass(2), G.CollisionField(spheres=np.array([[0.0, 0.0, 0.0, 0.1]], np.float32)), dev)
    x = torch.zeros(4, 8, 2, device=dev)
    with pytest.raises(ValueError, match='point robot'):
        ops.ee_cost_eval(x, point, torch.zeros(3, 4, device=dev), k_pos=1.0)
    h = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    out, tgt = torch.zeros(4, device=dev), torch.zeros(3, 4, device=dev)
    rc = h.mpb_ee_cost_eval(p(x), p(point.buf), p(tgt), p(out), None, 4, 8, 2, 2, 1, 8, 4, 0, 0, 1.0, 0.0, 0, 0.0, 0.0, 0.0, 1.0, 0, None)
    assert rc == 2 and 'point robot' in h.mpb_last_error().decode()
    far = G.CollisionField(spheres=np.array([[1.0e6, 1.0e6, 1.0e6, 1.0]], np.float32))
    panda = ops.DeviceGeometry(G.RobotPanda(), far, dev)
    x7 = torch.zeros(4, 8, 7, device=dev)
    rc = h.mpb_ee_cost_eval(p(x7), p(panda.buf), p(tgt), p(out), None, 4, 8, 7, 6, 1, 8, 4, 0, 0, 1.0, 0.0, 0, 0.0, 0.0, 0.0, 1.0, 0, None)
    assert rc == 1 and 'joints' in h.mpb_last_error().decode()
