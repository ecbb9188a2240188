"""The moving-obstacle kernels (mpb_moving_collision_eval / _grad / _check) and the classes in front of them against the fp64
restatement of tests/moving_obstacle_checks.py.  Shapes: B = 21 trajectories; R in {2, 8, 64, 65, 130} rows (one lane serves up to three
rows); d = D and d = 2 D; h_begin in {0, 1}; the cases of moving_obstacle_checks.CASES (the one at the layout's limits: R = 65)."""
import pytest
import torch

import moving_obstacle_checks as M

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23


def _mo(name, R, dev):
    from motion_planning_baselines_amd import ops
    robot, field = M.case(name)
    return robot, field, ops.DeviceMovingObstacles(robot, field, dev, R)


@pytest.mark.parametrize('name', M.CASES)
def test_cost_of_every_row_and_out_against_fp64(gpu_device, name):
    """Per-row cost on EVERY row to bar(E32_cost), E32 = the fp32 torch restatement's own worst error on the same inputs, both in units of
    budget = max(1, active spheres); out to the same bar summed over its rows plus the fp32 summation's own rounding (a lane adds
    ceil(R / 64) values, the wave reduction six levels, two products: (ceil(R / 64) + 8) half-ulps of the sum of non-negative terms), as
    tests/test_gpu_self_collision.py holds it.
    Measured on an MI355X (worst over R, d, h_begin; E32 / kernel): panda_s 4.8e-8 / 4.6e-8; panda_sb 6.0e-8 / 6.0e-8; panda_b 1.0e-7 /
    1.5e-7; arm12 6.4e-8 / 9.4e-8; point3 6.2e-8 / 7.5e-8; point2 4.9e-8 / 4.9e-8; one 9.0e-8 / 1.0e-7; limit 3.8e-8 / 4.8e-8; the bar
    is 4.8e-7 (4 ulp) throughout."""
    from motion_planning_baselines_amd import ops
    for R in M.rows_of(name):
        robot, field, mo = _mo(name, R, gpu_device)
        D = robot.q_dim
        r = M.reference(name, R)
        bar = M.bar(r.E32_cost)
        for d in (D, 2 * D):
            x = M.trajs(name, R, d).to(gpu_device)
            for h_begin in (0, 1):
                k_sigma, weight = 4.0, 0.75
                out, pw = ops.moving_collision_eval(x, mo, k_sigma, weight=weight, h_begin=h_begin, per_waypoint=True)
                pw, out = pw.cpu().double(), out.cpu().double()
                want = r.c64.clone()
                want[:, :h_begin] = 0.0
                assert bool((pw[:, :h_begin] == 0).all())
                e = float(((pw - want).abs() / r.budget).max())
                tot = want.sum(-1)
                eo = (out / (k_sigma * weight) - tot).abs()
                allow = bar * r.budget[:, h_begin:].sum(-1) + ((R + 63) // 64 + 8) * 0.5 * ULP * tot
                print(f'{name} R={R} d={d} h_begin={h_begin}: E32 {r.E32_cost:.2e} kernel {e:.2e} bar {bar:.2e}; out worst {float((eo / allow).max()):.2f} of its allowance')
                assert e <= bar, (R, d, h_begin, e, bar)
                assert bool((eo <= allow).all()), (R, d, h_begin)


@pytest.mark.parametrize('name', M.CASES)
def test_every_gradient_element_of_every_conditioned_row(gpu_device, name):
    """Every element of d out / d trajs of every conditioned row to bar(E32_grad) (units of budget); rows the classifier excludes are
    finite; velocity columns and rows below h_begin are exactly 0; grad's out equals eval's bit for bit.
    Measured on an MI355X (worst over R; E32 / kernel / bar): panda_s 1.7e-7 / 2.2e-7 / 6.8e-7; panda_sb 2.1e-7 / 4.0e-7 / 8.2e-7;
    panda_b 3.6e-7 / 3.2e-7 / 1.4e-6; arm12 2.1e-7 / 3.4e-7 / 8.5e-7; point3 2.5e-7 / 2.5e-7 / 1.0e-6; point2 5.2e-7 / 5.2e-7 / 2.1e-6;
    one 2.3e-7 / 3.1e-7 / 9.2e-7; limit 1.6e-7 / 1.9e-7 / 6.5e-7."""
    from motion_planning_baselines_amd import ops
    for R in M.rows_of(name):
        robot, field, mo = _mo(name, R, gpu_device)
        D = robot.q_dim
        r = M.reference(name, R)
        bar, cond = M.bar(r.E32_grad), r.conditioned
        for d in (D, 2 * D):
            x = M.trajs(name, R, d).to(gpu_device)
            for h_begin in (0, 1):
                k_sigma, weight = 2.0, 0.5
                out, grad = ops.moving_collision_grad(x, mo, k_sigma, weight=weight, h_begin=h_begin)
                assert torch.equal(out, ops.moving_collision_eval(x, mo, k_sigma, weight=weight, h_begin=h_begin))     # the same sums in the same order
                g = grad.cpu().double()
                assert bool(torch.isfinite(g).all())
                assert bool((g[..., D:] == 0).all()) and bool((g[:, :h_begin] == 0).all())
                want = r.g64.clone()
                want[:, :h_begin] = 0.0
                e = (g[..., :D] / (k_sigma * weight) - want).abs().amax(-1) / r.budget
                worst = float(e[cond].max())
                print(f'{name} R={R} d={d} h_begin={h_begin}: E32 {r.E32_grad:.2e} kernel {worst:.2e} bar {bar:.2e} '
                      f'({int((~cond).sum())} of {cond.numel()} rows not conditioned)')
                assert worst <= bar, (R, d, h_begin, worst, bar)


def test_accumulate_is_the_prefill_plus_a_fresh_evaluation_bit_for_bit(gpu_device):
    """out and grad equal prefill + fresh BIT FOR BIT; the velocity channels of an accumulated grad are left alone; two runs give
    identical bits."""
    from motion_planning_baselines_amd import ops
    for name, R, wide in (('panda_sb', 65, False), ('point2', 130, True)):
        robot, field, mo = _mo(name, R, gpu_device)
        D = robot.q_dim
        d = 2 * D if wide else D
        x = M.trajs(name, R, d).to(gpu_device)
        gen = torch.Generator().manual_seed(2)
        pre_out = torch.randn(M.B, generator=gen).to(gpu_device)
        pre_grad = torch.randn(M.B, R, d, generator=gen).to(gpu_device)
        fresh = ops.moving_collision_eval(x, mo, 3.0, weight=0.7)
        acc = ops.moving_collision_eval(x, mo, 3.0, weight=0.7, out=pre_out.clone(), accumulate=True)
        assert float(fresh.abs().max()) > 0 and torch.equal(acc, pre_out + fresh)
        f_out, f_grad = ops.moving_collision_grad(x, mo, 3.0, weight=0.7)
        a_out, a_grad = ops.moving_collision_grad(x, mo, 3.0, weight=0.7, out=pre_out.clone(), grad=pre_grad.clone(), accumulate=True)
        assert float(f_grad.abs().max()) > 0 and torch.equal(a_out, pre_out + f_out)
        assert torch.equal(a_grad[..., :D], pre_grad[..., :D] + f_grad[..., :D]) and torch.equal(a_grad[..., D:], pre_grad[..., D:])
        again_out, again_grad = ops.moving_collision_grad(x, mo, 3.0, weight=0.7)
        assert torch.equal(again_out, f_out) and torch.equal(again_grad, f_grad) and torch.equal(ops.moving_collision_eval(x, mo, 3.0, weight=0.7), fresh)


@pytest.mark.parametrize('name', M.CASES)
def test_predicate_equals_the_oracle_off_the_hinge_boundary(gpu_device, name):
    """Per row: the flag equals the oracle's wherever every sphere is at least DELTA off its hinge boundary -- on at least 97 % of the
    rows --; flag == (gap > 0); the gap is the per-row cost; or_into ORs the flags and adds the gap."""
    from motion_planning_baselines_amd import ops
    R = M.rows_of(name)[-1]
    robot, field, mo = _mo(name, R, gpu_device)
    r = M.reference(name, R)
    x = M.trajs(name, R, 2 * robot.q_dim).to(gpu_device)
    flag, gap = ops.moving_collision_check(x, mo, with_gap=True)
    assert flag.shape == gap.shape == (M.B, R)
    decided = r.cl.min_abs >= M.DELTA
    assert int(decided.sum()) >= 0.97 * decided.numel()
    assert torch.equal(flag.cpu()[decided], r.cl.contact[decided])
    assert torch.equal(flag, gap > 0)
    assert float(((gap.cpu().double() - r.c64).abs() / r.budget).max()) <= M.bar(r.E32_cost)
    gen = torch.Generator().manual_seed(4)
    before = (torch.rand(M.B, R, generator=gen) < 0.3).to(gpu_device)
    gap0 = torch.rand(M.B, R, generator=gen).to(gpu_device)
    f2, g2 = ops.moving_collision_check(x, mo, flag=before.clone(), gap=gap0.clone())
    assert torch.equal(f2, before | flag) and torch.equal(g2, gap0 + gap)
    assert torch.equal(ops.moving_collision_check(x, mo, flag=before.clone()), before | flag)


def test_a_frozen_field_agrees_with_the_static_kernels(gpu_device):
    """K = 1: the field means the static CollisionField of at(t); the static kernels (tested before this member existed) on
    DeviceGeometry(robot, field.at(t)) agree per row and per gradient element within the same bars."""
    from motion_planning_baselines_amd import ops
    name = 'one'
    for R in (8, 65):
        robot, field, mo = _mo(name, R, gpu_device)
        D = robot.q_dim
        r = M.reference(name, R)
        geom = ops.DeviceGeometry(robot, field.at(field.t_start), gpu_device)
        x = M.trajs(name, R, 2 * D).to(gpu_device)
        _, pw = ops.moving_collision_eval(x, mo, 1.0, h_begin=0, per_waypoint=True)
        _, pw_s = ops.cost_collision_eval(x, geom, 1.0, h_begin=0, per_waypoint=True)
        assert float(((pw.cpu().double() - pw_s.cpu().double()).abs() / r.budget).max()) <= M.bar(r.E32_cost)
        _, g = ops.moving_collision_grad(x, mo, 1.0, h_begin=0)
        _, g_s = ops.cost_collision_grad(x, geom, 1.0, h_begin=0)
        e = (g.cpu().double() - g_s.cpu().double())[..., :D].abs().amax(-1) / r.budget
        assert float(e[r.conditioned].max()) <= M.bar(r.E32_grad)


def test_update_with_a_shifted_field_equals_a_fresh_buffer(gpu_device):
    """update(field.shifted(dt)) re-packs into the SAME device buffer: bit for bit the outputs of a buffer built from the shifted field;
    a field of other shapes is refused."""
    from motion_planning_baselines_amd import geometry as G, ops
    robot, field, mo = _mo('panda_sb', 65, gpu_device)
    x = M.trajs('panda_sb', 65, robot.q_dim).to(gpu_device)
    before = ops.moving_collision_grad(x, mo, 2.0)
    ptr = mo.buf.data_ptr()
    moved = field.shifted(0.8)
    assert mo.update(moved) is mo and mo.buf.data_ptr() == ptr and mo.field is moved
    fresh = ops.DeviceMovingObstacles(robot, moved, gpu_device, 65)
    assert torch.equal(mo.buf, fresh.buf)
    got, want = ops.moving_collision_grad(x, mo, 2.0), ops.moving_collision_grad(x, fresh, 2.0)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and not torch.equal(got[0], before[0])
    with pytest.raises(ValueError, match='update'):
        mo.update(M.case('panda_s')[1])


def test_rows_that_are_not_the_buffers_are_refused_by_both_numbers(gpu_device):
    from motion_planning_baselines_amd import _lib, ops
    robot, field, mo = _mo('panda_s', 65, gpu_device)
    x = M.trajs('panda_s', 64, robot.q_dim).to(gpu_device)
    for call in (lambda: ops.moving_collision_eval(x, mo, 1.0), lambda: ops.moving_collision_grad(x, mo, 1.0), lambda: ops.moving_collision_check(x, mo)):
        with pytest.raises(_lib.MPBError, match=r'H = 64 .*n_rows = 65'):
            call()
    with pytest.raises(ValueError):
        ops.moving_collision_eval(x[..., :robot.q_dim - 1].contiguous(), mo, 1.0)
    assert ops.moving_collision_eval(M.trajs('panda_s', 65, robot.q_dim)[:0].to(gpu_device).contiguous(), mo, 1.0).shape == (0,)


def test_a_header_changed_behind_the_library_is_answered_with_nan(gpu_device):
    """The kernels compare the header with the numbers the launcher read once for that address: a buffer rewritten in place without
    mpb_moving_invalidate gets NaN (in collision), not an evaluation with stale sizes."""
    from motion_planning_baselines_amd import ops
    robot, field, mo = _mo('panda_sb', 8, gpu_device)
    x = M.trajs('panda_sb', 8, robot.q_dim).to(gpu_device)
    assert bool(torch.isfinite(ops.moving_collision_eval(x, mo, 1.0)).all())
    for word in (2, 4, 5, 6, 7):                             # n_dof, n_links, n_rows, n_spheres, n_boxes
        keep = int(mo.buf.view(torch.int32)[word])
        mo.buf.view(torch.int32)[word] = keep - 1
        out, grad = ops.moving_collision_grad(x, mo, 1.0)
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(grad[..., :robot.q_dim]).all())
        assert bool(ops.moving_collision_check(x, mo).all())
        mo.buf.view(torch.int32)[word] = keep
    assert bool(torch.isfinite(ops.moving_collision_eval(x, mo, 1.0)).all())
