"""The self-collision kernels (mpb_self_collision_eval / _grad / _check) and the classes in front of them against the fp64 oracle of
tests/self_collision_checks.py.  Shapes: B = 21 trajectories; H in {2, 8, 64, 65, 130} (one lane serves up to three waypoints);
d = D and d = 2 D; h_begin in {0, 1}; robots: the Panda, a 5-joint chain, the 12-joint chain of collision_kinks.scene() and a chain at the
limit of 64 collision spheres."""
import ctypes

import numpy as np
import pytest
import torch

import self_collision_checks as S

pytestmark = pytest.mark.gpu
HS = (2, 8, 64, 65, 130)
ULP = 2.0 ** -23


def _sc(name, dev):
    from motion_planning_baselines_amd import ops
    robot, field = S.case(name)
    return robot, field, ops.DeviceSelfCollision(robot, field, dev)


@pytest.mark.parametrize('name', S.CASES)
def test_cost_of_every_waypoint_and_out_against_fp64(gpu_device, name):
    """Per-waypoint cost on EVERY waypoint to bar(E32), E32 = the fp32 torch oracle's own worst error on the same inputs, both in units
    of max(1, active pairs); out to the same bar summed over its waypoints plus the fp32 summation's own rounding (a lane adds
    ceil(H / 64) values, the wave reduction six levels, two products: (ceil(H / 64) + 8) half-ulps of the sum of non-negative terms).
    Measured on an MI355X (worst over H, d, h_begin): Panda E32 6.6e-8, kernel 7.3e-8; 5-joint chain 8.1e-8 / 6.1e-8; 12-joint chain
    6.2e-8 / 5.5e-8; 64 spheres 1.2e-7 / 1.3e-7; the bar is 4.8e-7 (4 ulp) throughout."""
    from motion_planning_baselines_amd import ops
    robot, field, sc = _sc(name, gpu_device)
    D = robot.q_dim
    for H in HS:
        r = S.reference(name, H)
        bar = S.bar(r.E32_cost)
        for d in (D, 2 * D):
            x = S.trajs(name, H, d).to(gpu_device)
            for h_begin in (0, 1):
                k_sigma, weight = 4.0, 0.75
                out, pw = ops.self_collision_eval(x, sc, k_sigma, weight=weight, h_begin=h_begin, per_waypoint=True)
                pw, out = pw.cpu().double(), out.cpu().double()
                want = r.c64.clone()
                want[:, :h_begin] = 0.0
                assert bool((pw[:, :h_begin] == 0).all())
                e = float(((pw - want).abs() / r.budget).max())
                tot = want.sum(-1)
                eo = (out / (k_sigma * weight) - tot).abs()
                allow = bar * r.budget[:, h_begin:].sum(-1) + ((H + 63) // 64 + 8) * 0.5 * ULP * tot
                print(f'{name} H={H} d={d} h_begin={h_begin}: E32 {r.E32_cost:.2e} kernel {e:.2e} bar {bar:.2e}; out worst {float((eo / allow).max()):.2f} of its allowance')
                assert e <= bar, (H, d, h_begin, e, bar)
                assert bool((eo <= allow).all()), (H, d, h_begin)


@pytest.mark.parametrize('name', S.CASES)
def test_every_gradient_element_of_every_conditioned_waypoint(gpu_device, name):
    """Every element of d out / d trajs of every conditioned waypoint to bar(E32) (units of max(1, active pairs)); waypoints the
    classifier excludes are finite; velocity channels and rows below h_begin are exactly 0.
    Measured on an MI355X (worst over H): Panda E32 1.4e-7, kernel 1.7e-7 (bar 5.4e-7); 5-joint chain 1.3e-7 / 1.2e-7; 12-joint chain
    1.9e-7 / 1.3e-7; 64 spheres 3.9e-7 / 3.4e-7 (bar 1.6e-6)."""
    from motion_planning_baselines_amd import ops
    robot, field, sc = _sc(name, gpu_device)
    D = robot.q_dim
    for H in HS:
        r = S.reference(name, H)
        bar, cond = S.bar(r.E32_grad), r.cl.conditioned
        for d in (D, 2 * D):
            x = S.trajs(name, H, d).to(gpu_device)
            for h_begin in (0, 1):
                k_sigma, weight = 2.0, 0.5
                out, grad = ops.self_collision_grad(x, sc, k_sigma, weight=weight, h_begin=h_begin)
                out_eval = ops.self_collision_eval(x, sc, k_sigma, weight=weight, h_begin=h_begin)
                assert torch.equal(out, out_eval)                                         # the same sums in the same order
                g = grad.cpu().double()
                assert bool(torch.isfinite(g).all())
                assert bool((g[..., D:] == 0).all()) and bool((g[:, :h_begin] == 0).all())
                want = r.g64.clone()
                want[:, :h_begin] = 0.0
                e = (g[..., :D] / (k_sigma * weight) - want).abs().amax(-1) / r.budget
                worst = float(e[cond].max())
                print(f'{name} H={H} d={d} h_begin={h_begin}: E32 {r.E32_grad:.2e} kernel {worst:.2e} bar {bar:.2e} '
                      f'({int((~cond).sum())} of {cond.numel()} waypoints not conditioned)')
                assert worst <= bar, (H, d, h_begin, worst, bar)


def test_home_poses_cost_nothing(gpu_device):
    from motion_planning_baselines_amd import ops
    robot, field, sc = _sc('panda', gpu_device)
    x = torch.tensor(S.PANDA_HOME, dtype=torch.float32).repeat(5, 70, 1).to(gpu_device).contiguous()
    out, grad = ops.self_collision_grad(x, sc, 1.0e4, h_begin=0)
    out2, pw = ops.self_collision_eval(x, sc, 1.0e4, h_begin=0, per_waypoint=True)
    assert bool((out == 0).all()) and bool((grad == 0).all()) and bool((out2 == 0).all()) and bool((pw == 0).all())
    assert not bool(ops.self_collision_check(x[0, :3].contiguous(), sc).any())


def test_accumulate_is_the_prefill_plus_a_fresh_evaluation_bit_for_bit(gpu_device):
    """accumulate adds the fresh value onto the old one in ONE fp32 rounding (add_rounded in csrc/mpb_member_cost.h keeps the
    compiler from contracting old + scale * x into an fma): out and grad equal prefill + fresh BIT FOR BIT; the velocity channels of
    an accumulated grad are left alone; two runs give identical bits."""
    from motion_planning_baselines_amd import ops
    robot, field, sc = _sc('panda', gpu_device)
    D = robot.q_dim
    for H, d in ((65, D), (130, 2 * D)):
        x = S.trajs('panda', H, d).to(gpu_device)
        gen = torch.Generator().manual_seed(2)
        pre_out = torch.randn(S.B, generator=gen).to(gpu_device)
        pre_grad = torch.randn(S.B, H, d, generator=gen).to(gpu_device)
        fresh = ops.self_collision_eval(x, sc, 3.0, weight=0.7)
        acc = ops.self_collision_eval(x, sc, 3.0, weight=0.7, out=pre_out.clone(), accumulate=True)
        assert float(fresh.abs().max()) > 0 and torch.equal(acc, pre_out + fresh)
        f_out, f_grad = ops.self_collision_grad(x, sc, 3.0, weight=0.7)
        a_out, a_grad = ops.self_collision_grad(x, sc, 3.0, weight=0.7, out=pre_out.clone(), grad=pre_grad.clone(), accumulate=True)
        assert float(f_grad.abs().max()) > 0 and torch.equal(a_out, pre_out + f_out)
        assert torch.equal(a_grad[..., :D], pre_grad[..., :D] + f_grad[..., :D]) and torch.equal(a_grad[..., D:], pre_grad[..., D:])
        again_out, again_grad = ops.self_collision_grad(x, sc, 3.0, weight=0.7)
        assert torch.equal(again_out, f_out) and torch.equal(again_grad, f_grad) and torch.equal(ops.self_collision_eval(x, sc, 3.0, weight=0.7), fresh)


@pytest.mark.parametrize('name', S.CASES)
def test_predicate_equals_the_oracle_off_the_hinge_boundary(gpu_device, name):
    from motion_planning_baselines_amd import ops
    robot, field, sc = _sc(name, gpu_device)
    r = S.reference(name, 130)
    q = r.q.reshape(-1, robot.q_dim).to(gpu_device).contiguous()
    flag, gap = ops.self_collision_check(q, sc, with_gap=True)
    decided = (r.cl.min_abs >= S.DELTA).reshape(-1)
    want = r.cl.contact.reshape(-1)
    assert int(decided.sum()) > 0.98 * decided.numel()
    assert torch.equal(flag.cpu()[decided], want[decided])
    assert torch.equal(flag, gap > 0)
    assert float(((gap.cpu().double() - r.c64.reshape(-1)).abs() / r.budget.reshape(-1)).max()) <= S.bar(r.E32_cost)
    # or_into keeps earlier flags and adds onto an earlier gap
    gen = torch.Generator().manual_seed(4)
    before = (torch.rand(q.shape[0], generator=gen) < 0.3).to(gpu_device)
    gap0 = torch.rand(q.shape[0], generator=gen).to(gpu_device)
    f2, g2 = ops.self_collision_check(q, sc, flag=before.clone(), gap=gap0.clone())
    assert torch.equal(f2, before | flag) and torch.equal(g2, gap0 + gap)
    assert torch.equal(ops.self_collision_check(q, sc, flag=before.clone()), before | flag)


def test_planning_task_ors_the_self_predicate_in(gpu_device):
    """compute_collision with self_field = the obstacle flags OR the self flags; random_coll_free_q returns only configurations the
    ORACLE calls free of both (wherever it can decide: DELTA off either hinge boundary)."""
    import collision_kinks as K
    from motion_planning_baselines_amd import geometry as G, ops
    from motion_planning_baselines_amd.robot_field import PlanningTask
    from oracle.geometry_ref import make_ref_geometry
    robot, sfield = S.case('panda')
    field = G.env_spheres_3d(0)
    ta = dict(device=gpu_device, dtype=torch.float32)
    task = PlanningTask(robot, field, self_field=sfield, tensor_args=ta, seed=3)
    plain = PlanningTask(robot, field, tensor_args=ta, seed=3)
    q = S.uniform_q(robot, 3000, seed=5).to(gpu_device)
    both = task.compute_collision(q.reshape(30, 100, -1))
    obst, selff = plain.compute_collision(q), ops.self_collision_check(q, task.self_geom)
    assert both.shape == (30, 100) and torch.equal(both.reshape(-1), obst | selff)
    assert int(selff.sum()) > 0 and int((selff & ~obst).sum()) > 0 and int((obst & ~selff).sum()) > 0
    free = task.random_coll_free_q(500, max_samples=700)
    assert free.shape == (500, robot.q_dim) and not bool(task.compute_collision(free).any())
    q64 = free.cpu().double()
    rr64, rf64 = make_ref_geometry(robot, field, S.F64)
    a, b, T = S.pair_data(sfield, S.F64)
    cl = S.classify(rr64, a, b, T, q64)
    ob = K.classify(rr64, rf64, q64).fields[0]
    assert not bool((cl.contact & (cl.min_abs >= S.DELTA)).any())
    assert not bool((ob.active & (ob.a.abs() >= S.DELTA)).any())


def test_cost_classes_against_the_oracle(gpu_device):
    """CostCollision(field=SelfCollisionField) and a CostComposite that holds one: eval = the members one by one; eval_with_grad = the
    oracle; get_linear_system = (-jacobian, costs, I / sigma^2) at B = 3, H = 5."""
    from motion_planning_baselines_amd import geometry as G
    from motion_planning_baselines_amd.planners.costs import cost_functions as C
    dev = gpu_device
    ta = dict(device=dev, dtype=torch.float32)
    robot, sfield = S.case('panda')
    D, H = robot.q_dim, 65
    r = S.reference('panda', H)
    x = S.trajs('panda', H, 2 * D).to(dev)
    sigma = 0.25
    cs = C.CostCollision(robot, H, field=sfield, sigma_coll=sigma, tensor_args=ta)
    co = C.CostCollision(robot, H, field=G.env_spheres_3d(0), sigma_coll=0.5, tensor_args=ta)
    gp = C.CostGPTrajectory(robot, H, 0.04, sigma_gp=2.0, tensor_args=ta)
    assert cs.is_self and not co.is_self
    want = r.c64[:, 1:].sum(-1) / sigma ** 2
    got = cs(x).cpu().double()
    allow = S.bar(r.E32_cost) * r.budget[:, 1:].sum(-1) / sigma ** 2 + 10 * 0.5 * ULP * want
    assert bool(((got - want).abs() <= allow).all())
    cost, grad = cs.eval_with_grad(x, weight=2.0)
    assert torch.equal(cost, 2.0 * cs(x)) or float((cost - 2.0 * cs(x)).abs().max()) <= ULP * float(cost.abs().max())
    e = (grad.cpu().double()[..., :D] * sigma ** 2 / 2.0 - torch.cat([torch.zeros_like(r.g64[:, :1]), r.g64[:, 1:]], 1)).abs().amax(-1) / r.budget
    assert float(e[r.cl.conditioned].max()) <= S.bar(r.E32_grad)
    # a composite: members one by one, in the order and with the roundings of its accumulating launches
    for members, w in (([co, cs, gp], [1.0, 2.0, 0.5]), ([cs, co], [0.3, 1.0]), ([cs], [1.5]), ([gp, cs], [1.0, 1.0])):
        comp = C.CostComposite(robot, H, members, weights_cost_l=w, tensor_args=ta)
        assert C.fusable_collision(comp) is None and comp.single_collision_term() is None
        assert all(not c.is_self for c, _ in comp.collision_terms()) and [c for c, _ in comp.self_terms()] == [cs]
        plan = C.device_plan(comp, dev)
        assert plan is not None and [c for c, _ in plan.selfs] == [cs] and (plan[0] is co) == (co in members)
        total = comp(x).cpu().double()
        one_by_one = sum(wi * m(x).cpu().double() for m, wi in zip(members, w))
        assert float((total - one_by_one).abs().max()) <= len(members) * ULP * float(one_by_one.abs().max())
    assert C.fusable_collision(cs) is None and C.fusable_collision(co) is not None
    with pytest.raises(AssertionError):
        C.MergedCollision([(co, 1.0), (cs, 1.0)])
    # the linear system at B = 3, H = 5
    Hs = 5
    xs = x[:3, 20:25].contiguous()
    cs5 = C.CostCollision(robot, Hs, field=sfield, sigma_coll=sigma, tensor_args=ta)
    A, b, K = cs5.get_linear_system(xs)
    assert A.shape == (3, Hs - 1, 2 * D * Hs) and b.shape == (3, Hs - 1, 1) and K.shape == (3, Hs - 1, Hs - 1)
    sub = lambda t: t[:3, 20:25]
    assert bool(sub(r.cl.contact)[:, 1:].any())
    for i in range(Hs - 1):
        cols = slice((i + 1) * 2 * D, (i + 1) * 2 * D + D)
        ei = (A[:, i, cols].cpu().double() + sub(r.g64)[:, i + 1]).abs().amax(-1) / sub(r.budget)[:, i + 1]
        ok = sub(r.cl.conditioned)[:, i + 1]
        assert float(ei[ok].max()) <= S.bar(r.E32_grad) if bool(ok.any()) else True
        rest = A[:, i].clone()
        rest[:, cols] = 0
        assert not bool(rest.any())
    assert float(((b[..., 0].cpu().double() - sub(r.c64)[:, 1:]).abs() / sub(r.budget)[:, 1:]).max()) <= S.bar(r.E32_cost)
    assert torch.equal(K, (torch.eye(Hs - 1, device=dev) / sigma ** 2).repeat(3, 1, 1))
    # through a composite (what GPMP2's dense route stacks)
    Ac, bc, Kc = C.CostComposite(robot, Hs, [C.CostCollision(robot, Hs, field=G.env_spheres_3d(0), sigma_coll=0.5, tensor_args=ta), cs5],
                                 tensor_args=ta).get_linear_system(xs)
    assert torch.equal(Ac[:, Hs - 1:], A) and torch.equal(bc[:, Hs - 1:], b) and torch.equal(Kc[:, Hs - 1:, Hs - 1:], K)


def test_abi_refusals_come_in_the_documented_order(gpu_device):
    """include/mpb.h: unsupported row width first, then bad shapes, then the empty batch (OK, nothing launched), then null / misaligned
    pointers, then the header."""
    from motion_planning_baselines_amd import _lib, ops
    from motion_planning_baselines_amd import self_layout as L
    lib = _lib.lib()
    robot, field, sc = _sc('panda', gpu_device)
    D = robot.q_dim
    x = S.trajs('panda', 8, D).to(gpu_device)
    out, grad, pw = torch.zeros(S.B, device=gpu_device), torch.zeros_like(x), None
    P = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    null, stream = ctypes.c_void_p(0), ctypes.c_void_p(0)
    msg = lambda: lib.mpb_last_error().decode()
    with torch.cuda.device(gpu_device):
        for fn, g in ((lib.mpb_self_collision_eval, pw), (lib.mpb_self_collision_grad, grad)):
            call = lambda tr, sb, o, B=S.B, H=8, d=D, hb=1: fn(tr, sb, o, P(g), B, H, d, hb, 1.0, 1.0, 0, stream)
            assert call(null, null, null, B=-1, d=25) == 2 and 'MPB_MAX_DOF' in msg()               # 1. before everything else
            assert call(null, null, null, B=-1) == 1 and 'bad shape' in msg()                      # 2. before the pointers
            assert call(null, null, null, H=0) == 1 and call(null, null, null, hb=-1) == 1 and call(null, null, null, d=0) == 1
            assert call(null, null, null, B=0) == 0                                                # 3. the empty batch needs no pointers
            assert call(null, P(sc.buf), P(out)) == 1 and 'null pointer' in msg()                  # 4.
            assert call(P(x), null, P(out)) == 1 and call(P(x), P(sc.buf), null) == 1
            assert call(P(x), ctypes.c_void_p(sc.buf.data_ptr() + 4), P(out)) == 1 and 'aligned' in msg()
            bad = sc.buf.clone()
            bad.view(torch.int32)[0] ^= 1
            lib.mpb_self_invalidate(P(bad))                                                        # (a new buffer at a possibly reused address)
            assert call(P(x), P(bad), P(out)) == 1 and 'magic' in msg()                            # 5. the header
            big = sc.buf.clone()
            big.view(torch.int32)[4] = L.SELF_MAX_LINKS + 1
            lib.mpb_self_invalidate(P(big))
            assert call(P(x), P(big), P(out)) == 2 and 'MPB_SELF_MAX_LINKS' in msg()
            assert call(P(x[..., :D - 1].contiguous()), P(sc.buf), P(out), d=D - 1) == 1 and 'narrower' in msg()
            assert call(P(x), P(sc.buf), P(out)) == 0
        assert lib.mpb_self_collision_grad(P(x), P(sc.buf), P(out), null, S.B, 8, D, 1, 1.0, 1.0, 0, stream) == 1       # grad is required
        q = x.reshape(-1, D).contiguous()
        flag = torch.zeros(q.shape[0], dtype=torch.bool, device=gpu_device)
        chk = lambda qq, sb, f, N=q.shape[0], Dd=D: lib.mpb_self_collision_check(qq, sb, f, null, N, Dd, 0, stream)
        assert chk(null, null, null, N=-1, Dd=13) == 2
        assert chk(null, null, null, N=-1) == 1 and chk(null, null, null, Dd=0) == 1
        assert chk(null, null, null, N=0) == 0
        assert chk(null, P(sc.buf), P(flag)) == 1 and chk(P(q), null, P(flag)) == 1 and chk(P(q), P(sc.buf), null) == 1
        assert chk(P(q), ctypes.c_void_p(sc.buf.data_ptr() + 4), P(flag)) == 1
        assert chk(P(q), P(sc.buf), P(flag), Dd=D - 1) == 1 and 'joints' in msg()
        assert chk(P(q), P(sc.buf), P(flag)) == 0
    torch.cuda.synchronize()
    # the wrappers refuse on the host what would be refused there
    with pytest.raises(ValueError):
        ops.self_collision_eval(x.cpu(), sc, 1.0)
    with pytest.raises(ValueError):
        ops.self_collision_eval(x, sc, 1.0, accumulate=True)
    with pytest.raises(ValueError):
        ops.self_collision_check(x.reshape(-1, D)[:, :D - 1].contiguous(), sc)
    assert ops.self_collision_eval(x[:0].contiguous(), sc, 1.0).shape == (0,)


def test_a_reused_device_address_is_read_again(gpu_device):
    """The library reads a self buffer's header once per address; DeviceSelfCollision announces its (possibly reused) address with
    mpb_self_invalidate, so a second robot whose buffer lands where the first one's was is evaluated with ITS numbers."""
    from motion_planning_baselines_amd import ops
    for name in ('panda', 'arm5', 'panda', 'chain64'):
        robot, field, sc = _sc(name, gpu_device)
        r = S.reference(name, 8)
        _, pw = ops.self_collision_eval(S.trajs(name, 8, robot.q_dim).to(gpu_device), sc, 1.0, h_begin=0, per_waypoint=True)
        assert float(((pw.cpu().double() - r.c64).abs() / r.budget).max()) <= S.bar(r.E32_cost)
        del sc


def test_a_header_changed_behind_the_library_is_answered_with_nan(gpu_device):
    """The kernels compare the header (magic, n_dof, n_links, n_pairs) with the numbers the launcher read once for that address: a
    buffer rewritten in place without mpb_self_invalidate gets NaN (in collision), not an evaluation with stale sizes; once announced,
    the header is read again and refused on the host."""
    from motion_planning_baselines_amd import _lib, ops
    robot, field, sc = _sc('panda', gpu_device)
    x = S.trajs('panda', 8, robot.q_dim).to(gpu_device)
    assert bool(torch.isfinite(ops.self_collision_eval(x, sc, 1.0)).all())
    for word in (2, 4, 5):                                   # n_dof, n_links, n_pairs
        keep = int(sc.buf.view(torch.int32)[word])
        sc.buf.view(torch.int32)[word] = keep - 1
        out, grad = ops.self_collision_grad(x, sc, 1.0)
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(grad[..., :robot.q_dim]).all())
        assert bool(ops.self_collision_check(x.reshape(-1, robot.q_dim).contiguous(), sc).all())
        sc.buf.view(torch.int32)[word] = keep
    assert bool(torch.isfinite(ops.self_collision_eval(x, sc, 1.0)).all())
    sc.buf.view(torch.int32)[2] -= 1
    _lib.lib().mpb_self_invalidate(ctypes.c_void_p(sc.buf.data_ptr()))
    with pytest.raises(_lib.MPBError, match='transforms'):
        ops.self_collision_eval(x, sc, 1.0)


def test_a_buffer_evicted_from_the_header_table_is_read_again(gpu_device):
    """The library keeps the headers of 16 buffer addresses, replaced in turn.  Seventeen live buffers of the smallest chain the validator
    takes (2 spheres, 1 pair; two joints, so that the pair's distance follows q_1), each with a margin -- so a cost -- of its own,
    evaluated once each at B = 1, H = 2: the seventeenth takes the first one's place, and the first, read again, gives the bits of its
    first evaluation."""
    from motion_planning_baselines_amd import geometry as G, ops
    tfs = np.stack([G._mdh(0.0, 0.0, 0.1), G._mdh(0.0, 0.3, 0.0)])
    robot = G.RobotSerialChain(tfs, [1, 2], [(0.0, 0.0, 0.0), (0.2, 0.0, 0.0)], [0.05, 0.05], q_min=[-2.0, -2.0], q_max=[2.0, 2.0])
    x = torch.tensor([[[0.3, 0.5], [-0.4, 2.0]]], device=gpu_device)                      # centres 0.49 and 0.28 apart
    scs = [ops.DeviceSelfCollision(robot, G.SelfCollisionField(robot, margin=0.5 + 0.01 * i, pairs=[(0, 1)]), gpu_device) for i in range(17)]
    assert len({sc.buf.data_ptr() for sc in scs}) == 17 and (scs[0].n_links, scs[0].n_pairs) == (2, 1)
    first = [ops.self_collision_eval(x, sc, 2.0, h_begin=0, per_waypoint=True) for sc in scs]
    assert len({float(out) for out, _ in first}) == 17 and all(bool((pw > 0).all()) for _, pw in first)
    out, pw = ops.self_collision_eval(x, scs[0], 2.0, h_begin=0, per_waypoint=True)
    assert torch.equal(out, first[0][0]) and torch.equal(pw, first[0][1])
