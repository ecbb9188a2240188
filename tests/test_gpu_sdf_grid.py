"""The SDF-grid kernels (csrc/mpb_sdf_grid.hip) against the fp64 oracle of tests/sdf_grid_checks.py: the builder node by node, the sampler
value and gradient, cost and gradient per waypoint and per element on four robots, accumulation bit for bit, the predicate, and the grid
built on the GPU against the same grid supplied from the host.  Bars: FACTOR times the fp32 restatement's own worst error on the same
inputs (collision_kinks.bar); nothing is fixed in advance."""
import functools

import numpy as np
import pytest
import torch

import sdf_grid_checks as S

pytestmark = pytest.mark.gpu
K_SIGMA, WEIGHT = 2.5, 0.7


@functools.lru_cache(maxsize=None)
def _device_grid(name, dev):
    """The case's grid with HOST-SUPPLIED node values (the fp64 oracle's, rounded to fp32) on the device: a build error cannot hide here."""
    from motion_planning_baselines_amd import ops
    c = S.case(name)
    return ops.DeviceSDFGrid(c.robot, c.grid, dev)


# ------------------------------------------------------------------------------------------------
# build
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scene,lo,dims,cell', [('sb3d', (-0.9, -0.7, -0.5), (9, 7, 5), 0.23), ('sb3d', (-0.95, 0.1, -0.2), (70, 3, 2), 0.027),
                                                ('dense2d', (-1.0, -0.9), (12, 9, 1), 0.19)])
def test_build_every_node_against_the_oracle(gpu_device, scene, lo, dims, cell):
    """mpb_sdf_grid_build on env_spheres_boxes_3d() (9 x 7 x 5; 70 x 3 x 2: a dimension beyond one wave, 420 nodes: a ragged last block)
    and env_dense_2d() (12 x 9 x 1, planar): every node against the fp64 oracle's signed_distance at the node position (the header's
    fp32 lo and cell in fp64).  Bar: FACTOR * the fp32 restatement's worst error on those nodes."""
    from motion_planning_baselines_amd import geometry as G, ops
    field = G.env_spheres_boxes_3d() if scene == 'sb3d' else G.env_dense_2d()
    hi = tuple(l + (n - 1) * cell - 0.3 * cell for l, n in zip(lo, dims))             # ceil((hi - lo) / cell) + 1 = n
    gf = G.GridSDFField.from_field(field, lo, hi, cell)
    assert gf.dims == dims and gf.planar == (scene == 'dense2d')
    sdf = ops.DeviceSDFGrid(G.RobotPointMass(3 if scene == 'sb3d' else 2), gf, gpu_device)
    got = sdf.nodes.cpu()
    g64 = S.grid_data(np.zeros(dims[::-1], np.float32), gf.lo, gf.cell, gf.inv_cell, S.F64)
    g32 = S.grid_data(np.zeros(dims[::-1], np.float32), gf.lo, gf.cell, gf.inv_cell, S.F32)
    want = S.exact_sdf(field, S.node_positions(g64), S.F64)
    e32 = float((S.exact_sdf(field, S.node_positions(g32), S.F32).double() - want).abs().max())
    err = float((got.double() - want).abs().max())
    print(f'build {scene} {dims}: E32 {e32:.3e}, kernel {err:.3e}, bar {S.FACTOR * e32:.3e}')
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    assert err <= S.FACTOR * e32
    assert float(want.min()) < 0 < float(want.max())                                   # nodes inside obstacles and outside
    sdf2 = ops.DeviceSDFGrid(G.RobotPointMass(3 if scene == 'sb3d' else 2), gf, gpu_device)
    assert torch.equal(sdf2.nodes, sdf.nodes)                                          # two builds give equal bits


# ------------------------------------------------------------------------------------------------
# sample
# ------------------------------------------------------------------------------------------------
def _sample_grid(planar):
    """A lattice whose numbers are exact in binary (lo -1, cell 1/8, 17 nodes per axis: u is an integer at every node) holding the oracle's
    distances to env_spheres_boxes_3d() quantised to multiples of 2^-12: differences and sums of such values are exact in fp32, so the
    lerp form returns the node's bits also at an axis' LAST node, where f = 1 (with arbitrary fp32 values v0 + (v1 - v0) may round)."""
    from motion_planning_baselines_amd import geometry as G
    field = G.env_spheres_boxes_3d()
    layout = G.GridSDFField.from_field(field, (-1, -1, -1), (1, 1, 1), 0.125, planar=planar)
    v = np.round(S.oracle_nodes(field, layout).astype(np.float64) * 4096.0) / 4096.0
    return G.GridSDFField(v.astype(np.float32), (-1, -1, -1), 0.125, margin=0.04)


@pytest.mark.parametrize('planar', [False, True])
def test_sample_value_and_gradient(gpu_device, planar):
    from motion_planning_baselines_amd import geometry as G, ops
    gf = _sample_grid(planar)
    assert gf.dims == (17, 17, 1 if planar else 17)
    sdf = ops.DeviceSDFGrid(G.RobotPointMass(3), gf, gpu_device) if not planar else ops.DeviceSDFGrid(G.RobotPointMass(2), gf, gpu_device)
    g64 = S.grid_data(gf.values, gf.lo, gf.cell, gf.inv_cell, S.F64)
    g32 = S.grid_data(gf.values, gf.lo, gf.cell, gf.inv_cell, S.F32)
    # every node position: the node's bits
    xn = S.node_positions(g32).reshape(-1, 3)
    s, g = ops.sdf_grid_sample(xn.to(gpu_device).contiguous(), sdf, with_grad=True)
    assert torch.equal(s.cpu(), g32.nodes.reshape(-1))
    assert bool(torch.isfinite(g).all())
    # 2000 random points, some of them outside the box
    rng = np.random.RandomState(11)
    x = torch.from_numpy(rng.uniform(-1.15, 1.15, (2000, 3)).astype(np.float32))
    s, g = (t.cpu() for t in ops.sdf_grid_sample(x.to(gpu_device), sdf, with_grad=True))
    s64, gr64 = S.sample_grad(g64, x.double())
    s32, gr32 = S.sample_grad(g32, x)
    off_face = S.face_distance(g64, x.double()) >= S.DELTA
    E32s, E32g = float((s32.double() - s64).abs().max()), float((gr32.double() - gr64).abs().amax(-1)[off_face].max())
    es, eg = float((s.double() - s64).abs().max()), float((g.double() - gr64).abs().amax(-1)[off_face].max())
    print(f'sample planar={planar}: value E32 {E32s:.3e} kernel {es:.3e}; gradient E32 {E32g:.3e} kernel {eg:.3e}; '
          f'{int((~S.inside_box(g64, x.double())).sum())} outside, {int((~off_face).sum())} on a face')
    assert es <= S.bar(E32s) and eg <= S.bar(E32g)
    assert int(off_face.sum()) > 1900
    # outside the box on each side of each axis: the clamped value and exactly 0.0 along the clamped axes
    inner = torch.from_numpy(rng.uniform(-0.9, 0.9, (64, 3)).astype(np.float32))
    for axis in range(2 if planar else 3):
        for side, edge in ((-1.0, -1.0), (1.0, 1.0)):
            out, clamped = inner.clone(), inner.clone()
            out[:, axis] = edge + side * torch.from_numpy(rng.uniform(0.01, 0.5, 64).astype(np.float32))
            clamped[:, axis] = edge
            so, go = (t.cpu() for t in ops.sdf_grid_sample(out.to(gpu_device), sdf, with_grad=True))
            sc, gc = (t.cpu() for t in ops.sdf_grid_sample(clamped.to(gpu_device), sdf, with_grad=True))
            assert torch.equal(so, sc), (axis, side)
            assert not bool(go[:, axis].any()), (axis, side)
            others = [a for a in range(3) if a != axis]
            assert torch.equal(go[:, others], gc[:, others])
            s64o, g64o = S.sample_grad(g64, out.double())
            assert float((so.double() - s64o).abs().max()) <= S.bar(E32s) and not bool(g64o[:, axis].any())
    if planar:                                              # z is ignored
        shifted = x.clone()
        shifted[:, 2] += 3.0
        s2, g2 = (t.cpu() for t in ops.sdf_grid_sample(shifted.to(gpu_device), sdf, with_grad=True))
        assert torch.equal(s2, s) and torch.equal(g2, g) and not bool(g[:, 2].any())


def test_sample_autograd_op(gpu_device):
    from motion_planning_baselines_amd import geometry as G, ops
    from motion_planning_baselines_amd.robot_field import DeviceGridField, sdf_grid_sample
    gf = _sample_grid(False)
    sdf = ops.DeviceSDFGrid(G.RobotPointMass(3), gf, gpu_device)
    rng = np.random.RandomState(3)
    x = torch.from_numpy(rng.uniform(-0.9, 0.9, (5, 6, 1, 3)).astype(np.float32)).to(gpu_device).requires_grad_(True)
    s = sdf_grid_sample(x, sdf)
    assert s.shape == (5, 6, 1)
    (s * 2.0).sum().backward()
    s0, g0 = ops.sdf_grid_sample(x.detach().reshape(-1, 3).contiguous(), sdf, with_grad=True)
    assert torch.equal(s.detach().reshape(-1), s0) and torch.equal(x.grad.reshape(-1, 3), 2.0 * g0)
    cost = DeviceGridField(sdf).compute_cost(None, x.detach())
    thr = torch.tensor([G.RobotPointMass(3).radius], dtype=torch.float32, device=gpu_device) + 0.04        # margin + r in fp32, as the kernels add them
    assert torch.equal(cost.reshape(-1), torch.relu(thr - s0))


# ------------------------------------------------------------------------------------------------
# cost and gradient
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H', [8, 64, 70])
@pytest.mark.parametrize('name', S.CASES)
def test_cost_and_gradient_per_waypoint_and_element(gpu_device, name, H):
    """B = 21 trajectories of H waypoints (H = 70: a second trip with six live lanes), d = D and d = 2 D, h_begin 0 and 1: every cost
    on every waypoint and every gradient element on the conditioned ones within bar(E32), in units of k_sigma * weight *
    max(1, active spheres); per_waypoint is the un-scaled cost and 0 below h_begin; the velocity channels of a fresh gradient are 0."""
    from motion_planning_baselines_amd import ops
    r = S.reference(name, H)
    sdf = _device_grid(name, gpu_device)
    D = r.case.robot.q_dim
    bar_c, bar_g = S.bar(r.E32_cost), S.bar(r.E32_grad)
    cond = r.cl.conditioned
    n_contact = int(r.cl.contact.sum())
    assert n_contact >= 10 and int((r.cl.contact & cond).sum()) >= 10
    worst_c = worst_g = 0.0
    for d in (D, 2 * D):
        x = S.trajs(name, H, d).to(gpu_device)
        assert torch.equal(x[..., :D].cpu(), r.q)
        for h_begin in (0, 1):
            keep = (torch.arange(H) >= h_begin).double()
            out, pw = ops.sdf_grid_eval(x, sdf, K_SIGMA, weight=WEIGHT, h_begin=h_begin, per_waypoint=True)
            out_g, grad = ops.sdf_grid_grad(x, sdf, K_SIGMA, weight=WEIGHT, h_begin=h_begin)
            out, pw, out_g, grad = out.cpu(), pw.cpu(), out_g.cpu(), grad.cpu()
            assert torch.equal(out, out_g)                                     # the two kernels sum alike
            assert not bool(pw[:, :h_begin].any())
            ec = (pw.double() - r.c64 * keep).abs() / r.budget
            worst_c = max(worst_c, float(ec.max()))
            assert float(ec.max()) <= bar_c, (d, h_begin, float(ec.max()), bar_c)
            want_out = K_SIGMA * WEIGHT * (r.c64 * keep).sum(-1)
            # (+ the sum's own roundings: two trips, six reduction levels, two products -- ten of at most 2^-24 relative each)
            allow = K_SIGMA * WEIGHT * (bar_c * (r.budget * keep).sum(-1) + 8 * 2.0 ** -23 * (r.c64 * keep).sum(-1))
            assert bool(((out.double() - want_out).abs() <= allow).all())
            eg = (grad[..., :D].double() / (K_SIGMA * WEIGHT) - r.g64 * keep[:, None]).abs().amax(-1) / r.budget
            worst_g = max(worst_g, float(eg[cond].max()))
            assert float(eg[cond].max()) <= bar_g, (d, h_begin, float(eg[cond].max()), bar_g)
            assert not bool(grad[:, :h_begin].any()) and not bool(grad[..., D:].any())
    print(f'{name} H={H}: {n_contact} waypoints in contact, {int((~cond).sum())} not conditioned; cost E32 {r.E32_cost:.3e} kernel {worst_c:.3e} '
          f'bar {bar_c:.3e}; gradient E32 {r.E32_grad:.3e} kernel {worst_g:.3e} bar {bar_g:.3e}')


@pytest.mark.parametrize('name', ['panda', 'point2d'])
def test_accumulate_is_bit_exact_and_runs_repeat(gpu_device, name):
    """accumulate=True onto random out / grad equals torch.add of the buffer and a fresh evaluation bit for bit (the kernel adds the
    fresh value in ONE rounding), the velocity channels are left alone, and two runs give equal bits."""
    from motion_planning_baselines_amd import ops
    H = 70
    sdf = _device_grid(name, gpu_device)
    D = S.case(name).robot.q_dim
    x = S.trajs(name, H, 2 * D).to(gpu_device)
    gen = torch.Generator().manual_seed(5)
    out0 = torch.randn(S.B, generator=gen).to(gpu_device)
    grad0 = torch.randn(S.B, H, 2 * D, generator=gen).to(gpu_device)
    fresh_out, fresh_grad = ops.sdf_grid_grad(x, sdf, K_SIGMA, weight=WEIGHT)
    again_out, again_grad = ops.sdf_grid_grad(x, sdf, K_SIGMA, weight=WEIGHT)
    assert torch.equal(fresh_out, again_out) and torch.equal(fresh_grad, again_grad) and float(fresh_out.max()) > 0
    out, grad = out0.clone(), grad0.clone()
    ops.sdf_grid_grad(x, sdf, K_SIGMA, weight=WEIGHT, out=out, grad=grad, accumulate=True)
    assert torch.equal(out, out0 + fresh_out)
    assert torch.equal(grad[..., :D], grad0[..., :D] + fresh_grad[..., :D]) and torch.equal(grad[..., D:], grad0[..., D:])
    out = out0.clone()
    ops.sdf_grid_eval(x, sdf, K_SIGMA, weight=WEIGHT, out=out, accumulate=True)
    assert torch.equal(out, out0 + ops.sdf_grid_eval(x, sdf, K_SIGMA, weight=WEIGHT))
    with pytest.raises(ValueError, match='accumulate'):
        ops.sdf_grid_eval(x, sdf, K_SIGMA, accumulate=True)


# ------------------------------------------------------------------------------------------------
# predicate
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', S.CASES)
def test_predicate_against_the_oracle(gpu_device, name):
    """On the case's configurations the predicate equals the oracle's c > 0 wherever no sphere is in the hinge band; the gap is the cost;
    or_into ORs the flags and adds the gap."""
    from motion_planning_baselines_amd import ops
    c = S.case(name)
    sdf = _device_grid(name, gpu_device)
    rr, g, thr = S.data(c, S.F64)
    q = S.uniform_q(c.robot, c.n_q)
    cl = S.classify(rr, g, thr, q.double())
    c64 = S.oracle_cost(rr, g, thr, q.double())
    flag, gap = (t.cpu() for t in ops.sdf_grid_check(q.to(gpu_device), sdf, with_gap=True))
    decided = ~cl.band
    assert int(decided.sum()) >= c.n_q - 8 and 0.1 < float(cl.contact.double().mean()) < 0.6
    assert torch.equal(flag[decided], (c64 > 0)[decided])
    assert torch.equal(flag, gap > 0)
    r32 = S.data(c, S.F32)
    E32 = float(((S.oracle_cost(*r32, q).double() - c64).abs() / cl.n_active.clamp_min(1)).max())
    assert float(((gap.double() - c64).abs() / cl.n_active.clamp_min(1)).max()) <= S.bar(E32)
    gen = torch.Generator().manual_seed(2)
    flag0 = (torch.rand(c.n_q, generator=gen) < 0.3).to(gpu_device)
    gap0 = torch.rand(c.n_q, generator=gen).to(gpu_device)
    f2, g2 = flag0.clone(), gap0.clone()
    ops.sdf_grid_check(q.to(gpu_device), sdf, with_gap=True, flag=f2, gap=g2)
    assert torch.equal(f2.cpu(), flag0.cpu() | flag) and torch.equal(g2.cpu(), gap0.cpu() + gap)
    assert ops.sdf_grid_check(q[:0].to(gpu_device), sdf).numel() == 0                   # an empty batch launches nothing


def test_corrupted_header_reads_as_nan_and_the_validator_raises(gpu_device):
    """A buffer whose header changes AFTER the library has read it: the kernels compare the header with what they were launched with and
    answer NaN / in collision; the host validator refuses the same words."""
    from motion_planning_baselines_amd import _lib, ops, sdf_layout as L
    c = S.case('point3d')
    sdf = ops.DeviceSDFGrid(c.robot, c.grid, gpu_device)
    x = S.trajs('point3d', 8, 3).to(gpu_device)
    q = S.uniform_q(c.robot, 100).to(gpu_device)
    assert bool(torch.isfinite(ops.sdf_grid_eval(x, sdf, 1.0)).all())                   # (the header is read here)
    nx = int(L.header(sdf.host)['dims'][0])
    sdf.buf[7:8].copy_(torch.tensor([nx - 1], dtype=torch.int32).view(torch.float32))   # dims[0] on the device
    out, pw = ops.sdf_grid_eval(x, sdf, 1.0, per_waypoint=True)
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(pw).all())
    out, grad = ops.sdf_grid_grad(x, sdf, 1.0)
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(grad).all())
    flag, gap = ops.sdf_grid_check(q, sdf, with_gap=True)
    assert bool(flag.all()) and bool(torch.isnan(gap).all())
    s = ops.sdf_grid_sample(q.contiguous(), sdf)
    assert bool(torch.isnan(s).all())
    bad = sdf.buf.cpu().numpy()
    with pytest.raises(_lib.MPBError, match='mpb_sdf_grid_check'):
        _lib.sdf_grid_check(bad)
    # announced, the address is read again: the corrupted header is refused by name
    _lib.check(_lib.lib().mpb_sdf_grid_invalidate(ops._ptr(sdf.buf)), 'mpb_sdf_grid_invalidate')
    with pytest.raises(_lib.MPBError, match='mpb_sdf_grid_eval'):
        ops.sdf_grid_eval(x, sdf, 1.0)


def test_a_buffer_evicted_from_the_header_table_is_read_again(gpu_device):
    """The library keeps the headers of 16 buffer addresses, replaced in turn.  Seventeen live buffers of the smallest grid
    mpb_sdf_grid_check takes (2 x 2 x 1 nodes under a planar point robot), each with node values -- so a cost -- of its own, evaluated
    once each at B = 1, H = 2: the seventeenth takes the first one's place, and the first, read again, gives the bits of its first
    evaluation."""
    from motion_planning_baselines_amd import geometry as G, ops
    robot = G.RobotPointMass(2)
    x = torch.tensor([[[0.25, 0.5], [0.75, 0.125]]], device=gpu_device)
    sdfs = [ops.DeviceSDFGrid(robot, G.GridSDFField(np.array([[0.01, 0.02], [0.03, 0.04]], np.float32) - 0.001 * i, (0.0, 0.0), 1.0, margin=0.05),
                              gpu_device) for i in range(17)]
    assert len({sdf.buf.data_ptr() for sdf in sdfs}) == 17 and sdfs[0].dims == (2, 2, 1)
    first = [ops.sdf_grid_eval(x, sdf, 2.0, h_begin=0, per_waypoint=True) for sdf in sdfs]
    assert len({float(out) for out, _ in first}) == 17 and all(bool((pw > 0).all()) for _, pw in first)
    out, pw = ops.sdf_grid_eval(x, sdfs[0], 2.0, h_begin=0, per_waypoint=True)
    assert torch.equal(out, first[0][0]) and torch.equal(pw, first[0][1])


# ------------------------------------------------------------------------------------------------
# built against supplied
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['panda', 'point2d'])
def test_grid_built_on_the_gpu_against_the_same_grid_supplied(gpu_device, name):
    """from_field on the GPU and the same lattice filled from the fp32 oracle give per-waypoint costs that differ by no more than the
    build bar (FACTOR * the fp32 restatement's worst node error) times the number of active spheres: s is a convex combination of nodes."""
    from motion_planning_baselines_amd import geometry as G, ops
    c = S.case(name)
    built = ops.DeviceSDFGrid(c.robot, c.layout, gpu_device)
    v32 = S.oracle_nodes(c.field, c.layout, S.F32)
    supplied = ops.DeviceSDFGrid(c.robot, G.GridSDFField(v32[0] if c.layout.planar else v32, c.layout.lo[:2] if c.layout.planar else c.layout.lo,
                                                         c.layout.cell, margin=c.layout.margin), gpu_device)
    e_nodes = float((torch.from_numpy(v32).double() - torch.from_numpy(c.grid.values).double()).abs().max())       # fp32 oracle against fp64 oracle, both rounded
    build_bar = S.FACTOR * e_nodes
    node_diff = float((built.nodes.cpu().double() - torch.from_numpy(v32).double().reshape(built.nodes.shape)).abs().max())
    x = S.trajs(name, 64, c.robot.q_dim).to(gpu_device)
    _, pa = ops.sdf_grid_eval(x, built, 1.0, h_begin=0, per_waypoint=True)
    _, pb = ops.sdf_grid_eval(x, supplied, 1.0, h_begin=0, per_waypoint=True)
    n_active = S.reference(name, 64).cl.n_active.clamp_min(1).double()
    ratio = float(((pa.cpu().double() - pb.cpu().double()).abs() / n_active).max())
    print(f'{name}: nodes built vs fp32 oracle differ by {node_diff:.3e}; build bar {build_bar:.3e}; costs differ by {ratio:.3e} per active sphere')
    assert float(pa.max()) > 0 and ratio <= build_bar
