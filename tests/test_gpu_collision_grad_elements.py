"""GPU: EVERY element of the analytic collision gradient against the fp64 oracle, off the kinks.

The fraction-style gradient tests (diff > 2e-4 max|g| + 2e-4 |g| for up to 0.3 % of the elements) let a small class of wrong
elements, a small error everywhere, and unnamed exclusions through.  Here tests/collision_kinks.py decides from the fp64
oracle ALONE which waypoints sit on a kink of the hinge cost; on every other waypoint, none left out,

    e = max_j |g_kernel - g_fp64| / (k_sigma * weight) / sum_f s_f max(1, n_active_f)   <=   4 * max(E32, 2^-23)

with E32 the same quantity for the fp32 oracle's autograd (its maximum over the case's conditioned waypoints, computed
here).  The factor 4: the kernels' sincos is up to ~2 ulp where torch's is at most 1, v_sqrt is 1 ulp, the fma association
differs -- and a factor two above that.  The floor is one fp32 ulp of a unit direction.  At excluded waypoints the gradient
must be finite; velocity channels and rows below h_begin exactly 0.  Each case prints how many waypoints it judged, the
excluded share (capped at 3 % of those in contact) and its worst e against E32.

One case per gradient walker of csrc/mpb_geom.h (point_cost<true>, spheres_nearest_grid<1>, waypoint_cost<true>,
waypoint_cost_grid_grad, waypoint_cost_grid_grad_model<PandaModel>), asserted from the packed header and geom_flags, plus
points_cost_kernel<true>, fk_points_vjp_kernel, the GPMP2 linearisation's rows and the tie conventions the kernel comments
write down ("first on ties, as torch.max", lowest obstacle index wins, a sphere's centre gives zero)."""
import numpy as np
import pytest
import torch

import collision_kinks as K

pytestmark = pytest.mark.gpu
K_SIGMA, WEIGHT = 4.0, 1.5


# ------------------------------------------------------------------------------------------------
# which walker a geometry buffer gets (the choices of collision_cost_kernel<true> / gpmp2_linearize_kernel, read from the
# header words and geom_flags alone)
# ------------------------------------------------------------------------------------------------
def _grid_usable(h):
    from motion_planning_baselines_amd import geometry as G
    return int(h['version']) == G.GEOM_VERSION and 0 < int(h['n_cells']) <= G.GRID_MAX_CELLS and int(h['n_sph']) <= G.GRID_MAX_SPH


def walkers(geom):
    from motion_planning_baselines_amd import geometry as G
    from motion_planning_baselines_amd.model_gen import MODEL_IDS
    model = (geom.flags & G.GEOM_FLAG_MODEL_MASK) == MODEL_IDS['panda'] and bool(geom.flags & G.GEOM_FLAG_ALL_GRIDS)
    out = []
    for h in G.fields(geom.host):
        point = int(h['kind']) == G.KIND_POINT
        ug = _grid_usable(h) and (not point or int(h['n_sph']) > 48)
        if model:
            assert ug and int(h['model']) == MODEL_IDS['panda']
            out.append('grid_model')
        elif ug:
            out.append('grid_point' if point else 'grid_table')
        else:
            out.append('point_cost' if point else 'exhaustive')
    return out


def spheres_in_overflowing_cells(geom, pos):
    """How many of the positions (..., 3) fall into a cell of the (first field's) compact grid that lists more than GRID_SLOTS
    obstacles: there the grid walkers test every obstacle."""
    from motion_planning_baselines_amd import geometry as G
    h = G.header(geom.host)
    dims, lo, inv = np.asarray(h['grid_dims']), np.asarray(h['grid_lo'], np.float64), np.asarray(h['grid_inv'], np.float64)
    cell = np.floor((pos.reshape(-1, 3).numpy() - lo) * inv).astype(np.int64)
    inside = ((cell >= 0) & (cell < dims)).all(-1)
    lin = cell[inside, 0] + dims[0] * (cell[inside, 1] + dims[1] * cell[inside, 2])
    words = geom.host.view(np.uint32)[int(h['off_grid']):int(h['off_grid']) + int(h['n_cells'])]
    return int((words[lin] == G.GRID_OVERFLOW).sum())


def make_geom(ref, dev, **kw):
    from motion_planning_baselines_amd import ops
    if len(ref.fields) == 1:
        return ops.DeviceGeometry(ref.robot, ref.fields[0], dev, **kw)
    return ops.DeviceGeometry(ref.robot, ref.fields, dev, scales=ref.scales, **kw)


def report(tag, cl_cond, n_contact, share, worst, E32):
    print(f'{tag}: judged {int(cl_cond.sum())} of {cl_cond.numel()} waypoints ({n_contact} in contact, {share * 100:.2f} % of them '
          f'excluded), worst e {worst:.3e} against E32 {E32:.3e} (bar {K.bar(E32):.3e})')


# ------------------------------------------------------------------------------------------------
# 3.1  forward kinematics and its VJP: no kinks, every element judged
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['panda_s3d', 'arm5', 'arm12'])
@pytest.mark.parametrize('angles', ['limits', 'pm20'])
def test_fk_points_and_vjp(gpu_device, name, angles):
    from motion_planning_baselines_amd import ops
    ref = K.reference(name, 64)
    D = ref.robot.q_dim
    gen = torch.Generator().manual_seed(11)
    if angles == 'limits':
        q = K.trajs(name, 37, D)
    else:                       # the range fast_sincos documents (csrc/mpb_geom.h)
        q = (40.0 * torch.rand(K.B, 37, D, generator=gen) - 20.0).contiguous()
    geom = make_geom(ref, gpu_device, keep_all_links=True)
    L = geom.n_links
    pts = ops.fk_collision_points(q.to(gpu_device), geom).cpu()
    q64 = q.double().requires_grad_(True)
    q32 = q.clone().requires_grad_(True)
    p64, p32 = ref.rr64.fk_map_collision(q64), ref.rr32.fk_map_collision(q32)
    assert pts.shape == p64.shape == (K.B, 37, L, 3)
    reach = float(p64.detach().norm(dim=-1).max())
    E32 = float((p32.detach().double() - p64.detach()).abs().max())
    err = float((pts.double() - p64.detach()).abs().max())
    print(f'fk {name} {angles}: position error {err:.3e} against E32_pos {E32:.3e}, reach {reach:.2f} m')
    assert err <= K.FACTOR * max(E32, K.ULP * reach)
    if angles == 'limits':
        assert err <= K.DELTA / 4
    # J^T g with unit-norm cotangents per collision sphere, normalised by the number of spheres
    cot = torch.randn(K.B, 37, L, 3, generator=gen)
    cot = (cot / cot.norm(dim=-1, keepdim=True)).contiguous()
    gq = ops.fk_collision_points_vjp(q.to(gpu_device), geom, cot.to(gpu_device)).cpu()
    g64, = torch.autograd.grad((p64 * cot.double()).sum(), q64)
    g32, = torch.autograd.grad((p32 * cot).sum(), q32)
    E32 = float((g32.double() - g64).abs().max()) / L
    e = float((gq.double() - g64).abs().max()) / L
    print(f'fk vjp {name} {angles}: worst e {e:.3e} against E32 {E32:.3e}')
    assert gq.shape == (K.B, 37, D) and e <= K.bar(E32)


# ------------------------------------------------------------------------------------------------
# 3.2  the field's direction per collision sphere, at given fp32 points (no FK error enters)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,grid', [('panda_s3d', True), ('panda_boxes_only', False), ('panda_many', False)])
def test_field_direction_per_sphere(gpu_device, name, grid):
    from motion_planning_baselines_amd import geometry as G, ops
    ref = K.reference(name, 64)
    geom = make_geom(ref, gpu_device, keep_all_links=True)
    assert _grid_usable(G.header(geom.host)) == grid                 # points_cost_kernel: grid walk / exhaustive branch
    pts = ref.rr32.fk_map_collision(ref.q).contiguous()             # some fp32 points near the obstacles; classified AT these values
    cl = K.classify_points(ref.rf64[0], pts.double())
    gout = (0.5 + torch.rand(K.B, 64, generator=torch.Generator().manual_seed(5))).contiguous()
    gp = ops.field_cost_points_vjp(pts.to(gpu_device), geom, gout.to(gpu_device)).cpu()
    want = -cl.direction * cl.active.unsqueeze(-1)                  # d cost / d x_l = -grad sd_min where the hinge is active
    x32 = pts.clone().requires_grad_(True)
    g32, = torch.autograd.grad(ref.rf32[0].compute_cost(None, x32).sum(), x32)
    cond = cl.conditioned
    n, nc, share = K.excluded_share(types_ns(cl))
    E32 = float((g32.double() - want).abs()[cond].max())
    got = gp.double() / gout.double()[..., None, None]
    worst = float((got - want).abs()[cond].max())
    report(f'field direction {name}', cond, n, share, worst, E32)
    assert torch.isfinite(gp).all()
    assert share <= K.CAP and nc >= 100
    assert worst <= K.bar(E32)
    inactive = cond.unsqueeze(-1) & ~cl.active
    assert int(inactive.sum()) > 0 and bool((gp[inactive] == 0).all())


def types_ns(cl):
    """A one-field classification in the shape excluded_share() reads (n_active with a field axis)."""
    import types
    return types.SimpleNamespace(n_active=cl.n_active.unsqueeze(-1), conditioned=cl.conditioned)


# ------------------------------------------------------------------------------------------------
# 3.3  ops.cost_collision_grad, one case per walker
# ------------------------------------------------------------------------------------------------
GRAD_CASES = [
    # scene, DeviceGeometry arguments, H, d / D, h_begin, walker per field
    ('point2d_dense', {}, 64, 2, 1, ['point_cost']),
    ('point3d', {}, 150, 1, 0, ['point_cost']),                          # 16 spheres; the lane loop wraps twice
    ('point3d_56', {}, 64, 1, 1, ['grid_point']),
    ('point2d_56', {}, 37, 2, 0, ['grid_point']),
    ('panda_s3d', {}, 64, 2, 1, ['grid_model']),
    ('panda_s3d', dict(use_model=False), 37, 1, 0, ['grid_table']),
    ('panda_s3d', dict(keep_all_links=True), 150, 1, 1, ['grid_model']),
    ('panda_s3d', dict(use_model=False, keep_all_links=True), 64, 2, 0, ['grid_table']),
    ('panda_crowded', {}, 64, 2, 1, ['grid_model']),                     # overflowing cells
    ('panda_crowded', dict(use_model=False), 64, 1, 0, ['grid_table']),
    ('panda_boxes', {}, 64, 1, 1, ['grid_model']),                       # the grid walk's box loop
    ('panda_many', {}, 37, 1, 1, ['exhaustive']),
    ('panda_boxes_only', {}, 150, 2, 0, ['exhaustive']),
    ('panda_sb', {}, 64, 1, 1, ['exhaustive']),
    ('arm1', {}, 64, 2, 1, ['grid_table']),
    ('arm5', {}, 37, 1, 0, ['grid_table']),
    ('arm12', {}, 64, 2, 1, ['grid_table']),
    ('panda_two_fields', {}, 64, 2, 1, ['grid_model', 'grid_model']),    # scales (0.5, 2.0)
    ('panda_two_fields', dict(use_model=False), 64, 1, 0, ['grid_table', 'grid_table']),
]


@pytest.mark.parametrize('name,kw,H,dmul,h_begin,walker', GRAD_CASES,
                         ids=[f'{c[0]}-{"-".join(c[1]) or "default"}-H{c[2]}-d{c[3]}D-hb{c[4]}' for c in GRAD_CASES])
def test_cost_collision_grad_every_element(gpu_device, name, kw, H, dmul, h_begin, walker):
    from motion_planning_baselines_amd import ops
    ref = K.reference(name, H)
    D = ref.robot.q_dim
    d = dmul * D
    x = K.trajs(name, H, d)
    assert torch.equal(x[..., :D], ref.q)
    geom = make_geom(ref, gpu_device, **kw)
    assert walkers(geom) == walker, walkers(geom)
    if name == 'panda_crowded':
        assert spheres_in_overflowing_cells(geom, ref.cl.pos.float().double()) > 100
    buf = torch.full((K.B, H, d), float('nan'), device=gpu_device)       # every element must be written
    _, grad = ops.cost_collision_grad(x.to(gpu_device), geom, K_SIGMA, weight=WEIGHT, h_begin=h_begin, grad=buf)
    g = grad.cpu()
    g64, e32 = ref.g64.clone(), ref.e32.clone()
    g64[:, :h_begin] = 0
    e32[:, :h_begin] = 0
    cond = ref.cl.conditioned
    n, nc, share = K.excluded_share(ref.cl)
    E32 = float(e32[cond].max())
    e = (g[..., :D].double() / (K_SIGMA * WEIGHT) - g64).abs().amax(-1) / ref.budget
    worst = float(e[cond].max())
    report(f'cost_collision_grad {name} {kw} H={H} d={d} h_begin={h_begin} {walker}', cond, n, share, worst, E32)
    assert torch.isfinite(g).all()
    assert bool((g[..., D:] == 0).all())                                 # velocity channels
    assert bool((g[:, :h_begin] == 0).all())                             # rows below h_begin
    assert share <= K.CAP and nc >= 100
    assert float(g64.abs().max()) > 0
    assert worst <= K.bar(E32), (worst, E32)


# ------------------------------------------------------------------------------------------------
# 3.4  ops.gpmp2_collision_rows
# ------------------------------------------------------------------------------------------------
ROW_CASES = [('panda_s3d', {}, 64), ('point2d_dense', {}, 64), ('arm5', {}, 37), ('panda_boxes_only', {}, 150),
             ('panda_two_fields', {}, 64), ('panda_two_fields', dict(use_model=False), 64)]


@pytest.mark.parametrize('name,kw,H', ROW_CASES, ids=[f'{c[0]}-{"-".join(c[1]) or "default"}-H{c[2]}' for c in ROW_CASES])
def test_gpmp2_rows_per_waypoint(gpu_device, name, kw, H):
    """n_interp = 0: per field h_t = -grad and c_t of the waypoint itself, times sqrt(s_f); row 0 takes no factor."""
    from motion_planning_baselines_amd import ops
    ref = K.reference(name, H)
    D = ref.robot.q_dim
    x = K.trajs(name, H, 2 * D)
    geom = make_geom(ref, gpu_device, **kw)
    jac = ops.gpmp2_collision_rows(x.to(gpu_device), geom, 0).cpu()
    assert jac.shape == (len(ref.fields), K.B, H, D + 1) and torch.isfinite(jac).all()
    assert bool((jac[:, :, 0] == 0).all())
    for f, s in enumerate(ref.scales):
        clf = ref.cl.fields[f]
        _, g64 = K.oracle_cost_grad(ref.rr64, [ref.rf64[f]], [1.0], ref.q.double())
        _, g32 = K.oracle_cost_grad(ref.rr32, [ref.rf32[f]], [1.0], ref.q)
        den = clf.n_active.clamp_min(1).double()
        cond = clf.conditioned.clone()
        cond[:, 0] = False
        n, nc, share = K.excluded_share(types_ns(clf))
        rows = jac[f].double() / float(np.sqrt(np.float32(s)))
        for what, got, w64, w32 in (('h', rows[..., :D], -g64, -g32.double()),
                                    ('c', rows[..., D:], ref.c64[f].unsqueeze(-1), ref.c32[f].double().unsqueeze(-1))):
            E32 = float(((w32 - w64).abs().amax(-1) / den)[cond].max())
            worst = float(((got - w64).abs().amax(-1) / den)[cond].max())
            report(f'gpmp2 rows {name} {kw} H={H} field {f} {what}', cond, n, share, worst, E32)
            assert worst <= K.bar(E32), (what, f, worst, E32)
        assert share <= K.CAP and nc >= 100


@pytest.mark.parametrize('name', ['panda_s3d', 'point2d_dense', 'panda_boxes_only'])
def test_gpmp2_rows_with_interpolation(gpu_device, name):
    """n_interp = 2 at H = 16: the row of support point t carries the gradients of the interpolated waypoints of its two
    segments.  A row is judged when every interpolated waypoint that flows into it is conditioned."""
    from motion_planning_baselines_amd import ops
    from oracle import planners_ref as O
    H, n_interp = 16, 2
    ref = K.reference(name, 64)                                          # (geometry objects only)
    D = ref.robot.q_dim
    x = K.trajs(name, H, 2 * D)
    geom = make_geom(ref, gpu_device)
    jac = ops.gpmp2_collision_rows(x.to(gpu_device), geom, n_interp).cpu()
    h64, c64 = O.gpmp2_collision_rows(x.double(), ref.rr64, ref.rf64, D, n_interp=n_interp)
    h32, c32 = O.gpmp2_collision_rows(x, ref.rr32, ref.rf32, D, n_interp=n_interp)
    # which interpolated waypoints flow into which support row: interpolate the identity
    W = O.interpolate_trajs(torch.eye(H, dtype=torch.float64).unsqueeze(0), n_interp)[0]      # (Hi, H)
    flows = W != 0
    flows[0] = False                                                      # the interpolated trajectory's row 0 takes no factor
    assert W.shape == ((H - 1) * (n_interp + 1) + 1, H) and int(flows[:, 1:-1].sum(0).min()) == 2 * n_interp + 1
    cl = K.classify(ref.rr64, ref.rf64, O.interpolate_trajs(x.double(), n_interp)[..., :D])
    fl = flows.double()
    n_act = (cl.n_active[..., 0].double() @ fl)[:, 1:]                    # (B, H-1): active spheres that flow into the row
    bad = ((~cl.conditioned).double() @ fl)[:, 1:]
    judged, contact = bad == 0, n_act > 0
    den = n_act.clamp_min(1)
    E32 = float(((h32[0].double() - h64[0]).abs().amax(-1) / den)[judged].max())
    worst = float(((jac[0, :, 1:, :D].double() - h64[0]).abs().amax(-1) / den)[judged].max())
    share = 1.0 - float((judged & contact).sum()) / float(contact.sum())
    print(f'gpmp2 rows n_interp=2 {name}: judged {int(judged.sum())} of {judged.numel()} rows ({int(contact.sum())} in contact, '
          f'{share * 100:.2f} % of them excluded), worst e {worst:.3e} against E32 {E32:.3e} (bar {K.bar(E32):.3e})')
    assert torch.isfinite(jac).all()
    assert int((judged & contact).sum()) * 2 >= int(contact.sum()) > 20
    assert worst <= K.bar(E32), (worst, E32)
    # c_t stays the support point's own cost
    own = cl.conditioned[:, ::n_interp + 1][:, 1:]
    den_c = cl.n_active[:, ::n_interp + 1, 0][:, 1:].clamp_min(1).double()
    E32c = float(((c32[0].double() - c64[0]).abs() / den_c)[own].max())
    worst_c = float(((jac[0, :, 1:, D].double() - c64[0]).abs() / den_c)[own].max())
    print(f'gpmp2 rows n_interp=2 {name}: c_t worst e {worst_c:.3e} against E32 {E32c:.3e}')
    assert worst_c <= K.bar(E32c) and float(jac[0, :, 0, D].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------
# 3.5  the written conventions, on exactly representable inputs, against the fp32 oracle's autograd
# ------------------------------------------------------------------------------------------------
def _fillers(n):
    """n small spheres on a lattice far from the origin: they make the obstacle count cross grid_usable_grad's n_sph > 48 and
    come after the obstacles under test in index order."""
    c = np.array([(x, y, z) for x in (1.5, 1.75, 2.0, 2.25) for y in (1.5, 1.75, 2.0, 2.25) for z in (1.5, 1.75, 2.0, 2.25)])[:n]
    return np.concatenate([c, np.full((n, 1), 0.0625)], 1)


CONVENTIONS = {
    # obstacle spheres, boxes, the query points, and d cost / d x written out where the convention decides it
    'sphere_centre': ([[0, 0, 0, 0.5]], None, [[0, 0, 0]], [[0, 0, 0]]),
    'box_inner_diagonal': (None, [[0, 0, 0, 0.5, 0.5, 0.5]],                      # ax == ay > az: the first axis; sign of p
                           [[0.25, 0.25, 0], [-0.25, 0.25, 0], [0, 0.25, 0.25], [0.125, -0.25, -0.25], [0.25, 0.25, 0.25]],
                           [[-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0], [-1, 0, 0]]),
    'two_spheres_lower_index': ([[-0.5, 0, 0, 0.25], [0.5, 0, 0, 0.25]], None, [[0, 0, 0], [0, 0.125, 0]], [[-1, 0, 0], None]),
    'two_spheres_lower_index_swapped': ([[0.5, 0, 0, 0.25], [-0.5, 0, 0, 0.25]], None, [[0, 0, 0], [0, 0.125, 0]], [[1, 0, 0], None]),
    'sphere_wins_against_box': ([[-0.5, 0, 0, 0.25]], [[0.75, 0, 0, 0.5, 0.5, 0.5]], [[0, 0, 0]], [[-1, 0, 0]]),
}


@pytest.mark.parametrize('grid', [False, True], ids=['point_cost', 'grid_point'])
@pytest.mark.parametrize('case', list(CONVENTIONS))
def test_written_conventions(gpu_device, case, grid):
    from motion_planning_baselines_amd import geometry as G, ops
    from oracle.geometry_ref import make_ref_geometry
    spheres, boxes, points, expect = CONVENTIONS[case]
    n_fill = 52 if grid else 0
    sph = np.concatenate([np.zeros((0, 4)) if spheres is None else np.asarray(spheres, np.float64), _fillers(n_fill)])
    robot = G.RobotPointMass(3, radius=0.25, q_limits=(-1.0, 1.0))
    field = G.CollisionField(spheres=sph.astype(np.float32) if len(sph) else None,
                             boxes=None if boxes is None else np.asarray(boxes, np.float32), margin=0.25)
    geom = ops.DeviceGeometry(robot, field, gpu_device)
    assert walkers(geom) == (['grid_point'] if grid else ['point_cost'])
    x = torch.tensor([points], dtype=torch.float32)                       # (1, P, 3)
    _, grad = ops.cost_collision_grad(x.to(gpu_device), geom, 1.0, weight=1.0, h_begin=0)
    g = grad.cpu()[0]
    rr, rf = make_ref_geometry(robot, field)
    xg = x.clone().requires_grad_(True)
    cost = rf.compute_cost(xg, rr.fk_map_collision(xg))
    want, = torch.autograd.grad(cost.sum(), xg)
    assert bool((cost > 0).all()) and torch.isfinite(g).all()
    print(f'{case} {"grid" if grid else "loop"}: kernel {g.tolist()} oracle {want[0].tolist()}')
    for p, e in enumerate(expect):
        if e is not None:               # decided by the convention alone: exact, on both sides
            assert g[p].tolist() == [float(v) for v in e], (case, p, g[p])
            assert want[0, p].tolist() == [float(v) for v in e], (case, p, want[0, p])
        else:                           # a generic direction on the chosen obstacle: to rounding
            assert float((g[p] - want[0, p]).abs().max()) <= K.FACTOR * K.ULP, (case, p, g[p], want[0, p])
            assert float(g[p, 0]) * float(want[0, p, 0]) > 0
