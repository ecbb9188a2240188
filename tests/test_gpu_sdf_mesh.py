"""The SDF grid from triangle meshes on the GPU (mpb_sdf_grid_build_mesh) against the definition restated in tests/sdf_mesh_checks.py.
A: every node against the fp64 restatement, bar(E32) from the fp32 restatement's own error, the sign at every node off the exclusions;
B: culled and exhaustive builds as BITS; C: poses, the union flag, unsigned meshes, refusals; D: the layers above the kernel --
update_mesh, CHOMP and PlanningTask on a mesh torus."""
import functools

import numpy as np
import pytest
import torch

import sdf_grid_checks as S
import sdf_mesh_checks as K
from collision_kinks import CAP, DELTA, bar

pytestmark = pytest.mark.gpu

# grids, none a multiple of the wave's block of 4 x 4 x 4 (planar 8 x 8) nodes: (dims, lo, cell)
GRIDS = {'21x17x13': ((21, 17, 13), (-0.83, -0.66, -0.47), 0.08), '2x2x2': ((2, 2, 2), (-0.2, -0.1, -0.15), 0.3),
         '5x4x1': ((5, 4, 1), (-0.57, -0.43), 0.25), '9x130x3': ((9, 130, 3), (-0.05, -0.78, -0.01), 0.012)}
# one group, a full group, a padded second group (unsigned and signed), many groups; the other generators on the odd grids
CASES = [('box12', '21x17x13'), ('torus64', '21x17x13'), ('open65', '21x17x13'), ('ico80', '21x17x13'), ('ico1280', '21x17x13'), ('lprism20', '2x2x2'),
         ('twoboxes24', '5x4x1'), ('ico80', '9x130x3'), ('lprism20', '9x130x3'), ('torus64', '5x4x1')]


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    assert a.dtype == np.float32
    return np.ascontiguousarray(a).view(np.int32)


def _field(items, grid, margin=0.05):
    from motion_planning_baselines_amd import geometry as G
    dims, lo, cell = GRIDS[grid]
    hi = [lo[a] + (dims[a] - 1) * cell - 1e-6 for a in range(len(lo))]
    f = G.GridSDFField.from_mesh(items, lo, hi, cell, margin=margin, planar=dims[2] == 1)
    assert f.dims == dims and f.values is None
    return f


def _grid(items, grid, dev):
    """a TriangleMesh or a list of (TriangleMesh, pose) -> DeviceSDFGrid under a point robot"""
    from motion_planning_baselines_amd import geometry as G, ops
    f = _field(items, grid)
    return ops.DeviceSDFGrid(G.RobotPointMass(2 if f.planar else 3), f, dev)


def _hold(name, grid, got, pose=None, what=''):
    """every node of `got` (nz, ny, nx) against the restatement: the value within bar(E32), the sign off the exclusions"""
    dims, lo, cell = GRIDS[grid]
    ref = K.reference(name, dims, lo, cell, pose)
    v = got.detach().cpu().numpy().reshape(-1).astype(np.float64)
    e = float(np.abs(v - ref.r64.v).max()) / ref.scale
    ex = K.excluded(ref.r64, DELTA) if K.mesh(name).signed else np.abs(ref.r64.v) <= DELTA      # (an unsigned mesh takes no sign from a normal)
    wrong = int(((v < 0) != (ref.r64.v < 0))[~ex].sum())
    print(f'{name} on {grid}{what}: kernel error {e:.3e}, E32 {ref.E32:.3e}, bar {bar(ref.E32):.3e} (units of {ref.scale:.2f}); '
          f'{int(ex.sum())} of {v.size} nodes excluded from the sign, {wrong} signs differ, {int((ref.r64.v < 0).sum())} inside')
    assert e <= bar(ref.E32)
    assert wrong == 0 and float(ex.mean()) <= CAP
    return ref


# ------------------------------------------------------------------------------------------------
# A. node values
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,grid', CASES)
def test_every_node_against_the_fp64_restatement(gpu_device, name, grid):
    sdf = _grid(K.mesh(name), grid, gpu_device)
    dims = GRIDS[grid][0]
    assert sdf.dims == dims and sdf.nodes.shape == dims[::-1] and bool(torch.isfinite(sdf.nodes).all())
    ref = _hold(name, grid, sdf.nodes)
    if K.mesh(name).signed and grid == '21x17x13':
        assert int((ref.r64.v < 0).sum()) > 10                       # the grid does reach inside


# ------------------------------------------------------------------------------------------------
# B. culling is exact
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,grid', CASES + [('far', '21x17x13'), ('enclosing', '21x17x13'), ('far', '5x4x1'), ('enclosing', '2x2x2'), ('patch', '21x17x13')])
def test_culled_and_exhaustive_builds_have_the_same_bits(gpu_device, name, grid):
    from motion_planning_baselines_amd import ops
    sdf = _grid(K.mesh(name), grid, gpu_device)
    culled = sdf.nodes.clone()
    sdf.nodes.fill_(float('nan'))
    full = ops.sdf_grid_build_mesh(sdf.meshes[0], sdf, cull=False)
    assert full.data_ptr() == sdf.nodes.data_ptr() and bool(torch.isfinite(full).all())
    assert torch.equal(culled.view(torch.int32), full.view(torch.int32))
    sdf.nodes.fill_(float('nan'))
    assert torch.equal(ops.sdf_grid_build_mesh(sdf.meshes[0], sdf).view(torch.int32), culled.view(torch.int32))       # a second call: the same bits
    if name == 'far':
        assert float(culled.min()) > 5.0
    if name == 'enclosing':
        assert float(culled.max()) < -5.0


# ------------------------------------------------------------------------------------------------
# C. pose, union, unsigned, refusals
# ------------------------------------------------------------------------------------------------
POSE = K.pose_of((1.0, -2.0, 0.5), 0.7, (0.11, -0.07, 0.05))


def test_a_null_pose_and_an_identity_pose_give_the_same_bits(gpu_device):
    from motion_planning_baselines_amd import ops
    sdf = _grid(K.mesh('lprism20'), '21x17x13', gpu_device)
    none = sdf.nodes.clone()
    eye = ops.sdf_grid_build_mesh(sdf.meshes[0], sdf, pose=np.eye(4)[:3])
    assert torch.equal(none.view(torch.int32), eye.view(torch.int32))
    assert torch.equal(sdf.update_mesh(np.eye(4)).view(torch.int32), none.view(torch.int32))


@pytest.mark.parametrize('name', ['lprism20', 'ico80'])
def test_a_posed_mesh_matches_the_restatement_and_the_transformed_mesh(gpu_device, name):
    from motion_planning_baselines_amd import geometry as G, ops
    grid = '21x17x13'
    posed = _grid([(K.mesh(name), POSE)], grid, gpu_device)
    ref = _hold(name, grid, posed.nodes, pose=np.asarray(POSE, np.float32), what=' under a pose')
    moved = _grid(K.mesh(name).transformed(np.asarray(POSE, np.float32)), grid, gpu_device)
    d = float((posed.nodes - moved.nodes).abs().max()) / ref.scale
    print(f'{name}: posed build against the build of the host-transformed mesh {d:.3e}, bar {bar(ref.E32):.3e}')
    assert d <= bar(ref.E32)
    with pytest.raises(ValueError, match='orthonormal'):
        ops.sdf_grid_build_mesh(posed.meshes[0], posed, pose=np.asarray(POSE) * 1.01)


def test_union_flag_is_the_elementwise_minimum(gpu_device):
    from motion_planning_baselines_amd import geometry as G, ops
    grid = '21x17x13'
    b1 = G.TriangleMesh(*K.box((-0.5, -0.4, -0.3), (-0.1, 0.0, 0.1)))
    b2 = G.TriangleMesh(*K.box((0.15, 0.1, -0.1), (0.5, 0.45, 0.3)))
    one, two = _grid(b1, grid, gpu_device).nodes, _grid([(b2, POSE)], grid, gpu_device).nodes
    both = _grid([(b1, None), (b2, POSE)], grid, gpu_device)
    want = torch.minimum(one, two)
    assert torch.equal(both.nodes.view(torch.int32), want.view(torch.int32)) and not torch.equal(want, one) and not torch.equal(want, two)
    # a mesh on top of a from_field build
    field = G.env_spheres_3d()
    dims, lo, cell = GRIDS[grid]
    by_field = ops.DeviceSDFGrid(G.RobotPointMass(3), G.GridSDFField.from_field(field, lo, [lo[a] + (dims[a] - 1) * cell - 1e-6 for a in range(3)], cell), gpu_device)
    assert by_field.dims == dims
    base = by_field.nodes.clone()
    mesh = ops.DeviceMesh(b1, gpu_device)
    got = ops.sdf_grid_build_mesh(mesh, by_field, combine=True)
    assert torch.equal(got.view(torch.int32), torch.minimum(base, one).view(torch.int32)) and not torch.equal(got, base)


def test_unsigned_mesh_is_distance_minus_thickness(gpu_device):
    from motion_planning_baselines_amd import geometry as G
    with pytest.raises(ValueError, match='closed'):
        G.TriangleMesh(*K.torus_patch(16, 8, drop=16, **K.TORUS))     # the same triangles as a signed mesh: open
    sdf = _grid(K.mesh('patch'), '21x17x13', gpu_device)              # never refused for being open
    ref = _hold('patch', '21x17x13', sdf.nodes)
    thick = np.float32(K.mesh('patch').thickness)
    want = np.sqrt(ref.r64.d2) - float(thick)
    assert float(np.abs(ref.r64.v - want).max()) == 0.0 and float(sdf.nodes.min()) >= -float(thick)
    assert float(sdf.nodes.min()) < 0.02                             # some node lies close to the surface


def test_op_refuses_what_it_cannot_take(gpu_device):
    from motion_planning_baselines_amd import _lib, geometry as G, ops
    sdf = _grid(K.mesh('ico80'), '21x17x13', gpu_device)
    mesh = sdf.meshes[0]
    built = sdf.nodes.clone()
    on_cpu = ops.DeviceMesh(K.mesh('ico80'), 'cpu')
    with pytest.raises(ValueError, match='must live on the GPU'):
        ops.sdf_grid_build_mesh(on_cpu, sdf)
    import ctypes
    h, ptr = _lib.lib(), lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)
    with torch.cuda.device(gpu_device):                              # the C entry point itself: the wrapper forms its flags from two bools
        assert h.mpb_sdf_grid_build_mesh(ptr(mesh.buf), None, ptr(sdf.buf), 8, stream) == 1 and 'unknown flag bits 0x8' in h.mpb_last_error().decode()
        assert h.mpb_sdf_grid_build_mesh(ptr(mesh.buf), None, ptr(sdf.buf), 3, stream) == 0       # both known flags together
    assert torch.equal(sdf.nodes.view(torch.int32), built.view(torch.int32))                     # (min with itself, exhaustively)
    with pytest.raises(TypeError):
        ops.sdf_grid_build_mesh(sdf, sdf)
    with pytest.raises(ValueError, match='update_mesh'):
        ops.DeviceSDFGrid(G.RobotPointMass(3), G.GridSDFField(np.zeros((3, 3, 3), np.float32), (0, 0, 0), 0.1), gpu_device).update_mesh([None])
    with pytest.raises(ValueError, match='2 poses for 1 objects'):
        sdf.update_mesh([None, None])
    # the header overwritten after the first call: the launch is sized by what was read then, the kernel sees the difference, nothing is written
    keep = mesh.buf[:16].clone()
    sdf.nodes.fill_(7.0)
    mesh.buf.view(torch.int32)[2:4] = torch.tensor([64, 1], dtype=torch.int32, device=gpu_device)         # n_tri, n_groups of another mesh
    ops.sdf_grid_build_mesh(mesh, sdf)
    assert bool((sdf.nodes == 7.0).all())
    mesh.buf[:16] = keep
    assert torch.equal(ops.sdf_grid_build_mesh(mesh, sdf).view(torch.int32), built.view(torch.int32))


# ------------------------------------------------------------------------------------------------
# D. layers
# ------------------------------------------------------------------------------------------------
def test_update_mesh_rebuilds_in_place_and_the_cost_follows(gpu_device):
    """Pose 1, then pose 2 through update_mesh: the nodes are those of a fresh build under pose 2, ops.sdf_grid_eval on Panda trajectories
    equals, bit for bit, the same call on a GridSDFField holding those nodes, and nothing but the node section changes."""
    from motion_planning_baselines_amd import geometry as G, ops
    robot = G.RobotPanda(dt=0.04)
    lo, hi, cell = (-1.2, -1.0, -0.3), (1.2, 1.0, 1.0), 0.06
    mesh = G.TriangleMesh(*K.icosphere(1, 0.3))
    p1, p2 = K.pose_of((0, 0, 1), 0.3, (0.5, 0.1, 0.5)), K.pose_of((1, 1, 0), 1.1, (0.35, -0.2, 0.6))
    sdf = ops.DeviceSDFGrid(robot, G.GridSDFField.from_mesh(mesh, lo, hi, cell, margin=0.03, pose=p1), gpu_device)
    x = S.trajs('panda', 8, robot.q_dim).to(gpu_device)
    c1 = ops.sdf_grid_eval(x, sdf, 2.5)
    nodes1 = sdf.nodes.clone()
    ptr, header, mesh_ptr, mesh_words = sdf.buf.data_ptr(), sdf.buf[:32].clone(), sdf.meshes[0].buf.data_ptr(), sdf.meshes[0].buf.clone()
    nodes = sdf.update_mesh([p2])
    assert nodes.data_ptr() == sdf.nodes.data_ptr() and sdf.buf.data_ptr() == ptr and torch.equal(sdf.buf[:32], header)
    assert sdf.meshes[0].buf.data_ptr() == mesh_ptr and torch.equal(sdf.meshes[0].buf.view(torch.int32), mesh_words.view(torch.int32))
    fresh = ops.DeviceSDFGrid(robot, G.GridSDFField.from_mesh(mesh, lo, hi, cell, margin=0.03, pose=p2), gpu_device)
    assert torch.equal(nodes.view(torch.int32), fresh.nodes.view(torch.int32)) and not torch.equal(nodes, nodes1)
    c2, pw2 = ops.sdf_grid_eval(x, sdf, 2.5, per_waypoint=True)
    by_values = ops.DeviceSDFGrid(robot, G.GridSDFField(nodes.cpu().numpy(), lo, cell, margin=0.03), gpu_device)
    cf, pwf = ops.sdf_grid_eval(x, by_values, 2.5, per_waypoint=True)
    assert torch.equal(c2, cf) and torch.equal(pw2, pwf) and float(c2.max()) > 0 and not torch.equal(c1, c2)
    # the field now stands for pose 2; update_occupancy on a mesh-sourced field leaves its source alone
    assert np.array_equal(sdf.field.source[0][1], np.asarray(p2, np.float32)) and sdf.field.source[0][0] is mesh
    assert torch.equal(ops.DeviceSDFGrid(robot, sdf.field, gpu_device).nodes.view(torch.int32), fresh.nodes.view(torch.int32))
    source = sdf.field.source
    sdf.update_occupancy(np.zeros(sdf.dims[::-1], np.uint8))
    assert sdf.field.source is source
    assert torch.equal(sdf.update_mesh(p1).view(torch.int32), nodes1.view(torch.int32))         # and back, a single pose for the one object
    assert torch.equal(ops.sdf_grid_eval(x, sdf, 2.5), c1)


TORUS = dict(lo=(-0.9, -0.9, -0.4), hi=(0.89, 0.89, 1.39), cell=0.06, margin=0.05)
TORUS_POSE = K.pose_of((1, 0, 0), np.pi / 2, (0.55, 0.0, 0.55))    # the axis along y, clear of a robot base at the origin


@functools.lru_cache(maxsize=None)
def _torus_mesh():
    from motion_planning_baselines_amd import geometry as G
    return G.TriangleMesh(*K.torus(12, 8, R=0.25, r=0.08))


def _torus_field():
    from motion_planning_baselines_amd import geometry as G
    f = G.GridSDFField.from_mesh(_torus_mesh(), TORUS['lo'], TORUS['hi'], TORUS['cell'], margin=TORUS['margin'], pose=TORUS_POSE)
    assert f.dims == (31, 31, 31)
    return f


def _grid_data(robot, values, field):
    return (S.ref_robot(robot, S.F64), S.grid_data(values, field.lo, field.cell, field.inv_cell, S.F64), S.thresholds(robot, np.float32(field.margin), S.F64))


def test_chomp_on_a_mesh_torus_equals_the_planner_on_the_builders_nodes(gpu_device):
    """CHOMP on the planned device path with CostCollision(field=GridSDFField.from_mesh(torus)), 3 iterations at B = 4, H = 16, against
    the same planner over GridSDFField(values=<the nodes the builder produced, read back>): bit for bit.  At least two start waypoints
    are in contact, and the grid member moves the result."""
    from motion_planning_baselines_amd import geometry as G, ops
    from motion_planning_baselines_amd.planners.chomp import CHOMP
    from motion_planning_baselines_amd.planners.costs import cost_functions as C
    dev = gpu_device
    B, H = 4, 16
    robot = G.RobotPanda(dt=0.04)
    D = robot.q_dim
    ta = dict(device=dev, dtype=torch.float32)
    by_mesh = _torus_field()
    values = ops.DeviceSDFGrid(robot, by_mesh, dev).nodes.cpu().numpy()
    assert float(values.min()) < -0.03 and float(values.max()) > 0.5
    by_values = G.GridSDFField(values, TORUS['lo'], TORUS['cell'], margin=TORUS['margin'])
    rr, g64, thr = _grid_data(robot, values, by_values)
    t = torch.linspace(0, 1, H).reshape(1, H, 1)
    for seed in range(200):                                  # straight lines between uniform configurations: the first seed with contact
        qa, qb = S.uniform_q(robot, B, seed=100 + seed), S.uniform_q(robot, B, seed=300 + seed)
        x0 = (qa[:, None] * (1 - t) + qb[:, None] * t).contiguous()
        cl = S.classify(rr, g64, thr, x0.double())
        if int(cl.contact[:, 1:-1].sum()) >= 2 and bool(cl.inside.all()):
            break
    n_contact = int(cl.contact[:, 1:].sum())
    print(f'seed {seed}: {n_contact} of {B * (H - 1)} start waypoints in contact with the torus')
    assert n_contact >= 2

    def planner(field, w_grid=1.0):
        cg = C.CostCollision(robot, H, field=field, sigma_coll=0.2, tensor_args=ta)
        sm = C.CostSmoothnessCHOMP(robot, H, tensor_args=ta)
        comp = C.CostComposite(robot, H, [cg, sm], weights_cost_l=[w_grid, 1e-7], tensor_args=ta)
        plan = C.device_plan(comp, dev)
        assert plan is not None and plan[0] is None and plan.own == [(cg, w_grid)]
        return CHOMP(n_dof=D, n_support_points=H, num_particles_per_goal=B, opt_iters=1, dt=robot.dt, start_state=x0[0, 0].to(dev), cost=comp,
                     weight_prior_cost=1e-8, initial_particle_means=x0.to(dev), step_size=1e-4, grad_clip=1e4, pos_only=True, tensor_args=ta)
    pl, ref, off = planner(by_mesh), planner(by_values), planner(by_values, w_grid=0.0)
    for it in range(3):
        pl.optimize()
        ref.optimize()
        off.optimize()
        assert torch.equal(pl._particle_means, ref._particle_means), it
    assert bool(torch.isfinite(pl._particle_means).all())
    assert float((pl._particle_means - off._particle_means).abs().max()) > 1e-4          # the member acts


def test_planning_task_samples_free_of_the_mesh_torus(gpu_device):
    from motion_planning_baselines_amd import geometry as G, ops
    from motion_planning_baselines_amd.robot_field import PlanningTask
    robot = G.RobotPanda(dt=0.04)
    ta = dict(device=gpu_device, dtype=torch.float32)
    by_mesh = _torus_field()
    task = PlanningTask(robot, G.env_spheres_3d(), sdf_field=by_mesh, tensor_args=ta)
    q = S.uniform_q(robot, 512).to(gpu_device)
    by_grid = ops.sdf_grid_check(q, task.sdf_geom)
    assert 0 < int(by_grid.sum()) < 512 and torch.equal(task.compute_collision(q), ops.collision_check(q, task.geom) | by_grid)
    free = task.random_coll_free_q(16)
    assert free.shape == (16, robot.q_dim)
    # the fp64 restatement of the whole grid (29 791 nodes x 192 triangles), its nodes as the oracle's grid
    nodes = K.node_positions(by_mesh.dims, TORUS['lo'], TORUS['cell'], np.asarray(TORUS_POSE, np.float32))
    r64 = K.restate(G.pack_mesh(_torus_mesh()), nodes, np.float64)
    e = float(np.abs(task.sdf_geom.nodes.cpu().numpy().reshape(-1).astype(np.float64) - r64.v).max())
    rr, g64, thr = _grid_data(robot, r64.v.astype(np.float32).reshape(by_mesh.dims[::-1]), by_mesh)
    cl = S.classify(rr, g64, thr, free.cpu().double())
    print(f'built nodes against the fp64 restatement {e:.3e}; largest hinge of the 16 free configurations on the restatement\'s nodes: '
          f'{float(cl.hinge.max()):.3e} (slack {S.DELTA:.0e})')
    assert float(cl.hinge.max()) <= S.DELTA
