"""CPU: host-side logic of the product (no compute calls): the C-ABI library loads and exports every
symbol include/mpb.h declares, geometry packing round-trips through the library's validator, and the
planner constants match the reference's (golden) R / Sigma / scale_tril bit for bit."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, product_geometry_from_golden


def test_library_exports_every_declared_symbol():
    from motion_planning_baselines_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'mpb.h')).read()
    declared = set(re.findall(r'\b(mpb_[a-z0-9_]+)\s*\(', hdr))
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    h = _lib.lib()
    for name in declared:
        assert hasattr(h, name)
    assert (h.mpb_version() & 0xFFFF) == _lib.ABI_VERSION == int(re.search(r'#define MPB_ABI_VERSION (\d+)', hdr).group(1))
    # the product library exports the product ABI ONLY: the test aids live in a library of their own (include/mpb_debug.h)
    assert not [n for n in declared if n.startswith('mpb_debug')]
    import subprocess
    syms = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r' T (mpb_[a-z0-9_]+)$', syms, flags=re.M))
    assert exported == declared, exported ^ declared
    dhdr = open(os.path.join(ROOT, 'include', 'mpb_debug.h')).read()
    ddecl = set(re.findall(r'\b(mpb_[a-z0-9_]+)\s*\(', dhdr))
    assert ddecl == set(_lib.DEBUG_SIGNATURES), ddecl ^ set(_lib.DEBUG_SIGNATURES)
    dh = _lib.debug_lib()
    for name in ddecl:
        assert hasattr(dh, name)


def test_binding_refuses_a_library_of_another_abi_version(tmp_path, monkeypatch):
    """signatures change positionally between ABI versions -- a library that reports another MPB_ABI_VERSION (an
    old build_variants/*.so through MPB_LIB_PATH) must be refused at load time, not called with shifted arguments."""
    import subprocess
    from motion_planning_baselines_amd import _lib
    src = tmp_path / 'old.c'
    names = [n for n in _lib.SIGNATURES if n not in ('mpb_version', 'mpb_last_error')]
    src.write_text('int mpb_version(void) { return %d; }\nconst char *mpb_last_error(void) { return ""; }\n' % (_lib.ABI_VERSION - 1)
                   + ''.join('int %s(void) { return 0; }\n' % n for n in names))
    so = tmp_path / 'libold.so'
    subprocess.check_call(['gcc', '-shared', '-fPIC', str(src), '-o', str(so)])
    monkeypatch.setattr(_lib, 'LIB_PATH', str(so))
    monkeypatch.setattr(_lib, '_lib', None)
    with pytest.raises(_lib.MPBError, match='ABI version'):
        _lib.lib()


def test_geometry_pack_validates_and_rejects_corruption():
    from motion_planning_baselines_amd import _lib, geometry as G
    for robot, field in [(G.RobotPanda(), G.env_spheres_3d()), (G.RobotPointMass(2), G.env_dense_2d()),
                         (G.RobotPointMass(3), G.env_spheres_3d()), (G.RobotPointMass(2), G.env_grid_circles_2d())]:
        buf = G.pack_geometry(robot, field)
        _lib.geom_check(buf)
        bad = buf.copy()
        G.header(bad)['magic'] ^= 1
        with pytest.raises(_lib.MPBError):
            _lib.geom_check(bad)
        bad = buf.copy()
        G.header(bad)['total'] += 4
        with pytest.raises(_lib.MPBError):
            _lib.geom_check(bad)
        with pytest.raises(_lib.MPBError):
            _lib.geom_check(buf[:20])


def test_cull_table_is_conservative():
    """Every (link position, obstacle) pair within the hinge threshold must pass the cheap test."""
    from motion_planning_baselines_amd import geometry as G
    robot, field = G.RobotPanda(), G.env_spheres_3d()
    buf = G.pack_geometry(robot, field)
    h = G.header(buf)
    n_sph = h['n_sph']
    cull = buf[h['off_cull']:h['off_cull'] + 8 * ((n_sph + 3) // 4 * 4)].reshape(-1, 8)
    rng = np.random.RandomState(0)
    T = field.margin + robot.link_radius.max() + field.spheres[:, 3]
    for o in range(n_sph):
        c = field.spheres[o, :3].astype(np.float64)
        d = rng.randn(20000, 3)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        x = (c + d * (T[o] * rng.uniform(0.0, 1.0, (20000, 1)))).astype(np.float32)   # inside the threshold ball
        xx = (x * x).sum(1, dtype=np.float32)
        t = xx + x[:, 0] * cull[o, 0] + x[:, 1] * cull[o, 1] + x[:, 2] * cull[o, 2]
        assert (t < cull[o, 3]).all()
    assert (cull[n_sph:, 3] < -1e29).all()


@pytest.mark.parametrize('name', ['stomp_pm2d_c1', 'stomp_panda_t1', 'stomp_pm2d_h48'])
def test_stomp_constants_match_reference(name):
    from motion_planning_baselines_amd.planners.stomp import precision_to_scale_tril, stomp_precision_matrix
    g = load_golden(name)
    cpu = dict(device='cpu', dtype=torch.float32)
    R = stomp_precision_matrix(int(g['H']), float(g['dt']), float(g['sigma_spectral']), cpu)
    assert torch.equal(R, torch.from_numpy(g['R']))
    assert torch.equal(torch.inverse(R), torch.from_numpy(g['Sigma']))
    assert torch.equal(precision_to_scale_tril(R), torch.from_numpy(g['L']))


def test_chomp_constants_match_reference():
    from motion_planning_baselines_amd.planners.chomp import chomp_precision_matrix
    g = load_golden('chomp_pm2d_dense')
    R = chomp_precision_matrix(dt=float(g['dt']), n_support_points=int(g['H']), tensor_args=dict(device='cpu', dtype=torch.float32))
    assert torch.equal(R, torch.from_numpy(g['R']))


def test_planner_refuses_cpu_device():
    from motion_planning_baselines_amd._lib import MPBError
    from motion_planning_baselines_amd.planners.stomp import STOMP
    with pytest.raises(MPBError):
        STOMP(n_dof=2, n_support_points=64, num_particles_per_goal=2, num_samples=4, opt_iters=1, dt=0.04,
              start_state=torch.zeros(2), initial_particle_means=torch.zeros(2, 64, 2),
              tensor_args=dict(device='cpu', dtype=torch.float32))


def test_product_geometry_round_trip():
    g = load_golden('chomp_panda')
    robot, field = product_geometry_from_golden(g)
    from motion_planning_baselines_amd import geometry as G
    buf = G.pack_geometry(robot, field, prune_static=False)
    h = G.header(buf)
    assert h['n_links'] == len(g['link_radius']) and h['n_sph'] == len(g['spheres'])


def test_static_link_pruning_is_conservative():
    """pack_geometry leaves out only collision spheres whose hinge is zero for EVERY joint configuration: spheres on
    frame 1 whose circle about the first joint axis stays clear of all obstacles.  Checked by brute force with the oracle's
    FK over a dense sweep of q1 (the other joints cannot move frame 1) and random full configurations."""
    from motion_planning_baselines_amd import geometry as G
    from oracle.geometry_ref import make_ref_geometry
    robot = G.RobotPanda()
    for field in (G.env_spheres_3d(seed=0), G.env_spheres_3d(seed=3),
                  G.CollisionField(spheres=np.array([[0.12, 0.05, 0.18, 0.05], [0.5, 0.0, 0.5, 0.1]]), margin=0.05),
                  G.CollisionField(boxes=np.array([[0.2, 0.0, 0.1, 0.05, 0.05, 0.05]]), margin=0.05)):
        rs, fs = robot.spec(), field.spec()
        keep = G.links_that_can_touch(rs, fs)
        assert keep[np.asarray(rs['link_frame']) != 1].all()                  # later frames are never dropped
        rr, rf = make_ref_geometry(robot, field, dict(device='cpu', dtype=torch.float64))
        q = torch.zeros(4096, 7, dtype=torch.float64)
        q[:, 0] = torch.linspace(-3.2, 3.2, 4096)
        q[:, 1:] = 6.0 * torch.rand(4096, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) - 3.0
        pts = rr.fk_map_collision(q)                                          # (N, L, 3)
        sd = rf.signed_distance(pts)                                          # (N, L)
        hinge = (float(fs['margin']) + torch.as_tensor(rs['link_radius'], dtype=torch.float64) - sd).clamp_min(0)
        worst = hinge.max(0).values.numpy()
        assert (worst[~keep] == 0).all(), worst[~keep]
        buf = G.pack_geometry(robot, field)
        assert G.header(buf)['n_links'] == int(keep.sum())
    # the synthetic C3 scene keeps obstacles off the base axis: the three base-link spheres go
    assert int(G.links_that_can_touch(robot.spec(), G.env_spheres_3d(seed=0).spec()).sum()) == 28


def test_cost_term_specs_merge_into_one_launch():
    """CostComposite groups its trajectory-only members into as few mpb_cost_terms_eval launches as possible."""
    from motion_planning_baselines_amd import geometry as G
    from motion_planning_baselines_amd.planners.costs import cost_functions as C
    robot = G.RobotPointMass(2, radius=0.01, dt=0.1)
    ta = dict(device='cpu', dtype=torch.float32)
    H = 16
    gp = C.CostGPTrajectory(robot, H, 0.1, sigma_gp=0.5, tensor_args=ta)
    gp_other_dt = C.CostGPTrajectory(robot, H, 0.2, sigma_gp=0.5, tensor_args=ta)
    sm = C.CostSmoothnessCHOMP(robot, H, tensor_args=ta)
    jl = C.CostJointLimits(robot, H, tensor_args=ta)
    coll = C.CostCollision(robot, H, field=G.env_dense_2d(), sigma_coll=0.1, tensor_args=ta)
    comp = C.CostComposite(robot, H, [coll, gp, sm, jl], weights_cost_l=[1.0, 2.0, 3.0, 4.0], tensor_args=ta)
    colls, groups, other = comp.device_plan('cpu')
    assert [c is coll for c, _ in colls] == [True] and not other and len(groups) == 1
    g = groups[0]
    assert g['terms'] == {'gp', 'smooth', 'jlim'}
    assert g['k_gp'] == pytest.approx(2.0 / 0.25) and g['k_smooth'] == 3.0 and g['k_jlim'] == 4.0 and g['dt'] == 0.1
    # same term twice, or two different dt: separate launches
    assert len(C.CostComposite(robot, H, [gp, gp], tensor_args=ta).device_plan('cpu')[1]) == 2
    assert len(C.CostComposite(robot, H, [sm, gp_other_dt], tensor_args=ta).device_plan('cpu')[1]) == 2
    # what the planners can fuse
    assert C.device_plan(comp, 'cpu') is not None
    # several collision members are chained into one evaluator: weight * k_0 * sum_f s_f cost_f
    coll2 = C.CostCollision(robot, H, field=G.env_grid_circles_2d(), sigma_coll=0.2, tensor_args=ta)
    plan = C.device_plan(C.CostComposite(robot, H, [coll, coll2], weights_cost_l=[2.0, 3.0], tensor_args=ta), 'cpu')
    merged, w0, groups0 = plan
    assert isinstance(merged, C.MergedCollision) and w0 == 2.0 and groups0 == []
    assert merged.k_sigma == pytest.approx(100.0) and merged.scales == pytest.approx([1.0, (3.0 * 25.0) / (2.0 * 100.0)])
    assert C.device_plan(C.CostComposite(robot, H, [coll] * 5, tensor_args=ta), 'cpu') is None      # more than four fields
    assert C.device_plan(lambda x: x, 'cpu') is None                                                   # user callable
    # no CPU fallback: evaluating on CPU tensors raises instead of computing
    with pytest.raises(ValueError, match='no CPU path'):
        gp(torch.zeros(2, H, 4))
    with pytest.raises(ValueError, match='no CPU path'):
        comp(torch.zeros(2, H, 4))


def test_oracle_trajectory_utilities():
    """Build-defined interpolation / resampling restatements: exact on straight lines, end points kept."""
    from oracle import planners_ref as O
    x = torch.stack([torch.linspace(0, 1, 5), torch.linspace(2, 0, 5)], -1)[None]           # (1,5,2) straight line
    xi = O.interpolate_trajs(x, 3)
    assert xi.shape == (1, 17, 2)
    assert torch.allclose(xi[0, :, 0], torch.linspace(0, 1, 17), atol=1e-6)
    assert torch.equal(xi[:, ::4], x)
    path = np.array([[0., 0.], [1., 0.], [1., 3.]])                                            # L-shaped, length 4
    out = O.resample_path(path, 9, 0.5).numpy()
    seg = np.linalg.norm(np.diff(out[:, :2], axis=0), axis=1)
    assert np.allclose(seg, 0.5)                                                               # uniform in arc length
    assert np.allclose(out[0, :2], path[0]) and np.allclose(out[-1, :2], path[-1])
    assert np.allclose(out[1:-1, 2:], (path[-1] - path[0]) / (8 * 0.5)) and np.all(out[[0, -1], 2:] == 0)


def test_chained_geometry_buffers():
    """Several collision fields in one buffer: header word `next` links them, `fscale` carries the per-field scale;
    the C-ABI validator walks the chain."""
    from motion_planning_baselines_amd import geometry as G
    from motion_planning_baselines_amd import _lib
    from motion_planning_baselines_amd._lib import MPBError
    robot = G.RobotPointMass(2, radius=0.01)
    f1, f2 = G.env_dense_2d(), G.env_grid_circles_2d()
    one = G.pack_geometry(robot, f1)
    two = G.pack_geometry(robot, [f1, f2], scales=[1.0, 0.25])
    assert G.count_fields(one) == 1 and G.count_fields(two) == 2
    first, second = G.fields(two)
    assert all(np.array_equal(first[name], G.header(one)[name]) for name in G.HEADER_DTYPE.names if name != 'next')
    assert first['next'] == one.size and second['fscale'] == np.float32(0.25) and first['fscale'] == 1.0
    assert second.tobytes() == two[one.size:one.size + G.GEOM_HEADER_WORDS].tobytes()
    _lib.geom_check(one)
    _lib.geom_check(two)
    bad = two.copy()
    G.header(bad)['next'] = one.size - 4           # next header inside the first field
    with pytest.raises(MPBError):
        _lib.geom_check(bad)
    bad = two.copy()
    G.header(bad, one.size)['fscale'] = -1.0       # negative scale
    with pytest.raises(MPBError):
        _lib.geom_check(bad)
    with pytest.raises(MPBError):                  # second field for a different robot
        _lib.geom_check(np.concatenate([_link(one), G.pack_geometry(G.RobotPointMass(3, radius=0.01), G.env_spheres_3d())]))
    with pytest.raises(AssertionError):
        G.pack_geometry(robot, [f1] * 5)


def _link(buf):
    b = buf.copy()
    from motion_planning_baselines_amd import geometry as G
    G.header(b)['next'] = b.size
    return b


def test_gp_prior_scale_tril_matches_reference():
    """Per-dof dense scale_tril from the bidiagonal factor == the sub-matrix of the reference's dense
    MultivariateNormal scale_tril (golden from MultiMPPrior, fp64)."""
    from conftest import load_golden
    from motion_planning_baselines_amd.planners.base import gp_prior_factor, gp_prior_scale_tril
    g = load_golden('gp_prior_d2_h8')
    D, H = int(g['D']), int(g['H'])
    Ud, Uo = gp_prior_factor(H, float(g['dt']), float(g['sigma_start']), float(g['sigma_gp']), float(g['sigma_goal']))
    Tm = gp_prior_scale_tril(Ud, Uo)
    assert Tm.shape == (2 * H, 2 * H) and np.allclose(np.triu(Tm, 1), 0.0)
    full = g['scale_tril'][0]                                 # (2D*H, 2D*H), index t*2D + c
    for d in range(D):
        idx = np.array([[t * 2 * D + d, t * 2 * D + D + d] for t in range(H)]).reshape(-1)
        sub = full[np.ix_(idx, idx)]
        np.testing.assert_allclose(Tm, sub, rtol=1e-9, atol=1e-12 * np.abs(sub).max())


def test_ctypes_signatures_match_the_header():
    """Every prototype of include/mpb.h, parameter by parameter, against the ctypes argtypes of _lib.SIGNATURES
    (a mismatch would not fail to load -- it would pass garbage)."""
    import ctypes
    from motion_planning_baselines_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'mpb.h')).read()
    hdr = re.sub(r'/\*.*?\*/', ' ', hdr, flags=re.S)
    protos = re.findall(r'\b(?:int|size_t|const char \*|const char\*)\s*\**\s*(mpb_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;', hdr, flags=re.S)
    assert len(protos) == len(_lib.SIGNATURES)
    def ctype_of(param):
        param = ' '.join(param.split())
        if param in ('void', ''):
            return None
        if '*' in param:
            return ctypes.c_void_p
        base = param.rsplit(' ', 1)[0].replace('const ', '').strip()
        return {'int': ctypes.c_int, 'float': ctypes.c_float, 'uint64_t': ctypes.c_uint64, 'uint32_t': ctypes.c_uint32,
                'size_t': ctypes.c_size_t}[base]
    for name, params in protos:
        want = [t for t in (ctype_of(p) for p in params.split(',')) if t is not None]
        assert want == list(_lib.SIGNATURES[name]), (name, [t.__name__ for t in want], [t.__name__ for t in _lib.SIGNATURES[name]])


def test_robot_model_header_is_generated_from_geometry():
    """csrc/mpb_model_panda.h (the compile-time Panda tables the model kernels fold) is exactly what model_gen emits from
    geometry.py -- the single source of the numbers -- and the DH tables carry exact zeros / ones (what folds)."""
    import os
    from motion_planning_baselines_amd import geometry as G, model_gen
    path = os.path.join(os.path.dirname(G.__file__), 'csrc', 'mpb_model_panda.h')
    assert open(path).read() == model_gen.header_text('panda')
    tf = np.asarray(G.RobotPanda().spec()['joint_tf'])[:7, :, :3]
    assert set(np.unique(np.abs(tf))) <= {0.0, 1.0}


def test_geometry_model_tag_and_flags():
    """pack_geometry tags a buffer with the robot model only when the tables match bit for bit; mpb_geom_flags reports it
    (and the all-grids bit); mpb_geom_check refuses a forged tag."""
    from motion_planning_baselines_amd import _lib, geometry as G
    robot, field = G.RobotPanda(), G.env_spheres_3d()
    buf = G.pack_geometry(robot, field)
    h = G.header(buf)
    assert h['model'] == 1 and int(h['keep_mask']) == ((1 << 31) - 1) & ~0b111      # the three base spheres are pruned here
    _lib.geom_check(buf)
    # (one field; the cells of its broad-phase grid)
    n_cells = int(h['n_cells'])
    grids_one, cells = G.GEOM_FLAG_ALL_GRIDS | G.GEOM_FLAG_ONE_FIELD, n_cells << G.GEOM_FLAG_CELLS_SHIFT
    assert _lib.geom_flags(buf) == (1 | grids_one | cells)
    assert _lib.geom_flags(G.pack_geometry(robot, field, use_model=False)) == (grids_one | cells)
    full = G.pack_geometry(robot, field, prune_static=False)
    assert int(G.header(full)['keep_mask']) == (1 << 31) - 1 and _lib.geom_flags(full) == (1 | grids_one | cells)
    two = G.pack_geometry(robot, [field, G.env_spheres_3d(seed=5)])
    assert not (_lib.geom_flags(two) & G.GEOM_FLAG_ONE_FIELD)
    assert (_lib.geom_flags(two) & (G.GEOM_FLAG_MODEL_MASK | G.GEOM_FLAG_ALL_GRIDS)) == (1 | G.GEOM_FLAG_ALL_GRIDS)
    # a robot that is not the Panda bit for bit is not tagged
    other = G.RobotPanda()
    other.link_offset[5, 1] += 1e-4
    assert G.header(G.pack_geometry(other, field))['model'] == 0
    # a forged tag on that buffer is refused
    forged = G.pack_geometry(other, field, prune_static=False)
    G.header(forged)['model'] = 1
    G.header(forged)['keep_mask'] = (1 << 31) - 1
    with pytest.raises(_lib.MPBError):
        _lib.geom_check(forged)
    # point robot: no model, grid usable; box-only field: no grid at all
    pm = G.pack_geometry(G.RobotPointMass(2, radius=0.01), G.env_grid_circles_2d())
    below_cells = (1 << G.GEOM_FLAG_CELLS_SHIFT) - 1
    point_one = G.GEOM_FLAG_POINT | G.GEOM_FLAG_ONE_FIELD
    # 49 circles: too many for the in-register CHOMP kernel (POINT_SMALL)
    assert (_lib.geom_flags(pm) & below_cells) == (G.GEOM_FLAG_ALL_GRIDS | point_one)
    assert _lib.geom_flags(pm) >> G.GEOM_FLAG_CELLS_SHIFT == int(G.header(pm)['n_cells'])
    assert (_lib.geom_flags(G.pack_geometry(G.RobotPointMass(2, radius=0.01), G.env_dense_2d())) & below_cells) == (
        G.GEOM_FLAG_ALL_GRIDS | G.GEOM_FLAG_POINT_SMALL | point_one)
    boxes = G.CollisionField(boxes=np.array([[0.2, 0.2, 0.1, 0.1]], np.float32), margin=0.01)
    assert _lib.geom_flags(G.pack_geometry(G.RobotPointMass(2, radius=0.01), boxes)) == (G.GEOM_FLAG_POINT_SMALL | point_one)


def test_stomp_workspace_size():
    from motion_planning_baselines_amd import _lib
    from motion_planning_baselines_amd.geometry import GEOM_FLAG_ALL_GRIDS as GRIDS, GEOM_FLAG_ALL_LISTS as LISTS
    f = _lib.lib().mpb_stomp_workspace_bytes
    # header + 8-byte {value, tag} granules, two parities: the H = 64 kernel's exchange slots hold 912 granules, the generalised
    # kernel's 2064 -- which also serves H = 64 when the geometry carries list grids (round 6): the workspace fits either
    assert f(128, 32, 64, 14) == 4 * 320 + 8 * (2 * 128 * 2 * 2064)
    assert f(3, 5, 64, 7) == 4 * 320 and f(0, 32, 64, 14) == 0              # one workgroup per particle: the header only
    assert f(4096, 32, 64, 14) == 4 * 320                                   # at least as many particles as CUs: two batches, no exchange
    assert f(8, 32, 48, 14) == 4 * 320 + 8 * (2 * 8 * 2 * 2064)            # H != 64: the generalised kernel's exchange slots (2 + H*d <= 2064 granules)
    assert f(8, 32, 200, 14) == 4 * 320                                     # a shape no persistent kernel serves (H > 128)
    # which path a call takes is a pure host-side function of the shape, the geometry flags and the workspace size
    path = _lib.lib().mpb_stomp_run_path
    assert path(GRIDS | 1, f(128, 32, 64, 14), 128, 32, 64, 14) == 1       # exchange layout
    assert path(GRIDS | 1, 4 * 320 + 8 * (2 * 128 * 2 * 912), 128, 32, 64, 14) == 1    # ... which needs the smaller slots only
    assert path(LISTS | 1, f(128, 32, 64, 14), 128, 32, 64, 14) == 1 and path(LISTS | 1, 1 << 30, 128, 32, 100, 14) == 0   # list grids: H <= 64
    assert path(GRIDS | 1, 64, 128, 32, 64, 14) == 0                       # workspace too small: two-kernel loop
    assert path(GRIDS, 1280, 4096, 32, 64, 14) == 2 and path(GRIDS, 1280, 8, 16, 64, 7) == 2      # the header alone (MPB_STOMP_WS_HEADER_BYTES)
    assert path(0, 1 << 30, 128, 32, 64, 14) == 0 and path(GRIDS, 1 << 30, 128, 32, 200, 14) == 0
    assert path(GRIDS, 1 << 30, 128, 32, 128, 14) == 1 and path(GRIDS, 1280, 300, 32, 128, 14) == 2   # H = 128: generalised kernel
    assert path(GRIDS, 1 << 30, 2, 128, 32, 7) == 1 and path(GRIDS, 1 << 30, 128, 32, 64, 5) == 1  # S = 128; d = 5


def test_gpmp2_workspace_size():
    """mpb_gpmp2_workspace_bytes (GpLayout, csrc/mpb_gpmp2.h) against byte counts recorded from the library as it was before the layout
    had one definition: jac for MPB_MAX_FIELDS fields and the two diagonal vectors, each rounded up to 256 bytes, and the larger of the block
    form's elimination records and the low-rank area -- which is counted for every H, also beyond that form's tile."""
    from motion_planning_baselines_amd import _lib
    f = _lib.lib().mpb_gpmp2_workspace_bytes
    assert f(0, 64, 7) == 430600 and f(1, 2, 1) == 2944 and f(2, 8, 2) == 20736 and f(3, 64, 7) == 493624
    assert f(2, 128, 12) == 2495016 and f(2, 256, 7) == 4870696 and f(2048, 128, 7) == 352350208
    assert f(2, 1, 7) == 0 and f(2, 257, 7) == 0 and f(2, 8, 0) == 0 and f(2, 8, 13) == 0 and f(-1, 8, 2) == 0


def _gpmp2_refusal_calls():
    """(label, environment, entry point, arguments) of every refused GPMP2 call of the table below, and of the B == 0 / n_iters == 0
    calls that return before a launch.  Pointers are host memory: none of these calls may reach a kernel."""
    import ctypes
    buf = (ctypes.c_char * 1024)()
    ok = (ctypes.addressof(buf) + 255) & ~255                 # 256-byte aligned; + 16: 16-byte but not 256-byte aligned; + 4: neither
    _gpmp2_refusal_calls.keep = buf
    base = dict(x=ok, start=ok, goal=ok, geom=ok, ws=ok, B=2, H=8, D=2, n_interp=0, n_fields=1, n_iters=1)
    sig = (0.04, 1e-3, 1.0, 1e-3, 1e-2)                       # dt, sigma_start, sigma_gp, sigma_goal, sigma_coll
    pack = {
        'linearize': lambda a: (a['x'], a['geom'], 0, a['ws'], a['B'], a['H'], a['D'], a['n_interp'], None),
        'diag': lambda a: (a['ws'], None, a['B'], a['H'], a['D'], a['n_fields'], *sig, None),
        'solve': lambda a: (a['x'], a['start'], a['goal'], None, a['ws'], None, a['B'], a['H'], a['D'], a['n_fields'], *sig, 1e-2, 1, 1.0, None),
        'step': lambda a: (a['x'], a['start'], a['goal'], a['geom'], 0, a['ws'], None, a['B'], a['H'], a['D'], *sig, 1e-2, 1, 1.0,
                           a['n_iters'], a['n_interp'], a['n_fields'], None),
    }
    takes = {'linearize': ('x', 'geom', 'ws', 'n_interp'), 'diag': ('ws', 'n_fields'), 'solve': ('x', 'start', 'goal', 'ws', 'n_fields'),
             'step': ('x', 'start', 'goal', 'geom', 'ws', 'n_interp', 'n_fields', 'n_iters')}
    aligned = {'linearize': ('x', 'geom', 'ws'), 'diag': (), 'solve': ('x', 'ws'), 'step': ('x', 'geom', 'ws')}   # (solve never reads geom)
    shapes = [('H=1', dict(H=1)), ('H=257', dict(H=257)), ('D=0', dict(D=0)), ('D=13', dict(D=13)), ('B=-1', dict(B=-1)),
              ('n_interp=-1', dict(n_interp=-1)), ('n_interp=65', dict(n_interp=65)), ('n_fields=0', dict(n_fields=0)),
              ('n_fields=5', dict(n_fields=5)), ('n_iters=-1', dict(n_iters=-1))]

    def call(entry, label, env=None, **change):
        return ('%s %s' % (entry, label), env or {}, 'mpb_gpmp2_' + entry, pack[entry](dict(base, **change)))
    for entry in ('linearize', 'diag', 'solve', 'step'):
        for p in takes[entry]:
            if not p.startswith('n_'):
                yield call(entry, p + ' null', **{p: None})
        for p in aligned[entry]:
            yield call(entry, p + ' misaligned', **{p: ok + (16 if p == 'ws' else 4)})
        for label, change in shapes:
            if all(k in takes[entry] or k in 'BHD' for k in change):
                yield call(entry, label, **change)
        if entry != 'diag':                                    # (mpb_gpmp2_diag has no B == 0 return: it launches)
            yield call(entry, 'B=0', B=0)
    yield call('step', 'n_iters=0', n_iters=0)
    yield call('step', 'x misaligned, n_iters=0', x=ok + 4, n_iters=0)
    yield call('step', 'x misaligned, B=0', x=ok + 4, B=0)
    # the form refusals, of mpb_gpmp2_solve only (mpb_gpmp2_step may have enqueued the linearisation before it meets them)
    yield call('solve', 'D=9 H=129', D=9, H=129)
    yield call('solve', 'FORM=lr H=129', env=dict(MPB_GPMP2_FORM='lr'), H=129)
    yield call('solve', 'FORM=block D=9', env=dict(MPB_GPMP2_FORM='block'), D=9)


# what the library answered each of those calls before the entry points shared one argument check (code, mpb_last_error), with one
# exception: without a GPU the trailing hipGetLastError of the old mpb_gpmp2_step turned the two n_iters == 0 calls, which enqueue
# nothing, into MPB_E_HIP "no ROCm-capable device is detected"; on a GPU they answered MPB_OK, which is what is held here
GPMP2_REFUSALS = {
    'linearize x null': (1, 'mpb_gpmp2_linearize: null pointer'),
    'linearize geom null': (1, 'mpb_gpmp2_linearize: null pointer'),
    'linearize ws null': (1, 'mpb_gpmp2_linearize: null pointer'),
    'linearize x misaligned': (1, 'mpb_gpmp2_linearize: x / geom must be 16-byte aligned and the workspace 256-byte aligned'),
    'linearize geom misaligned': (1, 'mpb_gpmp2_linearize: x / geom must be 16-byte aligned and the workspace 256-byte aligned'),
    'linearize ws misaligned': (1, 'mpb_gpmp2_linearize: x / geom must be 16-byte aligned and the workspace 256-byte aligned'),
    'linearize H=1': (1, 'mpb_gpmp2_linearize: bad shape'),
    'linearize H=257': (1, 'mpb_gpmp2_linearize: bad shape'),
    'linearize D=0': (1, 'mpb_gpmp2_linearize: bad shape'),
    'linearize D=13': (1, 'mpb_gpmp2_linearize: bad shape'),
    'linearize B=-1': (1, 'mpb_gpmp2_linearize: bad shape'),
    'linearize n_interp=-1': (1, 'mpb_gpmp2_linearize: bad shape'),
    'linearize n_interp=65': (1, 'mpb_gpmp2_linearize: bad shape'),
    'linearize B=0': (0, None),
    'diag ws null': (1, 'mpb_gpmp2_diag: null pointer'),
    'diag H=1': (1, 'mpb_gpmp2_diag: bad shape'),
    'diag H=257': (1, 'mpb_gpmp2_diag: bad shape'),
    'diag D=0': (1, 'mpb_gpmp2_diag: bad shape'),
    'diag D=13': (1, 'mpb_gpmp2_diag: bad shape'),
    'diag B=-1': (1, 'mpb_gpmp2_diag: bad shape'),
    'diag n_fields=0': (1, 'mpb_gpmp2_diag: bad shape'),
    'diag n_fields=5': (1, 'mpb_gpmp2_diag: bad shape'),
    'solve x null': (1, 'mpb_gpmp2_solve: null pointer'),
    'solve start null': (1, 'mpb_gpmp2_solve: null pointer'),
    'solve goal null': (1, 'mpb_gpmp2_solve: null pointer'),
    'solve ws null': (1, 'mpb_gpmp2_solve: null pointer'),
    'solve x misaligned': (1, 'mpb_gpmp2_solve: x must be 16-byte aligned and the workspace 256-byte aligned'),
    'solve ws misaligned': (1, 'mpb_gpmp2_solve: x must be 16-byte aligned and the workspace 256-byte aligned'),
    'solve H=1': (1, 'mpb_gpmp2_solve: bad shape'),
    'solve H=257': (1, 'mpb_gpmp2_solve: bad shape'),
    'solve D=0': (1, 'mpb_gpmp2_solve: bad shape'),
    'solve D=13': (1, 'mpb_gpmp2_solve: bad shape'),
    'solve B=-1': (1, 'mpb_gpmp2_solve: bad shape'),
    'solve n_fields=0': (1, 'mpb_gpmp2_solve: bad shape'),
    'solve n_fields=5': (1, 'mpb_gpmp2_solve: bad shape'),
    'solve B=0': (0, None),
    'step x null': (1, 'mpb_gpmp2_step: null pointer'),
    'step start null': (1, 'mpb_gpmp2_step: null pointer'),
    'step goal null': (1, 'mpb_gpmp2_step: null pointer'),
    'step geom null': (1, 'mpb_gpmp2_step: null pointer'),
    'step ws null': (1, 'mpb_gpmp2_step: null pointer'),
    'step x misaligned': (1, 'mpb_gpmp2_linearize: x / geom must be 16-byte aligned and the workspace 256-byte aligned'),
    'step geom misaligned': (1, 'mpb_gpmp2_linearize: x / geom must be 16-byte aligned and the workspace 256-byte aligned'),
    'step ws misaligned': (1, 'mpb_gpmp2_linearize: x / geom must be 16-byte aligned and the workspace 256-byte aligned'),
    'step H=1': (1, 'mpb_gpmp2_step: bad shape'),
    'step H=257': (1, 'mpb_gpmp2_step: bad shape'),
    'step D=0': (1, 'mpb_gpmp2_step: bad shape'),
    'step D=13': (1, 'mpb_gpmp2_step: bad shape'),
    'step B=-1': (1, 'mpb_gpmp2_step: bad shape'),
    'step n_interp=-1': (1, 'mpb_gpmp2_linearize: bad shape'),
    'step n_interp=65': (1, 'mpb_gpmp2_linearize: bad shape'),
    'step n_fields=0': (1, 'mpb_gpmp2_step: bad shape'),
    'step n_fields=5': (1, 'mpb_gpmp2_step: bad shape'),
    'step n_iters=-1': (1, 'mpb_gpmp2_step: bad shape'),
    'step B=0': (0, None),
    'step n_iters=0': (0, None),
    'step x misaligned, n_iters=0': (0, None),
    'step x misaligned, B=0': (0, None),
    'solve D=9 H=129': (2, 'mpb_gpmp2_solve: more than 8 degrees of freedom need the low-rank form (n_fields * (H - 1) <= 127, H <= 128)'),
    'solve FORM=lr H=129': (2, 'mpb_gpmp2_solve: MPB_GPMP2_FORM=lr, but n_fields * (H - 1) > 127'),
    'solve FORM=block D=9': (2, 'mpb_gpmp2_solve: more than 8 degrees of freedom need the low-rank form (n_fields * (H - 1) <= 127, H <= 128)'),
}


def test_gpmp2_refusals_keep_code_and_message(monkeypatch):
    """Every refusal of the four GPMP2 entry points keeps its code, its text and the entry point it names -- mpb_gpmp2_step reports the
    linearisation's alignment and n_interp tests under that stage's name, and only once an iteration runs.  Skipped where there is a GPU:
    a refusal that regressed would launch a kernel on the host pointers used here."""
    if torch.cuda.is_available():
        pytest.skip('host pointers: a refusal that regressed would reach a kernel')
    from motion_planning_baselines_amd import _lib
    h = _lib.lib()
    seen = {}
    for label, env, name, args in _gpmp2_refusal_calls():
        for var in ('MPB_GPMP2_FORM', 'MPB_GPMP2_SM', 'MPB_GPMP2_SPLIT'):
            monkeypatch.delenv(var, raising=False)
        for var, value in env.items():
            monkeypatch.setenv(var, value)
        code = getattr(h, name)(*args)
        seen[label] = (code, h.mpb_last_error().decode() if code else None)
    assert seen == GPMP2_REFUSALS, {k: (seen.get(k), GPMP2_REFUSALS.get(k)) for k in set(seen) | set(GPMP2_REFUSALS) if seen.get(k) != GPMP2_REFUSALS.get(k)}


@pytest.mark.parametrize('scene', ['spheres_3d', 'dense_2d', 'grid_circles_2d', 'large_3d'])
def test_broad_phase_grid_is_conservative_and_fits(scene):
    """geometry.build_grid: the grid fits the LDS image of the kernels (MPB_GRID_MAX_CELLS words), is refined below the
    coarse target when there is room, and is conservative -- every obstacle within reach (r_o + a_max) of a point is listed
    in the word of the point's cell (or the cell is marked overflow), with the cell index computed as the kernels do in fp32."""
    from motion_planning_baselines_amd import geometry as G
    rng = np.random.default_rng(5)
    if scene == 'spheres_3d':
        sph, a_max = G.env_spheres_3d().spheres, 0.13
    elif scene == 'dense_2d':
        sph, a_max = G.env_dense_2d().spheres, 0.02
    elif scene == 'grid_circles_2d':
        sph, a_max = G.env_grid_circles_2d().spheres, 0.015
    else:   # a scene too large for the coarse target cell: the builder has to coarsen
        c = rng.uniform(-6.0, 6.0, size=(40, 3))
        sph, a_max = np.concatenate([c, rng.uniform(0.1, 0.4, size=(40, 1))], 1).astype(np.float32), 0.13
    sph = np.asarray(sph, dtype=np.float32)
    g = G.build_grid(sph, a_max, planar=bool(np.ptp(sph[:, 2]) == 0.0))     # (pack_geometry passes planar for 2-D point robots)
    dims, lo, inv, words = g['dims'].astype(np.int64), g['lo'], g['inv'], g['words']
    n = len(sph)
    assert dims.prod() == len(words) <= G.GRID_MAX_CELLS and (dims >= 1).all() and (dims <= G.GRID_MAX_DIM).all()
    cell = 1.0 / inv.astype(np.float64)
    # geometry version 6: cells on a lattice through the origin, lo = (K - 1/2) h per axis
    K = g['K'].astype(np.int64)
    assert np.allclose(lo.astype(np.float64) * inv.astype(np.float64) + 0.5, K, atol=1e-3)
    assert g['k_lin'] == K[0] + dims[0] * (K[1] + dims[1] * K[2])
    if scene == 'large_3d':
        assert cell.max() > G.GRID_CELL                      # coarsened
    else:
        assert cell[dims > 1].max() <= G.GRID_CELL * 1.0001  # never coarser than the target when it fits
    planar = np.ptp(sph[:, 2]) == 0.0
    assert (dims[2] == 1) == bool(planar)
    # random points around the obstacles, cell index in fp32 exactly as grid_cell<true> (mpb_geom.h)
    k = rng.integers(0, n, size=20000)
    p = (sph[k, :3] + rng.normal(size=(20000, 3)).astype(np.float32) * (sph[k, 3:4] + a_max) * 1.2).astype(np.float32)
    if planar:
        p[:, 2] = sph[0, 2]
    f = np.floor(p * inv + (-lo * inv).astype(np.float32)).astype(np.float32)     # fma vs mul+add: inside the 1e-5 m slack
    f = np.clip(f, 0.0, (dims - 1).astype(np.float32))
    idx = ((f[:, 2] * np.float32(dims[1]) + f[:, 1]) * np.float32(dims[0]) + f[:, 0]).astype(np.int64)
    inside = ((p >= lo) & (p <= lo + dims / inv)).all(1)
    # ... and as grid_cell_rel does (persistent kernels, MPPI): fma(x, 1/h, 1.5 * 2^23) -- exact product, ONE rounding to the
    # integer grid of [2^23, 2^24), ties to even --, the linear index combined in the same float form, clamped
    MAGIC = 12582912.0
    t = (p.astype(np.float64) * inv.astype(np.float64) + MAGIC).astype(np.float32).astype(np.float64) - MAGIC      # round(x / h) per axis
    lin = t[:, 0] + dims[0] * (t[:, 1] + dims[1] * t[:, 2]) - g['k_lin']
    idx2 = np.clip(lin, 0, len(words) - 1).astype(np.int64)
    ins = ((t - K >= 0) & (t - K <= dims - 1)).all(1)                 # points whose cell lies inside the box on every axis
    assert (np.abs(idx2[ins & inside] - idx[ins & inside]) <= dims[0] * dims[1] + dims[0] + 1).all()
    for which, ii in (('floor', idx), ('lattice', idx2)):
        ww = words[ii]
        lst = G.grid_cell_slots(ww)
        d_ = np.linalg.norm(p[:, None, :3].astype(np.float64) - sph[None, :, :3].astype(np.float64), axis=2)
        near_ = d_ < (sph[None, :, 3].astype(np.float64) + a_max)
        for i in np.nonzero(near_.any(1))[0]:
            if ww[i] == G.GRID_OVERFLOW:
                continue
            need = set(np.nonzero(near_[i])[0].tolist())
            assert need <= set(lst[i].tolist()), (scene, which, i, need, lst[i])
    w = words[idx]
    listed = G.grid_cell_slots(w)
    d = np.linalg.norm(p[:, None, :3].astype(np.float64) - sph[None, :, :3].astype(np.float64), axis=2)
    near = d < (sph[None, :, 3].astype(np.float64) + a_max)                       # obstacles that can matter at p
    assert not near[~inside].any()                           # outside the grid box nothing is within reach by construction
    for i in np.nonzero(near.any(1))[0]:
        if w[i] == G.GRID_OVERFLOW:
            continue
        need = set(np.nonzero(near[i])[0].tolist())
        assert need <= set(listed[i].tolist()), (scene, i, need, listed[i])
    # slots fill in order and empty slots hold n (the far dummy of the obstacle table)
    ok = w != G.GRID_OVERFLOW
    used = listed[ok] != n
    assert (listed[ok] <= n).all() and (used[:, 1:] <= used[:, :-1]).all()


def test_bench_self_launch_command(monkeypatch):
    """`python bench.py --gpus N` started bare hands its N ranks to torch.distributed.run as fresh child processes BEFORE any
    GPU call, on 127.0.0.1, with the caller's own arguments, and returns the launcher's exit code."""
    import subprocess
    import bench
    seen = {}

    def fake_run(cmd, env=None, **kw):
        seen.update(cmd=cmd, env=env)
        return subprocess.CompletedProcess(cmd, 3)
    monkeypatch.setattr(subprocess, 'run', fake_run)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda *a, **k: (_ for _ in ()).throw(AssertionError('GPU touched before the launch')))
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.delenv('MPB_DIST_BACKEND', raising=False)
    monkeypatch.setattr(bench, 'visible_gpu_count', lambda: 8)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '4', '--steps', '20', '--warmup', '5'])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 3
    cmd = seen['cmd']
    assert cmd[1:4] == ['-m', 'torch.distributed.run', '--nnodes=1'] and cmd[cmd.index('--nproc-per-node') + 1] == '4'
    assert cmd[cmd.index('--master-addr') + 1] == '127.0.0.1' and int(cmd[cmd.index('--master-port') + 1]) > 0
    assert cmd[-6:] == ['--gpus', '4', '--steps', '20', '--warmup', '5'] and cmd[-7].endswith('bench.py')
    assert seen['env']['HSA_ENABLE_IPC_MODE_LEGACY'] == '0'


def test_bench_self_launch_preflight(monkeypatch, capsys, tmp_path):
    """`python bench.py --gpus N` on a node that shows fewer than N GPUs says so and exits non-zero BEFORE
    it starts a rank (and without touching the GPU: the count comes from the KFD topology); a gloo rehearsal (several ranks on
    one GPU) and an unreadable topology are let through."""
    import subprocess
    import bench
    started = []
    monkeypatch.setattr(subprocess, 'run', lambda cmd, env=None, **kw: started.append(cmd) or subprocess.CompletedProcess(cmd, 0))
    monkeypatch.setattr(torch.cuda, 'set_device', lambda *a, **k: (_ for _ in ()).throw(AssertionError('GPU touched before the launch')))
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.delenv('MPB_DIST_BACKEND', raising=False)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '8', '--steps', '20', '--warmup', '5'])
    monkeypatch.setattr(bench, 'visible_gpu_count', lambda: 1)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2 and not started
    err = capsys.readouterr().err
    assert '--gpus 8' in err and '1 GPU' in err
    monkeypatch.setenv('MPB_DIST_BACKEND', 'gloo')                       # rehearsal: ranks share GPUs
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 0 and len(started) == 1
    monkeypatch.delenv('MPB_DIST_BACKEND')
    monkeypatch.setattr(bench, 'visible_gpu_count', lambda: None)        # topology unreadable: the ranks will say what is wrong
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 0 and len(started) == 2
    # the count itself: nodes with SIMDs only, cut down by a *_VISIBLE_DEVICES list
    import builtins
    import os as _os
    nodes = tmp_path / 'nodes'
    for i, simd in enumerate((0, 0, 256, 256, 256)):
        (nodes / str(i)).mkdir(parents=True)
        (nodes / str(i) / 'properties').write_text('cpu_cores_count %d\nsimd_count %d\n' % (0 if simd else 64, simd))
    monkeypatch.undo()
    real_listdir, real_open = _os.listdir, builtins.open
    root = '/sys/class/kfd/kfd/topology/nodes'
    monkeypatch.setattr(_os, 'listdir', lambda p: real_listdir(str(nodes)) if p == root else real_listdir(p))
    monkeypatch.setattr(builtins, 'open', lambda f, *a, **k: real_open(str(f).replace(root, str(nodes)), *a, **k))
    for v in ('ROCR_VISIBLE_DEVICES', 'HIP_VISIBLE_DEVICES', 'CUDA_VISIBLE_DEVICES'):
        monkeypatch.delenv(v, raising=False)
    assert bench.visible_gpu_count() == 3
    monkeypatch.setenv('HIP_VISIBLE_DEVICES', '0,2')
    assert bench.visible_gpu_count() == 2


def test_headline_kernels_have_no_scratch():
    """The persistent STOMP kernels run at their register budget (16 waves per workgroup: 128 VGPRs): a change anywhere in
    their phases can tip loop invariants into scratch -- it happened twice in round 4, once unnoticed for several commits
    (-4 % on the headline).  build() records what the compiler made of every kernel (csrc/kernel_resources.json,
    -Rpass-analysis=kernel-resource-usage); the instantiations the bench line runs must have 0 B of scratch."""
    import json
    from motion_planning_baselines_amd import build
    build.build(verbose=False)
    res = json.load(open(build.RESOURCES))

    def find(prefix):
        hits = {k: v for k, v in res.items() if k.startswith(prefix)}
        assert len(hits) == 1, (prefix, list(hits))
        return next(iter(hits.values()))
    must = ['_Z18stomp_fused_kernelILi14ELi1ELi1ELb0ELb0EE', '_Z18stomp_fused_kernelILi14ELi1ELi2ELb0ELb0EE',   # C3 (exchange), C5 (two batches): device noise, ONE field
            '_Z18stomp_fused_kernelILi14ELi1ELi1ELb1ELb0EE', '_Z18stomp_fused_kernelILi14ELi1ELi2ELb1ELb0EE',   # ... and their injected-noise twins (parity tests)
            '_Z18stomp_fused_kernelILi14ELi1ELi1ELb0ELb1EE', '_Z18stomp_fused_kernelILi14ELi1ELi2ELb0ELb1EE',   # ... and the chained-field forms of all four
            '_Z18stomp_fused_kernelILi14ELi1ELi1ELb1ELb1EE',
            '_Z18stomp_fused_kernelILi7ELi1ELi1ELb0ELb0EE', '_Z18stomp_fused_kernelILi7ELi1ELi2ELb0ELb0EE',     # the same, pos_only
            '_Z18stomp_fused_kernelILi7ELi1ELi1ELb1ELb0EE', '_Z18stomp_fused_kernelILi7ELi1ELi2ELb1ELb0EE',
            '_Z18stomp_fused_kernelILi7ELi1ELi1ELb0ELb1EE',
            '_Z18stomp_fused_kernelILi7ELi1ELi1ELb1ELb1EE',
            '_Z21stomp_fused_hx_kernelILi14ELi1ELi2ELb0ELb0EE', '_Z21stomp_fused_hx_kernelILi14ELi1ELi2ELb1ELb0EE',   # H = 128: device / injected noise
            '_Z21stomp_fused_hx_kernelILi14ELi1ELi1ELb1ELb0EE',                                                       # H < 64, injected noise
            '_Z11mppi_kernelILi2ELb1ELb1ELb0EE', '_Z11mppi_kernelILi2ELb1ELb1ELb1EE']                     # the mppi entry (device / injected noise)
    for name in must:
        r = find(name)
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0, (name, r)
        assert r['vgprs'] + r.get('agprs', 0) <= 128, (name, r)
    # ---- every OTHER kernel of the library against a per-kernel budget: 0 B unless it is listed here with
    #      the value it has today -- a regression anywhere fails on the CPU box, an improvement asks for the table to be tightened
    budget = {   # demangled-prefix -> bytes of scratch per lane
        # MPPI with the exhaustive obstacle walk (a scene without a usable grid) on the matrix path
        'mppi_kernel<0,false,true,true>': 20, 'mppi_kernel<0,false,false,true>': 8,
        'mppi_kernel<2,false,true,false>': 44, 'mppi_kernel<2,false,true,true>': 48,
        'gpmp2_solve_kernel<7,true,true>': 32,     # several collision fields AND the Sherman-Morrison form (256 registers + 7)
        # persistent STOMP, two batches per workgroup (P > 128): the table-driven walk, and the chained-field forms of the models
        # (mostly the injected-noise twins: only the parity tests of several fields at P > 128 come here)
        'stomp_fused_kernel<14,0,2,true,true>': 32, 'stomp_fused_kernel<7,0,2,true,true>': 32, 'stomp_fused_kernel<7,0,2,false,true>': 16,
        'stomp_fused_kernel<14,1,2,true,true>': 48, 'stomp_fused_kernel<7,1,2,true,true>': 36, 'stomp_fused_kernel<7,1,2,false,true>': 16,
        'stomp_fused_hx_kernel<0,0,1,true,false>': 8, 'stomp_fused_hx_kernel<0,0,2,true,false>': 120,   # run-time d, table-driven walk
        'stomp_fused_hx_kernel<0,0,2,false,false>': 68,
        'stomp_fused_hx_kernel<7,1,1,true,false>': 8,   # H < 64
        # list-grid instantiations (round 6: scenes beyond 63 obstacle spheres, H <= 64)
        'stomp_fused_hx_kernel<0,0,1,false,true>': 28, 'stomp_fused_hx_kernel<0,0,1,true,true>': 80,
        'stomp_fused_hx_kernel<14,1,1,false,true>': 8, 'stomp_fused_hx_kernel<14,1,1,true,true>': 8,
        'stomp_fused_hx_kernel<7,1,1,false,true>': 8, 'stomp_fused_hx_kernel<7,1,1,true,true>': 8,
    }

    def short(mangled):
        m = re.match(r'_Z\d+([a-z0-9_]+?)I(.*?)EEv', mangled)
        if not m:
            return mangled
        args = re.findall(r'L([ib])(\d+)E', m.group(2) + 'E')
        return '%s<%s>' % (m.group(1), ','.join(('true' if v == '1' else 'false') if t == 'b' else v for t, v in args))
    seen = set()
    for k, v in res.items():
        name = short(k)
        allowed = budget.get(name, 0)
        assert v.get('scratch', 0) <= allowed, (name, v.get('scratch'), 'budget', allowed)
        if name in budget:
            seen.add(name)
            assert v.get('scratch', 0) >= allowed // 2, ('tighten the budget of ' + name, v.get('scratch'), allowed)
    assert seen == set(budget), set(budget) - seen


def test_model_tag_requires_hinges_below_one():
    """The compile-time robot-model kernels take relu(hinge) as the [0, 1] clamp of the instruction encoding (csrc/mpb_geom.h, UNIT):
    pack_geometry tags a buffer with the model only while margin + largest collision sphere + deepest possible penetration < 1 m, and
    mpb_geom_check refuses a tagged buffer that violates it (a scene like that runs on the table-driven walk)."""
    from motion_planning_baselines_amd import geometry as G, _lib
    robot = G.RobotPanda()
    ok = G.pack_geometry(robot, G.env_spheres_3d())
    assert G.header(ok)['model'] != 0
    _lib.geom_check(ok)
    big = G.CollisionField(spheres=np.array([[0.5, 0.5, 0.5, 0.9], [-0.6, 0.2, 0.4, 0.1]], np.float32), margin=0.05)
    buf = G.pack_geometry(robot, big)
    assert G.header(buf)['model'] == 0                       # 0.05 + 0.08 + 0.9 >= 1: no model tag
    _lib.geom_check(buf)
    forged = buf.copy()
    G.header(forged)['model'] = G.header(ok)['model']
    G.header(forged)['keep_mask'] = G.header(ok)['keep_mask']
    with pytest.raises(_lib.MPBError):
        _lib.geom_check(forged)


def test_grid_lattice_far_and_negative_scenes():
    """Geometry version 6: the grid's origin sits on the lattice lo = (K - 1/2) h for scenes anywhere near the origin (negative K
    included) and mpb_geom_check verifies header word k_lin against it; a scene too far away for fp32 to resolve its cells gets no grid."""
    from motion_planning_baselines_amd import geometry as G, _lib
    robot = G.RobotPointMass(3, radius=0.02)
    rng = np.random.default_rng(1)
    for shift in ([0, 0, 0], [-7.3, 2.1, -0.4], [55.0, -31.0, 12.0]):
        sph = np.concatenate([rng.uniform(-1, 1, (12, 3)) + np.array(shift), rng.uniform(0.05, 0.2, (12, 1))], 1).astype(np.float32)
        buf = G.pack_geometry(robot, G.CollisionField(spheres=sph, margin=0.03))
        h = G.header(buf)
        assert h['n_cells'] > 0
        _lib.geom_check(buf)
        lo, inv, dims = h['grid_lo'].astype(np.float64), h['grid_inv'].astype(np.float64), h['grid_dims']
        K = np.rint(lo * inv + 0.5)
        assert np.abs(lo * inv + 0.5 - K).max() < 1e-3 and h['k_lin'] == int(K[0] + dims[0] * (K[1] + dims[1] * K[2]))
        bad = buf.copy()
        G.header(bad)['k_lin'] += 1
        with pytest.raises(_lib.MPBError):
            _lib.geom_check(bad)
    far = np.array([[1.0e6, -1.0e6, 3.0e5, 0.1]], np.float32)
    buf = G.pack_geometry(robot, G.CollisionField(spheres=far, margin=0.03))
    assert G.header(buf)['n_cells'] == 0 and not (_lib.geom_flags(buf) & G.GEOM_FLAG_ALL_GRIDS)
    _lib.geom_check(buf)


def test_dpp_weighted_sum_keeps_its_wait_states(tmp_path):
    """The persistent STOMP kernels accumulate the softmax-weighted sum with v_fmac_f32_dpp ... row_newbcast:k, written as inline
    assembly (mpb_common.h, fmac_row_bcast_seq).  The compiler's hazard recogniser does not look into inline assembly and the
    hardware does not interlock a DPP read against a preceding vector write of its source (2 wait states) or of exec (5):
    the block opens with its own `s_nop 4`.  Checked on the code objects the library was linked from: every
    row_newbcast:0 fmac is directly preceded by that s_nop, the k-th fmac of a block by the (k-1)-th, and no fmac of a block
    writes the register the block reads through DPP."""
    import shutil
    import subprocess
    from motion_planning_baselines_amd import build
    build.build(verbose=False)
    objdump = '/opt/rocm/lib/llvm/bin/llvm-objdump'
    if not os.path.exists(objdump):
        pytest.skip('llvm-objdump not in this image')
    n_blocks = 0
    for src in ('mpb_stomp_fused', 'mpb_stomp_fused_hx'):
        obj = str(tmp_path / (src + '.o'))
        shutil.copy(os.path.join(build.CSRC, src + '.o'), obj)
        subprocess.run([objdump, '--offloading', obj], check=True, capture_output=True, cwd=str(tmp_path))
        co = [f for f in os.listdir(tmp_path) if f.startswith(src + '.o.') and 'gfx950' in f]
        assert len(co) == 1, co
        text = subprocess.run([objdump, '-d', str(tmp_path / co[0])], check=True, capture_output=True, text=True).stdout
        ins = [l.split('//')[0].strip() for l in text.splitlines() if l.startswith('\t')]
        for i, l in enumerate(ins):
            m = re.match(r'v_fmac_f32_dpp (v\d+), (v\d+), (v\d+) row_newbcast:(\d+) ', l)
            if not m:
                continue
            acc, a, _, k = m.group(1), m.group(2), m.group(3), int(m.group(4))
            assert acc != a, l
            if k == 0:
                n_blocks += 1
                assert ins[i - 1] == 's_nop 4', (src, ins[i - 3:i + 1])
            else:
                p = re.match(r'v_fmac_f32_dpp (v\d+), (v\d+), (v\d+) row_newbcast:(\d+) ', ins[i - 1])
                assert p and int(p.group(4)) == k - 1 and p.group(1) == acc and p.group(2) == a, (src, ins[i - 2:i + 1])
    assert n_blocks >= 20           # every instantiation of both kernels carries at least one block


def _big_scene(seed=0, n_sph=200, n_box=32):
    from motion_planning_baselines_amd import geometry as G
    return G.env_spheres_boxes_3d(seed, n_sph, n_box)


def test_list_grid_pack_check_flags_and_candidate_sets():
    """Geometry version 7 (round 6): a field with more than 63 obstacle spheres carries a LIST grid -- any number of candidates per
    cell, boxes culled like spheres.  pack_geometry builds it, mpb_geom_check accepts it (and refuses forged ranges), mpb_geom_flags
    reports ALL_LISTS (and not ALL_GRIDS: the compact-grid kernels must not take it), the persistent launcher takes it up to H = 64; and the
    candidate sets are CONSERVATIVE: for random query points every sphere / box within (margin + largest collision sphere) of the
    point is listed in the point's cell, found the way the kernels find it (cell = round(x / h) - K on the lattice)."""
    from motion_planning_baselines_amd import geometry as G, _lib
    robot, field = G.RobotPanda(), _big_scene()
    buf = G.pack_geometry(robot, field)
    h = G.header(buf)
    assert h['version'] == G.GEOM_VERSION_LIST and h['n_sph'] == 200 and h['n_box'] == 32
    _lib.geom_check(buf)
    fl = _lib.geom_flags(buf)
    assert (fl & G.GEOM_FLAG_ALL_LISTS) and not (fl & G.GEOM_FLAG_ALL_GRIDS) and (fl >> G.GEOM_FLAG_CELLS_SHIFT) == h['n_cells']
    lib = _lib.lib()
    assert lib.mpb_stomp_run_path(fl, 1 << 30, 128, 32, 64, 14) != 0 and lib.mpb_stomp_run_path(fl, 1 << 30, 128, 32, 48, 7) != 0
    assert lib.mpb_stomp_run_path(fl, 1 << 30, 128, 32, 128, 14) == 0           # two horizon chunks leave no LDS for the tables
    # a compact-grid scene is untouched; two fields: one needs the list grid -> both take it
    small = G.env_spheres_3d()
    assert G.header(G.pack_geometry(robot, small))['version'] == G.GEOM_VERSION
    two = G.pack_geometry(robot, [small, field])
    assert G.header(two)['version'] == G.GEOM_VERSION_LIST
    assert (_lib.geom_flags(two) & (G.GEOM_FLAG_ALL_LISTS | G.GEOM_FLAG_ALL_GRIDS)) == G.GEOM_FLAG_ALL_LISTS
    _lib.geom_check(two)
    # forged ranges are refused
    off_grid, n_cells, total = int(h['off_grid']), int(h['n_cells']), int(h['total'])
    off_cand = off_grid + (n_cells + G.GRID_PAD - 1) // G.GRID_PAD * G.GRID_PAD
    bad = buf.copy()
    w = bad.view(np.uint32)
    i = int(np.argmax(G.list_cell_fields(w[off_grid:off_grid + n_cells])[1]))
    w[off_grid + i] = (4 * (total - off_cand) - 1) | (5 << G.LIST_NSPH_SHIFT)   # range runs past the candidate bytes
    with pytest.raises(_lib.MPBError):
        _lib.geom_check(bad)
    bad = buf.copy()
    bad.view(np.uint8)[4 * off_cand] = 250                                       # a sphere index that does not exist
    w = bad.view(np.uint32)
    w[off_grid] = 0 | (1 << G.LIST_NSPH_SHIFT)
    with pytest.raises(_lib.MPBError):
        _lib.geom_check(bad)
    # ---- conservative candidate sets
    fs, rs = field.spec(), robot.spec()
    a_max = float(fs['margin']) + float(np.max(rs['link_radius']))
    inv = h['grid_inv'].astype(np.float64)
    dims = h['grid_dims'].astype(np.int64)
    lo = h['grid_lo'].astype(np.float64)
    K = np.rint(lo * inv + 0.5).astype(np.int64)
    words = buf.view(np.uint32)[off_grid:off_grid + n_cells]
    cand = buf.view(np.uint8)[4 * off_cand:]
    rng = np.random.RandomState(1)
    pts = rng.uniform(-1.0, 1.0, (4000, 3))
    sph, box = fs['spheres'].astype(np.float64), fs['boxes'].astype(np.float64)
    checked = 0
    for p in pts:
        cell = np.rint(p * inv).astype(np.int64) - K
        d_s = np.linalg.norm(p - sph[:, :3], axis=1) - sph[:, 3]
        q = np.abs(p - box[:, :3]) - box[:, 3:6]
        d_b = np.linalg.norm(np.maximum(q, 0), axis=1) + np.minimum(q.max(1), 0)
        near_s, near_b = set(np.nonzero(d_s < a_max)[0]), set(np.nonzero(d_b < a_max)[0])
        if np.any(cell < 0) or np.any(cell >= dims):
            assert not near_s and not near_b, 'a point outside the grid must be beyond every threshold'
            continue
        st, ns, nb, overflows = G.list_cell_fields(words[cell[0] + dims[0] * (cell[1] + dims[1] * cell[2])])
        if overflows:
            continue
        assert near_s <= set(cand[st:st + ns].tolist()), (p, near_s)
        assert near_b <= set(cand[st + ns:st + ns + nb].tolist()), (p, near_b)
        checked += bool(near_s or near_b)
    assert checked > 500


@pytest.mark.parametrize('offset_m', [0.0, 2500.0, 5000.0, 40000.0])
def test_scene_far_from_the_origin_packs_and_checks(offset_m):
    """mpb_geom_check accepted the grid origin only within an ABSOLUTE 1e-3 of a lattice point, which the fp32 rounding
    of lo and 1 / h exceeds beyond |K| ~ 16 700 cells (~2 km at C3's cell size) -- scenes that build_grid packs (it allows |K| + dims <
    65 536) were refused by the C check.  The tolerance now scales with |K|: whatever pack_geometry produces passes the check, with a
    grid where fp32 still resolves the cells and without one beyond."""
    from motion_planning_baselines_amd import geometry as G, _lib
    base = G.env_spheres_3d()
    sph = base.spheres.copy()
    sph[:, 0] += offset_m
    field = G.CollisionField(spheres=sph, margin=base.margin)
    buf = G.pack_geometry(G.RobotPanda(), field)
    _lib.geom_check(buf)                                   # must not raise
    n_cells = int(G.header(buf)['n_cells'])
    if offset_m <= 5000.0:
        assert n_cells > 0 and (_lib.geom_flags(buf) & G.GEOM_FLAG_ALL_GRIDS)
    else:
        assert n_cells == 0 and not (_lib.geom_flags(buf) & G.GEOM_FLAG_ALL_GRIDS)      # too far for the fp32 cell index: the exhaustive evaluators serve it


def test_geometry_layout_header_is_generated_from_geometry():
    """include/mpb_geom_layout.h (header word indices, limits, versions, kinds, cell-word fields, geom_flags: what the C side compiles
    in) is exactly what model_gen emits from the table in geometry.py."""
    from motion_planning_baselines_amd import model_gen
    assert model_gen.LAYOUT_HEADER == os.path.join(ROOT, 'include', 'mpb_geom_layout.h')
    assert open(model_gen.LAYOUT_HEADER).read() == model_gen.layout_header_text()
    assert not model_gen.stale_headers()


def test_rrt_layout_header_is_generated_from_the_table():
    """include/mpb_rrt_layout.h (statuses, stop reasons, the pool limit, magics, header sizes, header word indices: what the C side
    compiles in) is exactly what model_gen emits from the table in rrt_layout.py."""
    from motion_planning_baselines_amd import model_gen
    assert model_gen.RRT_LAYOUT_HEADER == os.path.join(ROOT, 'include', 'mpb_rrt_layout.h')
    assert open(model_gen.RRT_LAYOUT_HEADER).read() == model_gen.rrt_layout_header_text()
    assert model_gen.RRT_LAYOUT_HEADER in model_gen.generated_headers() and not model_gen.stale_headers()


def test_rrt_layout_public_numbers_are_pinned():
    """The RRT workspaces have ONE definition (the table in rrt_layout.py, emitted as include/mpb_rrt_layout.h): these literals -- the
    only ones outside that header -- are ABI 7's, and keep an edit of the table from renumbering a word unnoticed."""
    from motion_planning_baselines_amd import model_gen, ops, rrt_layout as R
    assert R.STATUS == ('RUNNING', 'FOUND', 'EXHAUSTED_ITERS', 'START_OR_GOAL_IN_COLLISION', 'POOL_EMPTY', 'TREE_FULL', 'PATH_TOO_LONG')
    assert (ops.RRT_RUNNING, ops.RRT_FOUND, ops.RRT_EXHAUSTED_ITERS, ops.RRT_START_OR_GOAL_IN_COLLISION, ops.RRT_POOL_EMPTY,
            ops.RRT_TREE_FULL, ops.RRT_PATH_TOO_LONG) == (0, 1, 2, 3, 4, 5, 6)
    assert R.STOP == ('RUNNING', 'ITERS', 'COST_CONVERGED', 'AFTER_SUCCESS', 'TREE_FULL', 'POOL_EMPTY')
    assert (ops.RRT_STOP_RUNNING, ops.RRT_STOP_ITERS, ops.RRT_STOP_COST_CONVERGED, ops.RRT_STOP_AFTER_SUCCESS, ops.RRT_STOP_TREE_FULL,
            ops.RRT_STOP_POOL_EMPTY) == (0, 1, 2, 3, 4, 5)
    assert ops.RRT_STATUS_NAMES == R.STATUS and ops.RRT_STOP_NAMES == R.STOP
    assert R.MAX_PRE_SAMPLES == 16384 and (R.POOL_INDEX_BITS, R.POOL_PER_WORD) == (16, 2)
    assert R.GLOBAL_WORDS == 16 and R.GLOBAL == ('magic', 'B', 'max_nodes', 'n_pre', 'D', 'Dp')
    assert set(R.KINDS) == {'connect', 'star'}
    assert (R.KINDS['connect'].magic, R.KINDS['connect'].hdr_words) == (0x52525443, 16)
    assert (R.KINDS['star'].magic, R.KINDS['star'].hdr_words) == (0x52525453, 32)
    assert R.header_index('connect') == dict(status=(0, 'i4', 1), iters=(1, 'i4', 1), counts=(2, 'i4', 2), swap=(4, 'i4', 1),
                                             pool_len=(5, 'i4', 1))
    star = ('status', 'iters', 'count', 'goal', 'pool_len', 'stop_reason', 'best_cost_iters', 'iters_after_first_success',
            'best_cost_eps', 'rewires', 'informed_rejections', 'first_cost', 'first_iter', 'first_count')
    assert R.header_index('star') == {name: (i, 'f4' if name in ('best_cost_eps', 'first_cost') else 'i4', 1)
                                      for i, name in enumerate(star)}
    assert [name for name, _, _ in R.KINDS['connect'].sections] == ['nodes', 'parents', 'pool']
    assert [name for name, _, _ in R.KINDS['star'].sections] == ['goal_q', 'nodes', 'parents', 'd', 'cost', 'cand', 'pool']
    # ... and the C side gets those very numbers
    lines = model_gen.rrt_layout_header_text().splitlines()
    for line in ('#define MPB_RRT_RUNNING 0', '#define MPB_RRT_PATH_TOO_LONG 6', '#define MPB_RRT_STOP_POOL_EMPTY 5',
                 '#define MPB_RRT_MAX_PRE_SAMPLES 16384', '#define MPB_RRT_GLOBAL_WORDS 16', '#define MPB_RRT_CONNECT_MAGIC 0x52525443',
                 '#define MPB_RRT_STAR_MAGIC 0x52525453', '#define MPB_RRT_CONNECT_HDR_WORDS 16', '#define MPB_RRT_STAR_HDR_WORDS 32',
                 '    MPB_RRTG_DP = 5,', '    MPB_RRTC_COUNTS = 2,', '    MPB_RRTC_SWAP = 4,', '    MPB_RRTC_POOL_LEN = 5,',
                 '    MPB_RRTS_STOP_REASON = 5,', '    MPB_RRTS_BEST_COST_EPS = 8,', '    MPB_RRTS_FIRST_COUNT = 13,'):
        assert line in lines, line


@pytest.mark.parametrize('kind', ('connect', 'star'))
def test_rrt_layout_total_equals_the_librarys(kind):
    """The offset arithmetic of the C side (rrt_layout / rrs_layout) is held to the table: for every shape of the sweep -- every Dp
    padding, odd and even pool counts, B = 0 -- the table's total is what mpb_rrt_*_workspace_bytes answers."""
    from motion_planning_baselines_amd import _lib, rrt_layout as R
    f = getattr(_lib.lib(), f'mpb_rrt_{kind}_workspace_bytes')
    for B in (0, 1, 5):
        for max_nodes in (2, 3, 101):
            for n_pre in (1, 2, 999, 16384):
                for D in range(1, 13):
                    assert 4 * R.offsets(kind, B, max_nodes, n_pre, D).total == f(B, max_nodes, n_pre, D), (B, max_nodes, n_pre, D)


def test_rrt_pool_limits_agree():
    from motion_planning_baselines_amd import _lib, ops, rrt_layout as R
    assert ops.RRT_MAX_PRE_SAMPLES == R.MAX_PRE_SAMPLES == 16384
    for kind in R.KINDS:
        f = getattr(_lib.lib(), f'mpb_rrt_{kind}_workspace_bytes')
        assert f(1, 2, 16384, 2) > 0 and f(1, 2, 16385, 2) == 0 and 'n_pre' in _lib.lib().mpb_last_error().decode()


def test_geometry_header_table_is_32_distinct_words():
    from motion_planning_baselines_amd import geometry as G
    names = [name for name, _, _ in G.HEADER_WORDS]
    assert sum(n for _, _, n in G.HEADER_WORDS) == 32 == G.GEOM_HEADER_WORDS
    assert G.HEADER_DTYPE.itemsize == 128 and len(set(names)) == len(names) and tuple(names) == G.HEADER_DTYPE.names
    assert {typ for _, typ, _ in G.HEADER_WORDS} <= {'i4', 'u4', 'f4'}
    # the record is a view: writes by name land in the buffer's own words, at the field's offset
    buf = np.zeros(100, np.float32)
    G.header(buf, 40)['n_sph'] = 9
    G.header(buf, 40)['grid_inv'] = [1.0, 2.0, 3.0]
    assert buf.view(np.int32)[46] == 9 and list(buf[63:66]) == [1.0, 2.0, 3.0] and np.count_nonzero(buf) == 4


def test_geometry_layout_public_numbers_are_pinned():
    """The packed-geometry layout has ONE definition (the table in geometry.py, emitted as include/mpb_geom_layout.h): these literals
    -- the only ones outside that header -- keep an edit of the table from renumbering the ABI unnoticed."""
    from motion_planning_baselines_amd import geometry as G, model_gen
    words = ['magic', 'version', 'kind', 'n_dof', 'n_tf', 'n_links', 'n_sph', 'n_box', 'margin', 'off_tf', 'off_links', 'off_sph', 'off_box',
             'total', 'off_cull', 'off_fs', 'off_grid', 'grid_dims', 'grid_dims', 'grid_dims', 'grid_lo', 'grid_lo', 'grid_lo', 'grid_inv',
             'grid_inv', 'grid_inv', 'n_cells', 'next', 'fscale', 'model', 'keep_mask', 'k_lin']
    assert [name for name, _, n in G.HEADER_WORDS for _ in range(n)] == words
    assert [G.HEADER_DTYPE.fields[name][1] // 4 for name in words] == [words.index(name) for name in words]
    floats = {'margin', 'grid_lo', 'grid_inv', 'fscale'}
    assert {name: typ for name, typ, _ in G.HEADER_WORDS} == {name: 'f4' if name in floats else 'u4' if name == 'keep_mask' else 'i4'
                                                               for name in words}
    assert (G.GEOM_FLAG_MODEL_MASK, G.GEOM_FLAG_ALL_GRIDS, G.GEOM_FLAG_POINT_SMALL, G.GEOM_FLAG_POINT, G.GEOM_FLAG_ONE_FIELD,
            G.GEOM_FLAG_ALL_LISTS, G.GEOM_FLAG_CELLS_SHIFT, G.GEOM_FLAG_CELLS_MASK) == (0xFF, 0x100, 0x200, 0x400, 0x1000, 0x2000, 16, 0x1FFF)
    assert (G.GEOM_MAGIC, G.GEOM_VERSION, G.GEOM_VERSION_LIST, G.KIND_POINT, G.KIND_CHAIN) == (0x4D504247, 6, 7, 0, 1)
    assert (G.MAX_FIELDS, G.MAX_DOF, G.GEOM_HEADER_WORDS) == (4, 12, 32)
    assert (G.GRID_MAX_CELLS, G.GRID_PAD, G.GRID_MAX_SPH) == (4096, 1024, 63)
    assert (G.LIST_MAX_SPH, G.LIST_MAX_BOX, G.LIST_MAX_CAND, G.LIST_CELL_MAX_SPH, G.LIST_CELL_MAX_BOX) == (255, 127, 16384, 126, 62)
    assert (G.GRID_SLOTS, G.GRID_SLOT_BITS, G.GRID_SLOT_MASK, G.GRID_OVERFLOW) == (4, 8, 0xFF, 0xFFFFFFFE)
    assert (G.LIST_START_MASK, G.LIST_NSPH_SHIFT, G.LIST_NSPH_MASK, G.LIST_NBOX_SHIFT, G.LIST_NBOX_MASK) == ((1 << 15) - 1, 15, (1 << 7) - 1, 22, (1 << 6) - 1)
    assert (G.LIST_OVERFLOW, G.LIST_RESERVED) == (1 << 31, 0b111 << 28)
    # ... and the C side gets those very numbers
    hdr = model_gen.layout_header_text()
    for i, name in enumerate(words):
        if words.index(name) == i:
            assert re.search(r'^    MPB_GW_%s = %d,$' % (name.upper(), i), hdr, flags=re.M), name
    for line in ('#define MPB_GEOM_FLAG_ALL_LISTS 0x2000', '#define MPB_GEOM_FLAG_CELLS_MASK 0x1FFF', '#define MPB_GRID_OVERFLOW 0xFFFFFFFEu',
                 '#define MPB_LIST_RESERVED 0x70000000u', '#define MPB_GRID_MAX_SPH 63', '#define MPB_MAX_DOF 12', '#define MPB_GEOM_VERSION_LIST 7'):
        assert line in hdr.splitlines(), line


def test_list_grid_cell_words_round_trip_by_name():
    """Every cell word of the packed crowded scene, decoded with the named fields, gives back the candidate set build_list_grid made for
    the cell; mpb_geom_check accepts the buffer and refuses it once one reserved bit of a cell word is set."""
    from motion_planning_baselines_amd import geometry as G, _lib
    robot, field = G.RobotPanda(), _big_scene()
    buf = G.pack_geometry(robot, field)
    h = G.header(buf)
    fs, rs = field.spec(), robot.spec()
    grid = G.build_list_grid(fs['spheres'].reshape(-1, 4), fs['boxes'].reshape(-1, 6), float(fs['margin']) + float(np.max(rs['link_radius'])))
    n_cells, off_grid = int(h['n_cells']), int(h['off_grid'])
    assert h['version'] == G.GEOM_VERSION_LIST and n_cells == grid['words'].size and list(h['grid_dims']) == list(grid['dims'])
    off_cand = off_grid + (n_cells + G.GRID_PAD - 1) // G.GRID_PAD * G.GRID_PAD
    words = buf.view(np.uint32)[off_grid:off_grid + n_cells]
    cand = buf.view(np.uint8)[4 * off_cand:4 * int(h['total'])]
    assert np.array_equal(words, grid['words']) and np.array_equal(cand, grid['cand'])
    assert not (words & G.LIST_RESERVED).any()
    # the sets the builder lists per cell, recomputed the way it defines them: spheres, then boxes, each in ascending index order,
    # ranges back to back from byte 0
    start, n_sph, n_box, overflows = G.list_cell_fields(words)
    assert not overflows.any() and n_sph.max() <= G.LIST_CELL_MAX_SPH and n_box.max() <= G.LIST_CELL_MAX_BOX
    ends = np.cumsum(n_sph.astype(np.int64) + n_box)
    assert np.array_equal(start, ends - n_sph - n_box) and ends[-1] == grid['stats']['cand_bytes'] <= cand.size
    assert int(n_sph.max()) == grid['stats']['max_sph'] and int(n_box.max()) == grid['stats']['max_box']
    for i in range(n_cells):
        s, b = cand[start[i]:start[i] + n_sph[i]], cand[start[i] + n_sph[i]:start[i] + n_sph[i] + n_box[i]]
        assert (np.diff(s.astype(np.int64)) > 0).all() and (np.diff(b.astype(np.int64)) > 0).all()
        assert (s < h['n_sph']).all() and (b < h['n_box']).all()
    _lib.geom_check(buf)
    reserved_bit = G.LIST_RESERVED & -G.LIST_RESERVED
    bad = buf.copy()
    bad.view(np.uint32)[off_grid + n_cells // 2] |= reserved_bit
    with pytest.raises(_lib.MPBError, match='list-grid cell out of range'):
        _lib.geom_check(bad)


def test_mppi_plan_of_every_tested_shape():
    """mpb_mppi_plan (the function mpb_mppi_step launches by) at n_cu = 256, for every shape of tests/mppi_path_cases.py and every
    MPPI shape the suite ran before it: noise path, waves, grid words and LDS bytes are pinned.  The tests that claim to cover a
    path assert it again on the device; this one says, without a GPU, which of them a retuned launcher has moved."""
    import mppi_path_cases as M
    from motion_planning_baselines_amd import ops
    from motion_planning_baselines_amd._lib import MPBError
    seen = set()
    shapes = [(k, cs[:5], M.Plan(*cs[5:9])) for k, cs in M.CASES.items()] + [('earlier', sh, pl) for sh, pl in M.EARLIER]
    for tag, (NP, S, T, c, scene), want in shapes:
        flags, has_geom = M.scene_flags(scene)
        for has_eps in (False, True):          # (injected or drawn: another instantiation, the same layout)
            got = ops.mppi_plan(flags if has_geom else None, NP, S, T, c, has_eps=has_eps, n_cu=256)
            assert tuple(got) == tuple(want), (tag, (NP, S, T, c, scene), 'plan moved: %s -> %s' % (tuple(want), tuple(got)))
        assert got.lds_bytes <= 160 * 1024
        seen.add((got.noise_mode, got.grid_words > 0))
    # between them: every noise path with the grid and without it
    assert seen == {(m, g) for m in (ops.MPPI_NOISE_GLOBAL, ops.MPPI_NOISE_LDS, ops.MPPI_NOISE_MATRIX) for g in (False, True)}
    # what a caller meets beyond the matrix path's reach: the per-lane LDS product while the transposed factor fits, then global memory
    assert ops.mppi_plan(None, 2, 16, 128, 1, n_cu=256).noise_mode == ops.MPPI_NOISE_LDS
    assert ops.mppi_plan(None, 2, 16, 128, 2, n_cu=256).noise_mode == ops.MPPI_NOISE_GLOBAL
    assert ops.mppi_plan(None, 2, 120, 64, 2, n_cu=256).noise_mode == ops.MPPI_NOISE_LDS
    # the code is the launcher's: a bad shape and a controls slab beyond LDS are refused as mpb_mppi_step refuses them
    with pytest.raises(MPBError, match='bad shape'):
        ops.mppi_plan(None, 2, 0, 64, 2, n_cu=256)
    with pytest.raises(MPBError, match='too large'):
        ops.mppi_plan(None, 2, 1024, 256, 4, n_cu=256)
    # two problems per CU: eight waves, and a grid that leaves room for the second workgroup
    assert ops.mppi_plan(None, 511, 32, 64, 2, n_cu=256).waves == 16 and ops.mppi_plan(None, 512, 32, 64, 2, n_cu=256).waves == 8
