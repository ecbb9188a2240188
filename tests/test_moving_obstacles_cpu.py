"""Host side of the moving-obstacle field (geometry.MovingObstacleField, pack_moving_obstacles, mpb_moving_check, the generated layout
header), what the compiler made of its kernels, and the conditions the GPU tests' inputs are held to -- by the fp64 oracle alone.  No GPU:
everything here runs on the build host."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT
import moving_obstacle_checks as M

NAMES = ('mpb_moving_check', 'mpb_moving_invalidate', 'mpb_moving_collision_eval', 'mpb_moving_collision_grad', 'mpb_moving_collision_check')


def test_layout_header_is_generated_and_the_public_numbers_are_pinned():
    from motion_planning_baselines_amd import _lib, build, geometry as G, model_gen, moving_layout as L, self_layout
    assert open(model_gen.MOVING_LAYOUT_HEADER).read() == model_gen.moving_layout_header_text()
    assert not model_gen.stale_headers()
    assert (L.MOVING_MAGIC, L.MOVING_VERSION, L.MOVING_HEADER_WORDS, L.MOVING_ROW_PAD, L.MOVING_ALIGN) == (0x4D50424D, 1, 16, 64, 4)
    assert (L.MOVING_MAX_ROWS, L.MOVING_MAX_SPHERES, L.MOVING_MAX_BOXES, L.MOVING_MAX_LINKS) == (1024, 64, 16, 64)
    assert L.MOVING_MAGIC.to_bytes(4, 'big') == b'MPBM'
    assert [n for n, _, _ in L.HEADER_WORDS] == ['magic', 'version', 'n_dof', 'n_tf', 'n_links', 'n_rows', 'n_spheres', 'n_boxes', 'margin',
                                                 'off_tf', 'off_links', 'off_radii', 'off_half', 'off_centres', 'total']
    text = open(model_gen.MOVING_LAYOUT_HEADER).read()
    for line in ('MPB_VW_MAGIC = 0,', 'MPB_VW_N_ROWS = 5,', 'MPB_VW_N_SPHERES = 6,', 'MPB_VW_MARGIN = 8,', 'MPB_VW_OFF_CENTRES = 13,', 'MPB_VW_TOTAL = 14,',
                 '#define MPB_MOVING_MAGIC 0x4D50424D', '#define MPB_MOVING_MAX_ROWS 1024', '#define MPB_MOVING_MAX_SPHERES 64',
                 '#define MPB_MOVING_MAX_BOXES 16', '#define MPB_MOVING_ROW_PAD 64'):
        assert line in text, line
    # the largest buffer stays a few MB; the other headers are untouched; the build depends on the new header
    assert 4 * L.offsets(13, 64, 1024, 64, 16)['total'] < 4 << 20
    assert (G.GEOM_HEADER_WORDS, G.GEOM_MAGIC, self_layout.SELF_MAGIC) == (32, 0x4D504247, 0x4D504253)
    assert 'mpb_moving_layout.h' in open(build.__file__).read() and 'mpb_moving_obstacles.hip' in build.SOURCES
    assert (_lib.lib().mpb_version() & 0xFFFF) == _lib.ABI_VERSION == 7                 # additive: the ABI version stays


def test_library_exports_the_entry_points():
    from motion_planning_baselines_amd import _lib
    h = _lib.lib()
    text = open(os.path.join(ROOT, 'include', 'mpb.h')).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(h, name), name
        assert f'int {name}(' in text, name


def test_rows_are_numpy_interp_per_component_with_held_ends():
    from motion_planning_baselines_amd import geometry as G
    for name in M.CASES:
        robot, field = M.case(name)
        for R in (1, 2, 7, 65):
            t = field.times(R)
            assert t.shape == (R,) and t[0] == field.t_start and (R == 1 or abs(t[-1] - field.t_end) < 1e-12)
            if R > 1:
                assert np.array_equal(t, field.t_start + np.arange(R) * (field.t_end - field.t_start) / (R - 1))
            sc, bc = field.rows(R)
            assert sc.shape == (R, field.n_spheres, 3) and bc.shape == (R, field.n_boxes, 3) and sc.dtype == bc.dtype == np.float64
            for got, keys in ((sc, field.sphere_centers), (bc, field.box_centers)):
                for o in range(keys.shape[1]):
                    for k in range(3):
                        assert np.array_equal(got[:, o, k], np.interp(t, field.t_key, keys[:, o, k]))
    robot, field = M.case('panda_sb')                        # the window overhangs: held at the first / last keyframe
    sc, bc = field.rows(130)
    t = field.times(130)
    before, after = t < field.t_key[0], t > field.t_key[-1]
    assert before.sum() > 3 and after.sum() > 3
    assert np.array_equal(sc[before], np.broadcast_to(field.sphere_centers[0], sc[before].shape))
    assert np.array_equal(bc[after], np.broadcast_to(field.box_centers[-1], bc[after].shape))
    planar = M.case('point2')[1]                             # two coordinates given: z = 0, the 2-D box half height
    assert not planar.sphere_centers[..., 2].any() and not planar.box_centers[..., 2].any() and np.all(planar.box_half[:, 2] == G.BOX_2D_HALF_Z)


def test_at_and_shifted_agree_with_rows():
    from motion_planning_baselines_amd import geometry as G
    robot, field = M.case('panda_sb')
    R = 9
    t = field.times(R)
    sc, bc = field.rows(R)
    for h in range(R):
        f = field.at(t[h])
        assert isinstance(f, G.CollisionField) and f.margin == field.margin
        assert np.array_equal(f.spheres, np.concatenate([sc[h], field.sphere_radii[:, None]], 1).astype(np.float32))     # rounded once
        assert np.array_equal(f.boxes, np.concatenate([bc[h], field.box_half], 1).astype(np.float32))
    dt = 0.37
    s = field.shifted(dt)
    assert (s.t_start, s.t_end) == (field.t_start + dt, field.t_end + dt) and np.array_equal(s.t_key, field.t_key)
    for a, b in zip(s.rows(R), field._centres(t + dt)):
        assert np.allclose(a, b, rtol=0, atol=1e-12)
    one = M.case('one')[1]                                   # K = 1: every time is the keyframe
    assert np.array_equal(one.at(-5.0).spheres, one.at(99.0).spheres) and np.array_equal(one.rows(3)[0][0], one.rows(3)[0][2])


def test_bad_arguments_raise_value_errors_that_name_the_argument():
    from motion_planning_baselines_amd import geometry as G
    c = np.zeros((2, 1, 3))
    ok = dict(t_key=[0.0, 1.0], sphere_centers=c, sphere_radii=[0.1])
    G.MovingObstacleField(**ok)
    for change, match in ((dict(t_key=[1.0, 1.0]), 't_key'), (dict(t_key=[]), 't_key'), (dict(t_key=[0.0, np.inf]), 't_key'),
                          (dict(sphere_centers=np.zeros((3, 1, 3))), 'sphere_centers'), (dict(sphere_centers=c + np.nan), 'sphere_centers'),
                          (dict(sphere_radii=[0.0]), 'sphere_radii'), (dict(sphere_radii=[0.1, 0.2]), 'sphere_radii'), (dict(sphere_radii=None), 'sphere_radii'),
                          (dict(box_centers=c), 'box_half'), (dict(box_centers=c, box_half=[[0.1, -0.1, 0.1]]), 'box_half'),
                          (dict(box_centers=np.zeros((2, 1, 4)), box_half=[[0.1, 0.1, 0.1]]), 'box_centers'),
                          (dict(sphere_centers=None, sphere_radii=None), 'at least one obstacle'), (dict(margin=np.nan), 'margin'),
                          (dict(t_start=np.nan), 't_start'), (dict(t_start=2.0, t_end=1.0), 't_end')):
        with pytest.raises(ValueError, match=match):
            G.MovingObstacleField(**{**ok, **change})
    field = G.MovingObstacleField(**ok)
    with pytest.raises(ValueError, match='MOVING_MAX_ROWS'):
        G.pack_moving_obstacles(G.RobotPanda(), field, 1025)
    with pytest.raises(ValueError, match='MOVING_MAX_SPHERES'):
        G.pack_moving_obstacles(G.RobotPanda(), G.MovingObstacleField([0.0], np.zeros((1, 65, 3)), np.full(65, 0.1)), 8)
    with pytest.raises(ValueError, match='MOVING_MAX_BOXES'):
        G.pack_moving_obstacles(G.RobotPanda(), G.MovingObstacleField([0.0], box_centers=np.zeros((1, 17, 3)), box_half=np.full((17, 3), 0.1)), 8)
    with pytest.raises(TypeError, match='MovingObstacleField'):
        G.pack_geometry(G.RobotPanda(), field)


def test_pack_round_trips_by_name_and_the_validator_rejects_corruption():
    from motion_planning_baselines_amd import _lib, geometry as G, moving_layout as L
    for name in M.CASES:
        robot, field = M.case(name)
        rs = robot.spec()
        for R in (1, 64, 65):
            buf = G.pack_moving_obstacles(robot, field, R)
            _lib.moving_check(buf)
            h, sec = L.header(buf), L.sections(buf)
            assert (int(h['magic']), int(h['version'])) == (L.MOVING_MAGIC, L.MOVING_VERSION)
            assert (int(h['n_dof']), int(h['n_tf']), int(h['n_links']), int(h['n_rows'])) == (robot.q_dim, rs['joint_tf'].shape[0], len(rs['link_radius']), R)
            assert (int(h['n_spheres']), int(h['n_boxes'])) == (field.n_spheres, field.n_boxes)
            assert float(h['margin']) == np.float32(field.margin) and int(h['total']) == buf.size and not h['reserved'].any()
            assert {k: int(h[k]) for k in L.offsets(0, 0, 1, 0, 0)} == L.offsets(int(h['n_tf']), int(h['n_links']), R, field.n_spheres, field.n_boxes)
            assert all(int(h[k]) % L.MOVING_ALIGN == 0 for k in ('off_tf', 'off_links', 'off_radii', 'off_half', 'off_centres'))
            assert np.array_equal(sec['joint_tf'], rs['joint_tf'].astype(np.float32)) and np.array_equal(sec['links'][:, 4], rs['link_radius'])
            assert np.array_equal(sec['links'][:, 1:4], rs['link_offset']) and not sec['links'][:, 5:].any()
            assert np.array_equal(sec['radii'], field.sphere_radii.astype(np.float32))
            assert np.array_equal(sec['half'][:, :3], field.box_half.astype(np.float32)) and not sec['half'][:, 3].any()
            sc, bc = field.rows(R)
            want = np.concatenate([sc, bc], 1).astype(np.float32).transpose(1, 2, 0)          # [obstacle][xyz][row], rounded once
            rp = L.rows_padded(R)
            assert sec['centres'].shape == (field.n_spheres + field.n_boxes, 3, rp) and rp % 64 == 0 and rp >= R
            assert np.array_equal(sec['centres'][:, :, :R], want)
            assert np.array_equal(sec['centres'][:, :, R:], np.broadcast_to(want[:, :, R - 1:R], sec['centres'][:, :, R:].shape))   # the last row repeated
    robot, field = M.case('panda_sb')
    buf = G.pack_moving_obstacles(robot, field, 65)
    geo = G.pack_geometry(robot, field.at(0.0), prune_static=False, use_model=False)           # the link rows are pack_geometry's, every link kept
    gh, sec = G.header(geo), L.sections(buf)
    assert np.array_equal(geo[int(gh['off_links']):int(gh['off_sph'])].reshape(-1, 8), sec['links'])
    assert np.array_equal(geo[int(gh['off_tf']):int(gh['off_links'])].reshape(-1, 3, 4), sec['joint_tf'])

    def refused(mutate, match):
        bad = buf.copy()
        mutate(bad)
        with pytest.raises(_lib.MPBError, match=match):
            _lib.moving_check(bad)
    oc = int(L.header(buf)['off_centres'])
    refused(lambda b: L.header(b).__setitem__('magic', L.MOVING_MAGIC ^ 1), 'magic')
    refused(lambda b: L.header(b).__setitem__('total', b.size + 4), 'total')
    refused(lambda b: L.header(b).__setitem__('n_spheres', L.MOVING_MAX_SPHERES + 1), 'MPB_MOVING_MAX_SPHERES')
    refused(lambda b: L.header(b).__setitem__('n_boxes', L.MOVING_MAX_BOXES + 1), 'MPB_MOVING_MAX_BOXES')
    refused(lambda b: L.header(b).__setitem__('n_rows', L.MOVING_MAX_ROWS + 1), 'MPB_MOVING_MAX_ROWS')
    refused(lambda b: b.__setitem__(oc + 7, np.nan), 'centre of obstacle 0 at row 7 is not finite')
    refused(lambda b: b.__setitem__(oc + 3 * 128 + 64, np.inf), 'centre of obstacle 1 at row 64 is not finite')
    refused(lambda b: b.__setitem__(oc + 100, 0.5), 'padding rows')
    refused(lambda b: b.__setitem__(int(L.header(b)['off_radii']), -1.0), 'radius')
    with pytest.raises(_lib.MPBError, match='total'):
        _lib.moving_check(np.concatenate([buf, np.zeros(4, np.float32)]))


@pytest.mark.parametrize('name', M.CASES)
def test_inputs_of_the_gpu_tests_meet_their_conditions(name):
    """By the fp64 oracle alone, per case and R >= 8: at most CAP of the rows in contact are excluded; at least a quarter of the rows are
    in contact; every obstacle is the nearest one of some active sphere; consecutive rows move every obstacle by at least 100 DELTA; the
    cost with the obstacles frozen at row 0 differs from the true cost by more than 1e-3 on at least half of the rows in contact (a
    kernel that ignores, shifts or wraps the row index cannot pass).  Two of these speak of motion: they are held where the definition
    lets the obstacles move -- between rows inside the keyframes' span (beyond it the centres are held), and not for the case of ONE
    keyframe, which is frozen by definition (its frozen cost IS its cost)."""
    robot, field = M.case(name)
    for R in M.rows_of(name):
        if R < 8:
            continue
        ic = M.input_conditions(name, R)
        print(f'{name} R={R}: excluded {ic.excluded:.4f}, in contact {ic.contact:.3f}, covered {ic.covered}, least step {ic.min_step:.2e} m, '
              f'differs from frozen {ic.frozen_differs:.3f}')
        assert ic.excluded <= M.CAP, (R, ic.excluded)
        assert ic.contact >= 0.25, (R, ic.contact)
        assert ic.covered, (R, ic.missing)
        if len(field.t_key) > 1:
            assert ic.min_step >= M.STEP, (R, ic.min_step)
            assert ic.frozen_differs >= 0.5, (R, ic.frozen_differs)
        else:
            assert ic.frozen_differs == 0.0


def test_moving_obstacle_kernels_have_no_scratch():
    """build() records what the compiler made of every kernel (csrc/kernel_resources.json): the three kernels keep q, dq and the sphere
    groups in registers -- 0 B of scratch, no vector spills, no LDS."""
    from motion_planning_baselines_amd import build
    build.build(verbose=False)
    res = json.load(open(build.RESOURCES))
    hits = {k: v for k, v in res.items() if k.startswith(('_Z18moving_cost_kernelILb0EE', '_Z18moving_cost_kernelILb1EE', '_Z19moving_check_kernel'))}
    assert len(hits) == 3, list(hits)
    for name, r in hits.items():
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['lds'] == 0, (name, r)
