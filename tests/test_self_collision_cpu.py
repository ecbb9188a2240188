"""Host side of the self-collision field (geometry.SelfCollisionField, pack_self_collision, mpb_self_check, the generated layout header)
and what the compiler made of its kernels.  No GPU: everything here runs on the build host."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
import self_collision_checks as S


def test_pair_builder_against_both_rules_rederived():
    """The default pair list is exactly: a < b with link_frame[b] - link_frame[a] >= gap, minus the pairs whose hinge is positive at every
    one of 1024 configurations drawn with RandomState(0) (fp64, the ORACLE's chain walk here, not the field's), sorted by (a, b)."""
    from motion_planning_baselines_amd import geometry as G
    robot = G.RobotPanda()
    rr = S.ref_robot(robot, S.F64)
    q = np.random.RandomState(0).uniform(robot.q_min_np.astype(np.float64), robot.q_max_np.astype(np.float64), (1024, robot.q_dim))
    x = rr.fk_map_collision(torch.from_numpy(q)).numpy()
    lf, r = robot.link_frame, robot.link_radius.astype(np.float64)
    counts = {}
    for gap, margin in ((3, 0.02), (3, 0.05), (2, 0.02), (1, 0.0)):
        want = []
        for a in range(len(lf)):
            for b in range(a + 1, len(lf)):
                if lf[b] - lf[a] < gap:
                    continue
                n = np.linalg.norm(x[:, a] - x[:, b], axis=-1)
                if np.all(margin + r[a] + r[b] - n > 0.0):
                    continue
                want.append((a, b))
        field = G.SelfCollisionField(robot, margin=margin, min_frame_gap=gap)
        assert field.pairs.tolist() == [list(p) for p in want], (gap, margin)
        counts[(gap, margin)] = len(want)
    # the counts DESIGN.md section 10 quotes
    assert counts == {(3, 0.02): 220, (3, 0.05): 219, (2, 0.02): 311, (1, 0.0): 382}


def test_panda_home_pose_is_free_and_bad_arguments_raise():
    from motion_planning_baselines_amd import geometry as G
    robot, field = S.case('panda')
    a, b, T = S.pair_data(field, S.F64)
    home = torch.tensor([S.PANDA_HOME], dtype=torch.float64)
    assert float(S.oracle_cost(S.ref_robot(robot, S.F64), a, b, T, home)) == 0.0
    n = len(robot.link_radius)
    for bad in ([(3, 3)], [(5, 2)], [(0, n)], [(-1, 4)], [(1, 9), (1, 9)]):
        with pytest.raises(ValueError):
            G.SelfCollisionField(robot, pairs=bad)
    assert G.SelfCollisionField(robot, pairs=[(1, 9), (0, 30)]).pairs.tolist() == [[1, 9], [0, 30]]     # an explicit list is kept as given
    with pytest.raises(ValueError, match='serial chains'):
        G.SelfCollisionField(G.RobotPointMass(2))


def test_pack_round_trips_by_name_and_the_validator_rejects_corruption():
    from motion_planning_baselines_amd import _lib, geometry as G, self_layout as L
    for name in S.CASES:
        robot, field = S.case(name)
        buf = G.pack_self_collision(robot, field)
        _lib.self_check(buf)
        h, sec = L.header(buf), L.sections(buf)
        rs = robot.spec()
        assert (int(h['magic']), int(h['version'])) == (L.SELF_MAGIC, L.SELF_VERSION)
        assert (int(h['n_dof']), int(h['n_tf']), int(h['n_links']), int(h['n_pairs'])) == (robot.q_dim, robot.q_dim + 1, len(rs['link_radius']), len(field.pairs))
        assert float(h['margin']) == np.float32(field.margin) and int(h['total']) == buf.size and not h['reserved'].any()
        assert np.array_equal(sec['joint_tf'], rs['joint_tf'].astype(np.float32))
        assert np.array_equal(sec['links'][:, 0].view(np.int32), rs['link_frame']) and np.array_equal(sec['links'][:, 1:4], rs['link_offset'])
        assert np.array_equal(sec['links'][:, 4], rs['link_radius']) and not sec['links'][:, 5:].any()
        assert np.array_equal(sec['pair_ab'], field.pairs)
        assert np.array_equal(sec['pair_T'], field.thresholds().astype(np.float32))         # rounded once from fp64
        # the link rows are pack_geometry's, every link kept
        geo = G.pack_geometry(robot, G.CollisionField(spheres=[[9.0, 9.0, 9.0, 0.1]]), prune_static=False, use_model=False)
        gh = G.header(geo)
        assert np.array_equal(geo[int(gh['off_links']):int(gh['off_sph'])].reshape(-1, 8), sec['links'])
        assert np.array_equal(geo[int(gh['off_tf']):int(gh['off_links'])].reshape(-1, 3, 4), sec['joint_tf'])
    robot, field = S.case('panda')
    buf = G.pack_self_collision(robot, field)

    def refused(mutate, match):
        bad = buf.copy()
        mutate(bad)
        with pytest.raises(_lib.MPBError, match=match):
            _lib.self_check(bad)
    refused(lambda b: L.header(b).__setitem__('magic', L.SELF_MAGIC ^ 1), 'magic')
    refused(lambda b: L.header(b).__setitem__('total', b.size + 2), 'total')
    off = int(L.header(buf)['off_pairs'])
    refused(lambda b: b.view(np.uint32).__setitem__(off, 3 | (31 << L.SELF_PAIR_B_SHIFT)), 'a < b < n_links')        # b == n_links
    refused(lambda b: b.view(np.uint32).__setitem__(off, 7 | (7 << L.SELF_PAIR_B_SHIFT)), 'a < b < n_links')
    with pytest.raises(_lib.MPBError, match='total'):
        _lib.self_check(np.concatenate([buf, np.zeros(4, np.float32)]))                                                    # n_words != total
    with pytest.raises(ValueError, match='another robot'):
        G.pack_self_collision(S.case('arm5')[0], field)


def test_layout_header_is_generated_and_the_public_numbers_are_pinned():
    from motion_planning_baselines_amd import geometry as G, model_gen, self_layout as L
    assert open(model_gen.SELF_LAYOUT_HEADER).read() == model_gen.self_layout_header_text()
    assert not model_gen.stale_headers()                     # mpb_geom_layout.h included: adding the self layout changed none of it
    assert (L.SELF_MAGIC, L.SELF_VERSION, L.SELF_HEADER_WORDS, L.SELF_MAX_LINKS, L.SELF_MAX_PAIRS) == (0x4D504253, 1, 16, 64, 2016)
    assert (L.SELF_PAIR_WORDS, L.SELF_PAIR_B_SHIFT, L.SELF_PAIR_A_MASK) == (2, 16, 0xFFFF)
    assert [n for n, _, _ in L.HEADER_WORDS] == ['magic', 'version', 'n_dof', 'n_tf', 'n_links', 'n_pairs', 'margin', 'off_tf', 'off_links',
                                                 'off_pairs', 'total']
    text = open(model_gen.SELF_LAYOUT_HEADER).read()
    for line in ('MPB_SW_MAGIC = 0,', 'MPB_SW_N_LINKS = 4,', 'MPB_SW_N_PAIRS = 5,', 'MPB_SW_OFF_PAIRS = 9,', 'MPB_SW_TOTAL = 10,',
                 '#define MPB_SELF_MAGIC 0x4D504253', '#define MPB_SELF_MAX_LINKS 64', '#define MPB_SELF_MAX_PAIRS 2016'):
        assert line in text, line
    assert (G.GEOM_HEADER_WORDS, G.GEOM_MAGIC) == (32, 0x4D504247)                # the geometry header is untouched
    with pytest.raises(ValueError, match='SELF_MAX_LINKS'):
        big = S.make_chain64()
        G.SelfCollisionField(G.RobotSerialChain(big.joint_tf, list(big.link_frame) + [13], list(big.link_offset) + [(0, 0, 0.1)],
                                                list(big.link_radius) + [0.03], q_min=[-2.5] * 12, q_max=[2.5] * 12))


def test_excluded_share_of_the_gpu_tests_inputs_stays_under_the_cap():
    """The classifier may exclude at most CAP of the waypoints in contact, on the inputs the GPU tests use (RandomState(11), uniform in
    the joint limits, rounded to fp32): 4096 Panda configurations with margin 0.02 -- and about 15 % of them are in contact."""
    robot, field = S.case('panda')
    assert field.margin == 0.02
    q = S.uniform_q(robot, 4096).double()
    a, b, T = S.pair_data(field, S.F64)
    cl = S.classify(S.ref_robot(robot, S.F64), a, b, T, q)
    n, nc, share = S.excluded_share(cl)
    print(f'panda: {n} of 4096 in contact, {n - nc} excluded ({share:.4f}); DELTA band {int((cl.min_abs < S.DELTA).sum())}, '
          f'smallest centre distance {float(cl.min_n.min()):.4f} m')
    assert 0.10 < n / 4096 < 0.20
    assert share <= S.CAP


def test_self_collision_kernels_have_no_scratch():
    """build() records what the compiler made of every kernel (csrc/kernel_resources.json): the self-collision kernels index their
    sphere centres through LDS precisely so that nothing goes to scratch memory."""
    from motion_planning_baselines_amd import build
    build.build(verbose=False)
    res = json.load(open(build.RESOURCES))
    hits = {k: v for k, v in res.items() if k.startswith(('_Z16self_cost_kernelILb0EE', '_Z16self_cost_kernelILb1EE', '_Z17self_check_kernel'))}
    assert len(hits) == 3, list(hits)
    for name, r in hits.items():
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0, (name, r)
        assert r['lds'] == 0, (name, r)                      # (all LDS is dynamic: sized at launch from n_links)
