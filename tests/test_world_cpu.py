"""The world predicate without a GPU: the share of the test inputs no fp64 oracle can decide (restatements alone, the inputs of
tests/test_gpu_world.py), what the compiler made of the world kernels, the additive C-ABI and the order of its refusals, and
DeviceWorld's robot-consistency check on host packing."""
import ctypes
import json

import numpy as np
import pytest

import path_shortcut_checks as K
import world_checks as W

INVALID, UNSUPPORTED, HIP = 1, 2, 3


# ---- the inputs: each part refuses some alone, and at most CAP of them lie within a bar of a surface ------------------------------------
@pytest.mark.parametrize('name', W.SCENES)
def test_excluded_share_and_no_part_is_vacuous(name):
    sc = W.scene(name)
    union = []
    for label, q in W.inputs(name).items():
        d = W.decide(sc, q)
        print(f'{name} {label}: n {len(q)}, in collision {d.flag64.mean():.3f}, per part {(d.m64 > 0).sum(0).tolist()}, E32 {d.E32.tolist()}, '
              f'excused share {d.excused.mean():.4f}')
        assert d.excused.mean() <= W.CAP
        assert 0 < d.flag64.sum() < len(q)                                            # both answers occur
        union.append(d.m64)
    m = np.concatenate(union)
    for k, part in enumerate(W.PARTS):
        if sc.parts64[k] is not None:
            alone = (m[:, k] > 0) & (np.delete(m, k, axis=1) <= 0).all(1)
            assert alone.sum() > 0, f'{name}: no input is refused by the {part} part alone'


@pytest.mark.parametrize('name', W.SCENES)
def test_shortcut_inputs_are_decidable_and_hold_a_reject_by_one_part_alone(name):
    """The shortcut input set under the restatements alone: the fp32 restatement's log replays in fp64 with at most CAP undecidable
    candidates, iteration 0 of path 0 is a REJECT the grid alone causes, of path 1 one the self part alone causes."""
    sc, p = W.scene(name), W.shortcut_problem(name)

    def judge(b, it, pts):
        hit = np.nonzero((W.hinges(sc, pts, '32') > 0).any(1))[0]
        return int(hit[0]) if len(hit) else -1
    paths, lengths, log, stats = K._walk(p, judge)
    r64 = K.replay64(p, log)
    share = K.undecidable_share(r64.cands)
    codes = np.bincount((log & 0xFF).ravel(), minlength=5)
    print(f'{name}: IDLE / SKIP / REJECT / OVERFLOW / ACCEPT {codes.tolist()}, {len(r64.cands)} candidates, undecidable share {share:.4f}')
    assert share <= W.CAP and codes[K.REJECT] > 0 and codes[K.ACCEPT] > 0
    for b, part in enumerate(p.only):
        assert (log[b, 0] & 0xFF) == K.REJECT
        assert W.why_rejected(sc, p, b, log) == part


@pytest.mark.parametrize('name', W.SCENES)
def test_trajectories_hold_one_only_the_grid_and_one_only_self_refuses(name):
    sc, t = W.scene(name), W.trajectories(name)
    N, H, D = t.shape
    al = np.linspace(0.0, 1.0, 6, endpoint=False)[:, None]
    for n, part in ((N - 2, 'sdf'), (N - 1, 'self')):
        dense = np.concatenate([t[n, h] + (t[n, h + 1].astype(np.float64) - t[n, h]) * al for h in range(H - 1)] + [t[n, -1:]]).astype(np.float32)
        m = W.hinges(sc, dense)
        k = W.PARTS.index(part)
        if sc.parts64[k] is None:
            assert (m <= 0).all()
            continue
        assert m[:, k].max() > W.MARGIN and (np.delete(m, k, axis=1) < 0).all() and (m[[0, -1]] < 0).all()


# ---- the compiler's figures -------------------------------------------------------------------------------------------------------
def test_kernel_resources():
    """Every world kernel stays out of scratch and spills no vector register; its static LDS is its plain kernel's (the self blocks are
    dynamic LDS, sized at launch).  The plain kernels' own figures are pinned by the tests that introduced them."""
    from motion_planning_baselines_amd import build
    build.build(verbose=False)
    res = json.load(open(build.RESOURCES))
    want = {'_Z17rrtc_world_kernelILi0ELi0EEv7RrtArgs9WorldArgs': 50176, '_Z17rrtc_world_kernelILi7ELi1EEv7RrtArgs9WorldArgs': 50176,
            '_Z22rrtc_world_init_kernelILi0EEvPiPKfS2_S2_iiii9WorldArgs': 17408, '_Z22rrtc_world_init_kernelILi1EEvPiPKfS2_S2_iiii9WorldArgs': 17408,
            '_Z21shortcut_world_kernelILi0ELi0EEv6ScArgs9WorldArgs': 17408, '_Z21shortcut_world_kernelILi7ELi1EEv6ScArgs9WorldArgs': 17408,
            '_Z23traj_stats_world_kernelILi0EEvPKfmS1_PiS2_PfPhiiii9WorldArgs': 17456, '_Z23traj_stats_world_kernelILi1EEvPKfmS1_PiS2_PfPhiiii9WorldArgs': 17456,
            '_Z18world_check_kernelILi0ELi0EEvPKfS1_9WorldArgsPhPfii': 17408, '_Z18world_check_kernelILi0ELi1EEvPKfS1_9WorldArgsPhPfii': 17408,
            '_Z18world_check_kernelILi1ELi0EEvPKfS1_9WorldArgsPhPfii': 17408, '_Z18world_check_kernelILi1ELi1EEvPKfS1_9WorldArgsPhPfii': 17408}
    new = {k: v for k, v in res.items() if 'world' in k}
    assert sorted(new) == sorted(want), sorted(new)
    for name, r in new.items():
        print(name, r)
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['lds'] == want[name] and r['agprs'] == 0, (name, r)


# ---- the C-ABI: additive, and the refusals in the stated order ---------------------------------------------------------------------------
A, MIS = 0x10000, 0x10004          # an aligned and a misaligned address; nothing below reads either


def _msg(h):
    m = h.mpb_last_error()
    return m.decode() if m else ''


def test_abi_symbols_and_refusal_order():
    """The five entries exist.  Each makes its old entry's refusals first and under its own name, then refuses a misaligned world buffer
    before it reads any header; an aligned one gets as far as the header read, which needs a device (MPB_E_HIP here).  An empty batch
    is MPB_OK with both buffers null, as the old entries have it.  (A buffer packed for another n_dof is refused after the header read:
    tests/test_gpu_world.py.)"""
    from motion_planning_baselines_amd import _lib
    h = _lib.lib()
    for sym in ('mpb_world_collision_check', 'mpb_rrt_connect_init_world', 'mpb_rrt_connect_run_world', 'mpb_path_shortcut_world',
                'mpb_traj_collision_stats_world'):
        assert sym in _lib.SIGNATURES and hasattr(h, sym)
    n_bytes = h.mpb_rrt_connect_workspace_bytes(1, 8, 4, 7)

    calls = {
        'mpb_world_collision_check': lambda sdfb, selfb, n=1, D=7, q=A: h.mpb_world_collision_check(q, A, 0, sdfb, selfb, A, 0, n, D, None),
        'mpb_rrt_connect_init_world': lambda sdfb, selfb, n=1, D=7, q=A: h.mpb_rrt_connect_init_world(
            A, h.mpb_rrt_connect_workspace_bytes(max(n, 1), 8, 4, min(D, 12)), q, A, A, 0, sdfb, selfb, n, 8, 4, D, None),
        'mpb_rrt_connect_run_world': lambda sdfb, selfb, n=1, D=7, q=A: h.mpb_rrt_connect_run_world(
            A, h.mpb_rrt_connect_workspace_bytes(max(n, 1), 8, 4, min(D, 12)), A, 0, sdfb, selfb, q, 0, None, A, A, A, n, 8, 4, D, 16, 0, 1, 1, 0.1, 1.0,
            0, 0, None),
        'mpb_path_shortcut_world': lambda sdfb, selfb, n=1, D=7, q=A: h.mpb_path_shortcut_world(q, A, A, A, A, None, A, 0, sdfb, selfb, None, n, 8, D,
                                                                                                4, 0.1, 0, 0, None),
        'mpb_traj_collision_stats_world': lambda sdfb, selfb, n=1, D=7, q=A: h.mpb_traj_collision_stats_world(q, D, A, 0, sdfb, selfb, 2, A, A, A, None,
                                                                                                              n, 4, D, None),
    }
    assert n_bytes > 0
    for sym, call in calls.items():
        assert call(None, None, n=0) == 0, sym                                       # an empty batch, both buffers null: MPB_OK
        assert call(MIS, None, D=13) == UNSUPPORTED and sym in _msg(h) and 'MPB_MAX_DOF' in _msg(h)     # the old refusals come first ...
        assert call(MIS, None, q=None) == INVALID and 'null pointer' in _msg(h) and sym in _msg(h)      # ... all of them
        for sdfb, selfb in ((MIS, None), (None, MIS), (A, MIS)):
            assert call(sdfb, selfb) == INVALID and '16-byte aligned' in _msg(h) and 'self-collision buffer' in _msg(h), (sym, _msg(h))
        for sdfb, selfb in ((A, None), (None, A)):                                   # aligned: the header read is next
            assert call(sdfb, selfb) == HIP and sym in _msg(h), (sym, _msg(h))


# ---- DeviceWorld: all parts packed for one robot ------------------------------------------------------------------------------------------
def test_world_parts_must_share_a_robot():
    from motion_planning_baselines_amd import geometry as G, ops
    from test_gpu_generic_dof import make_arm
    sc = W.scene('panda')
    geom = G.pack_geometry(sc.robot, sc.field)
    sdf = G.pack_sdf_grid(sc.robot, sc.grid, with_nodes=False)
    own = G.pack_self_collision(sc.robot, sc.self_field)
    ops.check_world_parts(geom)
    ops.check_world_parts(geom, sdf, own)
    ops.check_world_parts(geom, None, own)
    arm12, arm7 = make_arm(12), make_arm(7)
    with pytest.raises(ValueError, match='SDF-grid buffer was packed for a robot of n_dof = 12'):
        ops.check_world_parts(geom, G.pack_sdf_grid(arm12, sc.grid, with_nodes=False), own)
    with pytest.raises(ValueError, match='self-collision buffer was packed for a robot of n_dof = 12'):
        ops.check_world_parts(geom, sdf, G.pack_self_collision(arm12, G.SelfCollisionField(arm12)))
    with pytest.raises(ValueError, match='joint transforms differ'):                 # the same width, another chain
        ops.check_world_parts(geom, G.pack_sdf_grid(arm7, sc.grid, with_nodes=False))
    with pytest.raises(ValueError, match='joint transforms differ'):
        ops.check_world_parts(G.pack_geometry(arm7, sc.field), sdf, own)
    other = G.RobotSerialChain(sc.robot.spec()['joint_tf'], sc.robot.spec()['link_frame'], sc.robot.spec()['link_offset'],
                               np.asarray(sc.robot.spec()['link_radius']) * 1.5, q_min=sc.robot.q_min_np, q_max=sc.robot.q_max_np)
    with pytest.raises(ValueError, match='link'):                                    # the same chain, other collision spheres
        ops.check_world_parts(geom, G.pack_sdf_grid(other, sc.grid, with_nodes=False), own)
    pm = W.scene('pm2d')
    ops.check_world_parts(G.pack_geometry(pm.robot, pm.field), G.pack_sdf_grid(pm.robot, pm.grid, with_nodes=False))
    with pytest.raises(TypeError):
        ops.DeviceWorld(geom)                                                        # host words are no DeviceGeometry
