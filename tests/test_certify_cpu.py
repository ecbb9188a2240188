"""Path certification on the CPU (no GPU): the generated layout header, the kernels' resources, the reach bound and the motion bound of
certify_layout.reach_table on three robots, and the fp64 restatement of the bisection (certify_checks.certify_ref) -- sound against a
dense resampling, COLLISION on the tunnelling scene the sampled validator passes, and below the cap of undecided paths on the
RRT-Connect paths of the rrt_panda_spheres golden."""
import json
import os

import numpy as np
import pytest
import torch

import certify_checks as C
from motion_planning_baselines_amd import certify_layout as CL

S = CL.CERT_DEFAULT_SLACK


def test_layout_header_is_generated_and_the_public_numbers_are_pinned():
    from motion_planning_baselines_amd import model_gen
    assert open(model_gen.CERTIFY_LAYOUT_HEADER).read() == model_gen.certify_layout_header_text()
    assert not model_gen.stale_headers()
    assert CL.STATUS == ('FREE', 'COLLISION', 'UNDECIDED_DEPTH', 'UNDECIDED_QUEUE', 'BAD_INPUT', 'BUFFER_CHANGED')
    assert CL.CERT_J_BITS + 12 == 32 and CL.CERT_MAX_ROWS == 4096 and CL.CERT_MAX_DEPTH == CL.CERT_J_BITS == 20
    assert CL.CERT_DEFAULT_SLACK == 32.0 * CL.CERT_E_MEASURED and 0.0 < CL.CERT_E_MEASURED < 1e-5
    # the midpoint parameter of the deepest level's last interval is exact in fp32
    j, d = 2 ** 20 - 1, 20
    assert float(np.float32(2 * j + 1) * np.float32(2.0 ** -(d + 1))) == (2 * j + 1) * 2.0 ** -(d + 1)


def test_abi_and_kernel_resources():
    """The entry points are declared, bound and exported (additive: the ABI version stays); both kernels have 0 B of scratch, no vector
    spills and no static LDS (the queue is dynamic LDS: its base stays 16-byte aligned)."""
    from motion_planning_baselines_amd import _lib, build, ops
    mpb_h = open(os.path.join(C.ROOT, 'include', 'mpb.h')).read()
    assert 'int mpb_clearance(' in mpb_h and 'int mpb_path_certify(' in mpb_h and '#include "mpb_certify_layout.h"' in mpb_h
    assert 'mpb_certify.hip' in build.SOURCES and (_lib.lib().mpb_version() & 0xFFFF) == _lib.ABI_VERSION == 7
    assert ops.CERT_STATUS_NAMES is CL.STATUS and ops.CERT_UNDECIDED_QUEUE == C.UNDECIDED_QUEUE and ops.CERT_DEFAULT_SLACK == S
    build.build(verbose=False)
    res = json.load(open(build.RESOURCES))
    for name in ('_Z16clearance_kernelPKfS0_PfPiii', '_Z19path_certify_kernel8CertArgs'):
        r = res[name]
        print(name, r)
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['lds'] == 0, (name, r)


@pytest.mark.parametrize('name', C.SCENES)
def test_reach_bound_and_motion_bound(name):
    """Over 10^4 uniform configurations |x_l(q) - origin_i(q)| <= rho_il for every joint i that moves sphere l (rho_il = 0 exactly
    where it does not); over 10^4 uniform pairs |x_l(b) - x_l(a)| <= Lambda_l(a, b).  No tolerance beyond 1e-12."""
    sc = C.scene(name)
    n = 10000
    q = sc.uniform(n, seed=1).astype(np.float64)
    if int(sc.rs['kind']) != 0:
        x, org = C.fk_with_origins(sc.rs, q)
        x_oracle = sc.ref(torch.float64)[0].fk_map_collision(torch.as_tensor(q)).numpy()
        assert np.abs(x - x_oracle).max() < 1e-12
        dist = np.linalg.norm(x[:, None, :, :] - org[:, :, None, :], axis=-1)              # (n, D, L)
        moves = np.arange(sc.D)[:, None] < np.asarray(sc.rs['link_frame'])[None, :]
        assert (sc.rho[~moves] == 0).all()
        worst = float((dist - sc.rho[None].astype(np.float64))[:, moves].max())
        print(f'{name}: max (|x_l - origin_i| - rho_il) = {worst:.3e}')
        assert worst <= 1e-12
    a, b = sc.uniform(n, seed=2).astype(np.float64), sc.uniform(n, seed=3).astype(np.float64)
    moved = np.linalg.norm(C.centres(sc, b) - C.centres(sc, a), axis=-1)
    lam = sc.motion_bound(a, b)
    print(f'{name}: max (|x_l(b) - x_l(a)| - Lambda_l) = {float((moved - lam).max()):.3e}, the tightest ratio {float((moved / lam).max()):.3f}')
    assert lam.shape == moved.shape and float((moved - lam).max()) <= 1e-12


@pytest.mark.parametrize('name', C.SCENES)
def test_restatement_is_sound(name):
    """Every FREE path's 2^(depth_max + 3)-point resampling per segment has fp64 clearance >= margin_cert - S, and every COLLISION
    witness has fp64 eta < -S; both answers occur."""
    sc = C.scene(name)
    paths = C.short_paths(sc, 24, 4, 0.1, seed=7)
    seen = {C.FREE: 0, C.COLLISION: 0}
    for p in paths:
        r = C.certify_ref(sc, p, S, max_depth=8)
        if r['status'] == C.FREE:
            dense = C.dense_clearance(sc, p, 2 ** (r['depth_max'] + 3))
            assert dense >= r['margin_cert'] - S and r['margin_cert'] > S, (dense, r)
        elif r['status'] == C.COLLISION:
            seg, t, link, eta = r['witness']
            e = sc.eta_links(C.witness_q(p, seg, t)[None])[0]
            assert e.min() == eta < -S and int(e.argmin()) == link
        seen[r['status']] = seen.get(r['status'], 0) + 1
    print(f'{name}: {seen}')
    assert seen[C.FREE] >= 1 and seen[C.COLLISION] >= 1


def test_tunnelling_scene_is_a_collision():
    """The sampled check at num_interpolation = 5 sees nothing; the restatement returns COLLISION with a witness inside the obstacle."""
    sc, path = C.tunnel_scene()
    t = np.arange(7) / 6.0
    sampled = sc.eta(path[0][None] + (path[1] - path[0])[None] * t[:, None])
    assert (sampled > 0).all()                                        # free at every sample the validator looks at
    r = C.certify_ref(sc, path, S)
    assert r['status'] == C.COLLISION
    seg, tw, link, eta = r['witness']
    q = C.witness_q(path, seg, tw)
    assert sc.eta(q[None])[0] < 0 and eta < 0 and seg == 0 and link == 0
    assert np.linalg.norm(q - [-0.25, 0.0]) < 0.01 + 0.005 + 0.005      # within obstacle radius + robot radius + margin of its centre


def test_depth_queue_and_edges():
    sc, path = C.tunnel_scene()
    # a segment that passes the obstacle at clearance 1e-4: y = the sum of the radii, the margin and 1e-4
    graze = np.array([[-0.5, 0.0201], [0.5, 0.0201]], np.float32)
    assert C.certify_ref(sc, graze, S, max_depth=4)['status'] == C.UNDECIDED_DEPTH
    r = C.certify_ref(sc, graze, S, max_depth=20)
    assert r['status'] == C.FREE and 0 < r['margin_cert'] <= 1.01e-4
    assert C.certify_ref(sc, graze, S, max_depth=20, max_intervals=1)['status'] == C.UNDECIDED_QUEUE
    far = np.array([[-0.5, 0.9], [-0.45, 0.9]], np.float32)
    r = C.certify_ref(sc, far, S, max_depth=0)
    assert r['status'] == C.FREE and r['depth_max'] == 0 and r['n_evals'] == 3
    assert C.certify_ref(sc, far[:1], S)['status'] == C.FREE and C.certify_ref(sc, far[:1], S)['depth_max'] == -1
    assert C.certify_ref(sc, np.array([[np.nan, 0.0], [0.0, 0.0]], np.float32), S)['status'] == C.BAD_INPUT
    assert C.certify_ref(sc, np.stack([far[0], far[0], far[1]]), S)['status'] == C.FREE      # a zero-length segment


def test_undecided_share_on_the_rrt_paths_stays_below_the_cap():
    """The fp64 restatement alone, at the default arguments, on the RRT-Connect paths of rrt_panda_spheres: the share of UNDECIDED
    paths is printed and stays below 10 %."""
    sc = C.scene('panda')
    res = [C.certify_ref(sc, p, S) for p in C.rrt_paths()]
    und = sum(r['status'] in (C.UNDECIDED_DEPTH, C.UNDECIDED_QUEUE) for r in res)
    print(f'rrt_panda_spheres: {len(res)} paths, statuses {[CL.STATUS[r["status"]] for r in res]}, depth_max {[r["depth_max"] for r in res]}, '
          f'undecided share {und / len(res):.3f}')
    assert und / len(res) < 0.10
