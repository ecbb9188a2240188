"""mpb_path_shortcut without a device: the symbol and its binding, the host-side refusals in the order include/mpb.h gives them,
what the compiler made of the kernel, and the properties of the definition as tests/path_shortcut_checks.py restates it."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import path_shortcut_checks as K
from conftest import ROOT

NAME = 'mpb_path_shortcut'
INVALID, UNSUPPORTED = 1, 2


def test_symbol_is_exported_and_bound_and_the_abi_version_stays():
    from motion_planning_baselines_amd import _lib, ops
    h = _lib.lib()
    assert NAME in _lib.SIGNATURES and hasattr(h, NAME) and len(_lib.SIGNATURES[NAME]) == 17
    hdr = open(os.path.join(ROOT, 'include', 'mpb.h')).read()
    assert re.search(r'int mpb_path_shortcut\(const float \*paths_in, const int \*lengths_in, float \*paths_out, int \*lengths_out,', hdr)
    assert (h.mpb_version() & 0xFFFF) == _lib.ABI_VERSION == 7                                  # additive: the ABI version stays
    for i, code in enumerate(ops.SHORTCUT_CODES):
        assert f'#define MPB_SHORTCUT_{code} {i}\n' in hdr and getattr(ops, 'SHORTCUT_' + code) == i == getattr(K, code)
    assert f'#define MPB_SHORTCUT_LOG_INDEX_SHIFT {ops.SHORTCUT_LOG_INDEX_SHIFT}\n' in hdr and K.SHIFT == ops.SHORTCUT_LOG_INDEX_SHIFT
    assert f'#define MPB_SHORTCUT_MAX_ITERS {ops.SHORTCUT_MAX_ITERS}\n' in hdr
    src = open(os.path.join(ROOT, 'motion_planning_baselines_amd', 'csrc', 'mpb_path_shortcut.hip')).read()
    assert f'#define SC_TAG 0x{ops.SHORTCUT_PHILOX_TAG:08X}u' in src
    rrt = open(os.path.join(ROOT, 'include', 'mpb_rrt_layout.h')).read()          # a stream of its own: not the RRT kernels' tags
    assert ops.SHORTCUT_PHILOX_TAG not in {int(m, 16) for m in re.findall(r'MAGIC (0x[0-9A-Fa-f]+)', rrt)}


def _call(h, **kw):
    p = ctypes.c_void_p
    a = dict(paths_in=4096, lengths_in=4096, paths_out=4096, lengths_out=4096, stats=4096, log=0, geom=4096, geom_flags=0, draws=0,
             N=3, Lmax=8, D=7, n_iters=4, check_step=0.1, seed=0, problem_offset=0)
    a.update(kw)
    rc = h.mpb_path_shortcut(p(a['paths_in']), p(a['lengths_in']), p(a['paths_out']), p(a['lengths_out']), p(a['stats']), p(a['log']),
                             p(a['geom']), a['geom_flags'], p(a['draws']), a['N'], a['Lmax'], a['D'], a['n_iters'], a['check_step'],
                             a['seed'], a['problem_offset'], p(0))
    return rc, h.mpb_last_error().decode()


def test_refusals_that_need_no_device_in_the_stated_order():
    """Nothing is launched by any of these calls: every pointer is null or a host address that is never dereferenced.  Each refusal is
    tried together with every later one: the earlier check answers."""
    from motion_planning_baselines_amd import _lib
    h = _lib.lib()
    nan, inf = float('nan'), float('inf')
    ladder = [(dict(D=13), UNSUPPORTED, 'MPB_MAX_DOF'),
              (dict(N=-1), INVALID, 'bad shape'),
              (dict(Lmax=1), INVALID, 'Lmax'),
              (dict(n_iters=-1), INVALID, 'n_iters'),
              (dict(check_step=0.0), INVALID, 'check_step'),
              (dict(stats=0), INVALID, 'null pointer'),
              (dict(geom=4096 + 8), INVALID, '16-byte aligned')]
    for i, (bad, code, word) in enumerate(ladder):
        rc, msg = _call(h, **bad)
        assert rc == code and msg.startswith(NAME) and word in msg, (bad, rc, msg)
        later = {}
        for other, _, _ in ladder[i + 1:]:
            later.update(other)
            rc, msg = _call(h, **bad, **later)
            assert rc == code and word in msg, (bad, later, rc, msg)
    assert _call(h, D=0)[0] == INVALID
    # the limit of Lmax: 160 KB of LDS less the 17 408 bytes of the staged grid, over 4 * Dp bytes per row
    for D, most in ((2, 9152), (4, 9152), (5, 4576), (7, 4576), (8, 4576), (9, 3050), (12, 3050)):
        assert most == (160 * 1024 - 17408) // (4 * ((D + 3) & ~3))
        rc, msg = _call(h, D=D, Lmax=most + 1, stats=0)
        assert rc == INVALID and 'Lmax' in msg and str(most) in msg, (D, msg)
        rc, msg = _call(h, D=D, Lmax=most, stats=0)
        assert rc == INVALID and 'null pointer' in msg, (D, msg)
    assert 'n_iters' in _call(h, n_iters=(1 << 20) + 1)[1] and 'null pointer' in _call(h, n_iters=1 << 20, stats=0)[1]
    for step in (-0.1, -0.0, nan, inf, -inf):
        rc, msg = _call(h, check_step=step)
        assert rc == INVALID and 'check_step' in msg, (step, msg)
    for ptr in ('paths_in', 'lengths_in', 'paths_out', 'lengths_out', 'stats', 'geom'):
        rc, msg = _call(h, **{ptr: 0})
        assert rc == INVALID and 'null pointer' in msg, ptr
    assert _call(h, N=0) == (0, _call(h, N=0)[1])                           # an empty batch: MPB_OK, nothing launched ...
    assert _call(h, N=0, stats=0)[0] == INVALID                             # ... but only after every check above


def test_the_kernel_keeps_out_of_scratch_and_leaves_the_rrt_kernels_alone():
    """build() records what the compiler made of every kernel (csrc/kernel_resources.json): no instantiation of the new kernel may
    spill to scratch, and its static LDS is the staged grid alone (the path is dynamic LDS).  The RRT kernels share mpb_rrt.h with it:
    their figures are those of the commit before this kernel existed."""
    from motion_planning_baselines_amd import build
    build.build(verbose=False)
    res = json.load(open(build.RESOURCES))
    new = {k: v for k, v in res.items() if 'path_shortcut_kernel' in k}
    assert sorted(new) == ['_Z20path_shortcut_kernelILi%dELi%dEEv6ScArgs' % dm for dm in ((0, 0), (2, 0), (3, 0), (7, 0), (7, 1))], sorted(new)
    for name, r in new.items():
        print(name, r)
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['lds'] == 17408, (name, r)
    f = lambda lds, spill, vgprs: dict(lds=lds, sgpr_spill=spill, sgprs=106, vgprs=vgprs, scratch=0, vgpr_spill=0, agprs=0, occupancy=1)
    before = {'_Z15rrt_star_kernelILi0ELi0EEv7RrsArgs': f(50688, 235, 203), '_Z15rrt_star_kernelILi2ELi0EEv7RrsArgs': f(50688, 120, 169),
              '_Z15rrt_star_kernelILi7ELi0EEv7RrsArgs': f(50688, 142, 183), '_Z15rrt_star_kernelILi7ELi1EEv7RrsArgs': f(50688, 145, 196),
              '_Z18rrt_connect_kernelILi0ELi0EEv7RrtArgs': f(50176, 140, 229), '_Z18rrt_connect_kernelILi2ELi0EEv7RrtArgs': f(50176, 44, 164),
              '_Z18rrt_connect_kernelILi3ELi0EEv7RrtArgs': f(50176, 46, 169), '_Z18rrt_connect_kernelILi7ELi0EEv7RrtArgs': f(50176, 50, 187),
              '_Z18rrt_connect_kernelILi7ELi1EEv7RrtArgs': f(50176, 53, 200)}
    assert {k: v for k, v in res.items() if 'rrt_connect_kernel' in k or 'rrt_star_kernel' in k} == before


# ---- the definition's properties on the input sets -------------------------------------------------------------------------------
def _len64(path):
    return float(np.linalg.norm(np.diff(path.astype(np.float64), axis=0), axis=1).sum()) if len(path) > 1 else 0.0


@pytest.mark.parametrize('name', K.SETS)
def test_restatement_properties(name):
    ref = K.reference(name)
    p, r32, r64 = ref.p, ref.r32, ref.r64
    # the two restatements end with the same bits (the replay follows the fp32 log where fp64 cannot decide, and asserts elsewhere)
    assert np.array_equal(r32.paths.view(np.uint32), r64.paths.view(np.uint32)) and np.array_equal(r32.lengths, r64.lengths)
    assert np.array_equal(r32.stats.view(np.uint32), r64.stats.view(np.uint32))
    codes = r32.log & 0xFF
    counts = np.bincount(codes.ravel(), minlength=5)
    share = K.undecidable_share(r64.cands)
    print(f'{name}: N {p.N} Lmax {p.Lmax} n_iters {p.n_iters}: IDLE / SKIP / REJECT / OVERFLOW / ACCEPT {counts.tolist()}; '
          f'{len(r64.cands)} candidates tested, undecidable share {share:.4f}; points per candidate max {max(c.n_pts for c in r64.cands)}; '
          f'E32 max {max(c.E32 for c in r64.cands):.2e}; median length after / before '
          f'{np.nanmedian(r32.stats[:, 3] / np.where(r32.stats[:, 2] > 0, r32.stats[:, 2], np.nan)):.3f}')
    assert counts[K.REJECT] > 0 and counts[K.ACCEPT] > 0 and counts[K.SKIP] > 0            # every verdict that needs geometry occurs
    assert share <= 0.02                                                                   # the cap of the undecidable share
    assert r32.stats[:, 0].sum() == len(r64.cands) and r32.stats[:, 1].sum() == counts[K.ACCEPT]
    eps32 = 2.0 ** -23
    for b in range(p.N):
        L0, L1 = int(p.lengths[b]), int(r32.lengths[b])
        if L0 < 3:
            assert L1 == L0 and np.array_equal(r32.paths[b].view(np.uint32), p.paths[b].view(np.uint32)) and not codes[b].any()
            continue
        assert 2 <= L1 <= p.Lmax
        assert r32.paths[b, 0].tobytes() == p.paths[b, 0].tobytes() and r32.paths[b, L1 - 1].tobytes() == p.paths[b, L0 - 1].tobytes()
        assert not r32.paths[b, L1:].any()
        # A shortcut between two points ON the polyline never lengthens it (triangle inequality).  An inserted row is such a point
        # rounded: q_a + t (q_b - q_a) in fp32 is off by at most (2 + 2 + 3) eps32 M <= 8 eps32 M per coordinate (the sub, the mul,
        # the add; |q| <= M, t < 1), delta = 8 eps32 M sqrt(D) in norm; the new piece lo -> P1 -> P2 -> hi is at most 4 delta longer
        # than the exact one.  Over the accepted candidates, plus the rounding of the fp64 sums over L segments:
        M = float(np.abs(p.paths[b, :L0]).max())
        bound = 4.0 * float(r32.stats[b, 1]) * 8.0 * eps32 * M * np.sqrt(p.D) + max(L0, L1) * 2.0 ** -50 * 2.0 * M * np.sqrt(p.D)
        assert _len64(r32.paths[b, :L1]) <= _len64(p.paths[b, :L0]) + bound, (b, _len64(r32.paths[b, :L1]), _len64(p.paths[b, :L0]), bound)
        assert abs(float(r32.stats[b, 3]) - _len64(r32.paths[b, :L1])) <= 1e-5 * max(1.0, _len64(r32.paths[b, :L1]))
    for c in r64.cands:                                          # every accepted segment's dense points are free in fp64 within the bar
        if c.code == K.ACCEPT:
            assert c.m64_max <= c.bar, (c.b, c.it, c.m64_max, c.bar)
    if p.Lmax in p.lengths[:3]:
        print(f'{name}: OVERFLOW decisions {counts[K.OVERFLOW]}')


def test_fixed_cases_of_the_definition():
    """The edges the GPU test holds the kernel to, on the restatement alone: the zig-zag, the snap to nodes, one segment, overflow."""
    p = K.problem('pm2d_grid')
    zig = K.ZIGZAG
    free = K.hinge_max(p.rr64, p.rf64, torch.from_numpy(K.dense_points(zig[0], zig[-1], 50)).double())
    assert float(free.max()) < -1e-3                             # the straight line is in free space
    q = K.with_inputs(p, zig[None], [5], np.array([[[0.0, K.ONE_BELOW]]], np.float32))
    r = K.restate32(q)
    assert r.lengths.tolist() == [2] and r.log.tolist() == [[K.ACCEPT]]
    assert np.array_equal(r.paths[0, :2].view(np.uint32), zig[[0, -1]].view(np.uint32))
    # both draws on one segment; u = 0 twice; an existing edge (0 and 0.25: nodes 0 and 1)
    q = K.with_inputs(p, zig[None], [5], np.array([[[0.3, 0.4], [0.0, 0.0], [0.0, 0.25]]], np.float32))
    r = K.restate32(q)
    assert (r.log & 0xFF).tolist() == [[K.SKIP] * 3] and r.lengths.tolist() == [5]
    # u = 0: t == 0, node 0 serves and no row is inserted for it
    r = K.restate32(K.with_inputs(p, zig[None], [5], np.array([[[0.6, 0.0]]], np.float32)))
    assert (r.log & 0xFF).tolist() == [[K.ACCEPT]] and r.lengths.tolist() == [4]
    assert np.array_equal(r.paths[0, [0, 2, 3]].view(np.uint32), zig[[0, 3, 4]].view(np.uint32))
    # a corner cut on a full path: OVERFLOW; with one spare row: ACCEPT and one node more
    cut = np.array([[[0.1, 0.4]]], np.float32)
    assert (K.restate32(K.with_inputs(p, zig[None], [5], cut)).log & 0xFF).tolist() == [[K.OVERFLOW]]
    grown = K.restate32(K.with_inputs(p, np.concatenate([zig, zig[:1] * 0])[None], [5], cut))
    assert (grown.log & 0xFF).tolist() == [[K.ACCEPT]] and grown.lengths.tolist() == [6]
