"""Host side of the SDF grid from triangle meshes (geometry.TriangleMesh, pack_mesh, GridSDFField.from_mesh, mpb_mesh_check,
mpb_sdf_grid_build_mesh): what TriangleMesh refuses, what pack_mesh promises, the validator on good and forged buffers, the argument
checks of the entry point, the generated header, what the compiler made of the kernel, and the definition restated in
tests/sdf_mesh_checks.py against closed forms and against its own culling rule.  No GPU: everything here runs on the build host."""
import ctypes
import json

import numpy as np
import pytest
import torch

import sdf_mesh_checks as K
from collision_kinks import CAP, DELTA

INVALID, UNSUPPORTED = 1, 2                                       # include/mpb.h MPB_E_INVALID, MPB_E_UNSUPPORTED
FIXTURES = ('box12', 'torus64', 'ico80', 'lprism20', 'twoboxes24', 'torus1024')


# ------------------------------------------------------------------------------------------------
# TriangleMesh, pack_mesh, mpb_mesh_check
# ------------------------------------------------------------------------------------------------
def test_triangle_mesh_refusals_name_the_rule():
    from motion_planning_baselines_amd import geometry as G, mesh_layout as M
    v, f = K.box(*K.BOX)
    m = G.TriangleMesh(v, f)
    assert m.n_tri == 12 and m.signed and m.vertices.dtype == np.float32 and m.faces.dtype == np.int64
    with pytest.raises(ValueError, match='closed'):                  # open
        G.TriangleMesh(v, f[:-1])
    flipped = f.copy()
    flipped[3] = flipped[3, ::-1]
    with pytest.raises(ValueError, match='consistently oriented'):   # one triangle flipped
        G.TriangleMesh(v, flipped)
    with pytest.raises(ValueError, match='inside out'):
        G.TriangleMesh(v, f[:, ::-1])
    with pytest.raises(ValueError, match='degenerate'):
        G.TriangleMesh(np.concatenate([v, [[0.0, 0.0, 9.0]]]), np.concatenate([f, [[0, 0, 8]]]), signed=False)
    thin = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0]])
    with pytest.raises(ValueError, match='degenerate'):              # collinear
        G.TriangleMesh(thin, [[0, 1, 2]], signed=False)
    for bad in (8, -1):
        g = f.copy()
        g[5, 1] = bad
        with pytest.raises(ValueError, match='out of range'):
            G.TriangleMesh(v, g)
    w = v.copy()
    w[2, 1] = np.nan
    with pytest.raises(ValueError, match='non-finite'):
        G.TriangleMesh(w, f)
    with pytest.raises(ValueError, match='thickness'):
        G.TriangleMesh(v, f, signed=True, thickness=0.01)
    with pytest.raises(ValueError, match='MESH_MAX_TRIS'):
        G.TriangleMesh(v, np.zeros((M.MESH_MAX_TRIS + 1, 3), np.int64), signed=False)
    assert M.MESH_MAX_TRIS == 2 ** 20
    # an open or flipped soup is fine unsigned
    assert G.TriangleMesh(v, f[:-1], signed=False, thickness=0.01).n_tri == 11 and G.TriangleMesh(v, flipped, signed=False).n_tri == 12
    for name in FIXTURES + ('ico1280', 'far', 'enclosing'):
        assert K.mesh(name).signed
    assert not K.mesh('open65').signed and K.mesh('open65').n_tri == 65 and not K.mesh('patch').signed


@pytest.mark.parametrize('name', FIXTURES + ('open65', 'patch', 'ico1280'))
def test_pack_mesh_properties(name):
    from motion_planning_baselines_amd import _lib, mesh_layout as M
    mesh, buf = K.mesh(name), K.packed(name)
    h, sec = M.header(buf), M.sections(buf)
    nt, ng = mesh.n_tri, -(-mesh.n_tri // 64)
    assert int(h['magic']) == M.MESH_MAGIC == 0x4D50424D and int(h['version']) == 1 and int(h['n_tri']) == nt and int(h['n_groups']) == ng
    assert int(h['off_tris']) == 16 and int(h['off_boxes']) == 16 + ng * 64 * 32 and int(h['total']) == buf.size == 16 + ng * 64 * 32 + ng * 8
    tris, boxes = sec['tris'], sec['boxes']
    # the records are the mesh's triangles, each once, and the padding repeats the last
    got = sorted(map(bytes, tris[:nt, 0:9]))
    assert got == sorted(map(bytes, mesh.vertices[mesh.faces].reshape(nt, 9)))
    assert np.array_equal(tris[nt:].view(np.int32), np.repeat(tris[nt - 1:nt], ng * 64 - nt, 0).view(np.int32))
    # every triangle inside its group's box, every box inside the header's
    corners = tris[:, 0:9].reshape(ng, 192, 3)
    assert bool((corners >= boxes[:, None, 0:3]).all()) and bool((corners <= boxes[:, None, 4:7]).all())
    assert bool((boxes[:, 0:3] >= h['bb_lo']).all()) and bool((boxes[:, 4:7] <= h['bb_hi']).all())
    # identical bits on every copy of an edge's and of a vertex's pseudonormal
    edges, verts = {}, {}
    for rec in tris[:nt]:
        p = [bytes(rec[0:3]), bytes(rec[3:6]), bytes(rec[6:9])]
        for e, (i, j) in enumerate(((0, 1), (1, 2), (2, 0))):
            edges.setdefault(frozenset((p[i], p[j])), set()).add(bytes(rec[12 + 3 * e:15 + 3 * e]))
        for c in range(3):
            verts.setdefault(p[c], set()).add(bytes(rec[21 + 3 * c:24 + 3 * c]))
    assert all(len(s) == 1 for s in edges.values()) and all(len(s) == 1 for s in verts.values())
    if mesh.signed:
        assert len(edges) == 3 * nt // 2
    n = tris[:nt, 9:12].astype(np.float64)
    assert float(np.abs(np.linalg.norm(n, axis=1) - 1.0).max()) < 1e-6
    _lib.mesh_check(buf)


@pytest.mark.parametrize('nt', [12, 63, 64, 65])
def test_pack_mesh_pads_the_last_group(nt):
    from motion_planning_baselines_amd import geometry as G, _lib, mesh_layout as M
    v, f = K.torus(8, 4, **K.TORUS)
    v2, f2 = K.box(*K.BOX)
    if nt == 12:
        mesh = G.TriangleMesh(v2, f2)
    elif nt == 65:
        mesh = K.mesh('open65')
    else:
        mesh = G.TriangleMesh(v, f[:nt], signed=nt == 64)
    buf = G.pack_mesh(mesh)
    h, tris = M.header(buf), M.sections(buf)['tris']
    assert int(h['n_tri']) == nt and int(h['n_groups']) == (2 if nt == 65 else 1) and tris.shape[0] == 64 * int(h['n_groups'])
    assert all(np.array_equal(t.view(np.int32), tris[nt - 1].view(np.int32)) for t in tris[nt:])
    _lib.mesh_check(buf)


def test_mesh_check_on_forged_buffers():
    from motion_planning_baselines_amd import _lib, mesh_layout as M
    good = K.packed('ico80').copy()
    _lib.mesh_check(good)
    h = _lib.lib()

    def refused(edit, what, code=INVALID):
        buf = good.copy()
        edit(buf, M.header(buf))
        rc = h.mpb_mesh_check(buf.ctypes.data_as(ctypes.c_void_p), int(buf.size))
        msg = h.mpb_last_error().decode()
        assert rc == code and msg.startswith('mpb_mesh_check') and what in msg, (rc, msg)
    refused(lambda b, hd: hd.__setitem__('magic', 0x4D504244), 'magic')                  # an SDF-grid buffer's magic
    refused(lambda b, hd: hd.__setitem__('version', 2), 'magic/version')
    refused(lambda b, hd: hd.__setitem__('n_tri', 0), 'MPB_MESH_MAX_TRIS', UNSUPPORTED)
    refused(lambda b, hd: hd.__setitem__('n_tri', M.MESH_MAX_TRIS + 1), 'MPB_MESH_MAX_TRIS', UNSUPPORTED)
    refused(lambda b, hd: hd.__setitem__('n_tri', 129), 'n_groups')
    refused(lambda b, hd: hd.__setitem__('n_groups', 3), 'n_groups')
    refused(lambda b, hd: hd.__setitem__('signed', 2), 'signed')
    refused(lambda b, hd: hd.__setitem__('thickness', -1.0), 'thickness')
    refused(lambda b, hd: hd.__setitem__('thickness', np.nan), 'thickness')
    refused(lambda b, hd: hd.__setitem__('off_tris', 32), 'offsets')
    refused(lambda b, hd: hd.__setitem__('off_boxes', int(hd['off_boxes']) + 8), 'offsets')
    refused(lambda b, hd: hd.__setitem__('total', int(hd['total']) + 1), 'offsets')
    refused(lambda b, hd: b.__setitem__(16 + 32 * 5 + 13, np.nan), 'not finite')
    refused(lambda b, hd: b.__setitem__(16 + 32 * 70 + 4, np.inf), 'not finite')
    refused(lambda b, hd: b.__setitem__(16 + 32 * 70 + 4, 50.0), 'outside the box of its group 1')
    refused(lambda b, hd: b.__setitem__(int(hd['off_boxes']) + 4, -50.0), 'box of group 0')
    refused(lambda b, hd: hd['bb_hi'].__setitem__(0, 0.0), "mesh's box")
    assert h.mpb_mesh_check(good.ctypes.data_as(ctypes.c_void_p), int(good.size) - 1) == INVALID
    assert h.mpb_mesh_check(ctypes.c_void_p(0), 100) == INVALID and h.mpb_mesh_check(good.ctypes.data_as(ctypes.c_void_p), 8) == INVALID


# ------------------------------------------------------------------------------------------------
# symbols, header, build
# ------------------------------------------------------------------------------------------------
def test_library_exports_the_symbols_and_refuses_null_and_misaligned_pointers():
    """Nothing is launched: every pointer is null or a host address that is never dereferenced."""
    from conftest import ROOT
    from motion_planning_baselines_amd import _lib
    h = _lib.lib()
    hdr = open(f'{ROOT}/include/mpb.h').read()
    assert 'int mpb_mesh_check(const float *mesh_host, int n_words);' in hdr
    assert 'int mpb_sdf_grid_build_mesh(const float *mesh, const float *pose_host, float *sdf, int flags, void *stream);' in hdr
    assert len(_lib.SIGNATURES['mpb_mesh_check']) == 2 and len(_lib.SIGNATURES['mpb_sdf_grid_build_mesh']) == 5
    assert hasattr(h, 'mpb_mesh_check') and hasattr(h, 'mpb_sdf_grid_build_mesh')
    assert (h.mpb_version() & 0xFFFF) == _lib.ABI_VERSION == 7                                  # additive: the ABI version stays
    p = ctypes.c_void_p
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    a += (-a) % 16
    name = 'mpb_sdf_grid_build_mesh'
    for mesh, sdf in ((0, a), (a, 0), (0, 0)):
        assert h.mpb_sdf_grid_build_mesh(p(mesh), p(0), p(sdf), 0, p(0)) == INVALID
        msg = h.mpb_last_error().decode()
        assert msg.startswith(name) and 'null pointer' in msg
    for mesh, sdf in ((a + 4, a), (a, a + 8)):
        assert h.mpb_sdf_grid_build_mesh(p(mesh), p(0), p(sdf), 0, p(0)) == INVALID and '16-byte aligned' in h.mpb_last_error().decode()
    assert h.mpb_sdf_grid_build_mesh(p(0), p(0), p(a + 4), 0xFF, p(0)) == INVALID and 'null pointer' in h.mpb_last_error().decode()    # null first


def test_generated_headers_are_up_to_date_and_carry_the_layout():
    from conftest import ROOT
    from motion_planning_baselines_amd import mesh_layout as M, model_gen
    assert model_gen.stale_headers() == []
    txt = open(f'{ROOT}/include/mpb_mesh_layout.h').read()
    assert txt == model_gen.mesh_layout_header_text()
    for line in ('#define MPB_MESH_MAGIC 0x4D50424D', '#define MPB_MESH_VERSION 1', '#define MPB_MESH_HEADER_WORDS 16', '#define MPB_MESH_MAX_TRIS 1048576',
                 '#define MPB_MESH_GROUP 64', '#define MPB_MESH_TRI_WORDS 32', '#define MPB_MESH_MIN 1', '#define MPB_MESH_NO_CULL 2', 'MPB_MW_TOTAL = 14,',
                 'MPB_TRI_N_FACE = 9,', 'MPB_FEAT_C = 6,'):
        assert line in txt, line
    assert M.HEADER_DTYPE.itemsize == 64 and '#include "mpb_mesh_layout.h"' in open(f'{ROOT}/include/mpb.h').read()


def test_mesh_kernel_has_no_scratch():
    from motion_planning_baselines_amd import build
    build.build(verbose=False)
    res = json.load(open(build.RESOURCES))
    hits = {k: v for k, v in res.items() if 'mesh_dist_kernel' in k}
    assert len(hits) == 1, list(hits)
    for name, r in hits.items():
        assert 'sdf_' not in name and 'occ_edt_' not in name
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0 and r['lds'] == 0, (name, r)


def test_from_mesh_argument_checks():
    from motion_planning_baselines_amd import geometry as G
    m = K.mesh('box12')
    f = G.GridSDFField.from_mesh(m, (-1, -1, -1), (1, 1, 1), 0.1)
    ff = G.GridSDFField.from_field(G.env_spheres_3d(), (-1, -1, -1), (1, 1, 1), 0.1)
    assert f.dims == ff.dims == (21, 21, 21) and f.values is None and f.margin == 0.05 and not f.planar
    assert isinstance(f.source, list) and f.source[0][0] is m and f.source[0][1] is None
    pose = K.pose_of((1, 2, 3), 0.4, (0.1, -0.2, 0.05))
    g = G.GridSDFField.from_mesh([(m, pose), (K.mesh('ico80'), None)], (-1, -1, -1), (1, 1, 1), 0.1, margin=0.02)
    assert len(g.source) == 2 and g.source[0][1].dtype == np.float32 and g.source[0][1].shape == (3, 4) and g.source[1][1] is None
    p = G.GridSDFField.from_mesh(m, (-1, -1), (1, 1), 0.1, planar=True)
    assert p.dims == (21, 21, 1) and p.planar and float(p.lo[2]) == 0.0
    assert G.GridSDFField.from_mesh(m, (-1, -1, 0.1), (1, 1, 0.1), 0.1, planar=True).dims == (21, 21, 1)
    bad = pose.copy()
    bad[:, 0] *= 1.001
    with pytest.raises(ValueError, match='orthonormal'):
        G.GridSDFField.from_mesh(m, (-1, -1, -1), (1, 1, 1), 0.1, pose=bad)
    mirror = pose.copy()
    mirror[:, 0] *= -1.0
    with pytest.raises(ValueError, match='determinant'):
        G.GridSDFField.from_mesh(m, (-1, -1, -1), (1, 1, 1), 0.1, pose=mirror)
    with pytest.raises(TypeError):
        G.GridSDFField.from_mesh(G.env_spheres_3d(), (-1, -1, -1), (1, 1, 1), 0.1)
    with pytest.raises(ValueError, match='SDF_MAX_DIM'):
        G.GridSDFField.from_mesh(m, (-1, -1, -1), (1, 1, 1), 0.001)
    with pytest.raises(ValueError, match='coordinates'):
        G.GridSDFField.from_mesh(m, (-1, -1), (1, 1), 0.1)


def test_ops_wrappers_refuse_before_anything_touches_the_device():
    from motion_planning_baselines_amd import ops
    with pytest.raises(TypeError):
        ops.sdf_grid_build_mesh(K.mesh('box12'), None)
    with pytest.raises(TypeError):
        ops.DeviceMesh(K.packed('box12'), 'cpu')


# ------------------------------------------------------------------------------------------------
# the restatement against closed forms, and against itself in fp32 and with culling
# ------------------------------------------------------------------------------------------------
def test_box_mesh_equals_the_analytic_box():
    g = K.GRID
    ref = K.reference('box12', g['dims'], g['lo'], g['cell'])
    lo, hi = (np.asarray(c, np.float32).astype(np.float64) for c in K.BOX)        # the box the packed fp32 vertices span
    want = K.box_sdf(ref.nodes.astype(np.float64), lo, hi)
    err = float(np.abs(ref.r64.v - want).max())
    inside = int((ref.r64.v < 0).sum())
    print(f'box: max |mesh - analytic| {err:.2e} on {want.size} nodes, {inside} inside; fp32 restatement against fp64 {ref.E32:.2e}')
    assert want.size == 33 * 29 * 21 and err <= 1e-15 and inside == int((want < 0).sum()) == 1248
    assert np.array_equal(ref.r32.v < 0, ref.r64.v < 0) and ref.E32 < 4e-7


def test_torus_mesh_has_the_analytic_torus_sign():
    g = K.GRID
    ref = K.reference('torus1024', g['dims'], g['lo'], g['cell'])
    want = K.torus_sdf(ref.nodes.astype(np.float64), **K.TORUS)
    off = np.abs(want) > 0.02
    wrong = int(((ref.r64.v < 0) != (want < 0))[off].sum())
    err = float(np.abs(ref.r64.v - want).max())
    print(f'torus: {wrong} sign errors on {int(off.sum())} nodes farther than 0.02 from the surface, {int((ref.r64.v < 0).sum())} inside, '
          f'max |mesh - analytic| {err:.2e} (the facets\' chord error); fp32 restatement against fp64 {ref.E32:.2e}')
    assert wrong == 0 and int(off.sum()) > 19000 and int((ref.r64.v < 0).sum()) > 1500 and err < 8e-3
    assert np.array_equal(ref.r32.v < 0, ref.r64.v < 0) and ref.E32 < 4e-7


@pytest.mark.parametrize('name', ['box12', 'torus1024'])
def test_excluded_share(name):
    g = K.GRID
    ref = K.reference(name, g['dims'], g['lo'], g['cell'])
    ex = K.excluded(ref.r64, DELTA)
    print(f'{name}: {int(ex.sum())} of {ex.size} nodes excluded, smallest normalised |s| {float(np.nanmin(ref.r64.s_norm)):.2f}')
    assert float(ex.mean()) <= CAP


COARSE = ((-0.71, -0.62, -0.43), 0.17)
CULL_CASES = [('ico80', (9, 7, 6)) + COARSE, ('lprism20', (6, 9, 5)) + COARSE, ('torus256', (9, 10, 6)) + COARSE, ('twoboxes24', (17, 13, 1)) + COARSE,
              ('far', (5, 5, 5)) + COARSE, ('enclosing', (5, 5, 5)) + COARSE, ('ico1280', (9, 8, 6), (0.1, -0.3, -0.1), 0.06)]


@pytest.mark.parametrize('name,dims,lo,cell', CULL_CASES)
def test_restated_culling_gives_the_winner_of_the_exhaustive_walk(name, dims, lo, cell):
    nodes = K.node_positions(dims, lo, cell)
    full = K.restate(K.packed(name), nodes, np.float32)
    winner, d2, visited, of = K.restate_culled(K.packed(name), nodes, K.slack_of(K.packed(name), nodes), K.wave_blocks(dims), np.float32)
    print(f'{name}: {visited} of {of} (wave, group) pairs visited')
    assert np.array_equal(winner, full.winner) and np.array_equal(d2.view(np.int32), full.d2.view(np.int32))
    assert sorted(np.unique(K.wave_blocks(dims)).tolist()) == list(range(dims[0] * dims[1] * dims[2]))
    assert visited < of or name != 'ico1280'                          # twenty groups: the rule does skip some
