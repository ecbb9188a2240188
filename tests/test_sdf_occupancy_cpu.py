"""Host side of the SDF grid from occupancy voxels (geometry.GridSDFField.from_occupancy, mpb_sdf_grid_build_occupancy): the oracle of
tests/sdf_occupancy_checks.py against all pairs, the derived bounds against the exact field, the argument checks, and what the compiler
made of the kernels.  No GPU: everything here runs on the build host."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

import sdf_occupancy_checks as O

INVALID = 1                                                      # include/mpb.h MPB_E_INVALID


@pytest.mark.parametrize('index', range(len(O.DIMS) * len(O.PATTERNS)))
def test_separable_transform_equals_all_pairs(index):
    """Every case the GPU tests use, the two multi-tile grids included, mask and complement: about a second for each of them at 27 720 nodes."""
    dims, name, occ = O.cases()[index]
    assert occ.shape == dims[::-1] and occ.dtype == np.uint8
    for mask in (occ, 1 - occ):
        d2 = O.edt_sq(mask)
        assert np.array_equal(d2, O.brute_sq(mask)), (dims, name)
        assert int(d2.min()) >= 1 and int(d2.max()) <= O.d2_none(mask.shape)
    assert np.array_equal(O.edt_sq(occ), O.edt_sq(1 - occ))       # D2 does not depend on which class is called solid; the sign does
    assert np.array_equal(O.case_d2(index), O.edt_sq(occ))


def test_patterns_are_what_the_gpu_tests_expect_of_them():
    seen = {}
    for dims, name, occ in O.cases():
        seen.setdefault(name, []).append((dims, occ))
        assert 0 < int(occ.sum()) < occ.size or name in ('bernoulli1', 'bernoulli99'), (dims, name)     # both classes present
    assert len(O.cases()) == len(O.DIMS) * len(O.PATTERNS) == 40
    for dims, occ in seen['checkerboard']:
        assert bool((O.edt_sq(occ) == 1).all())
    big = dict(seen['hollow_box'])[(40, 33, 21)]
    free_d2 = O.edt_to_sq(big != 0)
    assert big[10, 16, 20] == 0 and big[1, 16, 20] == 1 and free_d2[10, 16, 20] == 81          # free nodes enclosed by solid ones
    # all free / all occupied: D2_none everywhere, by both routes
    for shape in ((3, 4, 5), (1, 5, 7)):
        for v in (0, 1):
            m = np.full(shape, v, np.uint8)
            assert bool((O.edt_sq(m) == O.d2_none(shape)).all()) and bool((O.brute_sq(m) == O.d2_none(shape)).all())
    assert O.d2_none((3, 4, 5)) == 16 + 9 + 4 + 1 and O.d2_none((1, 5, 7)) == 36 + 16 + 1
    assert 3 * 1023 ** 2 + 1 < 2 ** 24


def test_oracle_nodes_are_three_fp32_roundings():
    cell = np.float32(0.03)
    occ = O.cases()[O.DIMS.index((5, 4, 3)) * len(O.PATTERNS)][2]
    v = O.oracle_nodes(occ, cell)
    d2 = O.edt_sq(occ)
    assert v.dtype == np.float32 and v.shape == occ.shape
    for idx in np.ndindex(occ.shape):
        root = np.float32(math.sqrt(float(d2[idx])))                 # fp64 root rounded to fp32 = the correctly rounded fp32 root
        want = cell * np.float32(root - np.float32(0.5))
        assert v[idx] == (-want if occ[idx] else want)
    # the fp32 root of every integer below 2^24 equals the rounded fp64 root: innocuous double rounding, on a sample across the range
    n = np.unique(np.concatenate([np.arange(1, 70000), np.random.RandomState(7).randint(1, 2 ** 24, 200000), [2 ** 24 - 1]]))
    assert np.array_equal(np.sqrt(n.astype(np.float32)), np.sqrt(n.astype(np.float64)).astype(np.float32))


def test_derived_bounds_against_the_exact_field():
    """env_spheres_3d() voxelised (sdf < 0 at the node) over [-1, 1]^3 at cell 0.05.  Every obstacle lies inside the grid and is a ball of
    radius >= (sqrt(3) / 2) cell, so: free nodes -(sqrt(3) - 1/2) cell <= sdf - v < cell / 2 (an occupied node has sdf < 0 and lies at
    distance cell sqrt(D2); a ball of radius (sqrt(3)/2) cell just under the nearest surface point contains a node); occupied nodes
    sdf - v > -cell / 2.  Slack 1e-6 cell for rounding."""
    import sdf_grid_checks as S
    from motion_planning_baselines_amd import geometry as G
    field = G.env_spheres_3d()
    cell, lo, dims = np.float32(0.05), (-1.0, -1.0, -1.0), (41, 41, 41)
    sph = np.asarray(field.spheres, np.float64)
    assert float(sph[:, 3].min()) >= math.sqrt(3.0) / 2.0 * float(cell)
    assert bool((np.abs(sph[:, :3]) + sph[:, 3:4] <= 1.0).all()) and len(field.boxes) == 0
    occ, sdf = O.voxelise(field, lo, dims, cell)
    v = O.oracle_nodes(occ, cell).astype(np.float64)
    c, slack = float(cell), 1e-6 * float(cell)
    diff = sdf - v
    free, solid = occ == 0, occ != 0
    print(f'free nodes: sdf - v in [{diff[free].min() / c:.3f}, {diff[free].max() / c:.3f}] cells; occupied: min {diff[solid].min() / c:.3f}, '
          f'{int(solid.sum())} of {occ.size} occupied')
    assert int(solid.sum()) > 100 and int(free.sum()) > 100
    assert float(diff[free].min()) >= -(math.sqrt(3.0) - 0.5) * c - slack and float(diff[free].max()) < 0.5 * c + slack
    assert float(diff[solid].min()) > -0.5 * c - slack


def test_from_occupancy_argument_checks():
    from motion_planning_baselines_amd import geometry as G
    occ = O.cases()[O.DIMS.index((5, 4, 3)) * len(O.PATTERNS)][2]
    f = G.GridSDFField.from_occupancy(occ, (-1.0, -0.5, 0.25), 0.1)
    assert f.dims == (5, 4, 3) and f.values is None and not f.planar and f.margin == 0.05 and f.cell == np.float32(0.1)
    assert isinstance(f.source, np.ndarray) and f.source.dtype == np.uint8 and np.array_equal(f.source, occ)
    assert np.array_equal(f.lo, np.asarray((-1.0, -0.5, 0.25), np.float32)) and f.inv_cell == np.float32(1.0) / np.float32(0.1)
    # any dtype is taken as != 0 and never becomes fp32; bool and uint8 stay what they are; a tensor stays a tensor
    for src in (occ.astype(np.float64) * -2.5, occ.astype(np.int32) * 7, occ.astype(bool), torch.from_numpy(occ), torch.from_numpy(occ).double() * 0.5,
                torch.from_numpy(occ).bool()):
        g = G.GridSDFField.from_occupancy(src, (0, 0, 0), 0.1, margin=0.02)
        assert g.dims == (5, 4, 3) and g.margin == 0.02 and g.values is None
        assert isinstance(g.source, torch.Tensor) == isinstance(src, torch.Tensor)
        got = g.source.numpy() if isinstance(g.source, torch.Tensor) else g.source
        assert got.dtype in (np.uint8, np.bool_) and got.itemsize == 1 and np.array_equal(got != 0, occ != 0)
    p = G.GridSDFField.from_occupancy(occ[0], (-1.0, -1.0), 0.1)                 # (ny, nx): planar, z = 0
    assert p.dims == (5, 4, 1) and p.planar and p.source.shape == (1, 4, 5) and float(p.lo[2]) == 0.0
    # rank
    for bad in (occ[0, 0], occ[None], np.zeros((), np.uint8), torch.from_numpy(occ)[0, 0]):
        with pytest.raises(ValueError, match='expected'):
            G.GridSDFField.from_occupancy(bad, (0, 0, 0), 0.1)
    # limits, by name
    with pytest.raises(ValueError, match='SDF_MAX_DIM'):
        G.GridSDFField.from_occupancy(np.zeros((2, 2, 1025), np.uint8), (0, 0, 0), 0.1)
    with pytest.raises(ValueError, match='SDF_MAX_DIM'):
        G.GridSDFField.from_occupancy(np.zeros((2, 1, 8), np.uint8), (0, 0, 0), 0.1)           # only nz may be 1
    with pytest.raises(ValueError, match='SDF_MAX_NODES'):
        G.GridSDFField.from_occupancy(np.zeros((129, 1024, 1024), bool), (0, 0, 0), 0.1)
    with pytest.raises(ValueError, match='cell'):
        G.GridSDFField.from_occupancy(occ, (0, 0, 0), 0.0)
    # planar against a chain: refused at pack time; the leading words of a 3-D one validate, and hold no node
    with pytest.raises(ValueError, match='planar'):
        G.pack_sdf_grid(G.RobotPanda(), p, with_nodes=False)
    from motion_planning_baselines_amd import _lib, sdf_layout as L
    head = G.pack_sdf_grid(G.RobotPanda(), f, with_nodes=False)
    h = L.header(head)
    assert tuple(h['dims']) == (5, 4, 3) and int(h['off_nodes']) == head.size and int(h['total']) == head.size + 60
    _lib.sdf_grid_check(head, n_words=int(h['total']))
    # from_field fields are what they were
    ff = G.GridSDFField.from_field(G.env_spheres_3d(), (-1, -1, -1), (1, 1, 1), 0.1)
    assert isinstance(ff.source, G.CollisionField) and ff.values is None and ff.dims == (21, 21, 21)


def test_ops_wrapper_refuses_before_anything_touches_the_device():
    import types
    from motion_planning_baselines_amd import ops
    sdf = types.SimpleNamespace(dims=(5, 4, 3), buf=torch.zeros(64), nodes=None)
    with pytest.raises(ValueError, match='must live on the GPU'):
        ops.sdf_grid_build_occupancy(torch.zeros(3, 4, 5, dtype=torch.uint8), sdf)
    with pytest.raises(ValueError, match='uint8 or bool'):
        ops.sdf_grid_build_occupancy(torch.zeros(3, 4, 5), sdf)
    with pytest.raises(ValueError, match='uint8 or bool'):
        ops.sdf_grid_build_occupancy(np.zeros((3, 4, 5), np.uint8), sdf)


def test_library_exports_the_symbol_and_refuses_null_pointers():
    """Nothing is launched: every pointer is null or a host address that is never dereferenced."""
    from conftest import ROOT
    from motion_planning_baselines_amd import _lib
    name = 'mpb_sdf_grid_build_occupancy'
    h = _lib.lib()
    assert name in _lib.SIGNATURES and hasattr(h, name) and len(_lib.SIGNATURES[name]) == 3
    assert f'int {name}(const unsigned char *occupancy, float *sdf, void *stream);' in open(f'{ROOT}/include/mpb.h').read()
    assert (h.mpb_version() & 0xFFFF) == _lib.ABI_VERSION == 7                                  # additive: the ABI version stays
    p = ctypes.c_void_p
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    a += (-a) % 16
    for occ, sdf in ((0, a), (a, 0), (0, 0)):
        assert h.mpb_sdf_grid_build_occupancy(p(occ), p(sdf), p(0)) == INVALID
        msg = h.mpb_last_error().decode()
        assert msg.startswith(name) and 'null pointer' in msg
    assert h.mpb_sdf_grid_build_occupancy(p(a), p(a + 4), p(0)) == INVALID and '16-byte aligned' in h.mpb_last_error().decode()
    assert h.mpb_sdf_grid_build_occupancy(p(0), p(a + 4), p(0)) == INVALID and 'null pointer' in h.mpb_last_error().decode()   # null first


def test_occupancy_kernels_have_no_scratch():
    """build() records what the compiler made of every kernel (csrc/kernel_resources.json): the transform's three kernels keep their
    state in registers and LDS -- nothing may go to scratch."""
    from motion_planning_baselines_amd import build
    build.build(verbose=False)
    res = json.load(open(build.RESOURCES))
    hits = {k: v for k, v in res.items() if 'occ_edt_' in k}
    assert len(hits) == 3, list(hits)                                # the x pass, the y / z pass, the y / z pass that writes fp32
    for name, r in hits.items():
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0, (name, r)
