"""The SDF grid from occupancy voxels by its definition alone (helper module; imported like sdf_grid_checks.py).

A node is the centre of a voxel of edge `cell`; occupancy[k, j, i] != 0 means that voxel is solid.  Integer part, exact: D2 of a free
node is the smallest squared index distance di^2 + dj^2 + dk^2 to an occupied node, D2 of an occupied node the smallest to a free
node, D2 = D2_none = (nx-1)^2 + (ny-1)^2 + (nz-1)^2 + 1 when the other class has no member.  Float part, bit-defined: the node value is
v = cell * (sqrt(D2) - 0.5) for a free node and -v for an occupied one, in fp32 as three separately rounded operations (numpy's fp32
sqrt is correctly rounded, as IEEE 754 asks of it; subtract; multiply), `cell` the fp32 number the header stores.  Nothing here runs
the code under test.

edt_sq is the separable transform (one pass per axis, every pass an exact min-plus with the parabola (i - j)^2) in int64; brute_sq is all
pairs; the CPU suite holds the two equal on the small cases below, so that the GPU tests may take edt_sq as their oracle.
"""
import functools

import numpy as np

BIG = np.int64(1) << 40                      # "no member of the other class yet": beyond every sum of three squares below 2^22

# (nx, ny, nz): below a wave; a line across a wave boundary on each axis; more than one tile; a general one
DIMS = ((7, 5, 1), (70, 3, 1), (5, 4, 3), (65, 2, 2), (2, 67, 2), (2, 2, 130), (257, 19, 5), (40, 33, 21))
PATTERNS = ('bernoulli30', 'bernoulli1', 'bernoulli99', 'checkerboard', 'hollow_box')


def d2_none(shape):
    nz, ny, nx = shape
    return (nx - 1) ** 2 + (ny - 1) ** 2 + (nz - 1) ** 2 + 1


def _min_plus_axis(f, axis):
    """g[i] = min_j f[j] + (i - j)^2 along `axis`, int64, exact."""
    f = np.moveaxis(f, axis, 0)
    n = f.shape[0]
    idx = np.arange(n, dtype=np.int64)
    out = np.empty_like(f)
    for i in range(n):
        w = ((idx - i) ** 2).reshape((n,) + (1,) * (f.ndim - 1))
        out[i] = (f + w).min(0)
    return np.moveaxis(out, 0, axis)


def edt_to_sq(target):
    """target (nz, ny, nx) bool -> int64 (nz, ny, nx): squared index distance of every node to the nearest True node (0 on it); >= BIG
    when there is none."""
    f = np.where(target, np.int64(0), BIG)
    for axis in (2, 1, 0):
        f = _min_plus_axis(f, axis)
    return f


def edt_sq(mask):
    """mask (nz, ny, nx), != 0 = occupied -> D2 (nz, ny, nx) int64 of the definition."""
    occ = np.asarray(mask) != 0
    d = np.where(occ, edt_to_sq(~occ), edt_to_sq(occ))
    return np.where(d >= BIG, np.int64(d2_none(occ.shape)), d)


def brute_sq(mask, rows=256):
    """The same by all pairs: every squared index distance between a free and an occupied node, formed ONCE -- its minimum along the
    occupied nodes is a free node's D2, its minimum along the free nodes an occupied node's -- in int32, `rows` free nodes at a time
    (27 720 nodes make 2 * 10^8 pairs: the whole matrix would not fit)."""
    occ = np.asarray(mask) != 0
    k, j, i = np.meshgrid(*(np.arange(n, dtype=np.int32) for n in occ.shape), indexing='ij')
    p = np.stack([k.ravel(), j.ravel(), i.ravel()], -1)
    o = occ.ravel()
    out = np.full(o.size, d2_none(occ.shape), np.int64)
    free, solid = p[~o], p[o]
    if len(free) and len(solid):
        d2_free = np.empty(len(free), np.int32)
        d2_solid = np.full(len(solid), np.iinfo(np.int32).max, np.int32)
        for a in range(0, len(free), rows):
            f = free[a:a + rows]
            d = (f[:, None, 0] - solid[None, :, 0]) ** 2
            d += (f[:, None, 1] - solid[None, :, 1]) ** 2
            d += (f[:, None, 2] - solid[None, :, 2]) ** 2
            d2_free[a:a + rows] = d.min(1)
            np.minimum(d2_solid, d.min(0), out=d2_solid)
        out[~o], out[o] = d2_free, d2_solid
    return out.reshape(occ.shape)


def nodes_from_d2(d2, occupancy, cell32):
    """D2 int -> node values fp32: +-cell * (sqrt(D2) - 0.5), three separately rounded fp32 operations."""
    d2 = np.asarray(d2)
    assert int(d2.max()) < 2 ** 24 and int(d2.min()) >= 1            # exact in fp32
    root = np.sqrt(d2.astype(np.float32))
    v = np.float32(cell32) * (root - np.float32(0.5))
    assert root.dtype == np.float32 and v.dtype == np.float32
    return np.where(np.asarray(occupancy) != 0, -v, v)


def oracle_nodes(occupancy, cell32):
    """occupancy (nz, ny, nx) or (ny, nx) -> node values (nz, ny, nx) fp32 of the definition."""
    occ = np.asarray(occupancy)
    occ = occ[None] if occ.ndim == 2 else occ
    return nodes_from_d2(edt_sq(occ), occ, cell32)


def pattern(name, dims, rng):
    """(nz, ny, nx) uint8"""
    nx, ny, nz = dims
    shape = (nz, ny, nx)
    if name.startswith('bernoulli'):
        return (rng.uniform(size=shape) < int(name[len('bernoulli'):]) / 100.0).astype(np.uint8)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing='ij')
    if name == 'checkerboard':                       # both signs in every line, the nearest other node one step away: D2 = 1 everywhere
        return ((i + j + k) % 2).astype(np.uint8)
    assert name == 'hollow_box'                      # a solid shell one node inside the boundary (on it along a short axis), free inside and outside

    def shell(a, n):
        lo, hi = (1, n - 2) if n >= 5 else (0, n - 1)
        return (a >= lo) & (a <= hi), ((a == lo) | (a == hi)) & (n > 1)
    (ix, ex), (iy, ey), (iz, ez) = shell(i, nx), shell(j, ny), shell(k, nz)
    return (ix & iy & iz & (ex | ey | ez)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def cases():
    """((dims, pattern name, occupancy uint8 (nz, ny, nx)), ...) drawn in this order from RandomState(7); treat as read-only."""
    rng = np.random.RandomState(7)
    return tuple((dims, name, pattern(name, dims, rng)) for dims in DIMS for name in PATTERNS)


@functools.lru_cache(maxsize=None)
def case_d2(index):
    """edt_sq of cases()[index], computed once and shared; treat as read-only."""
    return edt_sq(cases()[index][2])


def voxelise(field, lo, dims, cell):
    """occupancy (nz, ny, nx) uint8 of a product CollisionField: the exact signed distance (sdf_grid_checks.exact_sdf, fp64) is negative
    at the node; node positions from the fp32 lo and cell promoted to fp64, as the header holds them.  Returns (occupancy, sdf fp64)."""
    import sdf_grid_checks as S
    nx, ny, nz = dims
    lo3 = np.asarray(tuple(lo) + (0.0,) * (3 - len(lo)), np.float32)
    g = S.grid_data(np.zeros((nz, ny, nx), np.float32), lo3, np.float32(cell), np.float32(1.0) / np.float32(cell), S.F64)
    sdf = S.exact_sdf(field, S.node_positions(g), S.F64).numpy()
    return (sdf < 0).astype(np.uint8), sdf


def torus_occupancy(dims, lo, cell, R=0.25, r=0.08, centre=(0.55, 0.0, 0.55)):
    """A torus (axis along y through `centre`, major radius R, minor radius r: clear of a robot base at the origin) as an implicit function voxelised at the nodes: geometry the obstacle list
    cannot hold.  (nz, ny, nx) uint8."""
    nx, ny, nz = dims
    ax = [np.float64(np.float32(lo[a])) + np.arange(n) * np.float64(np.float32(cell)) - centre[a] for a, n in enumerate((nx, ny, nz))]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing='ij')
    return ((np.sqrt(x * x + z * z) - R) ** 2 + y * y < r * r).astype(np.uint8)
