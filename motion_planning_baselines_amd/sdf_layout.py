"""The packed SDF-grid buffer (geometry.pack_sdf_grid) in numbers: the ONLY definition of its magic, version, limits and header words.
model_gen.py emits include/mpb_sdf_layout.h from it (which include/mpb.h -- it says what each word means -- and csrc/mpb_sdf_grid.hip
include); tests/test_sdf_grid_cpu.py pins the public numbers as literals.  A buffer of its own, like the self-collision buffer: a grid
field has no obstacle list, and the geometry header's 32 words and its pinned numbers stay untouched.  No torch here: model_gen imports
it on a build host.
"""
import numpy as np

SDF_MAGIC = 0x4D504244       # 'MPBD'
SDF_VERSION = 1
SDF_HEADER_WORDS = 32
SDF_MAX_DIM = 1024           # nodes per axis
SDF_MAX_NODES = 1 << 27      # nodes of a grid (512 MB of fp32): every node index, and the buffer's word count, fits 32-bit arithmetic
SDF_MAX_LINKS = 256          # collision spheres of the robot
SDF_NODE_ALIGN = 4           # the node section starts at a multiple of this many words (16 bytes)

# The header: SDF_HEADER_WORDS 32-bit words, in this order -- (name, type, words); the rest is zero.  Ints are stored bit-exact in the
# fp32 buffer.  The sections follow in the order of their offsets:
#   joint_tf : n_tf x 12   (row-major 3x4)                                } the row formats of pack_geometry, EVERY link kept; a point
#   links    : n_links x 8 (frame:int, ox, oy, oz, radius, 0, 0, 0)       } robot has n_tf = 0 and one link row
#   nodes    : nx * ny * nz fp32 signed distances, node (i, j, k) at word (k * ny + j) * nx + i
HEADER_WORDS = (
    ('magic', 'i4', 1),        # SDF_MAGIC
    ('version', 'i4', 1),      # SDF_VERSION
    ('kind', 'i4', 1),         # geometry.KIND_POINT / KIND_CHAIN
    ('n_dof', 'i4', 1),
    ('n_tf', 'i4', 1),         # joint transforms: 0 (point robot) or n_dof + 1
    ('n_links', 'i4', 1),      # collision spheres of the robot
    ('margin', 'f4', 1),       # hinge margin
    ('dims', 'i4', 3),         # nx, ny, nz; nz == 1: planar (z ignored, bilinear)
    ('lo', 'f4', 3),           # position of node (0, 0, 0)
    ('cell', 'f4', 1),         # node spacing, one for all axes
    ('inv_cell', 'f4', 1),     # fl32(1 / cell): what the sampler multiplies by
    ('off_tf', 'i4', 1),       # word offsets of the sections from the header ...
    ('off_links', 'i4', 1),
    ('off_nodes', 'i4', 1),    # ... a multiple of SDF_NODE_ALIGN
    ('total', 'i4', 1),        # words of the buffer, header included
)
_named = sum(n for _, _, n in HEADER_WORDS)
HEADER_DTYPE = np.dtype([(name, typ, (n,)) if n > 1 else (name, typ) for name, typ, n in HEADER_WORDS]
                        + [('reserved', 'i4', (SDF_HEADER_WORDS - _named,))])
assert HEADER_DTYPE.itemsize == 4 * SDF_HEADER_WORDS

# what include/mpb_sdf_layout.h carries besides the word indices: (heading, C literal form, names), each as MPB_<name>
C_LAYOUT = (
    ('magic, version', '0x%X', ('SDF_MAGIC',)),
    (None, '%d', ('SDF_VERSION',)),
    ('limits', '%d', ('SDF_HEADER_WORDS', 'SDF_MAX_DIM', 'SDF_MAX_NODES', 'SDF_MAX_LINKS', 'SDF_NODE_ALIGN')),
)


def header(buf):
    """The header of a packed SDF-grid buffer as a numpy record over HEADER_WORDS: a VIEW (reads and writes by name go to the buffer's
    own words)."""
    words = np.asarray(buf)[:SDF_HEADER_WORDS]
    assert words.dtype.itemsize == 4 and words.size == SDF_HEADER_WORDS, 'a packed SDF-grid buffer is an array of 32-bit words'
    return words.view(HEADER_DTYPE)[0]


def sections(buf):
    """{name: view} of the sections of a packed buffer: joint_tf (n_tf, 3, 4) fp32, links (n_links, 8) fp32, nodes (nz, ny, nx) fp32."""
    h = header(buf)
    f = np.asarray(buf).view(np.float32)
    n_tf, n_links = int(h['n_tf']), int(h['n_links'])
    nx, ny, nz = (int(v) for v in h['dims'])
    o_tf, o_l, o_n = int(h['off_tf']), int(h['off_links']), int(h['off_nodes'])
    return dict(joint_tf=f[o_tf:o_tf + 12 * n_tf].reshape(n_tf, 3, 4), links=f[o_l:o_l + 8 * n_links].reshape(n_links, 8),
                nodes=f[o_n:o_n + nx * ny * nz].reshape(nz, ny, nx))
