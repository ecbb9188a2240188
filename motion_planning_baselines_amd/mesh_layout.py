"""The packed triangle-mesh buffer (geometry.pack_mesh) in numbers: the ONLY definition of its magic, version, limits, header words and
record words.  model_gen.py emits include/mpb_mesh_layout.h from it (which include/mpb.h -- it says what each word means -- and
csrc/mpb_sdf_mesh.hip include).  A buffer of its own, like the SDF-grid buffer: a mesh is the SOURCE of a grid's node values
(mpb_sdf_grid_build_mesh), no kernel of a planner reads it.  No torch here: model_gen imports it on a build host.
"""
import numpy as np

MESH_MAGIC = 0x4D50424D      # 'MPBM'
MESH_VERSION = 1
MESH_HEADER_WORDS = 16
MESH_MAX_TRIS = 1 << 20      # triangles of a mesh: the padded record section stays below 2^25 words
MESH_GROUP = 64              # consecutive triangle records under one box
MESH_TRI_WORDS = 32          # one record: two 16-word uniform loads
MESH_BOX_WORDS = 8           # one group box: lo x y z, 0, hi x y z, 0 (one aligned 8-word uniform load)

# The header: MESH_HEADER_WORDS 32-bit words, in this order -- (name, type, words); the rest is zero.  Ints are stored bit-exact in the
# fp32 buffer.  The sections follow in the order of their offsets:
#   tris  : n_groups * MESH_GROUP records of MESH_TRI_WORDS words (TRI_WORDS below), sorted by the Morton code of the centroid; the
#           records beyond n_tri repeat record n_tri - 1
#   boxes : n_groups x MESH_BOX_WORDS, the fp32 box of the group's vertices (lo rounded down, hi rounded up)
HEADER_WORDS = (
    ('magic', 'i4', 1),        # MESH_MAGIC
    ('version', 'i4', 1),      # MESH_VERSION
    ('n_tri', 'i4', 1),        # triangles, 1..MESH_MAX_TRIS
    ('n_groups', 'i4', 1),     # ceil(n_tri / MESH_GROUP)
    ('signed', 'i4', 1),       # 1: closed and oriented, the node value carries the sign; 0: sqrt(d2) - thickness
    ('thickness', 'f4', 1),    # of an unsigned mesh (>= 0; 0 for a signed one)
    ('bb_lo', 'f4', 3),        # box of every group box
    ('bb_hi', 'f4', 3),
    ('off_tris', 'i4', 1),     # word offsets of the sections from the header: MESH_HEADER_WORDS ...
    ('off_boxes', 'i4', 1),    # ... off_tris + n_groups * MESH_GROUP * MESH_TRI_WORDS
    ('total', 'i4', 1),        # words of the buffer, header included
)
_named = sum(n for _, _, n in HEADER_WORDS)
HEADER_DTYPE = np.dtype([(name, typ, (n,)) if n > 1 else (name, typ) for name, typ, n in HEADER_WORDS]
                        + [('reserved', 'i4', (MESH_HEADER_WORDS - _named,))])
assert HEADER_DTYPE.itemsize == 4 * MESH_HEADER_WORDS

# one triangle record -- (name, words): vertices a, b, c (counter-clockwise seen from outside), the unit face normal, the pseudonormals
# of the edges ab, bc, ca (sum of the two faces' unit normals) and of the vertices a, b, c (angle-weighted sum of the faces' normals);
# the normals in the order of the feature codes FEATURES
TRI_WORDS = (('a', 3), ('b', 3), ('c', 3), ('n_face', 3), ('n_ab', 3), ('n_bc', 3), ('n_ca', 3), ('n_a', 3), ('n_b', 3), ('n_c', 3), ('pad', 2))
assert sum(n for _, n in TRI_WORDS) == MESH_TRI_WORDS
FEATURES = ('face', 'ab', 'bc', 'ca', 'a', 'b', 'c')       # feature f has its normal at word TRI_N_FACE + 3 * f of the record

# flags of mpb_sdf_grid_build_mesh
MESH_MIN = 1                 # node = min(what it holds, v)
MESH_NO_CULL = 2             # visit every group

# what include/mpb_mesh_layout.h carries besides the word indices: (heading, C literal form, names), each as MPB_<name>
C_LAYOUT = (
    ('magic, version', '0x%X', ('MESH_MAGIC',)),
    (None, '%d', ('MESH_VERSION',)),
    ('limits and strides', '%d', ('MESH_HEADER_WORDS', 'MESH_MAX_TRIS', 'MESH_GROUP', 'MESH_TRI_WORDS', 'MESH_BOX_WORDS')),
    ('flags of mpb_sdf_grid_build_mesh', '%d', ('MESH_MIN', 'MESH_NO_CULL')),
)


def header(buf):
    """The header of a packed mesh buffer as a numpy record over HEADER_WORDS: a VIEW."""
    words = np.asarray(buf)[:MESH_HEADER_WORDS]
    assert words.dtype.itemsize == 4 and words.size == MESH_HEADER_WORDS, 'a packed mesh buffer is an array of 32-bit words'
    return words.view(HEADER_DTYPE)[0]


def tri_index():
    """{name: first word of the field in a record}"""
    out, w = {}, 0
    for name, n in TRI_WORDS:
        out[name] = w
        w += n
    return out


def sections(buf):
    """{name: view} of the sections of a packed buffer: tris (n_groups * MESH_GROUP, MESH_TRI_WORDS) fp32, boxes (n_groups, MESH_BOX_WORDS)."""
    h = header(buf)
    f = np.asarray(buf).view(np.float32)
    ng, o_t, o_b = int(h['n_groups']), int(h['off_tris']), int(h['off_boxes'])
    return dict(tris=f[o_t:o_t + ng * MESH_GROUP * MESH_TRI_WORDS].reshape(ng * MESH_GROUP, MESH_TRI_WORDS),
                boxes=f[o_b:o_b + ng * MESH_BOX_WORDS].reshape(ng, MESH_BOX_WORDS))
