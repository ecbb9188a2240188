"""The packed moving-obstacle buffer (geometry.pack_moving_obstacles) in numbers: the ONLY definition of its magic, version, limits,
header words and section formats.  model_gen.py emits include/mpb_moving_layout.h from it (which include/mpb.h -- it says what each
word means -- and csrc/mpb_moving_obstacles.hip include); tests/test_moving_obstacles_cpu.py pins the public numbers as literals.  A
buffer of its own, like the self-collision and SDF-grid buffers: the obstacle centres carry a row (time) axis the geometry buffer has no
place for, and the geometry header's 32 words and its pinned numbers stay untouched.  No torch here: model_gen imports it on a build host.
"""
import numpy as np

MOVING_MAGIC = 0x4D50424D    # 'MPBM'
MOVING_VERSION = 1
MOVING_HEADER_WORDS = 16
MOVING_ROW_PAD = 64          # the row axis of the centre section is padded to a multiple of this (a wave's lanes): the last row repeated
MOVING_MAX_ROWS = 1024       # rows (time samples) of a trajectory
MOVING_MAX_SPHERES = 64      # moving spheres
MOVING_MAX_BOXES = 16        # moving boxes; with the spheres: (64 + 16) * 3 * 1024 words = 960 KB of centres at the most
MOVING_MAX_LINKS = 64        # collision spheres of the robot
MOVING_ALIGN = 4             # every section starts at a multiple of this many words (16 bytes)

# The header: MOVING_HEADER_WORDS 32-bit words, in this order -- (name, type, words); the rest is zero.  Ints are stored bit-exact in the
# fp32 buffer.  The sections follow in the order of their offsets, each at a multiple of MOVING_ALIGN words:
#   joint_tf : n_tf x 12   (row-major 3x4)                                } the row formats of pack_geometry, EVERY link kept; a point
#   links    : n_links x 8 (frame:int, ox, oy, oz, radius, 0, 0, 0)       } robot has n_tf = 0 and one link row
#   radii    : n_spheres fp32, zero-padded to a multiple of MOVING_ALIGN
#   half     : n_boxes x 4 (hx, hy, hz, 0)
#   centres  : (n_spheres + n_boxes) x 3 x rows_padded fp32 as [obstacle][x|y|z][row], spheres first, then boxes; rows_padded =
#              n_rows rounded up to a multiple of MOVING_ROW_PAD, the rows from n_rows on repeat row n_rows - 1
HEADER_WORDS = (
    ('magic', 'i4', 1),        # MOVING_MAGIC
    ('version', 'i4', 1),      # MOVING_VERSION
    ('n_dof', 'i4', 1),
    ('n_tf', 'i4', 1),         # joint transforms: 0 (point robot) or n_dof + 1
    ('n_links', 'i4', 1),      # collision spheres of the robot
    ('n_rows', 'i4', 1),       # rows of the trajectories the buffer serves: row h sees the obstacles at the field's time t_h
    ('n_spheres', 'i4', 1),
    ('n_boxes', 'i4', 1),
    ('margin', 'f4', 1),       # hinge margin
    ('off_tf', 'i4', 1),       # word offsets of the sections from the header ...
    ('off_links', 'i4', 1),
    ('off_radii', 'i4', 1),
    ('off_half', 'i4', 1),
    ('off_centres', 'i4', 1),
    ('total', 'i4', 1),        # words of the buffer, header included
)
_named = sum(n for _, _, n in HEADER_WORDS)
HEADER_DTYPE = np.dtype([(name, typ) for name, typ, _ in HEADER_WORDS] + [('reserved', 'i4', (MOVING_HEADER_WORDS - _named,))])
assert HEADER_DTYPE.itemsize == 4 * MOVING_HEADER_WORDS

# what include/mpb_moving_layout.h carries besides the word indices: (heading, C literal form, names), each as MPB_<name>
C_LAYOUT = (
    ('magic, version', '0x%X', ('MOVING_MAGIC',)),
    (None, '%d', ('MOVING_VERSION',)),
    ('limits', '%d', ('MOVING_HEADER_WORDS', 'MOVING_ROW_PAD', 'MOVING_MAX_ROWS', 'MOVING_MAX_SPHERES', 'MOVING_MAX_BOXES', 'MOVING_MAX_LINKS',
                      'MOVING_ALIGN')),
)


def _up(n, m):
    return (n + m - 1) // m * m


def rows_padded(n_rows):
    """Words of one component of one obstacle in the centre section."""
    return _up(int(n_rows), MOVING_ROW_PAD)


def offsets(n_tf, n_links, n_rows, n_spheres, n_boxes):
    """{off_tf, off_links, off_radii, off_half, off_centres, total} of a buffer with these counts: what the packer writes and the
    validator (mpb_moving_check) recomputes."""
    off_tf = MOVING_HEADER_WORDS
    off_links = off_tf + 12 * n_tf
    off_radii = off_links + 8 * n_links
    off_half = off_radii + _up(n_spheres, MOVING_ALIGN)
    off_centres = off_half + 4 * n_boxes
    total = off_centres + 3 * (n_spheres + n_boxes) * rows_padded(n_rows)
    return dict(off_tf=off_tf, off_links=off_links, off_radii=off_radii, off_half=off_half, off_centres=off_centres, total=total)


def header(buf):
    """The header of a packed moving-obstacle buffer as a numpy record over HEADER_WORDS: a VIEW (reads and writes by name go to the
    buffer's own words)."""
    words = np.asarray(buf)[:MOVING_HEADER_WORDS]
    assert words.dtype.itemsize == 4 and words.size == MOVING_HEADER_WORDS, 'a packed moving-obstacle buffer is an array of 32-bit words'
    return words.view(HEADER_DTYPE)[0]


def sections(buf):
    """{name: view} of the sections of a packed buffer: joint_tf (n_tf, 3, 4), links (n_links, 8), radii (n_spheres,), half (n_boxes, 4),
    centres (n_spheres + n_boxes, 3, rows_padded), all fp32."""
    h = header(buf)
    f = np.asarray(buf).view(np.float32)
    n_tf, n_links, n_rows, ns, nb = (int(h[k]) for k in ('n_tf', 'n_links', 'n_rows', 'n_spheres', 'n_boxes'))
    o_tf, o_l, o_r, o_h, o_c = (int(h[k]) for k in ('off_tf', 'off_links', 'off_radii', 'off_half', 'off_centres'))
    rp = rows_padded(n_rows)
    return dict(joint_tf=f[o_tf:o_tf + 12 * n_tf].reshape(n_tf, 3, 4), links=f[o_l:o_l + 8 * n_links].reshape(n_links, 8),
                radii=f[o_r:o_r + ns], half=f[o_h:o_h + 4 * nb].reshape(nb, 4),
                centres=f[o_c:o_c + 3 * (ns + nb) * rp].reshape(ns + nb, 3, rp))
