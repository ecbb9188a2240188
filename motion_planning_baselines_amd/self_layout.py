"""The packed self-collision buffer (geometry.pack_self_collision) in numbers: the ONLY definition of its magic, version, limits, header
words and pair word.  model_gen.py emits include/mpb_self_layout.h from it (which include/mpb.h -- it says what each word means -- and
csrc/mpb_self_collision.hip include); tests/test_self_collision_cpu.py pins the public numbers as literals.  A buffer of its own, not a
section of the geometry buffer: a self field has no obstacles, and the geometry header's 32 words and its pinned numbers stay untouched.
No torch here: model_gen imports it on a build host.
"""
import numpy as np

SELF_MAGIC = 0x4D504253      # 'MPBS'
SELF_VERSION = 1
SELF_HEADER_WORDS = 16
SELF_MAX_LINKS = 64          # collision spheres: the kernels keep every centre in LDS as [link][xyz][lane], 48 KB per wave at 64 (96 KB with gradients)
SELF_MAX_PAIRS = 2016        # 64 * 63 / 2
SELF_PAIR_WORDS = 2          # a pair: a | b << SELF_PAIR_B_SHIFT (indices into the link table, a < b), then T_ab = margin + r_a + r_b as fp32
SELF_PAIR_B_SHIFT = 16
SELF_PAIR_A_MASK = (1 << SELF_PAIR_B_SHIFT) - 1

# The header: SELF_HEADER_WORDS 32-bit words, in this order -- (name, type, words); the rest is zero.  Ints are stored bit-exact in the
# fp32 buffer.  The sections follow in the order of their offsets:
#   joint_tf : n_tf x 12   (row-major 3x4)                                } the row formats of pack_geometry; ALL links are kept: the pair
#   links    : n_links x 8 (frame:int, ox, oy, oz, radius, 0, 0, 0)       } indices are positions in the robot's table
#   pairs    : n_pairs x SELF_PAIR_WORDS
HEADER_WORDS = (
    ('magic', 'i4', 1),        # SELF_MAGIC
    ('version', 'i4', 1),      # SELF_VERSION
    ('n_dof', 'i4', 1),
    ('n_tf', 'i4', 1),         # joint transforms: n_dof + 1
    ('n_links', 'i4', 1),      # collision spheres of the robot
    ('n_pairs', 'i4', 1),
    ('margin', 'f4', 1),       # hinge margin (already inside every T_ab; kept for readers)
    ('off_tf', 'i4', 1),       # word offsets of the sections from the header ...
    ('off_links', 'i4', 1),
    ('off_pairs', 'i4', 1),
    ('total', 'i4', 1),        # words of the buffer, header included
)
_named = sum(n for _, _, n in HEADER_WORDS)
HEADER_DTYPE = np.dtype([(name, typ) for name, typ, _ in HEADER_WORDS] + [('reserved', 'i4', (SELF_HEADER_WORDS - _named,))])
assert HEADER_DTYPE.itemsize == 4 * SELF_HEADER_WORDS

# what include/mpb_self_layout.h carries besides the word indices: (heading, C literal form, names), each as MPB_<name>
C_LAYOUT = (
    ('magic, version', '0x%X', ('SELF_MAGIC',)),
    (None, '%d', ('SELF_VERSION',)),
    ('limits', '%d', ('SELF_HEADER_WORDS', 'SELF_MAX_LINKS', 'SELF_MAX_PAIRS')),
    ('pair word', '%d', ('SELF_PAIR_WORDS', 'SELF_PAIR_B_SHIFT')),
    (None, '0x%X', ('SELF_PAIR_A_MASK',)),
)


def header(buf):
    """The header of a packed self-collision buffer as a numpy record over HEADER_WORDS: a VIEW (reads and writes by name go to the
    buffer's own words)."""
    words = np.asarray(buf)[:SELF_HEADER_WORDS]
    assert words.dtype.itemsize == 4 and words.size == SELF_HEADER_WORDS, 'a packed self-collision buffer is an array of 32-bit words'
    return words.view(HEADER_DTYPE)[0]


def sections(buf):
    """{name: view} of the sections of a packed buffer: joint_tf (n_tf, 3, 4) fp32, links (n_links, 8) fp32, pair_ab (n_pairs, 2) int
    (a, b) decoded, pair_T (n_pairs,) fp32."""
    h = header(buf)
    f = np.asarray(buf).view(np.float32)
    n_tf, n_links, n_pairs = int(h['n_tf']), int(h['n_links']), int(h['n_pairs'])
    o_tf, o_l, o_p = int(h['off_tf']), int(h['off_links']), int(h['off_pairs'])
    pw = f[o_p:o_p + SELF_PAIR_WORDS * n_pairs].reshape(n_pairs, SELF_PAIR_WORDS)
    w = pw[:, 0].view(np.uint32)
    return dict(joint_tf=f[o_tf:o_tf + 12 * n_tf].reshape(n_tf, 3, 4), links=f[o_l:o_l + 8 * n_links].reshape(n_links, 8),
                pair_ab=np.stack([w & SELF_PAIR_A_MASK, w >> SELF_PAIR_B_SHIFT], -1).astype(np.int64), pair_T=pw[:, 1])
