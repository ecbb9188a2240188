"""The workspace and the decision log of the space-time RRT-Connect (planners.STRRTConnect, csrc/mpb_strrt.hip) in numbers: the ONLY
definition of its status values, magic, limits, global and per-problem header words, tree sections and log record.  model_gen.py emits
include/mpb_strrt_layout.h from it (which include/mpb.h -- it says what each word means -- and csrc/mpb_strrt.hip include), ops.py reads a
workspace by walking it, and tests/test_strrt_cpu.py holds the header text to the generator.  A layout of its own: a node carries a row
(its time on the moving-obstacle field's row grid) and there is no pool list, so rrt_layout.py and its header stay as they are.  No torch
here: model_gen imports it on a build host.
"""
import math
from collections import namedtuple

from .moving_layout import MOVING_MAX_ROWS

STATUS = ('RUNNING', 'FOUND', 'EXHAUSTED_ITERS', 'START_OR_GOAL_IN_COLLISION', 'HORIZON_TOO_SHORT', 'TREE_FULL', 'PATH_TOO_LONG')   # value = index
STRRT_MAGIC = 0x53545252        # 'STRR': word MAGIC of the workspace AND word 2 of the Philox counter of an iteration's draws
STRRT_MIN_ROWS = 3              # rows of the time grid: start row, at least one row to sample, goal row
STRRT_MAX_ROWS = MOVING_MAX_ROWS
STRRT_MAX_PRE_SAMPLES = 1 << 20  # configurations of the pre-sample array (nothing is deleted from it: no list in LDS)

# A workspace is 32-bit words: GLOBAL_WORDS words for the whole batch (the named ones first, the rest zero), then HDR_WORDS words per
# problem (the named ones first, the rest zero), then the sections in order -- each one array per problem, problems back to back.
STRRT_GLOBAL_WORDS = 16
GLOBAL = ('magic', 'B', 'max_nodes', 'D', 'Dp', 'n_rows')      # Dp: D rounded up to a multiple of 4 (node rows are float4s)
STRRT_HDR_WORDS = 16
HEADER = (('status', 'i4', 1), ('iters', 'i4', 1), ('counts', 'i4', 2), ('rejected_joins', 'i4', 1))   # counts: tree 0, tree 1
SECTIONS = (
    ('nodes', 'f4', lambda M, Dp: (2, M, Dp)),     # tree 0 is rooted at (start, row 0), tree 1 at (goal, row n_rows - 1)
    ('rows', 'i4', lambda M, Dp: (2, M)),          # the node's row of the time grid
    ('parents', 'i4', lambda M, Dp: (2, M)),       # -1: root; a child's row is greater (tree 0) / smaller (tree 1) than its parent's
)

# The decision log: STRRT_LOG_WORDS int32 per (problem, iteration).  Two extension records of STRRT_LOG_EXT_WORDS words each -- the
# extension of the iteration's tree towards the sample at word 0, the connect extension of the other tree at STRRT_LOG_EXT_WORDS -- and
# the re-check of a join at STRRT_LOG_JOIN.  What did not happen keeps STRRT_LOG_NONE, which the caller fills the log with.
LOG_EXT = ('tree', 'nearest', 'dh', 's', 'first', 'appended')   # first: first colliding point 1 .. s or -1; appended: node index or -1
STRRT_LOG_EXT_WORDS = len(LOG_EXT)
STRRT_LOG_JOIN = 2 * STRRT_LOG_EXT_WORDS                        # first failing row of the re-check, -1 when every row is free
STRRT_LOG_WORDS = 16
STRRT_LOG_NONE = -2

C_DEFINES = ('STRRT_MAGIC', 'STRRT_MIN_ROWS', 'STRRT_MAX_ROWS', 'STRRT_MAX_PRE_SAMPLES', 'STRRT_GLOBAL_WORDS', 'STRRT_HDR_WORDS',
             'STRRT_LOG_EXT_WORDS', 'STRRT_LOG_JOIN', 'STRRT_LOG_WORDS', 'STRRT_LOG_NONE')
Layout = namedtuple('Layout', 'Dp sections total')


def header_index():
    """{name: (index of the word -- of the first one where a name covers several --, type, words)} of a problem's header."""
    out, word = {}, 0
    for name, typ, n in HEADER:
        out[name] = (word, typ, n)
        word += n
    assert word <= STRRT_HDR_WORDS
    return out


def offsets(B, max_nodes, D):
    """Where the sections of a workspace lie: Layout(Dp, {name: (first word, type, (B, *shape))}, total words)."""
    Dp = (D + 3) // 4 * 4
    sections, o = {}, STRRT_GLOBAL_WORDS
    for name, typ, shape in (('hdr', 'i4', lambda M, Dp: (STRRT_HDR_WORDS,)),) + SECTIONS:
        sections[name] = (o, typ, (B,) + shape(max_nodes, Dp))
        o += math.prod(sections[name][2])
    return Layout(Dp, sections, o)
