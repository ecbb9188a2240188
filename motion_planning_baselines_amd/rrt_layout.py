"""The workspace of the batched sample-based planners (RRT-Connect, RRT* / informed RRT*) in numbers: the ONLY definition of the status
values, the stop reasons, the pool limit and the layout of the two workspaces.  model_gen.py emits include/mpb_rrt_layout.h from it (which
include/mpb.h -- it says what each word means -- and csrc/mpb_rrt.h include), ops.py reads a workspace by walking it, and
tests/test_host_logic.py pins the public numbers as literals and holds the offset arithmetic of the C side (rrt_layout / rrs_layout of the
two .hip files) to offsets() below.  No torch here: model_gen imports it on a build host.
"""
import math
from collections import namedtuple

STATUS = ('RUNNING', 'FOUND', 'EXHAUSTED_ITERS', 'START_OR_GOAL_IN_COLLISION', 'POOL_EMPTY', 'TREE_FULL', 'PATH_TOO_LONG')   # value = index
STOP = ('RUNNING', 'ITERS', 'COST_CONVERGED', 'AFTER_SUCCESS', 'TREE_FULL', 'POOL_EMPTY')    # RRT*: why a problem stopped; value = index
MAX_PRE_SAMPLES = 16384      # configurations of a pre-sample pool: the kernels keep the pool's index list in LDS

# A workspace is 32-bit words: GLOBAL_WORDS words for the whole batch (the named ones first, the rest zero), then the per-problem headers
# `hdr`, then the kind's sections in order -- each one array per problem, problems back to back.
GLOBAL_WORDS = 16
GLOBAL = ('magic', 'B', 'max_nodes', 'n_pre', 'D', 'Dp')       # Dp: D rounded up to a multiple of 4 (rows are float4s)
POOL_INDEX_BITS = 16                                           # a pool list: ceil(n_pre / POOL_PER_WORD) words of indices into
POOL_PER_WORD = 32 // POOL_INDEX_BITS                          # pre_samples, low bits first

# magic; prefix of the header-word names in C; words of a problem's header (the named ones first, the rest zero); the header words in
# order as (name, type, words); the sections after `hdr` in order as (name, type, per-problem shape from (max_nodes, Dp, pool_words)).
# Types: 'i4' int32, 'f4' fp32 bits, 'u4' pool words.
Kind = namedtuple('Kind', 'magic c_prefix hdr_words header sections')
KINDS = {
    'connect': Kind(0x52525443, 'MPB_RRTC_', 16, (
        ('status', 'i4', 1), ('iters', 'i4', 1), ('counts', 'i4', 2), ('swap', 'i4', 1), ('pool_len', 'i4', 1),     # counts: tree 0, tree 1
    ), (
        ('nodes', 'f4', lambda M, Dp, pw: (2, M, Dp)),         # tree 0 is rooted at the start, tree 1 at the goal
        ('parents', 'i4', lambda M, Dp, pw: (2, M)),           # -1: root
        ('pool', 'u4', lambda M, Dp, pw: (pw,)),
    )),
    'star': Kind(0x52525453, 'MPB_RRTS_', 32, (
        ('status', 'i4', 1), ('iters', 'i4', 1), ('count', 'i4', 1), ('goal', 'i4', 1), ('pool_len', 'i4', 1), ('stop_reason', 'i4', 1),
        ('best_cost_iters', 'i4', 1), ('iters_after_first_success', 'i4', 1), ('best_cost_eps', 'f4', 1), ('rewires', 'i4', 1),
        ('informed_rejections', 'i4', 1), ('first_cost', 'f4', 1), ('first_iter', 'i4', 1), ('first_count', 'i4', 1),
    ), (
        ('goal_q', 'f4', lambda M, Dp, pw: (Dp,)),
        ('nodes', 'f4', lambda M, Dp, pw: (M, Dp)),
        ('parents', 'i4', lambda M, Dp, pw: (M,)),             # -1: root; after a rewire a parent may follow its child
        ('d', 'f4', lambda M, Dp, pw: (M,)),                   # length of the edge to the parent
        ('cost', 'f4', lambda M, Dp, pw: (M,)),
        ('cand', 'i4', lambda M, Dp, pw: (3, M)),              # rewire candidates of the current iteration: index, d, edge verdict
        ('pool', 'u4', lambda M, Dp, pw: (pw,)),
    )),
}
Layout = namedtuple('Layout', 'Dp pool_words sections total')


def header_index(kind):
    """{name: (index of the word -- of the first one where a name covers several --, type, words)} of a kind's header."""
    out, word = {}, 0
    for name, typ, n in KINDS[kind].header:
        out[name] = (word, typ, n)
        word += n
    assert word <= KINDS[kind].hdr_words
    return out


def offsets(kind, B, max_nodes, n_pre, D):
    """Where the sections of a workspace lie: Layout(Dp, pool_words, {name: (first word, type, (B, *shape))}, total words)."""
    Dp, pool_words = (D + 3) // 4 * 4, (n_pre + POOL_PER_WORD - 1) // POOL_PER_WORD
    sections, o = {}, GLOBAL_WORDS
    for name, typ, shape in (('hdr', 'i4', lambda M, Dp, pw: (KINDS[kind].hdr_words,)),) + KINDS[kind].sections:
        sections[name] = (o, typ, (B,) + shape(max_nodes, Dp, pool_words))
        o += math.prod(sections[name][2])
    return Layout(Dp, pool_words, sections, o)
