"""Path timing among moving obstacles (ops.path_time_plan, csrc/mpb_path_timing.hip) in numbers: the ONLY definition of its status values,
limits, the fixed-point unit of a segment cost and the LDS a launch takes.  model_gen.py emits include/mpb_path_timing_layout.h from it
(which include/mpb.h -- it says what each name means -- and csrc/mpb_path_timing.hip include); tests/test_path_timing_cpu.py holds the
header text to the generator.  No workspace: everything a path needs between its phases lives in the workgroup's LDS.  No torch here:
model_gen imports it on a build host.
"""
from .moving_layout import MOVING_MAX_ROWS

STATUS = ('FOUND', 'START_BLOCKED', 'GOAL_NOT_HOLDABLE', 'SEGMENT_TOO_LONG', 'NO_TIMING', 'BUFFER_CHANGED')   # value = index
# the order in which a refusal wins: the first that applies (BUFFER_CHANGED -- the moving-obstacle buffer's header differs from what the
# launcher read -- before all of them: nothing of the buffer is trusted)
STATUS_ORDER = ('BUFFER_CHANGED', 'SEGMENT_TOO_LONG', 'START_BLOCKED', 'GOAL_NOT_HOLDABLE', 'NO_TIMING')
PT_MIN_SAMPLES = 2               # samples along a path: the start and the goal
PT_MAX_SAMPLES = 256             # one thread per sample, eight 32-bit words of a row of the bit table
PT_MIN_ROWS = 2                  # rows of the clock
PT_MAX_ROWS = MOVING_MAX_ROWS
PT_THREADS = 256                 # threads of the one workgroup a path gets
PT_COST_ONE = 65536              # a segment cost of 1 (the whole of one row's travel) in the fixed point the prefix sums are taken in
PT_SCRATCH_WORDS = 16            # reduction words behind the tables
PT_MAX_LDS_BYTES = 160 * 1024    # what one workgroup may take of a gfx950 compute unit's LDS

C_DEFINES = ('PT_MIN_SAMPLES', 'PT_MAX_SAMPLES', 'PT_MIN_ROWS', 'PT_MAX_ROWS', 'PT_THREADS', 'PT_COST_ONE', 'PT_SCRATCH_WORDS',
             'PT_MAX_LDS_BYTES')
# the LDS of a launch in 32-bit words, as a C macro of (n_links, n_samples, n_rows) and as lds_words() below: the sphere centres
# [link][xyz][sample], the bit table [word][row] (bit i & 31 of word i >> 5: sample i), the prefix sums C and the interval starts lo (one
# word per sample each), idx (one word per row), the scratch words
C_LDS_WORDS = '(3 * (L) * (S) + ((S) + 31) / 32 * (R) + 2 * (S) + (R) + MPB_PT_SCRATCH_WORDS)'


def lds_words(n_links, n_samples, n_rows):
    """32-bit words of LDS a launch takes (MPB_PT_LDS_WORDS of the generated header)."""
    L, S, R = int(n_links), int(n_samples), int(n_rows)
    return 3 * L * S + (S + 31) // 32 * R + 2 * S + R + PT_SCRATCH_WORDS


def lds_bytes(n_links, n_samples, n_rows):
    return 4 * lds_words(n_links, n_samples, n_rows)
