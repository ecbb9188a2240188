"""Space-time shortcutting of timed trajectories among moving obstacles (ops.st_shortcut, csrc/mpb_st_shortcut.hip) in numbers: the ONLY
definition of its status values, log codes, the shift of the log's row index, the Philox tag of its draws, the slack of its input gate,
its limits and the LDS a launch takes.  model_gen.py emits include/mpb_st_shortcut_layout.h from it (which include/mpb.h -- it says what
each name means -- and csrc/mpb_st_shortcut.hip include); tests/test_st_shortcut_cpu.py holds the header text to the generator.  No
workspace: a trajectory lives in its workgroup's LDS for the whole launch.  No torch here: model_gen imports it on a build host.
"""
from .moving_layout import MOVING_MAX_ROWS

# status of a trajectory, value = index; a refusal wins in this order (the first that applies), OK is what is left
STATUS = ('OK', 'NOT_VALID', 'BUFFER_CHANGED', 'INPUT_IN_COLLISION', 'INPUT_TOO_FAST')
STATUS_ORDER = ('NOT_VALID', 'BUFFER_CHANGED', 'INPUT_IN_COLLISION', 'INPUT_TOO_FAST')
# what an iteration did, the low bits of a log word; IDLE: the trajectory is not OK, nothing is drawn
LOG_CODES = ('IDLE', 'SKIP_SHORT', 'SKIP_FAST', 'SKIP_STRAIGHT', 'REJECT', 'ACCEPT')
STS_LOG_INDEX_SHIFT = 8          # a REJECT word carries the first colliding row above these bits
STS_PHILOX_TAG = 0x53545343      # 'STSC': word 2 of the Philox counter of an iteration's draws
STS_MIN_ROWS = 3                 # a first row, a row to replace, a last row
STS_MAX_ROWS = MOVING_MAX_ROWS
STS_MAX_ITERS = 1 << 20
# The input gate admits a step with tau <= 1 + 2^-16.  Both producers (STRRTConnect, time_paths_moving) keep every step within
# w (1 + 1e-5); tau's own three fp32 roundings add under 2e-7; 2^-16 = 1.53e-5 clears the sum.  Written so that C and Python read the
# same fp32 number: the slack is a power of two, 1 + 2^-16 is exact in fp32.
STS_GATE_SLACK_LOG2 = -16
STS_GATE_LIMIT = 1.0 + 2.0 ** STS_GATE_SLACK_LOG2
STS_GATE_LIMIT_C = '0x1.0001p+0f'
STS_STATIC_LDS_BYTES = 17408     # the staged broad-phase grid of the static predicate: 4 * MPB_GRID_MAX_CELLS + 16 * (MPB_GRID_MAX_SPH + 1)
STS_MAX_LDS_BYTES = 160 * 1024   # what one workgroup may take of a gfx950 compute unit's LDS

C_DEFINES = ('STS_LOG_INDEX_SHIFT', 'STS_PHILOX_TAG', 'STS_MIN_ROWS', 'STS_MAX_ROWS', 'STS_MAX_ITERS', 'STS_STATIC_LDS_BYTES',
             'STS_MAX_LDS_BYTES')
# the LDS of a launch in bytes, as a C macro of (n_rows, D) and as lds_bytes() below: the staged grid and the trajectory as [row][Dp]
# floats, Dp = D rounded up to a multiple of 4
C_LDS_BYTES = '(MPB_STS_STATIC_LDS_BYTES + 4 * (R) * (((D) + 3) / 4 * 4))'


def traj_lds_bytes(n_rows, D):
    """Bytes of dynamic LDS a launch takes: the trajectory as [row][Dp] floats."""
    return 4 * int(n_rows) * ((int(D) + 3) // 4 * 4)


def lds_bytes(n_rows, D):
    """Bytes of LDS a workgroup takes (MPB_STS_LDS_BYTES of the generated header)."""
    return STS_STATIC_LDS_BYTES + traj_lds_bytes(n_rows, D)
