"""Linear segments with parabolic blends (ops.path_blend, ops.path_blend_sample, csrc/mpb_path_blend.hip; definition and proofs:
DESIGN.md 10, include/mpb.h) in numbers: the ONLY definition of its status values and of the default sweep limit, and the host side of the
hand-off to the path certifier (joint_deviation, workspace_deviation: pure numpy, fp64).  model_gen.py emits include/mpb_blend_layout.h
from it (which include/mpb.h and the kernels include); tests/test_path_blend_cpu.py holds the header text to the generator.  No torch
here: model_gen imports it on a build host.
"""
import numpy as np

# status of a path, value = index; TOO_LONG is the sampler's alone (more rows than the output holds)
STATUS = ('OK', 'NOT_CONVERGED', 'DEGENERATE_SEGMENT', 'BAD_INPUT', 'TOO_LONG')

BLEND_DEFAULT_MAX_SWEEPS = 64          # a numpy prototype of the sweep loop converged within 15 on every input tried

C_DEFINES = ('BLEND_DEFAULT_MAX_SWEEPS',)


def joint_deviation(q, T, tb, lengths=None):
    """dev (N, H, D) fp64 from the rows q (N, H, D) and a blend's T (N, H-1), tb (N, H): dev_ik = |dv_ik| tb_i / 8, how far joint k
    leaves the polyline inside the blend of waypoint i (dv_i = v_i - v_{i-1}, v_i = dq_i / T_i, v_{-1} = v_{L-1} = 0).  Rows at and past
    a path's length, and paths whose T is zero (not OK), give 0."""
    q, T, tb = np.asarray(q, np.float64), np.asarray(T, np.float64), np.asarray(tb, np.float64)
    N, H, D = q.shape
    L = np.full(N, H) if lengths is None else np.asarray(lengths).astype(np.int64)
    seg = (np.arange(H - 1)[None, :] < (L - 1)[:, None]) & (T > 0)
    with np.errstate(divide='ignore', invalid='ignore'):
        v = np.where(seg[:, :, None], (q[:, 1:] - q[:, :-1]) / np.where(seg, T, 1.0)[:, :, None], 0.0)
    v = np.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0)
    zero = np.zeros((N, 1, D))
    dv = np.concatenate([v, zero], 1) - np.concatenate([zero, v], 1)
    way = np.arange(H)[None, :] < L[:, None]
    return np.where(way[:, :, None], np.abs(dv) * tb[:, :, None] / 8.0, 0.0)


def workspace_deviation(rho, dev):
    """(N,) fp64: max over waypoints i and collision spheres l of sum_k rho[k, l] dev[n, i, k] -- no collision sphere of the blended
    trajectory is farther than this from where it is on the polyline (rho: certify_layout.reach_table; a point robot's table of ones
    gives the 1-norm, which bounds its Euclidean step)."""
    return (np.asarray(dev, np.float64) @ np.asarray(rho, np.float64)).max(axis=(1, 2))
