"""The end-effector pose cost of DESIGN.md section 10 and its closed-form gradient, restated from the definition alone (helper module;
imported like ik_checks.py, whose chain / fk / pose_jacobian / pose_error it reuses).  Nothing here reads the code under test.

Per waypoint, (R, t) = fk(q), target [R* | t*], at unit k:
  position       e_p = t* - t,  c_p = |e_p|^2,                                   d c_p / dq = -2 J_v^T e_p
  full rotation  e_w of ik_checks.pose_error,  c_r = |e_w|^2,                    d c_r / dq = -2 J_w^T e_w
  tool axis a    u = R a, u* = R* a,  c_a = |u - u*|^2,                          d c_a / dq = -2 J_w^T (u x u*)
  c = c_p + (c_r or c_a)  (terms 'pos_rot', 'pos', 'pos_axis')

Every function takes the dtype from its inputs: fp64 is the reference, fp32 walks the same operation order in separate roundings, and its
distance from fp64 on the same inputs is E32; every bar is collision_kinks.bar(E32).  Units: a waypoint's cost error over max(1, c64), a
gradient element's error over max(1, largest |element| of that waypoint's fp64 gradient).  A waypoint whose fp64 theta >= pi - MARGIN is
left out of the full-rotation checks (the cut locus of c_r); at most CAP of the waypoints in range may be.
"""
import functools
import math
import types

import numpy as np
import torch

from collision_kinks import CAP, bar  # noqa: F401  (re-exported)
import ik_checks as K

MARGIN = 0.05
TERMS = ('pos_rot', 'pos', 'pos_axis')
AXIS = (0.0, 0.6, 0.8)                      # a unit vector of the tool frame that is no coordinate axis
ROBOTS = ('panda', 'arm12', 'arm9')


def waypoint_cost_grad(tf, q, target, terms, axis=AXIS):
    """q (M, D), target (M, 3, 4) -> c (M,), g (M, D) = d c / d q by the closed forms, theta (M,); unit k."""
    R, t, z, p = K.fk(tf, q)
    e, _, theta = K.pose_error(target, R, t)
    ep = e[:, :3]
    c = (ep[:, 0] * ep[:, 0] + ep[:, 1] * ep[:, 1]) + ep[:, 2] * ep[:, 2]
    m = None
    if terms == 'pos_rot':
        m = e[:, 3:]
        c = c + ((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
    elif terms == 'pos_axis':
        a = torch.tensor(axis, dtype=q.dtype)
        Rs = target[:, :, :3]
        u = torch.stack([(R[:, r, 0] * a[0] + R[:, r, 1] * a[1]) + R[:, r, 2] * a[2] for r in range(3)], -1)
        v = torch.stack([(Rs[:, r, 0] * a[0] + Rs[:, r, 1] * a[1]) + Rs[:, r, 2] * a[2] for r in range(3)], -1)
        d = u - v
        c = c + ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        m = K._cross(u, v)
    else:
        assert terms == 'pos'
    Jv = K._cross(z, t[:, None, :] - p)                                          # (M, D, 3)
    s = (Jv[..., 0] * ep[:, None, 0] + Jv[..., 1] * ep[:, None, 1]) + Jv[..., 2] * ep[:, None, 2]
    if m is not None:
        s = ((s + z[..., 0] * m[:, None, 0]) + z[..., 1] * m[:, None, 1]) + z[..., 2] * m[:, None, 2]
    return c, -2.0 * s, theta


def trajectory_cost_grad(tf, trajs, target, terms, h_begin, h_end, axis=AXIS):
    """trajs (B, H, d), target (B, H, 3, 4) (already expanded per trajectory and waypoint) -> c (B, H) and g (B, H, D), 0 outside the
    range, theta (B, H)."""
    B, H, _ = trajs.shape
    D = tf.shape[0] - 1
    c, g, th = waypoint_cost_grad(tf, trajs[:, :, :D].reshape(-1, D), target.reshape(-1, 3, 4), terms, axis)
    live = torch.zeros(H, dtype=torch.bool)
    live[h_begin:h_end] = True
    c, g, th = c.reshape(B, H), g.reshape(B, H, D), th.reshape(B, H)
    return torch.where(live[None], c, torch.zeros_like(c)), torch.where(live[None, :, None], g, torch.zeros_like(g)), th


def expand_target(target, B, H, per_waypoint):
    """A target in one of the four public shapes -> (B, H, 3, 4): trajectory b reads target b // (B / G)."""
    lead = target.dim() - (3 if per_waypoint else 2)
    t = target if lead == 1 else target[None]
    G = t.shape[0]
    assert B % G == 0
    t = t.repeat_interleave(B // G, 0)
    return t if per_waypoint else t[:, None].expand(B, H, 3, 4)


# ------------------------------------------------------------------------------------------------
# the input sets shared by tests/test_ee_cost_cpu.py and tests/test_gpu_ee_cost.py: fp32 numbers both precisions and the device start from
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(robot_name, B, H, wide=False, groups=None, per_waypoint=False):
    """trajs (B, H, D or 2 D) of test_gpu_edge_cases._trajs(robot, B, H, d, 11) (velocity columns NaN: they are never read) and the
    targets: fp64 FK of `last waypoint + RandomState(3).uniform(-0.6, 0.6)` of the first trajectory of each of `groups` goals (None: one
    per trajectory), rounded once to fp32; per_waypoint: the same with every waypoint perturbed on its own.  Treat as read-only."""
    from test_gpu_edge_cases import _trajs
    robot = K.robot_of(robot_name)
    D = robot.q_dim
    trajs = _trajs(robot, B, H, 2 * D if wide else D, 11)
    if wide:
        trajs[:, :, D:] = float('nan')
    G = B if groups is None else groups
    tf64, _, _ = K.chain(robot, torch.float64)
    rng = np.random.RandomState(3)
    lead = trajs[::B // G, :, :D].double()                                        # (G, H, D)
    if per_waypoint:
        qt = lead + torch.as_tensor(rng.uniform(-0.6, 0.6, (G, H, D)))
        target = K.pose_jacobian(tf64, qt.reshape(-1, D))[0].float().reshape(G, H, 3, 4)
    else:
        qt = lead[:, -1] + torch.as_tensor(rng.uniform(-0.6, 0.6, (G, D)))
        target = K.pose_jacobian(tf64, qt)[0].float()
    if G == 1:
        target = target[0]
    return types.SimpleNamespace(robot=robot, D=D, trajs=trajs, target=target.contiguous(), per_waypoint=per_waypoint)


@functools.lru_cache(maxsize=None)
def reference(robot_name, B, H, terms, h_begin, h_end, wide=False, groups=None, per_waypoint=False):
    """Computed once per case and shared: the fp64 and fp32 restatements, the mask of the checked waypoints, E32 of costs and gradients
    in the units above."""
    inp = inputs(robot_name, B, H, wide, groups, per_waypoint)
    out = {}
    for dt in (torch.float64, torch.float32):
        tf, _, _ = K.chain(inp.robot, dt)
        tgt = expand_target(inp.target.to(dt), B, H, per_waypoint)
        out[dt] = trajectory_cost_grad(tf, inp.trajs.to(dt), tgt, terms, h_begin, h_end)
    c64, g64, th64 = out[torch.float64]
    c32, g32, _ = out[torch.float32]
    live = torch.zeros(B, H, dtype=torch.bool)
    live[:, h_begin:h_end] = True
    keep = live & ((th64 < math.pi - MARGIN) if terms == 'pos_rot' else torch.ones_like(live))
    left_out = 1.0 - float(keep.sum()) / float(live.sum())
    ref = types.SimpleNamespace(inp=inp, c64=c64, g64=g64, th64=th64, c32=c32, g32=g32, live=live, keep=keep, left_out=left_out)
    ref.E32_c, ref.E32_g = cost_error(ref, c32), grad_error(ref, g32)
    return ref


def cost_error(ref, c):
    """Largest error of per-waypoint costs c (B, H) on the checked waypoints, over max(1, c64)."""
    e = (c.double() - ref.c64).abs() / ref.c64.clamp_min(1.0)
    return float(e[ref.keep].max())


def grad_error(ref, g):
    """Largest error of gradient elements g (B, H, D) on the checked waypoints, over max(1, largest |element| of the waypoint)."""
    e = (g.double() - ref.g64).abs().amax(-1) / ref.g64.abs().amax(-1).clamp_min(1.0)
    return float(e[ref.keep].max())


def wave_sum_f32(per_lane):
    """The fixed-order wave reduction of csrc/mpb_common.h on 64 fp32 lane values, restated: four neighbour exchanges inside each row
    of sixteen lanes (xor 1, xor 2, mirror of eight, mirror of sixteen), then (row0 + row1) + (row2 + row3)."""
    v = np.asarray(per_lane, dtype=np.float32).copy()
    i = np.arange(64)
    for perm in (i ^ 1, i ^ 2, 8 * (i // 8) + 7 - i % 8, 16 * (i // 16) + 15 - i % 16):
        v = (v + v[perm]).astype(np.float32)
    return np.float32(np.float32(v[0] + v[16]) + np.float32(v[32] + v[48]))


def ordered_sum_f32(per_wp):
    """out of one trajectory from its per-waypoint costs (H,) fp32 in the kernels' order: a lane sums its trips of 64 in ascending order,
    then the wave reduction."""
    c = np.asarray(per_wp, dtype=np.float32)
    lanes = np.zeros(64, np.float32)
    for h0 in range(0, len(c), 64):
        trip = np.zeros(64, np.float32)
        trip[:len(c[h0:h0 + 64])] = c[h0:h0 + 64]
        lanes = (lanes + trip).astype(np.float32)
    return wave_sum_f32(lanes)


# (robot, B, H, terms, h_begin, h_end, wide, groups, per_waypoint) -- the arguments of reference().  The full rotation term is checked
# where the fp64 restatement keeps the cap: one target per trajectory (every robot, one partial trip, two trips, the goal alone) and
# per-waypoint targets; the cases that are about indexing -- an explicit range, fewer targets than trajectories -- use the terms that
# leave nothing out (test_ee_cost_cpu.py asserts the cap on every case).
CASES = {}
for _r in ROBOTS:
    for _t in TERMS:
        CASES[f'{_r}-{_t}-path'] = (_r, 48, 37, _t, 1, 37)                       # one partial trip
for _t in TERMS:
    CASES[f'panda-{_t}-two-trips'] = ('panda', 5, 70, _t, 1, 70)
    CASES[f'panda-{_t}-goal-48'] = ('panda', 48, 37, _t, 36, 37)                 # lane form, a partial wave
    CASES[f'arm12-{_t}-goal-130'] = ('arm12', 130, 8, _t, 7, 8)                  # lane form, three workgroups, the last partial
CASES['panda-pos_axis-range-3-9'] = ('panda', 48, 37, 'pos_axis', 3, 9)
CASES['panda-pos_axis-wide'] = ('panda', 48, 37, 'pos_axis', 1, 37, True)      # d = 2 D, the velocity columns NaN
CASES['arm9-pos_rot-goal-130-wide'] = ('arm9', 130, 8, 'pos_rot', 7, 8, True)
CASES['panda-pos_axis-3-targets'] = ('panda', 48, 37, 'pos_axis', 1, 37, False, 3)
CASES['arm9-pos-1-target'] = ('arm9', 48, 37, 'pos', 1, 37, False, 1)
CASES['arm9-pos_axis-goal-3-targets'] = ('arm9', 48, 37, 'pos_axis', 36, 37, False, 3)
CASES['panda-pos_rot-per-waypoint'] = ('panda', 48, 37, 'pos_rot', 1, 37, False, None, True)
CASES['arm12-pos-per-waypoint-3-targets'] = ('arm12', 48, 37, 'pos', 1, 37, True, 3, True)
