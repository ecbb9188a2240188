"""Cartesian end-effector moves (straight-line tracking; include/mpb.h mpb_cartesian_path) restated from the
definition alone (helper module; imported like ik_checks.py, whose walk, pose error and damped-least-squares step it uses).  Nothing
here reads the code under test: the chain is a robot's spec()['joint_tf'] and its joint limits, the arithmetic is torch on the CPU.

Every function takes the dtype from its inputs.  In fp64 it is the reference; in fp32 it follows the same operation order in separate
fp32 roundings, and its distance from fp64 on the same inputs is E32, the source of every bar: collision_kinks.bar(E32).

  start:  [R_0 | t_0] = the pose of q_0
  turn:   E = R* R_0^T, w = vee(E - E^T) / 2, c = (tr E - 1) / 2, theta = atan2(|w|, c), a = w / |w|;
          theta > pi - 0.1: BAD_TARGET; else theta = 0 when |w| < 1e-6; position only: no rotation at all, rot_err = 0
  step k: s = k / K,  t_k = (1 - s) t_0 + s t*,  R_k = Rod(a, s theta) R_0,  Rod = cos I + sin [a]x + (1 - cos) a a^T;
          at most n_inner iterations of ik_checks (error, dls_step, clamp; a converged problem is frozen) from the last accepted
          configuration; not within the tolerances: LOST; else a joint moved by more than jump_max: JUMP; else accepted, n_ok = k
  rows:   0 = q_0; k <= n_ok accepted; beyond n_ok row n_ok again; errors: 0 in row 0, the rejected step's in row n_ok + 1, 0 after
"""
import functools
import math
import types

import numpy as np
import torch

from ik_checks import bar, chain, dls_step, fk, pose_error, robot_of, uniform_q  # noqa: F401  (bar: re-exported for the tests)

OK, LOST, JUMP, BAD_TARGET, COLLISION = 0, 1, 2, 3, 4
MAX_TURN = math.pi - 0.1
N_TARGETS, N_STARTS = 37, 3          # 111 lanes: a partial second wave, the target changing inside a wave
DAMPING, POS_TOL, ROT_TOL, JUMP_MAX = 0.1, 1e-3, 1e-2, 0.5
FULL, ELEMENT = (32, 4), (2, 1)      # (K, n_inner) of the full run and of the element-wise run
# the element-wise run's tolerances: half of a 0.05-0.25 m move in ONE damped step leaves a residual of millimetres, and with the default
# tolerances no step would be accepted -- every row would be q_0.  With these some problems accept a step or two and the others are lost.
ELEMENT_TOL = (1e-2, 5e-2)
JUMP_TIGHT = 0.02                    # the jump_max of the JUMP cases
CAP = 0.02                           # share of the problems whose n_ok may differ between fp32 and fp64
SETS = ('panda', 'panda_pos', 'arm12', 'arm4_pos')


def _cross(a, b):
    return torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def turn(R0, Rs):
    """The rotation from R0 to Rs (M, 3, 3 each) -> theta (M,) as atan2 gives it, unit axis a (M, 3) (zero where |w| < 1e-6), none (M,)."""
    E = [[(Rs[:, a, 0] * R0[:, b, 0] + Rs[:, a, 1] * R0[:, b, 1]) + Rs[:, a, 2] * R0[:, b, 2] for b in range(3)] for a in range(3)]
    w = torch.stack([0.5 * (E[2][1] - E[1][2]), 0.5 * (E[0][2] - E[2][0]), 0.5 * (E[1][0] - E[0][1])], -1)
    c = 0.5 * (((E[0][0] + E[1][1]) + E[2][2]) - 1.0)
    nw = torch.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
    theta = torch.atan2(nw, c)
    none = nw < 1e-6
    a = torch.where(none[:, None], torch.zeros_like(w), w / torch.where(none, torch.ones_like(nw), nw)[:, None])
    return theta, a, none


def rodrigues(a, phi):
    """Unit axes a (M, 3) (or zero), angles phi (M,) -> (M, 3, 3): cos I + sin [a]x + (1 - cos) a a^T."""
    sn, cs = torch.sin(phi), torch.cos(phi)
    v = 1.0 - cs
    ax, ay, az = a[:, 0], a[:, 1], a[:, 2]
    vx, vy, vz = v * ax, v * ay, v * az
    rows = [[vx * ax + cs, vx * ay - sn * az, vx * az + sn * ay],
            [vy * ax + sn * az, vy * ay + cs, vy * az - sn * ax],
            [vz * ax - sn * ay, vz * ay + sn * ax, vz * az + cs]]
    return torch.stack([torch.stack(r, -1) for r in rows], -2)


def _matmul3(A, B):
    return torch.stack([torch.stack([(A[:, i, 0] * B[:, 0, j] + A[:, i, 1] * B[:, 1, j]) + A[:, i, 2] * B[:, 2, j] for j in range(3)], -1)
                        for i in range(3)], -2)


def step_target(R0, t0, target, theta, a, k, K, position_only):
    """[R_k | t_k] (M, 3, 4) of step k; position only: the rotation block is the identity (it is never read)."""
    s = torch.tensor(float(k), dtype=t0.dtype) / torch.tensor(float(K), dtype=t0.dtype)
    tk = (1.0 - s) * t0 + s * target[:, :, 3]
    Rk = torch.eye(3, dtype=t0.dtype).expand(t0.shape[0], 3, 3) if position_only else _matmul3(rodrigues(a, s * theta), R0)
    return torch.cat([Rk, tk[:, :, None]], -1)


def start_and_turn(tf, target, q0, position_only):
    """-> R0, t0, theta (0 where there is no rotation), a, bad (M,) bool"""
    R0, t0, _, _ = fk(tf, q0)
    M = q0.shape[0]
    if position_only:
        return R0, t0, torch.zeros(M, dtype=q0.dtype), torch.zeros(M, 3, dtype=q0.dtype), torch.zeros(M, dtype=torch.bool)
    theta, a, none = turn(R0, target[:, :, :3])
    bad = ~(theta <= MAX_TURN)
    return R0, t0, torch.where(none, torch.zeros_like(theta), theta), a, bad


def cartesian_path(tf, target, q0, K, n_inner, damping=DAMPING, pos_tol=POS_TOL, rot_tol=ROT_TOL, jump_max=JUMP_MAX,
                   position_only=False, q_min=None, q_max=None):
    """target (M, 3, 4), q0 (M, D) -> namespace(q (M, K+1, D), pos_err, rot_err (M, K+1), n_ok, status (M,) int32)."""
    M, D = q0.shape
    n = 3 if position_only else 6
    R0, t0, theta, a, bad = start_and_turn(tf, target, q0, position_only)
    status = torch.where(bad, torch.full((M,), BAD_TARGET, dtype=torch.int32), torch.full((M,), OK, dtype=torch.int32))
    active = ~bad
    n_ok = torch.zeros(M, dtype=torch.int32)
    qa = q0.clone()
    rows, pes, ths = [q0.clone()], [torch.zeros(M, dtype=q0.dtype)], [torch.zeros(M, dtype=q0.dtype)]
    for k in range(1, K + 1):
        if not bool(active.any()):                           # (everything has stopped: the held rows)
            rows.append(qa.clone()); pes.append(torch.zeros_like(pes[0])); ths.append(torch.zeros_like(pes[0]))
            continue
        T = step_target(R0, t0, target, theta, a, k, K, position_only)
        q = qa.clone()
        for it in range(n_inner + 1):
            R, t, z, p = fk(tf, q)
            e, pe, th = pose_error(T, R, t)
            if position_only:
                th = torch.zeros_like(th)
            conv = (pe <= pos_tol) & ((th <= rot_tol) | bool(position_only))
            frozen = conv | ~active
            if it == n_inner or bool(frozen.all()):
                break
            J = torch.cat([_cross(z, t[:, None, :] - p), z], -1).transpose(1, 2)
            qn = q + dls_step(J[:, :n], e[:, :n], damping)
            if q_min is not None:
                qn = torch.minimum(torch.maximum(qn, q_min), q_max)
            q = torch.where(frozen[:, None], q, qn)
        jump = (q - qa).abs().amax(-1)
        lost, jumped = ~conv, ~(jump <= jump_max)
        accept = active & ~lost & ~jumped
        status = torch.where(active & lost, torch.full_like(status, LOST), torch.where(active & ~lost & jumped, torch.full_like(status, JUMP), status))
        n_ok = torch.where(accept, torch.full_like(n_ok, k), n_ok)
        qa = torch.where(accept[:, None], q, qa)
        rows.append(qa.clone())
        pes.append(torch.where(active, pe, torch.zeros_like(pe)))
        ths.append(torch.where(active, th, torch.zeros_like(th)))
        active = accept
    return types.SimpleNamespace(q=torch.stack(rows, 1), pos_err=torch.stack(pes, 1), rot_err=torch.stack(ths, 1), n_ok=n_ok, status=status)


def path_errors(tf64, target, q0, q_path, position_only):
    """fp64, from a path alone: per row k the pose error of q_path[:, k] against the fp64 step target of (q0, target) -> |e_p|, theta
    (M, K+1) each (row 0: against the start pose itself), and the distance of the hand from the straight segment t_0 .. t* (M, K+1)."""
    M, rows, D = q_path.shape
    K = rows - 1
    target, q0, q_path = target.double(), q0.double(), q_path.double()
    R0, t0, theta, a, _ = start_and_turn(tf64, target, q0, position_only)
    pes, ths, off = [], [], []
    seg = target[:, :, 3] - t0
    for k in range(rows):
        T = step_target(R0, t0, target, theta, a, k, K, position_only)
        R, t, _, _ = fk(tf64, q_path[:, k])
        _, pe, th = pose_error(T, R, t)
        pes.append(pe); ths.append(torch.zeros_like(th) if position_only else th)
        lam = (((t - t0) * seg).sum(-1) / (seg * seg).sum(-1).clamp_min(1e-300)).clamp(0.0, 1.0)
        off.append((t - (t0 + lam[:, None] * seg)).norm(dim=-1))
    return torch.stack(pes, 1), torch.stack(ths, 1), torch.stack(off, 1)


# ------------------------------------------------------------------------------------------------
# the input sets shared by tests/test_cartesian_cpu.py and tests/test_gpu_cartesian.py
# ------------------------------------------------------------------------------------------------
SEEDS = dict(panda=21, panda_pos=25, arm12=23, arm4_pos=24)
# The 4-joint arm's hand moves on a surface (its position Jacobian has rank 2 everywhere): a goal off that surface is lost at once, whatever
# the tracker does.  Its goals are therefore poses the arm can take -- start 0 displaced by up to this many rad per joint --, and the
# straight segment leaves the surface by its sag alone: short moves complete, long ones are lost on the way.  For the same reason a
# move long enough to turn a joint by more than JUMP_TIGHT per step is lost before it jumps; the odd targets therefore start where the
# hand has little leverage (second singular value of the position Jacobian within WEAK) and move along that joint direction.
ON_SURFACE = dict(arm4_pos=0.15)
WEAK = (0.06, 0.12)
WEAK_TURN = 0.9       # rad along that joint direction: about 0.03 rad per step of 32, for a hand move of some 0.1 m


def _weak_configurations(robot, tf64, mid, n, seed):
    """The first n of 4 000 uniform configurations, pulled to 0.7, whose position Jacobian's second singular value lies within WEAK, and
    the unit joint direction that belongs to it."""
    q = mid + 0.7 * (uniform_q(robot, (4000,), seed).double() - mid)
    _, t, z, p = fk(tf64, q)
    sv = torch.linalg.svdvals(_cross(z, t[:, None, :] - p).transpose(1, 2))[:, 1]
    keep = (sv >= WEAK[0]) & (sv <= WEAK[1])
    q = q[keep][:n]
    assert q.shape[0] == n
    weak = torch.linalg.svd(_cross(z, t[:, None, :] - p).transpose(1, 2)[keep][:n])[2][:, 1]      # the joint direction of that value
    return q, weak


SPREAD = 0.1          # the starts of one target: start 0 and two configurations within SPREAD rad of it, joint by joint


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def moved_goal(tf64, q_start, rng, turn_range):
    """The fp64 pose of q_start (M, D) moved by 0.05-0.25 m in a random direction and turned by an angle of turn_range about a random
    axis, rounded once to fp32: (M, 3, 4)."""
    M = q_start.shape[0]
    R0, t0, _, _ = fk(tf64, q_start.double())
    d = torch.as_tensor(_unit(rng, M) * rng.uniform(0.05, 0.25, (M, 1)))
    Rt = rodrigues(torch.as_tensor(_unit(rng, M)), torch.as_tensor(rng.uniform(turn_range[0], turn_range[1], M)))
    return torch.cat([_matmul3(Rt, R0), (t0 + d)[:, :, None]], -1).float()


@functools.lru_cache(maxsize=None)
def inputs(name):
    """name -> robot, position_only, the fp32 starts (37, 3, D) and goals (37, 3, 4).  Start 0 of a target is a uniform configuration
    pulled to 0.7 of the way from the centre of the joint range; its two other starts lie within SPREAD rad of it joint by joint (the
    goal is ONE pose per target: k neighbouring grasp configurations approaching the same pose); the goal is start 0's fp64 pose moved
    by 0.05-0.25 m and turned by 0-0.6 rad, rounded once to fp32 (arm4_pos: see ON_SURFACE).  numpy.random.RandomState(SEEDS[name]).
    Treat as read-only."""
    robot = robot_of(name)
    rng = np.random.RandomState(SEEDS[name])
    tf64, lo, hi = chain(robot, torch.float64)
    mid = 0.5 * (lo + hi)
    base = mid + 0.7 * (uniform_q(robot, (N_TARGETS,), SEEDS[name]).double() - mid)
    if name in ON_SURFACE:
        base[1::2], weak = _weak_configurations(robot, tf64, mid, N_TARGETS // 2, SEEDS[name] + 1)
    near = torch.as_tensor(rng.uniform(-SPREAD, SPREAD, (N_TARGETS, N_STARTS, robot.q_dim)))
    near[:, 0] = 0.0
    starts = torch.minimum(torch.maximum(base[:, None, :] + near, lo), hi).float()
    if name in ON_SURFACE:
        dq = torch.as_tensor(rng.uniform(-ON_SURFACE[name], ON_SURFACE[name], (N_TARGETS, robot.q_dim)))
        dq[1::2] = WEAK_TURN * weak
        Rg, tg, _, _ = fk(tf64, torch.minimum(torch.maximum(starts[:, 0].double() + dq, lo), hi))
        goal = torch.cat([Rg, tg[:, :, None]], -1).float()
    else:
        goal = moved_goal(tf64, starts[:, 0], rng, (0.0, 0.6))
    return types.SimpleNamespace(name=name, robot=robot, position_only=name.endswith('_pos'), starts=starts, goal=goal)


@functools.lru_cache(maxsize=None)
def bad_inputs():
    """Panda, 8 targets x 1 start: the start's pose turned by pi - 0.05 about a random axis (beyond MAX_TURN), the position moved as above."""
    robot = robot_of('panda')
    rng = np.random.RandomState(31)
    tf64, lo, hi = chain(robot, torch.float64)
    mid = 0.5 * (lo + hi)
    starts = (mid + 0.7 * (uniform_q(robot, (8,), 31).double() - mid)).float()[:, None, :]
    goal = moved_goal(tf64, starts[:, 0], rng, (math.pi - 0.05, math.pi - 0.05))
    return types.SimpleNamespace(name='panda', robot=robot, position_only=False, starts=starts, goal=goal)


def solve(inp, dtype, K, n_inner, jump_max=JUMP_MAX, tol=(POS_TOL, ROT_TOL), limits=True):
    """The restatement on an input set in `dtype`; fields shaped (N, S, ...)."""
    N, S, D = inp.starts.shape
    tf, lo, hi = chain(inp.robot, dtype)
    out = cartesian_path(tf, inp.goal.to(dtype).repeat_interleave(S, 0), inp.starts.to(dtype).reshape(-1, D), K, n_inner,
                         pos_tol=tol[0], rot_tol=tol[1], jump_max=jump_max, position_only=inp.position_only, q_min=lo if limits else None, q_max=hi if limits else None)
    return types.SimpleNamespace(q=out.q.reshape(N, S, K + 1, D), pos_err=out.pos_err.reshape(N, S, K + 1), rot_err=out.rot_err.reshape(N, S, K + 1),
                                 n_ok=out.n_ok.reshape(N, S), status=out.status.reshape(N, S))


def _reference(inp, K, n_inner, jump_max, tol):
    r64, r32 = solve(inp, torch.float64, K, n_inner, jump_max, tol), solve(inp, torch.float32, K, n_inner, jump_max, tol)
    same = r64.n_ok == r32.n_ok
    E = lambda k: float((getattr(r32, k).double() - getattr(r64, k))[same].abs().max())
    # the fp32 restatement's own evaluation error: what it reports at its accepted rows against the fp64 error of those rows
    N, S, rows, D = r32.q.shape
    pe64, th64, _ = path_errors(chain(inp.robot, torch.float64)[0], inp.goal.repeat_interleave(S, 0), inp.starts.reshape(-1, D),
                                r32.q.reshape(-1, rows, D), inp.position_only)
    acc = torch.arange(rows)[None, None, :] <= r32.n_ok[:, :, None]
    Ev = lambda rep, tru: float((rep.double() - tru.reshape(N, S, rows))[acc].abs().max())
    return types.SimpleNamespace(r64=r64, r32=r32, same=same, E32_q=E('q'), E32_pos=E('pos_err'), E32_rot=E('rot_err'),
                                 E32_pos_eval=Ev(r32.pos_err, pe64), E32_rot_eval=Ev(r32.rot_err, th64))


@functools.lru_cache(maxsize=None)
def reference(name, K, n_inner, jump_max=JUMP_MAX, tol=(POS_TOL, ROT_TOL)):
    """Computed once per (set, K, n_inner, jump_max, tolerances) and shared: the fp64 and fp32 restatements, where their n_ok agree, E32 of q, pos_err
    and rot_err over those problems, and the fp32 restatement's evaluation error at its accepted rows.  Treat as read-only."""
    return _reference(bad_inputs() if name == 'bad' else inputs(name), K, n_inner, jump_max, tol)
