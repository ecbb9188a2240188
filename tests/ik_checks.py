"""The end-effector pose, its geometric Jacobian and the damped-least-squares inverse kinematics of DESIGN.md section 10, restated
from the definition alone (helper module; imported like collision_kinks.py).  Nothing here reads the code under test: the chain
is a robot's spec()['joint_tf'] and its joint limits, the arithmetic is torch on the CPU.

Every function takes the dtype from its inputs.  In fp64 it is the reference; in fp32 it walks the same operation order -- the chain
frame by frame, the entries of J J^T joint by joint, the unpivoted Cholesky row by row, the two substitutions -- in separate fp32
roundings, and its distance from fp64 on the same inputs is E32, the source of every bar: collision_kinks.bar(E32).

  pose:  frame_{j+1} = frame_j P_j Rz(q_j), the end effector is frame_{D+1} = [R | t]
  J:     rows 0-2  z_j x (t - p_j),  rows 3-5  z_j   (z_j, p_j: axis and origin of joint j)
  error: e_p = t* - t;  E = R* R^T, w = vee(E - E^T) / 2, c = (tr E - 1) / 2, theta = atan2(|w|, c), e_w = (theta / |w|) w
         (plain w when |w| < 1e-6)
  step:  dq = J^T (J J^T + damping^2 I)^{-1} e,  q <- clamp(q + dq);  a converged problem is frozen
"""
import functools
import types

import numpy as np
import torch

from collision_kinks import DELTA, bar  # noqa: F401  (re-exported: the tests take them from here)

N_TARGETS, N_SEEDS = 64, 32
N_ITERS, DAMPING, POS_TOL, ROT_TOL = 64, 0.1, 1e-3, 1e-2
SETS = ('panda', 'panda_pos', 'arm12', 'arm9', 'arm4_pos')


def chain(robot, dtype):
    """(joint_tf (D+1, 3, 4), q_min (D,), q_max (D,)) of a product robot in `dtype`: the fp32 numbers the device is given."""
    tf = torch.as_tensor(np.asarray(robot.spec()['joint_tf'], dtype=np.float32)).to(dtype)
    assert tf.shape[0] == robot.q_dim + 1
    return tf, torch.as_tensor(robot.q_min_np).to(dtype), torch.as_tensor(robot.q_max_np).to(dtype)


def fk(tf, q):
    """q (M, D) -> R (M, 3, 3), t (M, 3), z (M, D, 3), p (M, D, 3)."""
    M, D = q.shape
    R = [[torch.full((M,), 1.0 if a == b else 0.0, dtype=q.dtype) for b in range(3)] for a in range(3)]
    t = [torch.zeros(M, dtype=q.dtype) for _ in range(3)]
    zs, ps = [], []
    for j in range(D + 1):
        P = tf[j]
        t = [((t[a] + R[a][0] * P[0, 3]) + R[a][1] * P[1, 3]) + R[a][2] * P[2, 3] for a in range(3)]
        A = [[(R[a][0] * P[0, b] + R[a][1] * P[1, b]) + R[a][2] * P[2, b] for b in range(3)] for a in range(3)]
        if j < D:
            c, s = torch.cos(q[:, j]), torch.sin(q[:, j])
            for a in range(3):
                A[a][0], A[a][1] = A[a][0] * c + A[a][1] * s, A[a][1] * c - A[a][0] * s
            zs.append(torch.stack([A[0][2], A[1][2], A[2][2]], -1))
            ps.append(torch.stack(t, -1))
        R = A
    return (torch.stack([torch.stack(r, -1) for r in R], -2), torch.stack(t, -1), torch.stack(zs, 1), torch.stack(ps, 1))


def pose_jacobian(tf, q):
    """q (M, D) -> pose (M, 3, 4) = [R | t] and J (M, 6, D)."""
    R, t, z, p = fk(tf, q)
    return torch.cat([R, t[:, :, None]], -1), torch.cat([_cross(z, t[:, None, :] - p), z], -1).transpose(1, 2)


def _cross(a, b):
    return torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _norm3(v):
    return torch.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def pose_error(target, R, t):
    """-> e (M, 6), |e_p| (M,), theta (M,)"""
    ep = target[:, :, 3] - t
    Rs = target[:, :, :3]
    E = [[(Rs[:, a, 0] * R[:, b, 0] + Rs[:, a, 1] * R[:, b, 1]) + Rs[:, a, 2] * R[:, b, 2] for b in range(3)] for a in range(3)]
    w = torch.stack([0.5 * (E[2][1] - E[1][2]), 0.5 * (E[0][2] - E[2][0]), 0.5 * (E[1][0] - E[0][1])], -1)
    c = 0.5 * (((E[0][0] + E[1][1]) + E[2][2]) - 1.0)
    nw = _norm3(w)
    theta = torch.atan2(nw, c)
    small = nw < 1e-6
    scale = torch.where(small, torch.ones_like(nw), theta / torch.where(small, torch.ones_like(nw), nw))
    return torch.cat([ep, scale[:, None] * w], -1), _norm3(ep), theta


def dls_step(J, e, damping):
    """dq (M, D) = J^T (J J^T + damping^2 I)^{-1} e; J (M, n, D), e (M, n), n = 6 or 3.  Unpivoted Cholesky, reciprocal pivots."""
    M, n, D = J.shape
    lam2 = torch.tensor(damping, dtype=J.dtype) * torch.tensor(damping, dtype=J.dtype)
    A = [[None] * n for _ in range(n)]
    for a in range(n):
        for b in range(a + 1):
            acc = J[:, a, 0] * J[:, b, 0]
            for j in range(1, D):
                acc = acc + J[:, a, j] * J[:, b, j]
            A[a][b] = acc + lam2 if a == b else acc
    L, inv = [[None] * n for _ in range(n)], [None] * n
    for i in range(n):
        for j in range(i + 1):
            s = A[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            if i == j:
                L[i][i] = torch.sqrt(s)
                inv[i] = 1.0 / L[i][i]
            else:
                L[i][j] = s * inv[j]
    y = [None] * n
    for i in range(n):
        s = e[:, i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s * inv[i]
    x = [None] * n
    for i in reversed(range(n)):
        s = y[i]
        for k in range(i + 1, n):
            s = s - L[k][i] * x[k]
        x[i] = s * inv[i]
    dq = []
    for j in range(D):
        acc = J[:, 0, j] * x[0]
        for a in range(1, n):
            acc = acc + J[:, a, j] * x[a]
        dq.append(acc)
    return torch.stack(dq, -1)


def ik_solve(tf, target, q0, n_iters=N_ITERS, damping=DAMPING, pos_tol=POS_TOL, rot_tol=ROT_TOL, position_only=False,
             q_min=None, q_max=None):
    """target (M, 3, 4), q0 (M, D) -> namespace(q, pos_err, rot_err, converged, iters), everything at the returned q."""
    q = q0.clone()
    used = torch.zeros(q.shape[0], dtype=torch.int32)
    n = 3 if position_only else 6
    for it in range(n_iters + 1):
        R, t, z, p = fk(tf, q)
        e, pe, th = pose_error(target, R, t)
        conv = (pe <= pos_tol) & ((th <= rot_tol) | bool(position_only))
        if it == n_iters or bool(conv.all()):
            break
        J = torch.cat([_cross(z, t[:, None, :] - p), z], -1).transpose(1, 2)
        qn = q + dls_step(J[:, :n], e[:, :n], damping)
        if q_min is not None:
            qn = torch.minimum(torch.maximum(qn, q_min), q_max)
        q = torch.where(conv[:, None], q, qn)
        used = used + (~conv).to(torch.int32)
    return types.SimpleNamespace(q=q, pos_err=pe, rot_err=th, converged=conv, iters=used)


# ------------------------------------------------------------------------------------------------
# the input sets shared by tests/test_ik_cpu.py and tests/test_gpu_ik.py
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def robot_of(name):
    from motion_planning_baselines_amd import geometry as G
    from test_gpu_generic_dof import make_arm
    return G.RobotPanda() if name.startswith('panda') else make_arm(int(name.split('_')[0][3:]))


def uniform_q(robot, shape, seed):
    """fp32 configurations uniform within the joint limits, numpy.random.RandomState(seed)."""
    rng = np.random.RandomState(seed)
    return torch.as_tensor(rng.uniform(robot.q_min_np.astype(np.float64), robot.q_max_np.astype(np.float64),
                                       tuple(shape) + (robot.q_dim,)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """name -> robot, position_only, the fp32 targets (64, 3, 4) (fp64 FK of RandomState(0) configurations, rounded once: both
    precisions and the device start from these numbers) and seeds (64, 32, D) (RandomState(1)).  Treat as read-only."""
    robot = robot_of(name)
    tf64, _, _ = chain(robot, torch.float64)
    q_t = uniform_q(robot, (N_TARGETS,), 0)
    target = pose_jacobian(tf64, q_t.double())[0].float()
    seeds = uniform_q(robot, (N_TARGETS, N_SEEDS), 1)
    return types.SimpleNamespace(name=name, robot=robot, position_only=name.endswith('_pos'), target=target, seeds=seeds, q_targets=q_t)


def solve_set(name, dtype, n_iters=N_ITERS, limits=True, target=None, seeds=None):
    """The restatement on a set's (or the given) inputs in `dtype`; fields shaped (N, S, ...)."""
    inp = inputs(name)
    target = inp.target if target is None else target
    seeds = inp.seeds if seeds is None else seeds
    N, S, D = seeds.shape
    tf, lo, hi = chain(inp.robot, dtype)
    out = ik_solve(tf, target.to(dtype).repeat_interleave(S, 0), seeds.to(dtype).reshape(-1, D), n_iters=n_iters,
                   position_only=inp.position_only, q_min=lo if limits else None, q_max=hi if limits else None)
    return types.SimpleNamespace(q=out.q.reshape(N, S, D), pos_err=out.pos_err.reshape(N, S), rot_err=out.rot_err.reshape(N, S),
                                 converged=out.converged.reshape(N, S), iters=out.iters.reshape(N, S))


@functools.lru_cache(maxsize=None)
def reference(name, n_iters=N_ITERS, limits=True):
    """Computed once per (set, budget, limits) and shared: the fp64 and fp32 restatements and E32 of q, pos_err and rot_err."""
    r64, r32 = solve_set(name, torch.float64, n_iters, limits), solve_set(name, torch.float32, n_iters, limits)
    E = lambda k: float((getattr(r32, k).double() - getattr(r64, k)).abs().max())
    return types.SimpleNamespace(r64=r64, r32=r32, E32_q=E('q'), E32_pos=E('pos_err'), E32_rot=E('rot_err'))


def fk_error(name, target, q):
    """fp64 pose error of configurations q (N, S, D) against target (N, 3, 4): |e_p| and theta, (N, S) each."""
    inp = inputs(name)
    N, S, D = q.shape
    tf, _, _ = chain(inp.robot, torch.float64)
    R, t, _, _ = fk(tf, q.double().reshape(-1, D))
    _, pe, th = pose_error(target.double().repeat_interleave(S, 0), R, t)
    return pe.reshape(N, S), th.reshape(N, S)


@functools.lru_cache(maxsize=None)
def free_scene():
    """Panda among env_spheres_3d(): targets = fp64 FK of the first 64 collision-free of 4 000 uniform configurations (RandomState(2);
    free by the fp64 oracle's collision cost), the seeds of the other sets, the fp64 restatement's solutions and which of them are
    converged AND free by the oracle.  Treat as read-only."""
    from motion_planning_baselines_amd import geometry as G
    from oracle.geometry_ref import make_ref_geometry
    robot, field = robot_of('panda'), G.env_spheres_3d()
    rr, rf = make_ref_geometry(robot, field, dict(device='cpu', dtype=torch.float64))
    in_collision = lambda q: rf.compute_cost(None, rr.fk_map_collision(q.double())) > 0
    cand = uniform_q(robot, (4000,), 2)
    q_t = cand[~in_collision(cand)][:N_TARGETS]
    assert q_t.shape[0] == N_TARGETS
    target = pose_jacobian(chain(robot, torch.float64)[0], q_t.double())[0].float()
    seeds = uniform_q(robot, (N_TARGETS, N_SEEDS), 1)
    r64 = solve_set('panda', torch.float64, target=target, seeds=seeds)
    free64 = r64.converged & ~in_collision(r64.q.reshape(-1, robot.q_dim)).reshape(N_TARGETS, N_SEEDS)
    return types.SimpleNamespace(robot=robot, field=field, target=target, seeds=seeds, r64=r64, free64=free64)
