"""Timing of the batched Cartesian end-effector moves against the same recursion composed in batched torch on the device.

    python scripts/bench_cartesian.py [--reps 20] [--sizes 128,4096,32768] [--starts 4] [--steps 32] [--inner 8]

Shape: Panda, N targets x S starts, the default settings of ops.cartesian_path (K = 32 steps, at most 8 damped-least-squares iterations per
step, damping 0.1, 1e-3 m / 1e-2 rad, jump_max 0.5); start 0 of a target is uniform within the middle 70 % of the joint range, its other
starts lie within 0.1 rad of it, the goal is start 0's pose moved by 0.05-0.25 m and turned by 0-0.6 rad; min of `reps` timed calls (events
around one call each, after a warm-up).
  fused     ops.cartesian_path (mpb_cartesian_path: the step targets, walk, J J^T, Cholesky, step and the accept test in registers, one
            lane per problem, one launch)
  composed  per step: the target by Rodrigues' formula, then per iteration batched forward kinematics in torch (one small matmul per
            joint), the error, torch.linalg.solve of J J^T + damping^2 I, the clamped step, a converged or stopped problem kept by
            torch.where (no early exit: the work a batched torch loop does), then the accept test and the row
Prints one line per N and a JSON line with all figures (milliseconds).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from motion_planning_baselines_amd import geometry as G, ops          # noqa: E402
from bench_ik import time_min, torch_fk                               # noqa: E402


def rot_error(Rs, R):
    E = Rs @ R.transpose(1, 2)
    w = 0.5 * torch.stack([E[:, 2, 1] - E[:, 1, 2], E[:, 0, 2] - E[:, 2, 0], E[:, 1, 0] - E[:, 0, 1]], -1)
    nw = torch.linalg.norm(w, dim=-1)
    return w, nw, torch.atan2(nw, 0.5 * (E.diagonal(dim1=1, dim2=2).sum(-1) - 1.0))


def hat(a):
    z = torch.zeros_like(a[:, 0])
    return torch.stack([torch.stack([z, -a[:, 2], a[:, 1]], -1), torch.stack([a[:, 2], z, -a[:, 0]], -1), torch.stack([-a[:, 1], a[:, 0], z], -1)], 1)


def torch_cartesian(tf, target, q0, lo, hi, K, n_inner, damping, pos_tol, rot_tol, jump_max):
    M = q0.shape[0]
    eye6 = damping * damping * torch.eye(6, device=q0.device)
    eye3 = torch.eye(3, device=q0.device)
    R0, t0, _, _ = torch_fk(tf, q0)
    w, nw, theta = rot_error(target[:, :, :3], R0)
    active = theta <= ops.CART_MAX_TURN
    status = torch.where(active, ops.CART_OK, ops.CART_BAD_TARGET).to(torch.int32)
    theta = torch.where(nw < 1e-6, torch.zeros_like(theta), theta)
    A = hat(w / nw.clamp_min(1e-6)[:, None])
    AA = A @ A
    qa, n_ok, rows = q0, torch.zeros(M, dtype=torch.int32, device=q0.device), [q0]
    for k in range(1, K + 1):
        s = k / K
        phi = (s * theta)[:, None, None]
        Rk = (eye3 + torch.sin(phi) * A + (1.0 - torch.cos(phi)) * AA) @ R0
        tk = (1.0 - s) * t0 + s * target[:, :, 3]
        q = qa
        for it in range(n_inner + 1):
            R, t, z, p = torch_fk(tf, q)
            w, nw, th = rot_error(Rk, R)
            ep = tk - t
            conv = (torch.linalg.norm(ep, dim=-1) <= pos_tol) & (th <= rot_tol)
            if it == n_inner:
                break
            e = torch.cat([ep, (th / nw.clamp_min(1e-6))[:, None] * w], -1)
            J = torch.cat([torch.linalg.cross(z, t[:, None, :] - p, dim=-1), z], -1).transpose(1, 2)      # (M, 6, D)
            y = torch.linalg.solve(J @ J.transpose(1, 2) + eye6, e)
            qn = torch.minimum(torch.maximum(q + (J.transpose(1, 2) @ y[:, :, None])[:, :, 0], lo), hi)
            q = torch.where((conv | ~active)[:, None], q, qn)
        jumped = (q - qa).abs().amax(-1) > jump_max
        accept = active & conv & ~jumped
        status = torch.where(active & ~conv, ops.CART_LOST, torch.where(active & conv & jumped, ops.CART_JUMP, status)).to(torch.int32)
        n_ok = torch.where(accept, k, n_ok).to(torch.int32)
        qa = torch.where(accept[:, None], q, qa)
        rows.append(qa)
        active = accept
    return torch.stack(rows, 1), n_ok, status


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--sizes', default='128,4096,32768')
    ap.add_argument('--starts', type=int, default=4)
    ap.add_argument('--steps', type=int, default=32)
    ap.add_argument('--inner', type=int, default=8)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    robot = G.RobotPanda()
    geom = ops.DeviceGeometry(robot, G.env_spheres_3d(), dev)
    tf = torch.as_tensor(robot.spec()['joint_tf'], dtype=torch.float32, device=dev)
    lo, hi = robot.q_min.to(dev), robot.q_max.to(dev)
    S, D, K = args.starts, robot.q_dim, args.steps
    rng = np.random.RandomState(0)
    rows = []
    for N in [int(v) for v in args.sizes.split(',')]:
        mid, half = 0.5 * (robot.q_min_np + robot.q_max_np), 0.5 * (robot.q_max_np - robot.q_min_np)
        base = mid + 0.7 * half * rng.uniform(-1.0, 1.0, (N, 1, D))
        near = rng.uniform(-0.1, 0.1, (N, S, D))
        near[:, 0] = 0.0
        starts = torch.from_numpy(np.clip(base + near, robot.q_min_np, robot.q_max_np).astype(np.float32)).to(dev)
        pose = ops.fk_ee_pose(starts[:, 0].contiguous(), geom)
        d = rng.standard_normal((N, 3))
        d *= rng.uniform(0.05, 0.25, (N, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
        a = rng.standard_normal((N, 3))
        a /= np.linalg.norm(a, axis=1, keepdims=True)
        A = hat(torch.from_numpy(a.astype(np.float32)).to(dev))
        ang = torch.from_numpy(rng.uniform(0.0, 0.6, N).astype(np.float32)).to(dev)[:, None, None]
        Rt = torch.eye(3, device=dev) + torch.sin(ang) * A + (1.0 - torch.cos(ang)) * (A @ A)
        goal = torch.cat([Rt @ pose[:, :, :3], (pose[:, :, 3] + torch.from_numpy(d.astype(np.float32)).to(dev))[:, :, None]], -1).contiguous()
        flat_g, flat_q = goal.repeat_interleave(S, 0), starts.reshape(-1, D)
        fused = lambda: ops.cartesian_path(goal, starts, geom, K, n_inner=args.inner, q_min=lo, q_max=hi)
        composed = lambda: torch_cartesian(tf, flat_g, flat_q, lo, hi, K, args.inner, 0.1, 1e-3, 1e-2, 0.5)
        n_ok, status = fused()[3:]
        n_ok_t = composed()[1].reshape(N, S)
        row = dict(N=N, S=S, K=K, n_inner=args.inner, fused_ms=time_min(fused, args.reps), composed_ms=time_min(composed, args.reps),
                   complete_share=float((status == ops.CART_OK).float().mean()), mean_fraction=float(n_ok.float().mean()) / K,
                   n_ok_agrees_with_composed=float((n_ok == n_ok_t).float().mean()))
        rows.append(row)
        print('N x S = %6d x %d: fused %.3f ms, composed %.3f ms; complete %.3f, mean fraction %.3f, n_ok as composed on %.4f' %
              (N, S, row['fused_ms'], row['composed_ms'], row['complete_share'], row['mean_fraction'], row['n_ok_agrees_with_composed']), flush=True)
        del starts, goal, flat_g, flat_q
        torch.cuda.empty_cache()
    print(json.dumps(dict(bench='cartesian', robot='panda', reps=args.reps, rows=rows)))


if __name__ == '__main__':
    main()
