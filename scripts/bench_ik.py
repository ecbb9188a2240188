"""Timing of the batched inverse kinematics against the same iteration composed in torch on the device.

    python scripts/bench_ik.py [--reps 20] [--sizes 128,4096,32768] [--seeds 32] [--iters 64]

Shape: Panda, N targets x S seeds, n_iters damped-least-squares steps (damping 0.1, 1e-3 m / 1e-2 rad); min of `reps` timed calls
(events around one call each, after a warm-up).
  fused     ops.ik_solve (mpb_ik_solve: walk, J J^T, Cholesky and step in registers, one lane per problem, one launch)
  composed  per iteration: batched forward kinematics in torch (one small matmul per joint), the error, torch.linalg.solve of
            J J^T + damping^2 I, the clamped step; every problem steps every iteration (no freezing, no early exit: the work a batched
            torch loop does), n_iters iterations
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


def time_min(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float('inf')
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def torch_fk(tf, q):
    """q (M, D) -> R (M, 3, 3), t (M, 3), z (M, D, 3), p (M, D, 3): the chain walk, batched over the problems."""
    M, D = q.shape
    R = torch.eye(3, device=q.device).expand(M, 3, 3)
    t = torch.zeros(M, 3, device=q.device)
    zs, ps = [], []
    c, s = torch.cos(q), torch.sin(q)
    for j in range(D + 1):
        t = t + R @ tf[j, :, 3]
        R = R @ tf[j, :, :3]
        if j < D:
            cj, sj = c[:, j, None], s[:, j, None]
            R = torch.stack([R[:, :, 0] * cj + R[:, :, 1] * sj, R[:, :, 1] * cj - R[:, :, 0] * sj, R[:, :, 2]], -1)
            zs.append(R[:, :, 2])
            ps.append(t)
    return R, t, torch.stack(zs, 1), torch.stack(ps, 1)


def torch_ik(tf, target, q, lo, hi, n_iters, damping):
    eye = damping * damping * torch.eye(6, device=q.device)
    for _ in range(n_iters):
        R, t, z, p = torch_fk(tf, q)
        E = target[:, :, :3] @ R.transpose(1, 2)
        w = 0.5 * torch.stack([E[:, 2, 1] - E[:, 1, 2], E[:, 0, 2] - E[:, 2, 0], E[:, 1, 0] - E[:, 0, 1]], -1)
        nw = torch.linalg.norm(w, dim=-1)
        theta = torch.atan2(nw, 0.5 * (E.diagonal(dim1=1, dim2=2).sum(-1) - 1.0))
        e = torch.cat([target[:, :, 3] - t, (theta / nw.clamp_min(1e-6))[:, None] * w], -1)
        J = torch.cat([torch.linalg.cross(z, t[:, None, :] - p, dim=-1), z], -1).transpose(1, 2)          # (M, 6, D)
        y = torch.linalg.solve(J @ J.transpose(1, 2) + eye, e)
        q = torch.minimum(torch.maximum(q + (J.transpose(1, 2) @ y[:, :, None])[:, :, 0], lo), hi)
    return q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--sizes', default='128,4096,32768')
    ap.add_argument('--seeds', type=int, default=32)
    ap.add_argument('--iters', type=int, default=64)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    robot = G.RobotPanda()
    geom = ops.DeviceGeometry(robot, G.env_spheres_3d(), dev)
    tf = torch.as_tensor(robot.spec()['joint_tf'], dtype=torch.float32, device=dev)
    lo, hi = robot.q_min.to(dev), robot.q_max.to(dev)
    S, D = args.seeds, robot.q_dim
    rng = np.random.RandomState(0)
    rows = []
    for N in [int(v) for v in args.sizes.split(',')]:
        u = lambda *shape: torch.from_numpy(rng.uniform(robot.q_min_np, robot.q_max_np, shape + (D,)).astype(np.float32)).to(dev)
        target = ops.fk_ee_pose(u(N), geom)
        seeds = u(N, S)
        flat_t, flat_q = target.repeat_interleave(S, 0), seeds.reshape(-1, D)
        fused = lambda: ops.ik_solve(target, seeds, geom, q_min=lo, q_max=hi, n_iters=args.iters, damping=0.1)
        composed = lambda: torch_ik(tf, flat_t, flat_q, lo, hi, args.iters, 0.1)
        conv = fused()[3]
        row = dict(N=N, S=S, n_iters=args.iters, fused_ms=time_min(fused, args.reps), composed_ms=time_min(composed, args.reps),
                   converged_share=float(conv.float().mean()), targets_solved=float(conv.any(1).float().mean()))
        rows.append(row)
        print('N x S = %6d x %d: fused %.3f ms, composed %.3f ms; converged share %.3f, targets with a solution %.3f' %
              (N, S, row['fused_ms'], row['composed_ms'], row['converged_share'], row['targets_solved']), flush=True)
        del target, seeds, flat_t, flat_q
        torch.cuda.empty_cache()
    print(json.dumps(dict(bench='ik', robot='panda', reps=args.reps, rows=rows)))


if __name__ == '__main__':
    main()
