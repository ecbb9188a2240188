"""Timing of the self-collision kernels against the composed route on the device.

    python scripts/bench_self_collision.py [--reps 20] [--sizes 128,4096,131072]

Shape: Panda, H = 64, d = 7, N trajectories; min of `reps` timed calls (events around one call each, after a warm-up).
  fused     ops.self_collision_eval / ops.self_collision_grad (mpb_self_collision_*: FK, pair loop and J^T in one kernel)
  composed  ops.fk_collision_points, then torch gather / norm / relu over the same pair list; the gradient by torch autograd through
            robot_field.DeviceRobot.fk_map_collision (whose backward is mpb_fk_collision_points_vjp)
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
from motion_planning_baselines_amd.robot_field import device_robot_field  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--sizes', default='128,4096,131072')
    ap.add_argument('--H', type=int, default=64)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    robot = G.RobotPanda()
    field = G.SelfCollisionField(robot)
    sc = ops.DeviceSelfCollision(robot, field, dev)
    drobot, _ = device_robot_field(robot, G.CollisionField(spheres=[[1.0e6, 1.0e6, 1.0e6, 1.0]]), dev)
    pa = torch.as_tensor(field.pairs[:, 0], device=dev)
    pb = torch.as_tensor(field.pairs[:, 1], device=dev)
    T = torch.as_tensor(field.thresholds(), dtype=torch.float32, device=dev)
    H, D = args.H, robot.q_dim
    rng = np.random.RandomState(0)
    rows = []
    for N in [int(v) for v in args.sizes.split(',')]:
        x = torch.from_numpy(rng.uniform(robot.q_min_np, robot.q_max_np, (N, H, D)).astype(np.float32)).to(dev)

        def composed_cost(q):
            pts = drobot.fk_map_collision(q)
            n = torch.sqrt(((pts[..., pa, :] - pts[..., pb, :]) ** 2).sum(-1).clamp_min(1e-30))
            return torch.relu(T - n).sum(-1)[:, 1:].sum(-1)

        def composed_eval():
            with torch.no_grad():
                return composed_cost(x)

        def composed_grad():
            q = x.detach().requires_grad_(True)
            return torch.autograd.grad(composed_cost(q).sum(), q)[0]
        f_eval, f_grad = ops.self_collision_eval(x, sc, 1.0), ops.self_collision_grad(x, sc, 1.0)[1]
        c_eval, c_grad = composed_eval(), composed_grad()
        row = dict(N=N, H=H,
                   eval_fused_ms=time_min(lambda: ops.self_collision_eval(x, sc, 1.0), args.reps),
                   eval_composed_ms=time_min(composed_eval, args.reps),
                   grad_fused_ms=time_min(lambda: ops.self_collision_grad(x, sc, 1.0), args.reps),
                   grad_composed_ms=time_min(composed_grad, args.reps),
                   eval_max_abs_diff=float((f_eval - c_eval).abs().max()), grad_max_abs_diff=float((f_grad - c_grad).abs().max()))
        rows.append(row)
        print('N = %6d: eval fused %.3f ms, composed %.3f ms; grad fused %.3f ms, composed %.3f ms' %
              (N, row['eval_fused_ms'], row['eval_composed_ms'], row['grad_fused_ms'], row['grad_composed_ms']), flush=True)
        del x, f_eval, f_grad, c_eval, c_grad
        torch.cuda.empty_cache()
    print(json.dumps(dict(bench='self_collision', robot='panda', pairs=int(len(field.pairs)), reps=args.reps, rows=rows)))


if __name__ == '__main__':
    main()
