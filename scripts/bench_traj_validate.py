"""Validation of a trajectory batch, Panda + env_spheres_3d, H = 64, n_interp = 5 (P = 379 dense points a trajectory), on the
(N, H, 14) state tensor a planner returns, at N = 128, 4 096 and 131 072 (C5's per-GPU load):

  fused     ops.traj_collision_stats on the state tensor in place (one launch of mpb_traj_collision_stats, no dense point stored);
  composed  the route the ops offered before it: a contiguous copy of the position half, ops.traj_interpolate (N x P x 7 floats
            materialised), ops.collision_check(with_gap) on the N * P points, then any / sum / max / first index in torch.

Timing: warm-up calls of both routes first, then HIP events around each call, the two routes alternating, min and median
over the repeats.  Both routes return the same four per-trajectory answers; the script checks that they agree before it
times them.  One size per process keeps a failure at one size from the others:

    timeout -k 10 300 python scripts/bench_traj_validate.py --n 4096 [--json OUT]

Without --n the three sizes run one after the other.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from motion_planning_baselines_amd import geometry as G, ops  # noqa: E402
from motion_planning_baselines_amd.robot_field import PlanningTask  # noqa: E402

H, N_INTERP, D, WARMUP = 64, 5, 7, 3
P = (H - 1) * (N_INTERP + 1) + 1


def make_states(task, N, seed=11):
    """(N, H, 2D) states: a short line between two configurations within the joint limits plus a sine bump (about a third of
    the dense points in collision, about half of the trajectories free); the velocity half is finite differences' stand-in."""
    gen = torch.Generator(device=task.device)
    gen.manual_seed(seed)
    span = task.q_max - task.q_min
    u = torch.rand(3, N, 1, D, device=task.device, generator=gen)
    a = task.q_min + span * u[0]
    t = torch.linspace(0, 1, H, device=task.device)[None, :, None]
    pos = a + 0.15 * span * (2 * u[1] - 1) * t + 0.05 * span * torch.sin(torch.pi * t) * (2 * u[2] - 1)
    return torch.cat([pos, torch.zeros_like(pos)], dim=-1).contiguous()


def fused(task, states):
    return ops.traj_collision_stats(states, task.geom, n_interp=N_INTERP)


def composed(task, states):
    pos = states[..., :D].contiguous()
    dense = ops.traj_interpolate(pos, N_INTERP)
    flag, gap = ops.collision_check(dense.reshape(-1, D), task.geom, with_gap=True)
    flag = flag.reshape(states.shape[0], P)
    count = flag.sum(1, dtype=torch.int32)
    first = torch.where(flag, torch.arange(P, device=flag.device, dtype=torch.int32), P).min(1)[0]
    first = torch.where(first == P, -1, first).to(torch.int32)
    return count, first, gap.reshape(states.shape[0], P).max(1)[0]


def timed(fn, task, states):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn(task, states)
    e1.record()
    torch.cuda.synchronize()
    del out
    return e0.elapsed_time(e1) * 1e-3


def bench(task, N, repeats):
    states = make_states(task, N)
    for _ in range(WARMUP):
        a, b = fused(task, states), composed(task, states)
    torch.cuda.synchronize()
    same = [bool(torch.equal(x, y)) for x, y in zip(a, b)]
    free = float((a[0] == 0).float().mean())
    intensity = float(a[0].sum(dtype=torch.int64)) / (N * P)
    del a, b
    tf, tc = [], []
    for _ in range(repeats):
        tf.append(timed(fused, task, states))
        tc.append(timed(composed, task, states))
    row = dict(N=N, H=H, n_interp=N_INTERP, P=P, fraction_free=free, collision_intensity=intensity, outputs_equal=same,
               fused_min_s=min(tf), fused_median_s=statistics.median(tf), composed_min_s=min(tc), composed_median_s=statistics.median(tc),
               dense_bytes_not_materialised=N * P * D * 4, points_per_s_fused=N * P / min(tf))
    print(f'N={N:7d}: fused min {min(tf) * 1e3:.3f} ms, median {row["fused_median_s"] * 1e3:.3f} ms; composed min {min(tc) * 1e3:.3f} ms, '
          f'median {row["composed_median_s"] * 1e3:.3f} ms; composed / fused (min) {min(tc) / min(tf):.2f}; {row["points_per_s_fused"] / 1e9:.2f} G points/s '
          f'fused; free {free:.3f}, intensity {intensity:.3f}; count / first / max_gap equal to the composed route: {same}', flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=None, help='one size (default: 128, 4096 and 131072 in turn)')
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    task = PlanningTask(G.RobotPanda(), G.env_spheres_3d(seed=0), tensor_args=dict(device=dev, dtype=torch.float32))
    rows = [bench(task, N, args.repeats) for N in ([args.n] if args.n else [128, 4096, 131072])]
    res_path = os.path.join(ROOT, 'motion_planning_baselines_amd', 'csrc', 'kernel_resources.json')
    if os.path.exists(res_path):
        for name, r in json.load(open(res_path)).items():
            if 'traj_collision_stats_kernel' in name:
                print(f'{name}: {r.get("vgprs")} VGPRs, {r.get("lds")} B LDS, occupancy {r.get("occupancy")}, scratch {r.get("scratch")}')
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(dict(rows=rows), fh, indent=1)


if __name__ == '__main__':
    main()
