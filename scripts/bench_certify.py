"""Path certification (mpb_path_certify), Panda + 16 spheres: RRT-Connect paths (step pi/80, radius pi/4, n_iters 2000, pool 2000) of
N = 128 and 4 096 independent start / goal problems, before and after 64 shortcut iterations, certified at the default arguments (and once
more at c_req = -margin / 10: these planners stop their extensions ON the margin surface, where no positive clearance can be proved).

Compared on the same paths: ops.traj_collision_stats, the sampled validator, at its default n_interp = 5 and at
n_interp = 2^depth_max - 1 -- the sampled check at the finest resolution the certificate went to (depth_max: the deepest level any path
of the batch reached).  The found paths are laid out as (n, Lmax, D) with the last node repeated past a path's length, so that both
kernels read the same rows (a repeated node is a zero-length segment: free wherever the node is).  No ratio is claimed: the sampled check
proves nothing between its samples at either resolution.

Timing: warm-up first, HIP events around each launch, 20 repeats, the minimum.  Also printed: the status shares, the mean number of
configurations a path's certificate evaluated, and how many paths the sampled check passes that the certifier refuses.

    python scripts/bench_certify.py [--json OUT]
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from motion_planning_baselines_amd import geometry as G, ops, workloads  # noqa: E402
from motion_planning_baselines_amd.planners.rrt_connect import RRTConnect  # noqa: E402
from motion_planning_baselines_amd.robot_field import PlanningTask  # noqa: E402

dev = torch.device('cuda:0')
ta = dict(device=dev, dtype=torch.float32)
robot, field = G.RobotPanda(), G.env_spheres_3d(seed=0)
task = PlanningTask(robot, field, tensor_args=ta, seed=5)
STEP, RADIUS, N_ITERS_RRT, N_PRE, LMAX, ITERS, REPEATS, WARMUP = np.pi / 80, np.pi / 4, 2000, 2000, 512, 64, 20, 2
pool = task.random_coll_free_q(N_PRE)


def rrt_paths(N):
    q = torch.from_numpy(workloads.collision_free_configs(robot, field, 2 * N, 91, dev))
    planner = RRTConnect(task=task, n_iters=N_ITERS_RRT, start_state_pos=q[:N], goal_state_pos=q[N:], step_size=STEP, n_radius=RADIUS,
                         tensor_args=ta, n_pre_samples=N_PRE, pre_samples=pool, max_path_nodes=LMAX, seed=7)
    paths, lengths, status = planner.optimize_batched()
    return paths.contiguous(), lengths.contiguous(), status == ops.RRT_FOUND


def as_trajs(paths, lengths, found):
    """The found paths as (n, Lmax, D), the last node repeated past a path's length."""
    p, ln = paths[found], lengths[found].long()
    H = max(int(ln.max()), 2)
    rows = torch.minimum(torch.arange(H, device=dev)[None, :], (ln - 1)[:, None])
    return torch.gather(p[:, :H], 1, rows[:, :, None].expand(-1, -1, p.shape[-1])).contiguous()


def timed(fn):
    for _ in range(WARMUP):
        fn()
    best, out = float('inf'), None
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e-3)
    return best, out


rows = []
for N in (128, 4096):
    paths, lengths, found = rrt_paths(N)
    short, short_len, _ = task.shortcut_paths(paths, lengths, n_iters=ITERS, check_step=STEP)
    for label, (p, ln) in (('rrt', (paths, lengths)), ('shortcut', (short, short_len))):
        trajs = as_trajs(p, ln, found)
        n, H = trajs.shape[0], trajs.shape[1]
        t_cert, cert = timed(lambda: task.certify_trajs(trajs))
        depth = max(int(cert.depth_max.max()), 0)
        fine = 2 ** depth - 1
        t_s5, s5 = timed(lambda: ops.traj_collision_stats(trajs, task.geom, n_interp=5))
        t_sf, sf = timed(lambda: ops.traj_collision_stats(trajs, task.geom, n_interp=fine))
        share = {name: float((cert.status == k).float().mean()) for k, name in enumerate(ops.CERT_STATUS_NAMES)}
        # the RRT planners stop extensions on the margin surface: the same paths held to 90 % of the margin (c_req = -margin / 10)
        relaxed = task.certify_trajs(trajs, c_req=-0.1 * field.margin)
        share_relaxed = {name: float((relaxed.status == k).float().mean()) for k, name in enumerate(ops.CERT_STATUS_NAMES)}
        row = dict(N=N, paths=label, found=n, rows=H, nodes_mean=float(ln[found].float().mean()), certify_seconds_min=t_cert,
                   n_evals_mean=float(cert.n_evals.float().mean()), depth_max=depth, status_share=share, status_share_relaxed=share_relaxed,
                   sampled_fine_collision_certifier_free=int(((sf[0] > 0) & cert.free).sum()),
                   sampled5_seconds_min=t_s5, sampled_fine_seconds_min=t_sf, n_interp_fine=fine,
                   sampled5_free_certifier_collision=int(((s5[0] == 0) & cert.collision).sum()),
                   sampled_fine_free_certifier_collision=int(((sf[0] == 0) & cert.collision).sum()),
                   sampled5_collision=int((s5[0] > 0).sum()), sampled_fine_collision=int((sf[0] > 0).sum()))
        rows.append(row)
        print(f'N={N:5d} {label:8s}: {n} paths of {row["nodes_mean"]:.1f} nodes in {H} rows; certify min {t_cert * 1e3:.3f} ms '
              f'({row["n_evals_mean"]:.0f} configurations per path, depth_max {depth}); shares '
              + ', '.join(f'{k} {v:.3f}' for k, v in share.items() if v > 0)
              + ' (at c_req = -margin / 10: ' + ', '.join(f'{k} {v:.3f}' for k, v in share_relaxed.items() if v > 0) + ')'
              + f'; traj_collision_stats n_interp 5 min {t_s5 * 1e3:.3f} ms ({row["sampled5_collision"]} in collision, '
              f'{row["sampled5_free_certifier_collision"]} passed that the certifier refuses), n_interp {fine} min {t_sf * 1e3:.3f} ms '
              f'({row["sampled_fine_collision"]} in collision, {row["sampled_fine_free_certifier_collision"]} passed that the certifier refuses, '
              f'{row["sampled_fine_collision_certifier_free"]} refused that the certifier calls FREE)',
              flush=True)
res_path = os.path.join(ROOT, 'motion_planning_baselines_amd', 'csrc', 'kernel_resources.json')
if os.path.exists(res_path):
    for name, r in json.load(open(res_path)).items():
        if 'path_certify_kernel' in name or 'clearance_kernel' in name:
            print(f'{name}: {r.get("vgprs")} VGPRs, {r.get("sgprs")} SGPRs, {r.get("lds")} B static LDS, occupancy {r.get("occupancy")}, '
                  f'scratch {r.get("scratch")}')
if '--json' in sys.argv:
    with open(sys.argv[sys.argv.index('--json') + 1], 'w') as fh:
        json.dump(dict(rows=rows), fh, indent=1)
