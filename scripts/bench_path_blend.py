"""Linear segments with parabolic blends (mpb_path_blend, mpb_path_blend_sample), Panda + 16 spheres: the workload of bench_certify.py --
RRT-Connect paths (step pi/80, radius pi/4, n_iters 2000, pool 2000) of N = 128 and 4 096 independent start / goal problems after 64
shortcut iterations -- certified (certify_paths) and blended under the Panda's data-sheet limits.

  blend      ops.path_blend on the found paths in place (one launch), at max_deviation = inf / 0.05 / 0.01
  sample     ops.path_blend_sample at dt = 1 ms, the output sized to the 90th percentile of the durations and to at most 20 000 rows
             (a near-duplicate waypoint beside a corner slows its neighbours by orders of magnitude: longer paths are TOO_LONG here)
  composed   the same sweep loop written in batched torch on the device (masked (N, H, D) tensors, one synchronisation per sweep for the
             "any violation" test, a cumulative sum for the timeline): what a caller without the kernel would run
  duration   the median over the paths of the blend's duration over ops.traj_retime's on the same path resampled to 64 rows uniform
             in arc length (the waypoint-index retiming needs evenly spread rows; its limits hold at the waypoints only)
  certified  the share of the found paths PlanningTask.blend_paths(certificate=...) certifies at each max_deviation

Timing: warm-up first, HIP events around each call, 20 repeats, the minimum.  No ratio is fixed in advance.

    python scripts/bench_path_blend.py [--json OUT]
"""
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from motion_planning_baselines_amd import geometry as G, ops, workloads  # noqa: E402
from motion_planning_baselines_amd.planners.rrt_connect import RRTConnect  # noqa: E402
from motion_planning_baselines_amd.robot_field import PlanningTask  # noqa: E402

if not torch.cuda.is_available():
    sys.exit('bench_path_blend.py needs a GPU: there is no CPU path')
dev = torch.device('cuda:0')
ta = dict(device=dev, dtype=torch.float32)
robot, field = G.RobotPanda(), G.env_spheres_3d(seed=0)
task = PlanningTask(robot, field, tensor_args=ta, seed=5)
STEP, RADIUS, N_ITERS_RRT, N_PRE, LMAX, ITERS, REPEATS, WARMUP, DT = np.pi / 80, np.pi / 4, 2000, 2000, 512, 64, 20, 2, 1e-3
DELTAS = (math.inf, 0.05, 0.01)
MAX_H = 256                                                      # MPB_MAX_H
MAX_ROWS = 20000
pool = task.random_coll_free_q(N_PRE)
V, A = robot.dq_max.to(dev), robot.ddq_max.to(dev)


def rrt_paths(N):
    q = torch.from_numpy(workloads.collision_free_configs(robot, field, 2 * N, 91, dev))
    planner = RRTConnect(task=task, n_iters=N_ITERS_RRT, start_state_pos=q[:N], goal_state_pos=q[N:], step_size=STEP, n_radius=RADIUS,
                         tensor_args=ta, n_pre_samples=N_PRE, pre_samples=pool, max_path_nodes=LMAX, seed=7)
    paths, lengths, status = planner.optimize_batched()
    return paths.contiguous(), lengths.contiguous(), status == ops.RRT_FOUND


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


def composed(p, ln, delta, max_sweeps=64):
    """The sweep loop of include/mpb.h in batched torch: (T, tb, tw, duration, sweeps)."""
    N, H, D = p.shape
    inf = torch.full((), math.inf, device=dev)
    seg = torch.arange(H - 1, device=dev)[None, :] < (ln - 1)[:, None]
    way = torch.arange(H, device=dev)[None, :] < ln[:, None]
    dq = torch.where(seg[:, :, None], p[:, 1:] - p[:, :-1], torch.zeros((), device=dev))
    T = torch.where(seg, (dq.abs() / V).amax(-1), torch.ones((), device=dev))
    z, col = torch.zeros(N, 1, D, device=dev), torch.full((N, 1), math.inf, device=dev)
    sweeps = 0
    while True:
        vel = dq / T[:, :, None]
        dv = torch.cat([vel, z], 1) - torch.cat([z, vel], 1)
        adv = dv.abs()
        tb, mdv = (adv / A).amax(-1), adv.amax(-1)
        Tm = torch.where(seg, T, inf)
        m = torch.minimum(torch.cat([col, Tm], 1), torch.cat([Tm, col], 1))
        if math.isfinite(delta):
            m = torch.minimum(m, torch.where(mdv > 0, (8.0 * delta) / mdv, inf))
        viol = way & (tb > m)
        if sweeps == max_sweeps or not bool(viol.any()):
            break
        f = torch.where(viol, torch.sqrt(m / tb), torch.ones((), device=dev))
        T = T / torch.minimum(f[:, :-1], f[:, 1:])
        sweeps += 1
    Ts = torch.where(seg, T, torch.zeros((), device=dev))
    tw = tb[:, :1] * 0.5 + torch.cat([torch.zeros(N, 1, device=dev), torch.cumsum(Ts, 1)], 1)
    last = (ln - 1).long()[:, None]
    return Ts, tb, tw, (torch.gather(tw, 1, last) + 0.5 * torch.gather(tb, 1, last))[:, 0], sweeps


rows = []
for N in (128, 4096):
    paths, lengths, found = rrt_paths(N)
    short, short_len, _ = task.shortcut_paths(paths, lengths, n_iters=ITERS, check_step=STEP)
    keep = found & (short_len >= 2) & (short_len <= MAX_H)
    H = int(short_len[keep].max())
    p, ln = short[keep][:, :H].contiguous(), short_len[keep].contiguous()
    n = p.shape[0]
    cert = task.certify_paths(p, ln)
    # the waypoint-index retiming on the same paths, resampled to 64 rows uniform in arc length
    rt = ops.traj_retime(ops.traj_resample(p, ln, 64, 1.0), V, A)
    rt_ok = rt.status == ops.RETIME_OK
    row = dict(N=N, found=n, rows=H, nodes_mean=float(ln.float().mean()), cert_free_share=float(cert.free.float().mean()), by_delta=[])
    for delta in DELTAS:
        md = None if math.isinf(delta) else delta
        t_blend, tm = timed(lambda: ops.path_blend(p, V, A, lengths=ln, max_deviation=md))
        ok = tm.status == ops.BLEND_OK
        n_rows = min(int(math.ceil(float(torch.quantile(tm.duration[ok], 0.9)) / DT)) + 1, MAX_ROWS)
        t_sample, _ = timed(lambda: ops.path_blend_sample(p, tm, DT, n_rows=n_rows))
        t_comp, comp = timed(lambda: composed(p, ln, delta))
        both = ok & rt_ok
        res = task.blend_paths(p, lengths=ln, max_deviation=md, certificate=cert)
        d = dict(max_deviation=delta, blend_seconds_min=t_blend, sample_seconds_min=t_sample, sample_rows=n_rows, composed_seconds_min=t_comp,
                 composed_sweeps=int(comp[4]), sweeps_max=int(tm.sweeps.max()), ok_share=float(ok.float().mean()),
                 duration_median=float(tm.duration[ok].median()), duration_max=float(tm.duration[ok].max()),
                 composed_duration_max_abs_diff=float((comp[3] - tm.duration)[ok].abs().max()),
                 duration_over_retime_median=float((tm.duration[both] / rt.duration[both]).median()),
                 certified_share=float(res.certified.float().mean()),
                 deviation_workspace_median=float(res.deviation_workspace[ok].median()))
        row['by_delta'].append(d)
        print(f'N={N:5d} delta {delta:5.2f}: {n} paths of {row["nodes_mean"]:.1f} nodes in {H} rows; blend min {t_blend * 1e3:.3f} ms '
              f'(sweeps up to {d["sweeps_max"]}, OK {d["ok_share"]:.3f}); sampling at 1 ms min {t_sample * 1e3:.3f} ms ({n} x {n_rows} rows); '
              f'composed torch min {t_comp * 1e3:.3f} ms ({d["composed_sweeps"]} sweeps, durations within {d["composed_duration_max_abs_diff"]:.2e} s); '
              f'median duration {d["duration_median"]:.3f} s = {d["duration_over_retime_median"]:.3f} x traj_retime\'s; certificate FREE '
              f'{row["cert_free_share"]:.3f}, certified {d["certified_share"]:.3f} (median deviation_workspace {d["deviation_workspace_median"]:.4f} m)',
              flush=True)
    rows.append(row)
res_path = os.path.join(ROOT, 'motion_planning_baselines_amd', 'csrc', 'kernel_resources.json')
if os.path.exists(res_path):
    for name, r in json.load(open(res_path)).items():
        if 'path_blend' in name:
            print(f'{name}: {r.get("vgprs")} VGPRs, {r.get("sgprs")} SGPRs, {r.get("lds")} B static LDS, occupancy {r.get("occupancy")}, '
                  f'scratch {r.get("scratch")}')
if '--json' in sys.argv:
    with open(sys.argv[sys.argv.index('--json') + 1], 'w') as fh:
        json.dump(dict(rows=rows), fh, indent=1)
