"""Batched RRT-Connect, Panda + 16 spheres (step pi/80, radius pi/4, n_iters 2000, pool 2000), device-drawn indices, to
completion, at B = 1, 16, 256 and 1024 independent start / goal problems.

Timing: warm-up runs first, HIP events around the WHOLE chunk sequence of a run (init + every launch), a status read
between chunks like RRTConnect.optimize_batched does, 10 repeats, min and median.  Prints iterations/s per problem
(iterations the slowest problem of the batch ran / time) and paths/s.  The CPU column -- the unmodified reference on the
golden problems, timed by tests/golden/make_rrt_goldens.py on its host -- is read from the golden.

With --star the same harness runs batched RRT* instead (radius pi/2, n_iters 400, n_iters_after_success 150, pool 1000 --
the shapes of tests/golden/rrt_star_panda_spheres.npz), device-drawn pool indices and goal draws, and also prints the
accepted rewires per problem.

    python scripts/bench_rrt.py [--star] [--json OUT]
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from motion_planning_baselines_amd import geometry as G, ops, workloads  # noqa: E402
from motion_planning_baselines_amd.robot_field import PlanningTask  # noqa: E402

dev = torch.device('cuda:0')
robot, field = G.RobotPanda(), G.env_spheres_3d(seed=0)
task = PlanningTask(robot, field, tensor_args=dict(device=dev, dtype=torch.float32), seed=5)
STAR = '--star' in sys.argv
STEP, RADIUS, TOTAL, N_PRE, CHUNK, LMAX, REPEATS, WARMUP = np.pi / 80, np.pi / 4, 2001, 2000, 1024, 512, 10, 3
if STAR:
    RADIUS, TOTAL, N_PRE, N_AFTER = np.pi / 2, 401, 1000, 150
pool = task.random_coll_free_q(N_PRE)
q_all = torch.from_numpy(workloads.collision_free_configs(robot, field, 2 * 1024, 91, dev)).to(dev)


def run_star(B, seed):
    starts, goals = q_all[:B].contiguous(), q_all[1024:1024 + B].contiguous()
    ws = ops.RRTStarWorkspace(B, TOTAL + 1, N_PRE, 7, dev)
    paths = torch.zeros(B, LMAX, 7, device=dev)
    lengths = torch.zeros(B, device=dev, dtype=torch.int32)
    costs = torch.zeros(B, device=dev)
    status = torch.zeros(B, device=dev, dtype=torch.int32)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    ops.rrt_star_init(ws.buf, ws, starts, goals, task.geom)
    for it in range(0, TOTAL, CHUNK):
        ops.rrt_star_run(ws.buf, ws, task.geom, pool, None, None, paths, lengths, costs, status, it, min(CHUNK, TOTAL - it), TOTAL,
                         STEP, RADIUS, n_iters_after_success=N_AFTER, seed=seed)
        if not bool((status == ops.RRT_RUNNING).any().item()):
            break
    e1.record()
    torch.cuda.synchronize()
    tr = ops.rrt_star_tree(ws)
    return e0.elapsed_time(e1) * 1e-3, int((status == ops.RRT_FOUND).sum()), int(tr['iters'].max()), float(tr['iters'].float().mean()), \
        float(tr['count'].float().mean()), float(tr['rewires'].float().mean())


def run(B, seed):
    if STAR:
        return run_star(B, seed)
    starts, goals = q_all[:B].contiguous(), q_all[1024:1024 + B].contiguous()
    ws = ops.RRTWorkspace(B, TOTAL + 1, N_PRE, 7, dev)
    paths = torch.zeros(B, LMAX, 7, device=dev)
    lengths = torch.zeros(B, device=dev, dtype=torch.int32)
    status = torch.zeros(B, device=dev, dtype=torch.int32)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    ops.rrt_connect_init(ws.buf, ws, starts, goals, task.geom)
    for it in range(0, TOTAL, CHUNK):
        ops.rrt_connect_run(ws.buf, ws, task.geom, pool, None, paths, lengths, status, it, min(CHUNK, TOTAL - it), TOTAL, STEP, RADIUS,
                            seed=seed)
        if not bool((status == ops.RRT_RUNNING).any().item()):
            break
    e1.record()
    torch.cuda.synchronize()
    tr = ops.rrt_connect_trees(ws)
    return e0.elapsed_time(e1) * 1e-3, int((status == ops.RRT_FOUND).sum()), int(tr['iters'].max()), float(tr['iters'].float().mean()), \
        float(tr['counts'].sum(1).float().mean())


rows = []
for B in (1, 16, 256, 1024):
    for w in range(WARMUP):
        run(B, 100 + w)
    res = [run(B, 7) for _ in range(REPEATS)]                  # the same seed: the same work in every repeat
    ts = [r[0] for r in res]
    _, found, it_max, it_mean, nodes = res[0][:5]
    row = dict(B=B, found=found, iters_max=it_max, iters_mean=it_mean, nodes_mean=nodes, seconds_min=min(ts),
               seconds_median=statistics.median(ts), paths_per_s=found / min(ts), iters_per_s_per_problem=it_max / min(ts))
    if STAR:
        row['rewires_mean'] = res[0][5]
    rows.append(row)
    print(f'B={B:5d}: {found}/{B} found, iterations max {it_max} mean {it_mean:.1f}, nodes/problem {nodes:.1f}; '
          f'min {min(ts) * 1e3:.3f} ms, median {row["seconds_median"] * 1e3:.3f} ms; {row["paths_per_s"]:.0f} paths/s, '
          f'{row["iters_per_s_per_problem"]:.0f} iterations/s per problem' + (f', rewires/problem {res[0][5]:.1f}' if STAR else ''), flush=True)
g = np.load(os.path.join(ROOT, 'tests', 'golden', 'rrt_star_panda_spheres.npz' if STAR else 'rrt_panda_spheres.npz'))
cpu = g['ref_seconds']
print(f'reference (CPU, fp32, the {len(cpu)} golden problems): median {np.median(cpu):.3f} s per path, {1.0 / np.median(cpu):.1f} paths/s, '
      f'{np.median(g["n_iterations"] / cpu):.0f} iterations/s')
res_path = os.path.join(ROOT, 'motion_planning_baselines_amd', 'csrc', 'kernel_resources.json')
if os.path.exists(res_path):
    for name, r in json.load(open(res_path)).items():
        if ('rrt_star_kernel' if STAR else 'rrt_connect_kernel') in name:
            print(f'{name}: {r.get("vgprs")} VGPRs, {r.get("lds")} B LDS, occupancy {r.get("occupancy")}, scratch {r.get("scratch")}')
if '--json' in sys.argv:
    with open(sys.argv[sys.argv.index('--json') + 1], 'w') as fh:
        json.dump(dict(planner='rrt_star' if STAR else 'rrt_connect', rows=rows, reference_median_seconds=float(np.median(cpu))), fh, indent=1)
