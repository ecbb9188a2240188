"""Space-time RRT-Connect (planners.STRRTConnect) beside the frozen-time RRTConnect on field.at(t_start): Panda, 16 static spheres, a
MovingObstacleField of 16 spheres + 4 boxes, R = 64 rows, B = 128, 1 024 and 4 096 independent start / goal problems, the same starts and
goals for both planners.

Per B it prints: the time of a whole run (HIP events around init + every launch, min of 20 after warm-up), the share of problems found,
the count of each status, and the share of each planner's output that PlanningTask.check_trajs_moving accepts (of all problems).  Starts
are free at t_start, goals at t_start and at t_end.  The frozen-time paths are resampled to R rows first (ops.traj_resample): they were
planned without a clock, so a path that crosses where an obstacle will be still counted as free to its planner.  No figure is fixed here.

    python scripts/bench_strrt.py [--json OUT]
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from motion_planning_baselines_amd import geometry as G, ops, workloads  # noqa: E402
from motion_planning_baselines_amd.planners import STRRTConnect  # noqa: E402
from motion_planning_baselines_amd.planners.rrt_connect import RRTConnect  # noqa: E402
from motion_planning_baselines_amd.robot_field import PlanningTask  # noqa: E402

dev = torch.device('cuda:0')
R, K, N_ITERS, N_PRE, REPEATS, WARMUP, HORIZON = 64, 5, 512, 4096, 20, 2, 8.0
robot, field = G.RobotPanda(), G.env_spheres_3d(seed=0, n_spheres=16)
rng = np.random.RandomState(17)
# 16 spheres + 4 boxes on keyframed paths in a shell around the base (0.45 .. 0.8 m from its axis, 0.15 .. 0.9 m high)
rad, th, z = rng.uniform(0.45, 0.8, (K, 20)), rng.uniform(-np.pi, np.pi, (K, 20)), rng.uniform(0.15, 0.9, (K, 20))
centres = np.stack([rad * np.cos(th), rad * np.sin(th), z], -1)
moving = G.MovingObstacleField(np.linspace(0.0, HORIZON, K), centres[:, :16], rng.uniform(0.04, 0.07, 16), centres[:, 16:],
                               rng.uniform(0.04, 0.07, (4, 3)), margin=0.03)
ta = dict(device=dev, dtype=torch.float32)
task = PlanningTask(robot, field, tensor_args=ta, seed=5)
frozen_task = PlanningTask(robot, [field, moving.at(moving.t_start)], tensor_args=ta, seed=5)
end_task = PlanningTask(robot, [field, moving.at(moving.t_end)], tensor_args=ta, seed=5)
# starts free at t_start, goals free at t_start (the frozen-time planner's scene) AND at t_end (where the clock finds them)
cand = torch.from_numpy(workloads.collision_free_configs(robot, field, 8 * 4096, 91, dev)).to(dev)
q_start = cand[:4 * 4096][~frozen_task.compute_collision(cand[:4 * 4096])][:4096]
q_goal = cand[4 * 4096:][~(frozen_task.compute_collision(cand[4 * 4096:]) | end_task.compute_collision(cand[4 * 4096:]))][:4096]
assert len(q_start) == 4096 and len(q_goal) == 4096


def timed(fn):
    best, out = float('inf'), None
    for i in range(WARMUP + REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        if i >= WARMUP:
            best = min(best, a.elapsed_time(b))
    return best, out


rows = []
for B in (128, 1024, 4096):
    starts, goals = q_start[:B].contiguous(), q_goal[:B].contiguous()
    st = STRRTConnect(task=task, moving_field=moving, n_rows=R, start_state_pos=starts, goal_state_pos=goals, n_iters=N_ITERS,
                      n_pre_samples=N_PRE, seed=3, tensor_args=ta)
    ms_st, rec = timed(lambda: st.optimize_batched())
    ok_st = ~task.check_trajs_moving(rec.trajs, moving)[0] & rec.found
    fr = RRTConnect(task=frozen_task, n_iters=N_ITERS, start_state_pos=starts, goal_state_pos=goals, step_size=np.pi / 80, n_radius=np.pi / 4,
                    n_pre_samples=N_PRE, seed=3, tensor_args=ta)
    ms_fr, (paths, lengths, status) = timed(lambda: fr.optimize_batched())
    found_fr = lengths > 0
    dense = ops.traj_resample(paths, torch.where(found_fr, lengths, torch.full_like(lengths, 2)), R, 1.0)[..., :robot.q_dim].contiguous()
    ok_fr = ~task.check_trajs_moving(dense, moving)[0] & found_fr
    row = dict(B=B, strrt_ms=ms_st, strrt_found=float(rec.found.float().mean()), strrt_accepted=float(ok_st.float().mean()),
               strrt_status={ops.STRRT_STATUS_NAMES[k]: int((rec.status == k).sum()) for k in range(len(ops.STRRT_STATUS_NAMES))},
               frozen_ms=ms_fr, frozen_found=float(found_fr.float().mean()), frozen_accepted=float(ok_fr.float().mean()))
    rows.append(row)
    print(json.dumps(row), flush=True)
if '--json' in sys.argv:
    with open(sys.argv[sys.argv.index('--json') + 1], 'w') as fh:
        json.dump(rows, fh, indent=1)
