"""Space-time shortcutting (ops.st_shortcut, PlanningTask.shortcut_trajs_moving) on the `ring` scene of scripts/bench_path_timing.py:
Panda, 16 static spheres, a MovingObstacleField of 16 spheres + 4 boxes that stay in a shell around the base, R = 64 rows.

Inputs per B = 128, 1 024 and 4 096 start / goal problems: (a) the plans STRRTConnect finds, (b) the timed paths time_paths_moving makes of
RRTConnect's paths on field.at(t_start).  Per input it times ONE launch of 64 iterations with recorded draws (HIP events, min of 20 after
warm-up) beside the composed route on the device -- per iteration the candidate rows in torch, ops.collision_check +
ops.moving_collision_check over them, a masked write -- and prints the share of candidates accepted, the median length after / before,
the share of outputs check_trajs_moving accepts, and how many trajectories the two routes leave with different rows (torch's fused
multiply-add is not promised to be the kernel's, so the composed route is a timing yardstick, not a bit reference).
Downstream: one start / goal problem, 64 STRRTConnect copies, CHOMP for 8 iterations on a composite of the static field, the moving field
and CHOMP's smoothness from the raw plans and from the shortcut plans: the median composite cost before and after, and the share
check_trajs_moving accepts.  No figure is fixed here.

    python scripts/bench_st_shortcut.py [--json OUT]
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from motion_planning_baselines_amd import ops  # noqa: E402
from bench_path_timing import fields, timed  # noqa: E402

R, N_ITERS, N_PRE, S, SC_ITERS = 64, 512, 4096, 128, 64


def composed(trajs, task, mo, w, draws):
    """The definition of include/mpb.h composed from what the project had before, for trajectories that pass the input gate: -> (trajs,
    checked (N,), accepted (N,))."""
    N, R_, D = trajs.shape
    tr = trajs.clone()
    rows = torch.arange(R_, device=tr.device)[None]
    checked, accepted = torch.zeros(N, device=tr.device), torch.zeros(N, device=tr.device)
    ar = torch.arange(N, device=tr.device)
    for it in range(draws.shape[1]):
        a, b = draws[:, it].amin(1).long(), draws[:, it].amax(1).long()
        qa, qb = tr[ar, a], tr[ar, b]
        span = (b - a).float()
        active = (b - a >= 2) & ~(((qb - qa).abs() / w).amax(1) > span)
        al = (rows - a[:, None]).float() / span.clamp_min(1.0)[:, None]
        cand = torch.addcmul(qa[:, None], (qb - qa)[:, None], al[..., None])
        inner = (rows > a[:, None]) & (rows < b[:, None])
        close = ((cand - tr).abs() <= 1e-8 + 1e-5 * tr.abs()).all(-1)
        active &= ~(close | ~inner).all(1)
        cand = torch.where(inner[..., None], cand, tr).contiguous()
        hit = ops.collision_check(cand.reshape(-1, D), task.geom).reshape(N, R_) | ops.moving_collision_check(cand, mo)
        ok = active & ~(hit & inner).any(1)
        tr = torch.where((ok[:, None] & inner)[..., None], cand, tr)
        checked += active
        accepted += ok
    return tr, checked, accepted


def length(tr):
    return (tr[:, 1:].double() - tr[:, :-1].double()).norm(dim=-1).sum(-1)


def measure(label, B, trajs, valid, task, moving, row):
    dev = trajs.device
    mo = task._moving_geom(moving, R)
    dt_row = (moving.t_end - moving.t_start) / (R - 1)
    w = torch.from_numpy((task.robot.dq_max_np.astype(np.float64) * dt_row).astype(np.float32)).to(dev)
    g = torch.Generator().manual_seed(11)
    draws = torch.randint(0, R, (B, SC_ITERS, 2), generator=g, dtype=torch.int32).to(dev)
    ms_k, got = timed(lambda: ops.st_shortcut(trajs, task.geom, mo, w, SC_ITERS, draws=draws, valid=valid))
    ok = got.ok
    n = int(ok.sum())
    sub, sub_draws = trajs[ok].contiguous(), draws[ok].contiguous()
    ms_c, (c_tr, c_checked, c_acc) = timed(lambda: composed(sub, task, mo, w, sub_draws))
    st = got.stats[ok]
    free = ~task.check_trajs_moving(got.trajs, moving)[0] & ok
    differ = int((c_tr != got.trajs[ok]).any(-1).any(-1).sum())
    row[label] = dict(inputs=int(valid.sum()), ok=n, status={ops.STS_STATUS_NAMES[k]: int((got.status == k).sum()) for k in range(len(ops.STS_STATUS_NAMES))},
                      kernel_ms=ms_k, composed_ms=ms_c, composed_over_kernel=ms_c / ms_k, checked=float(st[:, 0].sum()), accepted=float(st[:, 1].sum()),
                      accepted_share=float(st[:, 1].sum() / st[:, 0].sum().clamp_min(1)), composed_accepted=float(c_acc.sum()),
                      length_ratio_median=float((st[:, 3] / st[:, 2]).median()) if n else None,
                      length64_ratio_median=float((length(got.trajs[ok]) / length(trajs[ok])).median()) if n else None,
                      outputs_accepted_share=float(free.sum()) / max(n, 1), trajectories_differing_from_composed=differ)


def downstream(task, moving, q_start, q_goal, out):
    """CHOMP from raw STRRTConnect plans against the same plans shortcut: one problem, 64 copies."""
    from motion_planning_baselines_amd.planners import STRRTConnect
    from motion_planning_baselines_amd.planners.chomp import CHOMP
    from motion_planning_baselines_amd.planners.costs import cost_functions as C
    from motion_planning_baselines_amd import geometry as G
    dt = (moving.t_end - moving.t_start) / (R - 1)
    ta, robot = task.tensor_args, G.RobotPanda(dt=dt)             # (the task's robot with the clock's row spacing as its dt)
    st = STRRTConnect(task=task, moving_field=moving, n_rows=R, start_state_pos=q_start[None], goal_state_pos=q_goal[None], n_iters=N_ITERS,
                      n_pre_samples=N_PRE, seed=3, tensor_args=ta)
    rec = st.optimize_batched(n_copies=64)
    short = st.shortcut(rec, SC_ITERS)
    keep = rec.found & short.ok
    n = int(keep.sum())
    out['downstream'] = dict(copies=64, found=int(rec.found.sum()), used=n)
    if n == 0:
        return
    comp = C.CostComposite(robot, R, [C.CostCollision(robot, R, field=task.field, sigma_coll=0.3, tensor_args=ta),
                                      C.CostCollision(robot, R, field=moving, sigma_coll=0.2, tensor_args=ta),
                                      C.CostSmoothnessCHOMP(robot, R, tensor_args=ta)], weights_cost_l=[1.0, 1.0, 1e-3], tensor_args=ta)
    for label, seeds in (('raw', rec.trajs[keep].contiguous()), ('shortcut', short.trajs[keep].contiguous())):
        pl = CHOMP(n_dof=robot.q_dim, n_support_points=R, num_particles_per_goal=n, opt_iters=1, dt=dt, start_state=q_start, cost=comp,
                   weight_prior_cost=1e-3, initial_particle_means=seeds.clone(), step_size=0.01, grad_clip=1.0, pos_only=True, tensor_args=ta)
        before = comp.eval(seeds)
        for _ in range(8):
            pl.optimize()
        res = pl._particle_means[..., :robot.q_dim].contiguous()
        after = comp.eval(res)
        out['downstream'][label] = dict(seed_cost_median=float(before.median()), cost_median_after_8=float(after.median()),
                                        accepted_after_8=float((~task.check_trajs_moving(res, moving)[0]).float().mean()),
                                        length_median=float(length(res).median()))


def main():
    from motion_planning_baselines_amd import geometry as G, workloads
    from motion_planning_baselines_amd.planners import STRRTConnect
    from motion_planning_baselines_amd.planners.rrt_connect import RRTConnect
    from motion_planning_baselines_amd.robot_field import PlanningTask
    dev = torch.device('cuda:0')
    moving = fields()['ring']
    robot, field = G.RobotPanda(), G.env_spheres_3d(seed=0, n_spheres=16)
    ta = dict(device=dev, dtype=torch.float32)
    task = PlanningTask(robot, field, tensor_args=ta, seed=5)
    frozen_task = PlanningTask(robot, [field, moving.at(moving.t_start)], tensor_args=ta, seed=5)
    end_task = PlanningTask(robot, [field, moving.at(moving.t_end)], tensor_args=ta, seed=5)
    cand = torch.from_numpy(workloads.collision_free_configs(robot, field, 8 * 4096, 91, dev)).to(dev)
    q_start = cand[:4 * 4096][~frozen_task.compute_collision(cand[:4 * 4096])][:4096]
    q_goal = cand[4 * 4096:][~(frozen_task.compute_collision(cand[4 * 4096:]) | end_task.compute_collision(cand[4 * 4096:]))][:4096]
    assert len(q_start) == 4096 and len(q_goal) == 4096
    rows = []
    for B in (128, 1024, 4096):
        starts, goals = q_start[:B].contiguous(), q_goal[:B].contiguous()
        row = dict(scene='ring', B=B, R=R, iterations=SC_ITERS)
        rec = STRRTConnect(task=task, moving_field=moving, n_rows=R, start_state_pos=starts, goal_state_pos=goals, n_iters=N_ITERS,
                           n_pre_samples=N_PRE, seed=3, tensor_args=ta).optimize_batched()
        measure('strrt_plans', B, rec.trajs, rec.found, task, moving, row)
        rrt = RRTConnect(task=frozen_task, n_iters=N_ITERS, start_state_pos=starts, goal_state_pos=goals, step_size=np.pi / 80, n_radius=np.pi / 4,
                         n_pre_samples=N_PRE, seed=3, tensor_args=ta)
        paths, lengths, _ = rrt.optimize_batched()
        planned = lengths > 0
        lengths = torch.where(planned, lengths, torch.full_like(lengths, 2))
        tm = task.time_paths_moving(paths, moving, R, lengths=lengths, n_samples=S)
        measure('timed_paths', B, tm.trajs.contiguous(), (tm.found & planned).contiguous(), task, moving, row)
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = dict(rows=rows)
    downstream(task, moving, q_start[0].contiguous(), q_goal[0].contiguous(), out)
    print(json.dumps(out['downstream']), flush=True)
    if '--json' in sys.argv:
        with open(sys.argv[sys.argv.index('--json') + 1], 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
