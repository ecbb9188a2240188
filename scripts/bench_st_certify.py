"""Space-time certification (ops.traj_certify_moving, PlanningTask.certify_trajs_moving) on the `ring` scene of
scripts/bench_st_shortcut.py: Panda, 16 static spheres, a MovingObstacleField of 16 spheres + 4 boxes that stay in a shell around the base,
R = 64 rows.

Inputs per B = 128, 1 024 and 4 096 start / goal problems: the plans STRRTConnect finds, raw and after 64 iterations of its space-time
shortcut pass.  Per input it times ONE launch of the certifier at the default arguments, the required clearance raised by the field's
chord deviation as certify_trajs_moving raises it (HIP events, min of 20 after warm-up), and prints the status shares, the mean number
of configurations a certificate evaluated, the deepest level reached, and how many plans check_trajs_moving accepts that the certifier
refuses WITH A WITNESS; the same shares once more for the chord motion alone (c_req = 0, what ops.traj_certify_moving certifies).

Beside it, the only composed route there is today: interpolate the trajectory to (R - 1) k + 1 rows (ops.traj_interpolate), pack the
field again for that row count and ask ops.moving_collision_check OR ops.collision_check at every row -- at k = 8 and at the k that
matches the deepest level the certifier reached, k = 2^(depth_max + 1), capped where (R - 1) k + 1 would exceed MOVING_MAX_ROWS (the cap
is printed: beyond it the composed route does not exist).  The device part is timed; packing the finer buffer on the host is timed once
and printed apart.  The composed route proves nothing between its rows at either k, and its finer rows see the field's own motion, not
the chords: it is a timing yardstick, not a reference.  No figure is fixed here.

    python scripts/bench_st_certify.py [--json OUT]
"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from motion_planning_baselines_amd import moving_layout, ops, st_certify_layout  # noqa: E402
from bench_path_timing import fields, timed  # noqa: E402

R, N_ITERS, N_PRE, SC_ITERS = 64, 512, 4096, 64


def composed(trajs, task, mo_fine, k):
    """Any row of the k-times finer trajectory in collision, at its own time of the finer clock: (N,) bool."""
    fine = ops.traj_interpolate(trajs, k - 1)
    hit = ops.moving_collision_check(fine, mo_fine) | ops.collision_check(fine.reshape(-1, fine.shape[-1]), task.geom).reshape(fine.shape[:2])
    return hit.any(1)


def measure(label, trajs, task, moving, row):
    geom, reach = task._certify_buffers('bench_st_certify')
    mo = task._moving_geom(moving, R)
    dev = st_certify_layout.chord_deviation(moving, R)
    ms, cert = timed(lambda: ops.traj_certify_moving(trajs, geom, mo, reach, c_req=dev))
    n = trajs.shape[0]
    depth = max(int(cert.depth_max.max()), 0)
    accepted = ~task.check_trajs_moving(trajs, moving)[0]
    out = dict(plans=n, certify_ms=ms, chord_deviation=dev, depth_max=depth, n_evals_mean=float(cert.n_evals.float().mean()),
               status_share={name: float((cert.status == s).float().mean()) for s, name in enumerate(ops.CERT_STATUS_NAMES)},
               rows_accepted=int(accepted.sum()), rows_accepted_certifier_collision=int((accepted & cert.collision).sum()),
               witness_on_moving_obstacle=int((cert.collision & (cert.witness_obstacle >= 0)).sum()))
    chord = ops.traj_certify_moving(trajs, geom, mo, reach, c_req=0.0)      # the chord motion alone, c_req as given: what ops certifies
    out['chord_motion_only'] = dict(status_share={name: float((chord.status == s).float().mean()) for s, name in enumerate(ops.CERT_STATUS_NAMES)},
                                    depth_max=max(int(chord.depth_max.max()), 0), n_evals_mean=float(chord.n_evals.float().mean()),
                                    rows_accepted_certifier_collision=int((accepted & chord.collision).sum()),
                                    witness_on_moving_obstacle=int((chord.collision & (chord.witness_obstacle >= 0)).sum()))
    k_cap = (moving_layout.MOVING_MAX_ROWS - 1) // (R - 1)
    k_match = 2 ** (depth + 1)
    for name, k in (('k8', 8), ('k_match', min(k_match, k_cap))):
        t0 = time.perf_counter()
        mo_fine = task._moving_geom(moving, (R - 1) * k + 1)
        pack_s = time.perf_counter() - t0
        ms_c, hit = timed(lambda: composed(trajs, task, mo_fine, k))
        out[name] = dict(k=k, k_wanted=k if name == 'k8' else k_match, rows=(R - 1) * k + 1, composed_ms=ms_c, composed_over_certify=ms_c / ms,
                         pack_seconds_host=pack_s, in_collision=int(hit.sum()), free_certifier_collision=int((~hit & cert.collision).sum()),
                         collision_certifier_free=int((hit & cert.free).sum()))
    row[label] = out


def main():
    from motion_planning_baselines_amd import geometry as G, workloads
    from motion_planning_baselines_amd.planners import STRRTConnect
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
        planner = STRRTConnect(task=task, moving_field=moving, n_rows=R, start_state_pos=q_start[:B].contiguous(), goal_state_pos=q_goal[:B].contiguous(),
                               n_iters=N_ITERS, n_pre_samples=N_PRE, seed=3, tensor_args=ta)
        rec = planner.optimize_batched()
        short = planner.shortcut(rec, SC_ITERS)
        keep = rec.found & short.ok
        row = dict(scene='ring', B=B, R=R, found=int(rec.found.sum()))
        measure('raw_plans', rec.trajs[keep].contiguous(), task, moving, row)
        measure('shortcut_plans', short.trajs[keep].contiguous(), task, moving, row)
        rows.append(row)
        print(json.dumps(row), flush=True)
    res_path = os.path.join(ROOT, 'motion_planning_baselines_amd', 'csrc', 'kernel_resources.json')
    if os.path.exists(res_path):
        for name, r in json.load(open(res_path)).items():
            if 'traj_certify_moving_kernel' in name or 'moving_clearance_kernel' in name:
                print(f'{name}: {r.get("vgprs")} VGPRs, {r.get("sgprs")} SGPRs, {r.get("lds")} B static LDS, occupancy {r.get("occupancy")}, '
                      f'scratch {r.get("scratch")}')
    if '--json' in sys.argv:
        with open(sys.argv[sys.argv.index('--json') + 1], 'w') as fh:
            json.dump(dict(rows=rows), fh, indent=1)


if __name__ == '__main__':
    main()
