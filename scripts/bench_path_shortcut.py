"""Batched path shortcutting (mpb_path_shortcut), Panda + 16 spheres: RRT-Connect paths (step pi/80, radius pi/4, n_iters 2000, pool
2000) of N = 128 and 4 096 independent start / goal problems, 64 shortcut iterations per path at check_step pi/80.

Compared: ONE launch of the kernel against the composed torch route it replaces -- per iteration the positions, the two points and
the dense points of every path's candidate in torch (padded to the longest candidate), ONE ops.collision_check over all of them, the
verdicts read back and the accepted candidates spliced into the ragged paths on the host.  The composed route draws the same
uniforms and follows the same definition up to the snap of a point to a node (timing only: its paths are not compared bit for bit).

Timing: warm-up first, HIP events around the kernel launch, a host clock around the composed route (it ends in host work), 20 repeats,
the minimum.  Also printed: what the pass buys -- the median joint-space length after / before over the found paths, and GPMP2's median
cost after 8 iterations started from the resampled paths with and without the pass (HybridPlanner, 128 copies of one problem).

    python scripts/bench_path_shortcut.py [--json OUT]
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from motion_planning_baselines_amd import geometry as G, ops, workloads  # noqa: E402
from motion_planning_baselines_amd.planners.gpmp2 import GPMP2  # noqa: E402
from motion_planning_baselines_amd.planners.hybrid_planner import HybridPlanner  # noqa: E402
from motion_planning_baselines_amd.planners.multi_sample_based_planner import MultiSampleBasedPlanner  # noqa: E402
from motion_planning_baselines_amd.planners.rrt_connect import RRTConnect  # noqa: E402
from motion_planning_baselines_amd.robot_field import PlanningTask  # noqa: E402

dev = torch.device('cuda:0')
ta = dict(device=dev, dtype=torch.float32)
robot, field = G.RobotPanda(), G.env_spheres_3d(seed=0)
task = PlanningTask(robot, field, tensor_args=ta, seed=5)
STEP, RADIUS, N_ITERS_RRT, N_PRE, LMAX, ITERS, REPEATS, WARMUP, D = np.pi / 80, np.pi / 4, 2000, 2000, 512, 64, 20, 2, 7
pool = task.random_coll_free_q(N_PRE)


def rrt_paths(N):
    q = torch.from_numpy(workloads.collision_free_configs(robot, field, 2 * N, 91, dev))
    planner = RRTConnect(task=task, n_iters=N_ITERS_RRT, start_state_pos=q[:N], goal_state_pos=q[N:], step_size=STEP, n_radius=RADIUS,
                         tensor_args=ta, n_pre_samples=N_PRE, pre_samples=pool, max_path_nodes=LMAX, seed=7)
    paths, lengths, status = planner.optimize_batched()
    return paths.contiguous(), lengths.contiguous(), int((status == ops.RRT_FOUND).sum())


def kernel(paths, lengths, draws):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = ops.path_shortcut(paths, lengths, task.geom, ITERS, STEP, draws=draws)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3, out


def composed(paths, lengths, draws):
    """The route the kernel replaces: torch for the points, ops.collision_check per iteration, a host splice."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    N = paths.shape[0]
    host = [paths[b, :n].cpu().numpy() for b, n in enumerate(lengths.tolist())]
    accepted = 0
    for it in range(ITERS):
        L = torch.tensor([len(p) for p in host], device=dev)
        live = L >= 3
        pad = np.zeros((N, max(int(L.max()), 3), D), np.float32)
        for b, p in enumerate(host):                                  # (the ragged batch goes up again after every splice)
            pad[b, :len(p)] = p
        padded = torch.from_numpy(pad).to(dev)
        s = draws[:, it] * (L.clamp_min(2) - 1).float()[:, None]
        a = torch.minimum(s.long(), (L.clamp_min(3) - 2)[:, None])
        t = s - a.float()
        order = torch.argsort(a.float() + t, dim=1)
        a, t = torch.gather(a, 1, order), torch.gather(t, 1, order)
        idx = torch.arange(N, device=dev)
        pt = [padded[idx, a[:, k]] + t[:, k, None] * (padded[idx, a[:, k] + 1] - padded[idx, a[:, k]]) for k in (0, 1)]
        dist = torch.linalg.norm(pt[1] - pt[0], dim=1)
        n_pts = (dist / STEP).long() + 2
        live = live & (a[:, 0] != a[:, 1])
        P = int(n_pts[live].max()) if bool(live.any()) else 2
        al = torch.arange(P, device=dev)[None, :].float() / (n_pts[:, None] - 1).float()
        dense = pt[0][:, None, :] + (pt[1] - pt[0])[:, None, :] * al.clamp(max=1.0)[:, :, None]
        hit = ops.collision_check(dense.reshape(-1, D).contiguous(), task.geom).reshape(N, P)
        free = (live & ~hit.any(1)).cpu().numpy()
        a_h, t_h, p_h = a.cpu().numpy(), t.cpu().numpy(), [x.cpu().numpy() for x in pt]
        for b in np.nonzero(free)[0]:
            rows = [p_h[k][b][None] for k in (0, 1) if t_h[b, k] > 0]
            hi = a_h[b, 1] + 1 if t_h[b, 1] > 0 else a_h[b, 1]
            new = np.concatenate([host[b][:a_h[b, 0] + 1]] + rows + [host[b][hi:]])
            if len(new) <= LMAX:
                host[b] = new
                accepted += 1
    return time.perf_counter() - t0, accepted


def gpmp2_after(shortcut_iters, n=128, H=64, dt=0.15, opt_iters=8):
    q = workloads.collision_free_configs(robot, field, 2, 17, dev)
    start, goal = torch.from_numpy(q[0]), torch.from_numpy(q[1])
    rrt = RRTConnect(task=task, n_iters=N_ITERS_RRT, start_state_pos=start, goal_state_pos=goal, step_size=STEP, n_radius=RADIUS,
                     tensor_args=ta, n_pre_samples=N_PRE, pre_samples=pool, max_path_nodes=LMAX, seed=11)
    opt = GPMP2(robot=robot, n_dof=D, n_support_points=H, num_particles_per_goal=n, opt_iters=opt_iters, dt=dt, start_state=start.to(dev),
                step_size=1.0, multi_goal_states=goal[None].to(dev), initial_particle_means=torch.zeros(n, H, 2 * D, device=dev),
                collision_fields=[field], sigma_start=1e-5, sigma_gp=1e-2, sigma_coll=1e-5, sigma_goal_prior=1e-5,
                solver_params=dict(delta=1e-2, trust_region=True, method='cholesky'), tensor_args=ta)
    hyb = HybridPlanner(MultiSampleBasedPlanner(rrt, n_trajectories=n), opt, shortcut_iters=shortcut_iters, tensor_args=ta)
    trajs = hyb.optimize()
    free = task.compute_fraction_free_trajs(trajs.reshape(-1, H, 2 * D))
    return float(opt.costs.median()), free


rows = []
for N in (128, 4096):
    paths, lengths, found = rrt_paths(N)
    draws = torch.rand(N, ITERS, 2, device=dev, generator=torch.Generator(device=dev).manual_seed(3)).clamp_(max=1.0 - 2.0 ** -24)
    for _ in range(WARMUP):
        kernel(paths, lengths, draws)
        composed(paths, lengths, draws)
    res = [kernel(paths, lengths, draws) for _ in range(REPEATS)]
    t_kernel = min(r[0] for r in res)
    stats = res[0][1][2]
    ok = lengths > 0
    ratio = float((stats[ok, 3] / stats[ok, 2]).median())
    comp = [composed(paths, lengths, draws) for _ in range(REPEATS)]
    t_comp = min(c[0] for c in comp)
    row = dict(N=N, found=found, nodes_mean=float(lengths[ok].float().mean()), nodes_after_mean=float(res[0][1][1][ok].float().mean()),
               tested=float(stats[ok, 0].sum()), accepted=float(stats[ok, 1].sum()), accepted_composed=comp[0][1],
               kernel_seconds_min=t_kernel, composed_seconds_min=t_comp, length_ratio_median=ratio)
    rows.append(row)
    print(f'N={N:5d}: {found} paths of {row["nodes_mean"]:.1f} nodes (after: {row["nodes_after_mean"]:.1f}); {ITERS} iterations: kernel min '
          f'{t_kernel * 1e3:.3f} ms, composed torch route min {t_comp * 1e3:.1f} ms ({t_comp / t_kernel:.0f} x); candidates checked '
          f'{row["tested"]:.0f}, accepted {row["accepted"]:.0f} (composed: {comp[0][1]}); median length after / before {ratio:.3f}', flush=True)
gp = {k: gpmp2_after(k) for k in (0, ITERS)}
print(f'GPMP2 after 8 iterations from the resampled RRT-Connect paths (128 particles, H 64): median cost {gp[0][0]:.4g} without the pass, '
      f'{gp[ITERS][0]:.4g} with {ITERS} shortcut iterations; share of collision-free trajectories {gp[0][1]:.3f} / {gp[ITERS][1]:.3f}')
res_path = os.path.join(ROOT, 'motion_planning_baselines_amd', 'csrc', 'kernel_resources.json')
if os.path.exists(res_path):
    for name, r in json.load(open(res_path)).items():
        if 'path_shortcut_kernel' in name:
            print(f'{name}: {r.get("vgprs")} VGPRs, {r.get("lds")} B static LDS, occupancy {r.get("occupancy")}, scratch {r.get("scratch")}')
if '--json' in sys.argv:
    with open(sys.argv[sys.argv.index('--json') + 1], 'w') as fh:
        json.dump(dict(rows=rows, gpmp2_median_cost={str(k): v[0] for k, v in gp.items()},
                       gpmp2_free_share={str(k): v[1] for k, v in gp.items()}), fh, indent=1)
