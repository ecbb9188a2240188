"""The world predicate against the routes there were before it: the Panda, a table-and-shelf scene as triangle meshes in a
GridSDFField.from_mesh grid (cell 0.02 over [-1.2, 1.2]^2 x [-0.7, 1.5]: 122 x 122 x 112 nodes, 6.7 MB), env_spheres_3d() as the
obstacle list, SelfCollisionField(robot).  Run by hand on the GPU; not a test.

  predicate   ops.world_collision_check (one launch) against PlanningTask._in_collision of a plain task (three launches, the second
              and third ORing into the first's flags), N = 128 / 4 096 / 131 072 uniform configurations;
  validation  ops.traj_collision_stats on the world (one launch, no dense point stored) against ops.traj_interpolate followed by
              _in_collision on the N * P points and the reductions in torch, (N, 64, 14) states, n_interp = 5;
  rrt         RRTConnect.optimize_batched on the world, B = 256 problems, 2 000 iterations, device-drawn samples -- against the same
              planner on the obstacle list alone (what the tree cost before), on obstacles + grid, and on obstacles + self: what each
              part adds, the self part with its 23.8 KB LDS block per single-wave workgroup next to the 50 KB the kernel has.
              The route a user had before -- the tree loop composed from ops calls with _in_collision per extension -- is NOT timed:
              it is a Python loop of several launches and a device-to-host read per extension and per problem (10^5 and more
              round trips for this batch); no such loop exists in the package to be compared with.

Timing: every shape warmed up, then HIP events around each call, the routes of one comparison alternating, the MIN of 20 repeats (and
the median).  The routes are checked to agree before they are timed.

    timeout -k 10 600 python scripts/bench_world.py [--part predicate|validation|rrt] [--json OUT]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from motion_planning_baselines_amd import geometry as G, ops  # noqa: E402
from motion_planning_baselines_amd.planners.rrt_connect import RRTConnect  # noqa: E402
from motion_planning_baselines_amd.robot_field import PlanningTask  # noqa: E402

REPEATS, WARMUP, H, N_INTERP, D = 20, 3, 64, 5, 7
SIZES = (128, 4096, 131072)


def box_mesh(centre, half):
    """An axis-aligned box as 12 outward-facing triangles."""
    c, h = np.asarray(centre, np.float64), np.asarray(half, np.float64)
    v = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64) * h + c
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])
    return G.TriangleMesh(v.astype(np.float32), f.astype(np.int32))


def table_and_shelf():
    """A table top in front of the arm and a shelf of two boards, two sides and a back panel to its left."""
    parts = [((0.55, 0.0, 0.18), (0.30, 0.45, 0.02)),                                         # table top
             ((0.0, 0.75, 0.35), (0.30, 0.15, 0.012)), ((0.0, 0.75, 0.70), (0.30, 0.15, 0.012)),   # boards
             ((-0.31, 0.75, 0.50), (0.012, 0.15, 0.36)), ((0.31, 0.75, 0.50), (0.012, 0.15, 0.36)),  # sides
             ((0.0, 0.91, 0.50), (0.32, 0.012, 0.36))]                                           # back
    return [(box_mesh(c, h), None) for c, h in parts]


def tasks(dev):
    ta = dict(device=dev, dtype=torch.float32)
    robot, field = G.RobotPanda(dt=0.04), G.env_spheres_3d()
    grid = G.GridSDFField.from_mesh(table_and_shelf(), (-1.2, -1.2, -0.7), (1.2, 1.2, 1.5), 0.02, margin=0.03)
    own = G.SelfCollisionField(robot)
    plain = PlanningTask(robot, field, self_field=own, sdf_field=grid, tensor_args=ta, seed=1)
    world = PlanningTask(robot, field, self_field=own, sdf_field=grid, tensor_args=ta, seed=1, world_predicate=True)
    return plain, world


def timed(routes, repeats=REPEATS):
    """{name: (min ms, median ms)} of the callables in `routes`, alternating, HIP events around each call."""
    for _ in range(WARMUP):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in routes}
    for _ in range(repeats):
        for k, fn in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: (min(v), statistics.median(v)) for k, v in ms.items()}


def part_predicate(plain, world):
    out = {}
    for N in SIZES:
        q = world.random_q(N).contiguous()
        assert torch.equal(ops.world_collision_check(q, world.world), plain._in_collision(q))
        r = timed({'fused': lambda: ops.world_collision_check(q, world.world), 'three_launches': lambda: plain._in_collision(q)})
        out[N] = r
        print(f'predicate  N {N:7d}: fused {r["fused"][0]:.4f} ms (median {r["fused"][1]:.4f}), three launches {r["three_launches"][0]:.4f} ms '
              f'(median {r["three_launches"][1]:.4f}); in collision {float(plain._in_collision(q).float().mean()):.3f}', flush=True)
    return out


def make_states(task, N, seed=11):
    gen = torch.Generator(device=task.device)
    gen.manual_seed(seed)
    span = task.q_max - task.q_min
    u = torch.rand(3, N, 1, D, device=task.device, generator=gen)
    t = torch.linspace(0, 1, H, device=task.device)[None, :, None]
    pos = task.q_min + span * u[0] + 0.15 * span * (2 * u[1] - 1) * t + 0.05 * span * torch.sin(torch.pi * t) * (2 * u[2] - 1)
    return torch.cat([pos, torch.zeros_like(pos)], dim=-1).contiguous()


def part_validation(plain, world):
    P = (H - 1) * (N_INTERP + 1) + 1
    out = {}

    def composed(states):
        dense = ops.traj_interpolate(states[..., :D].contiguous(), N_INTERP)
        flag = plain._in_collision(dense.reshape(-1, D)).reshape(states.shape[0], P)
        first = torch.where(flag, torch.arange(P, device=flag.device, dtype=torch.int32), P).min(1)[0]
        return flag.sum(1, dtype=torch.int32), torch.where(first == P, -1, first).to(torch.int32)
    for N in SIZES:
        states = make_states(world, N)
        a, b = ops.traj_collision_stats(states, world.world, n_interp=N_INTERP), composed(states)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        r = timed({'fused': lambda: ops.traj_collision_stats(states, world.world, n_interp=N_INTERP), 'composed': lambda: composed(states)})
        out[N] = r
        print(f'validation N {N:7d}: fused {r["fused"][0]:.4f} ms (median {r["fused"][1]:.4f}), interpolate + three launches '
              f'{r["composed"][0]:.4f} ms (median {r["composed"][1]:.4f}); free trajectories {float((a[0] == 0).float().mean()):.3f}', flush=True)
    return out


def part_rrt(plain, world, B=256, n_iters=2000):
    """The tree on the world and on fewer parts.  Every planner draws the same samples (seed, pool) but decides other extensions, so
    the trees differ: the figures are what a user pays per batch, not the cost of the same work."""
    dev = world.device
    q = world.random_coll_free_q(2 * B + 2000)
    starts, goals, pool = q[:B].contiguous(), q[B:2 * B].contiguous(), q[2 * B:].contiguous()
    scenes = {'obstacles': plain.geom, 'obstacles+grid': ops.DeviceWorld(plain.geom, sdf=plain.sdf_geom),
              'obstacles+self': ops.DeviceWorld(plain.geom, self_collision=plain.self_geom), 'world': world.world}
    planners = {}
    for name, scene in scenes.items():
        p = RRTConnect(task=world, n_iters=n_iters, start_state_pos=starts, goal_state_pos=goals, step_size=np.pi / 80, n_radius=np.pi / 4,
                       tensor_args=world.tensor_args, n_pre_samples=len(pool), pre_samples=pool, seed=3, chunk_iters=n_iters + 1)
        p.scene = scene
        planners[name] = p
    r = timed({k: (lambda p=p: p.optimize_batched()) for k, p in planners.items()})
    for k, p in planners.items():
        found = int((p.optimize_batched()[2] == ops.RRT_FOUND).sum())
        print(f'rrt        B {B}, {n_iters} iterations, {k:15s}: {r[k][0]:.3f} ms (median {r[k][1]:.3f}), {found} found', flush=True)
    return r


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', choices=('predicate', 'validation', 'rrt'))
    ap.add_argument('--json')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_world.py needs a GPU: there is no CPU path and no figure without one')
    plain, world = tasks(torch.device('cuda:0'))
    results = {}
    for name, fn in (('predicate', part_predicate), ('validation', part_validation), ('rrt', part_rrt)):
        if args.part in (None, name):
            results[name] = {str(k): v for k, v in fn(plain, world).items()}
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(results, fh, indent=1)
