"""Timing of the SDF-grid kernels against the analytic collision kernels on the device.

    python scripts/bench_sdf_grid.py [--reps 20] [--sizes 128,4096,131072] [--cells 0.02,0.01]

Shape: Panda, H = 64, d = 7, N trajectories uniform in the joint limits; min of `reps` timed calls (events around one call each, after a
warm-up).  Two scenes: env_spheres_3d() (16 spheres, compact broad-phase grid) and env_spheres_boxes_3d() (200 spheres + 32 boxes: the
exhaustive walk outside persistent STOMP).  Per scene and cell size the grid over [-1.2, 1.2]^2 x [-0.7, 1.5] is built on the device
(GridSDFField.from_field -> mpb_sdf_grid_build, timed) and then
  grid      ops.sdf_grid_eval / ops.sdf_grid_grad (mpb_sdf_grid_*: FK, eight node loads per collision sphere, J^T in one kernel)
  analytic  ops.cost_collision_eval / ops.cost_collision_grad on the scene's obstacle list
are timed on the same trajectories.  Prints one line per (scene, cell, N) and a JSON line with all figures (milliseconds, grid MB).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from motion_planning_baselines_amd import geometry as G, ops          # noqa: E402

LO, HI = (-1.2, -1.2, -0.7), (1.2, 1.2, 1.5)


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
    ap.add_argument('--cells', default='0.02,0.01')
    ap.add_argument('--H', type=int, default=64)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    robot = G.RobotPanda()
    H, D = args.H, robot.q_dim
    sizes = [int(v) for v in args.sizes.split(',')]
    rng = np.random.RandomState(0)
    xs = {N: torch.from_numpy(rng.uniform(robot.q_min_np, robot.q_max_np, (N, H, D)).astype(np.float32)).to(dev) for N in sizes}
    rows = []
    for scene, field in (('spheres_3d', G.env_spheres_3d()), ('spheres_boxes_3d', G.env_spheres_boxes_3d())):
        geom = ops.DeviceGeometry(robot, field, dev)
        analytic = {}
        for N in sizes:
            x = xs[N]
            analytic[N] = (time_min(lambda: ops.cost_collision_eval(x, geom, 1.0), args.reps),
                           time_min(lambda: ops.cost_collision_grad(x, geom, 1.0), args.reps))
        for cell in [float(v) for v in args.cells.split(',')]:
            gf = G.GridSDFField.from_field(field, LO, HI, cell)
            sdf = ops.DeviceSDFGrid(robot, gf, dev)                       # (builds once: the warm-up of the timed builds below)
            builder = ops.DeviceGeometry(G.RobotPointMass(3), field, dev, use_model=False)
            build_ms = time_min(lambda: ops.sdf_grid_build(builder, sdf), min(args.reps, 5))
            mb = 4.0 * gf.dims[0] * gf.dims[1] * gf.dims[2] / 2 ** 20
            for N in sizes:
                x = xs[N]
                c_grid, c_an = ops.sdf_grid_eval(x, sdf, 1.0), ops.cost_collision_eval(x, geom, 1.0)
                row = dict(scene=scene, n_sph=int(len(field.spheres)), n_box=int(len(field.boxes)), cell=cell, dims=list(gf.dims), grid_mb=round(mb, 1),
                           build_ms=build_ms, N=N, H=H,
                           eval_grid_ms=time_min(lambda: ops.sdf_grid_eval(x, sdf, 1.0), args.reps), eval_analytic_ms=analytic[N][0],
                           grad_grid_ms=time_min(lambda: ops.sdf_grid_grad(x, sdf, 1.0), args.reps), grad_analytic_ms=analytic[N][1],
                           cost_rel_diff=float((c_grid - c_an).abs().max() / c_an.abs().max().clamp_min(1e-30)))
                rows.append(row)
                print('%-16s cell %.3f (%4.1f MB, build %.3f ms) N = %6d: eval grid %.3f ms, analytic %.3f ms; grad grid %.3f ms, analytic %.3f ms'
                      % (scene, cell, mb, build_ms, N, row['eval_grid_ms'], row['eval_analytic_ms'], row['grad_grid_ms'], row['grad_analytic_ms']),
                      flush=True)
            del sdf
            torch.cuda.empty_cache()
    print(json.dumps(dict(bench='sdf_grid', robot='panda', reps=args.reps, rows=rows)))


if __name__ == '__main__':
    main()
