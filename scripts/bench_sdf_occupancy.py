"""Timing of the SDF-grid build from occupancy voxels (mpb_sdf_grid_build_occupancy: the exact Euclidean distance transform, three
launches, in place in the node section) on the device.

    python scripts/bench_sdf_occupancy.py [--reps 20] [--cells 0.02,0.01]

Scenes: env_spheres_3d() (16 spheres) and env_spheres_boxes_3d() (200 spheres + 32 boxes), voxelised (sdf < 0 at the node: the nodes of
the grid GridSDFField.from_field builds, thresholded on the device) over [-1.2, 1.2]^2 x [-0.7, 1.5]: 122 x 122 x 112 nodes at cell 0.02,
242 x 242 x 222 at 0.01.  Per scene and cell: min of `reps` timed calls (events around one call each, after a warm-up) of
  occupancy   ops.sdf_grid_build_occupancy on the occupancy bytes resident on the device (what DeviceSDFGrid.update_occupancy launches)
  from_field  ops.sdf_grid_build of the same grid from the obstacle list
  scipy       scipy.ndimage.distance_transform_edt of the occupancy and of its complement on the host, when scipy imports (wall clock)
Prints one line per (scene, cell) and a JSON line with all figures (milliseconds).  Nothing is asserted on a time.
"""
import argparse
import json
import os
import sys
import time

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
    ap.add_argument('--cells', default='0.02,0.01')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    robot = G.RobotPointMass(3)
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    rows = []
    for scene, field in (('spheres_3d', G.env_spheres_3d()), ('spheres_boxes_3d', G.env_spheres_boxes_3d())):
        builder = ops.DeviceGeometry(robot, field, dev, use_model=False)
        for cell in [float(v) for v in args.cells.split(',')]:
            gf = G.GridSDFField.from_field(field, LO, HI, cell)
            sdf = ops.DeviceSDFGrid(robot, gf, dev)                       # (builds once from the obstacle list)
            occ = (sdf.nodes < 0).to(torch.uint8).contiguous()
            from_field_ms = time_min(lambda: ops.sdf_grid_build(builder, sdf), args.reps)
            occupancy_ms = time_min(lambda: ops.sdf_grid_build_occupancy(occ, sdf), args.reps)
            row = dict(scene=scene, n_sph=int(len(field.spheres)), n_box=int(len(field.boxes)), cell=cell, dims=list(gf.dims),
                       occupied=int(occ.sum()), occupancy_ms=occupancy_ms, from_field_ms=from_field_ms, scipy_ms=None)
            if ndimage is not None:
                host = occ.cpu().numpy() != 0
                best = float('inf')
                for _ in range(3):
                    t0 = time.perf_counter()
                    ndimage.distance_transform_edt(host)
                    ndimage.distance_transform_edt(~host)
                    best = min(best, (time.perf_counter() - t0) * 1e3)
                row['scipy_ms'] = best
            rows.append(row)
            print('%-16s cell %.3f %s (%d occupied): occupancy %.3f ms, from_field %.3f ms, scipy %s ms'
                  % (scene, cell, 'x'.join(str(d) for d in gf.dims), row['occupied'], occupancy_ms, from_field_ms,
                     'n/a' if row['scipy_ms'] is None else '%.1f' % row['scipy_ms']), flush=True)
            del sdf, occ
            torch.cuda.empty_cache()
    print(json.dumps(dict(bench='sdf_occupancy', reps=args.reps, rows=rows)))


if __name__ == '__main__':
    main()
