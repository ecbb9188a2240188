"""Record tests/golden/sample_based_bits.npz: everything the sample-based kernels leave behind on the cases of
tests/sample_based_bits.py, as integer arrays, from the library of the commit BEFORE a change that must not move a bit.

Runs on the GPU against that commit's library, selected with MPB_LIB_PATH (build it from a checkout of that commit); the commit's hash
goes into the fixture:

    MPB_LIB_PATH=/path/to/parent/libmpb_hip.so python tests/golden/make_sample_based_bits.py PARENT_COMMIT_HASH

Per case it looks over (radius, seed) for a run that meets the conditions of sample_based_bits.conditions on few enough nodes, picks
the starts and goals among configurations the library's own predicate calls free, and refuses to write a fixture in which a case
misses a condition; a fixture larger than the largest RRT golden is an error.  Only data is written."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.environ.get('MPB_GOLDEN_OUT') or os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.dont_write_bytecode = True

import sample_based_bits as S  # noqa: E402
from motion_planning_baselines_amd import _lib  # noqa: E402

MAX_BYTES = 91654                                   # tests/golden/rrt_star_panda_spheres.npz, the largest RRT golden
SCALES, SEEDS = (1.0, 0.5, 0.25, 0.125), range(48)


def main():
    commit = sys.argv[1]
    assert os.environ.get('MPB_LIB_PATH'), 'select the parent commit\'s library with MPB_LIB_PATH'
    print('library', _lib.LIB_PATH, 'parent commit', commit, flush=True)
    dev = torch.device('cuda:0')
    fixture = dict(parent_commit=np.frombuffer(commit.encode(), dtype=np.uint8))
    for kind, name in S.CASES:
        geom, q_min, q_max, pool, radius0 = S.scene(name, dev)
        informed = (kind, name) == S.INFORMED
        best = None
        for scale in SCALES:
            for seed in SEEDS:
                q = S.free_configs(geom, q_min, q_max, 2 * S.B, 1000 + seed, dev)
                out = S.run(kind, geom, dev, q[:S.B], q[S.B:], pool, radius0 * scale, seed, informed)
                cond, n_nodes = S.conditions(kind, out, radius0 * scale)
                if all(cond.values()) and (best is None or n_nodes < best[0]):
                    best = (n_nodes, scale, seed, q, out)
                if best is not None and best[0] <= S.NODE_CAP:
                    break
            if best is not None and best[0] <= S.NODE_CAP:
                break
        assert best is not None, f'{kind} {name}: no (radius, seed) meets the conditions; the last run gave {cond}'
        n_nodes, scale, seed, q, out = best
        print(f'{kind:8s}{name:14s} radius {radius0 * scale:.4f} seed {seed}: {n_nodes} nodes, status {out["status"].tolist()}, iters '
              f'{out["iters"].tolist()}, counts {(out["counts"] if kind == "connect" else out["count"]).tolist()}'
              + (f', rewires {out["rewires"].tolist()}, rejections {out["informed_rejections"].tolist()}' if kind == 'star' else ''),
              flush=True)
        fixture[f'{kind}.{name}'] = S.pack(out)
        fixture[f'{kind}.{name}.inputs'] = S.pack_inputs(q[:S.B], q[S.B:], radius0 * scale, seed)
    extra = S.run_extra(dev)
    fixture[S.EXTRA] = S.pack(extra)
    free = int((extra['edge_flag'] == 0).sum())
    accepted = _f32sum(extra['sc_stats'][:, 1])
    print(f'd3: {free}/64 edges free, {accepted:.0f} shortcuts accepted', flush=True)
    assert all(v.dtype in (np.uint32, np.uint8) for v in fixture.values())
    path = os.path.join(HERE, 'sample_based_bits.npz')
    np.savez_compressed(path, **fixture)
    size = os.path.getsize(path)
    print('wrote', path, size, 'bytes', flush=True)
    if size > MAX_BYTES:
        raise SystemExit(f'{size} bytes: larger than the largest RRT golden ({MAX_BYTES}); lower sample_based_bits.NODE_CAP')


def _f32sum(a):
    return float(np.ascontiguousarray(a).view(np.float32).sum())


if __name__ == '__main__':
    main()
