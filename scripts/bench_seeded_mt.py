"""noise='mt19937' at C3 (the headline's shape: Panda + spheres, P = 128, S = 32, H = 64, d = 14): STOMP it/s with the reference's
CPU-generator draws made on the CPU ('torch_cpu'), on the device generator ('torch') and by the device mt19937 ('mt19937'),
K iterations per optimize(), check='sync'; the reference examples' opt_iters=1 loop with 'mt19937'; the device time of one
16-iteration mt19937 draw split into its three launches (events); the host time to build the jump tables.  One JSON line.

    python scripts/bench_seeded_mt.py [--steps 20]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--blocks', type=int, default=3)
    args = ap.parse_args()
    from motion_planning_baselines_amd import mt19937 as MT, ops, workloads
    from motion_planning_baselines_amd.planners.stomp import STOMP
    from motion_planning_baselines_amd.planners.costs.cost_functions import CostCollision, CostComposite
    dev = torch.device('cuda:0')
    P, S, H = 128, 32, 64
    wl = workloads.panda_spheres_stomp(P, dev, H=H, S=S, pos_only=False)
    ta = dict(device=dev, dtype=torch.float32)
    cost = CostComposite(wl['robot'], H, [CostCollision(wl['robot'], H, field=wl['field'], sigma_coll=wl['sigma_coll'],
                                                        tensor_args=ta)], tensor_args=ta)
    d = wl['means0'].shape[-1]
    n = S * d * P * H
    K = args.steps
    # host: the jump tables of the shapes a K-iteration call draws (chunks of 16 and the remainder), built from scratch
    MT.jump_tables.cache_clear()
    MT.char_poly.cache_clear()
    MT._mod.cache_clear()
    t0 = time.perf_counter()
    MT.char_poly()
    t_phi = time.perf_counter() - t0
    t_tables = {}
    for calls in sorted({min(K, 16), K % 16 or 16}):
        t_tables[str(calls)] = MT.jump_tables(n, calls, MT.segments_per_call(n, calls))[3]
    out = {'metric': 'STOMP C3 iterations/s on identical seeds (torch CPU generator stream)', 'steps_per_optimize': K,
           'block': [S, d, P, H], 'normals_per_iteration': n, 'host_char_poly_s': t_phi, 'host_jump_tables_s': t_tables}

    def planner(noise, opt_iters):
        return STOMP(opt_iters=opt_iters, start_state=torch.from_numpy(wl['starts'][0]).to(dev), cost=cost,
                     initial_particle_means=wl['means0'], tensor_args=ta, noise=noise, seed=0, check='sync', **wl['params'])

    def rate(pl, calls, iters_per_call):
        torch.manual_seed(0)
        pl.optimize(opt_iters=iters_per_call)                         # warm-up: tables, buffers, workspace
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.blocks):
            pl._particle_means.copy_(wl['means0'])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                pl.optimize(opt_iters=iters_per_call)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / (calls * iters_per_call))
        t = sorted(ts)[len(ts) // 2]
        return {'value': 1.0 / t, 'unit': 'iters/s', 'ms_per_step': 1e3 * t}

    modes = {}
    for noise in ('torch_cpu', 'torch', 'mt19937'):
        modes[noise] = rate(planner(noise, K), 1, K)
        torch.cuda.empty_cache()
    out['modes'] = modes
    out['mt19937_opt_iters_1_loop'] = rate(planner('mt19937', 1), K, 1)
    # the device split of one 16-iteration draw
    buf = torch.empty(16, S, d, P, H, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    torch.manual_seed(0)
    gen = ops.TorchCpuGeneratorOnDevice(dev)
    gen.normal_(buf, 16)
    spl = []
    for _ in range(5):
        gen.normal_(buf, 16, events=ev)
        torch.cuda.synchronize()
        spl.append([ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), ev[2].elapsed_time(ev[3])])
    gen.store()
    spl.sort(key=sum)
    pre, jump, genr = spl[len(spl) // 2]
    tb = ops._mt_tables(n, 16, dev)
    out['device_ms_per_16_iteration_draw'] = {'prefix': pre, 'jump': jump, 'generate': genr, 'segments': tb.n_segs}
    out['device_ms_per_iteration'] = {'prefix': pre / 16, 'jump': jump / 16, 'generate': genr / 16, 'total': (pre + jump + genr) / 16}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
