"""Time parameterisation of a trajectory batch under the Panda's data-sheet limits, H = 64, on the (N, H, 14) state tensor a planner
returns, at N = 128, 4 096 and 131 072:

  fused     ops.traj_retime on the state tensor in place (one launch of mpb_traj_retime), and ops.traj_retime_sample at dt = 1 ms
            (up to N = 4 096: at 131 072 that batch is 12 GB);
  composed  the same recursion (include/mpb.h) in batched torch on the device: a Python loop over H, every step on (N, pairs) tensors.

Timing: warm-up calls first, then HIP events around each call, min and median over the repeats.  The composed route's x and t are
compared with the kernel's before anything is timed.

    timeout -k 10 300 python scripts/bench_retime.py [--n 4096] [--json OUT]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from motion_planning_baselines_amd import geometry as G, ops  # noqa: E402

H, D, WARMUP, DT = 64, 7, 3, 1e-3


def make_states(N, device, seed=11):
    """(N, H, 2D) states: a straight line between two configurations plus four sine harmonics of amplitude 0.3 / k; the velocity half is
    never read."""
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    s = torch.linspace(0, 1, H, device=device)[None, :, None]
    u = 3.0 * torch.rand(6, N, 1, D, device=device, generator=gen) - 1.5
    pos = u[0] + (u[1] - u[0]) * s
    for k in range(1, 5):
        pos = pos + (0.3 / k) * (u[1 + k] / 1.5) * torch.sin(k * torch.pi * s)
    return torch.cat([pos, torch.zeros_like(pos)], dim=-1).contiguous()


def composed(states, v_max, a_max, sdot_max=1e3):
    """The definition in batched torch: (x (N, H), t (N, H))."""
    q = states[..., :D]
    N = q.shape[0]
    p, c = torch.empty_like(q), torch.zeros_like(q)
    p[:, 1:-1] = (q[:, 2:] - q[:, :-2]) * 0.5
    c[:, 1:-1] = (q[:, 2:] - q[:, 1:-1]) - (q[:, 1:-1] - q[:, :-2])
    p[:, 0], p[:, -1] = q[:, 1] - q[:, 0], q[:, -1] - q[:, -2]
    inf = torch.tensor(float('inf'), device=q.device)
    one, A = torch.ones(N, 1, device=q.device), a_max.expand(N, D)
    xv = torch.minimum(torch.where(p != 0, v_max / p.abs(), inf).amin(-1), torch.tensor(sdot_max, device=q.device)) ** 2

    def lines(i, beta_next):
        a = torch.cat([p[:, i], p[:, i + 1] + 2 * c[:, i + 1], 2 * one], 1)
        b = torch.cat([c[:, i], c[:, i + 1], one], 1)
        cp, cn = torch.cat([A, A, beta_next[:, None]], 1), torch.cat([A, A, 0 * one], 1)
        s = a > 0
        return a, b, cp, (a.abs(), torch.where(s, b, -b), torch.where(s, cp, cn)), (-a.abs(), torch.where(s, -b, b), torch.where(s, cn, cp))

    beta = torch.zeros(N, H, device=q.device)
    for i in range(H - 2, 0, -1):
        a, b, cp, (a1, b1, c1), (a2, b2, c2) = lines(i, beta[:, i + 1])
        best = torch.minimum(xv[:, i], torch.where((a == 0) & (b != 0), cp / b.abs(), inf).amin(1))
        k = a1[:, :, None] * b2[:, None, :] - a2[:, None, :] * b1[:, :, None]
        num = a1[:, :, None] * c2[:, None, :] - a2[:, None, :] * c1[:, :, None]
        ok = (a != 0)[:, :, None] & (a != 0)[:, None, :] & (k > 0)
        beta[:, i] = torch.minimum(best, torch.where(ok, num / k, inf).reshape(N, -1).amin(1))
    x, t = torch.zeros(N, H, device=q.device), torch.zeros(N, H, device=q.device)
    for i in range(H - 1):
        a, _, _, (a1, b1, c1), _ = lines(i, beta[:, i + 1])
        u = torch.where(a != 0, (c1 - b1 * x[:, i, None]) / a1, inf).amin(1)
        x[:, i + 1] = torch.clamp_min(torch.minimum(beta[:, i + 1], x[:, i] + 2 * u), 0)
        t[:, i + 1] = t[:, i] + 2 / (x[:, i].sqrt() + x[:, i + 1].sqrt())
    return x, t


def timed(fn, repeats):
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return min(out), statistics.median(out)


def run(N, repeats, device):
    robot = G.RobotPanda()
    v, a = robot.dq_max.to(device), robot.ddq_max.to(device)
    states = make_states(N, device)
    tm = ops.traj_retime(states, v, a)
    x, t = composed(states, v, a)
    torch.cuda.synchronize()
    assert not bool(tm.status.any())
    M = float(tm.x.max())
    ex, et = float((x - tm.x).abs().max()) / M, float((t - tm.t).abs().max())
    assert ex < 1e-3 and et < 1e-3, (ex, et)
    sample = N <= 4096                                           # (at 131 072 the 1 ms batch is 12 GB: nobody samples all of them)
    rows = int(ops.traj_retime_sample(states, tm, DT)[0].shape[1]) if sample else None
    for _ in range(WARMUP):
        ops.traj_retime(states, v, a)
        if sample:
            ops.traj_retime_sample(states, tm, DT, n_rows=rows)
        composed(states, v, a)
    res = dict(N=N, H=H, D=D, repeats=repeats, dt=DT, sample_rows=rows, median_duration_s=float(tm.duration.median()),
               composed_x_rel_diff=ex, composed_t_abs_diff_s=et)
    res['retime_ms_min'], res['retime_ms_median'] = timed(lambda: ops.traj_retime(states, v, a), repeats)
    if sample:
        res['sample_ms_min'], res['sample_ms_median'] = timed(lambda: ops.traj_retime_sample(states, tm, DT, n_rows=rows), repeats)
    res['composed_ms_min'], res['composed_ms_median'] = timed(lambda: composed(states, v, a), repeats)
    res['speedup_min'] = res['composed_ms_min'] / res['retime_ms_min']
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=None)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_retime.py needs a GPU: there is no CPU path')
    device = torch.device('cuda:0')
    results = []
    for N in ([args.n] if args.n else [128, 4096, 131072]):
        r = run(N, args.repeats, device)
        results.append(r)
        print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(results, fh, indent=1)


if __name__ == '__main__':
    main()
