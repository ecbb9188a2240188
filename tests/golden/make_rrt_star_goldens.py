"""Generate the RRT* / informed RRT* golden vectors by running the UNMODIFIED reference RRTStar class.

Runs ONLY in the build container (it needs the reference checkout that oracle.ref_stub.import_reference() imports) and
reuses make_rrt_goldens.py (the task on the oracle geometry, the live timer, the pool of free configurations, FACTOR).
Only DATA is written, to rrt_star_<scene>.npz next to this script; no reference source is copied.

    python tests/golden/make_rrt_star_goldens.py            # every scene
    python tests/golden/make_rrt_star_goldens.py NAME ...   # only the named scenes (rrt_star_pm2d_grid, ...)

Per candidate problem the reference runs in fp32 and in fp64 on the same pool, seed, start and goal.  torch.randperm (the
pool index) and torch.rand (the goal draw) are recorded per iteration.  A candidate is ELIGIBLE when both runs have the
same OUTCOME: the recorded draws, node count and parents, pool length, iterations, goal index, path length, stop
reason, and the accepted rewires (iteration and node, in order -- two runs can differ in a rewire that a later one
overwrites and still end in the same tree) and the number of informed rejections.  Call counts are not compared: a node created by a clamped extension sits at n_radius from its parent up to
rounding, so its membership in the neighbour set flips between the two runs -- which never matters, because its rewire
test cannot pass.  Every decision input is therefore recorded under a key (iteration, call site, neighbour index), and
the envelopes are measured over the keys both runs have:
    E_gap  = max |hinge argument fp32 - fp64| over every collision decision,
    E_dist = max |distance fp32 - fp64| over every distance the planner evaluated,
    E_cost = max |cost fp32 - fp64| over all nodes of the final trees and all operands of the rewire tests,
    E_eps  = max relative difference between torch's fp32 norm and an fp64 norm of the same fp32 vector, over the two
             `< eps` decisions (goal detection rrt_star.py:216, the rewire's n_dist :249-250), floored at 2^-23.
Decision margins (fp64 run unless stated), each screened with FACTOR = 32 (make_rrt_goldens.py says why):
    hinge >= F E_gap; argmin, count, radius (extension) >= F E_dist;
    rewire   : |new.cost + d - n.cost| of every rewire test >= F E_cost, EXCEPT structural ties (exactly 0.0 in the fp32
               run and below 1e-12 in the fp64 run: both sides come from the same operations on the same bits);
    nbr      : |distance - n_radius| of the neighbours whose rewire test passes >= F E_dist, and the point count of
               their edge (count) >= F E_dist;
    informed : |d(start, s) + d(s, goal) - goal cost| >= F E_cost;   best: |goal cost - (best_cost_eps - cost_eps)| >= F E_cost;
    eps      : (fp32 run) |d - eps| / max(d, eps) of the two `< eps` decisions >= F E_eps.
The operands of a rewire test are not arguments of any patched function: they are read from the calling frame of
distance_q (sys._getframe) at the reference's call sites, identified by their line numbers in rrt_star.py.
"""
import contextlib
import io
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
import make_rrt_goldens as base  # noqa: E402
from make_rrt_goldens import FACTOR, G, HERE, ONLY, LiveTimer, RefTask, free_configs  # noqa: E402

import mp_baselines.planners.rrt_star as _ref  # noqa: E402
from mp_baselines.planners.rrt_star import RRTStar  # noqa: E402

N_KEEP = 12
# the reference's call sites of distance_fn / collision_fn in RRTStar._run_optimization (line numbers of rrt_star.py)
DIST_SITES = {197: 'informed', 202: 'nearest', 205: 'extend', 213: 'new_d', 214: 'new_d', 216: 'goal', 225: 'nbrs',
              244: 'rw_d', 246: 'rw_extend', 249: 'rw_ndist'}
COLL_SITES = {143: 'ends', 206: 'extend', 247: 'rewire'}
STOP_ITERS, STOP_COST, STOP_AFTER = 1, 2, 3                      # include/mpb.h MPB_RRT_STOP_*


def _run_frame():
    f = sys._getframe(2)
    while f is not None and f.f_code.co_name != '_run_optimization':
        f = f.f_back
    assert f is not None, 'called from outside RRTStar._run_optimization'
    return f


class StarTimer(LiveTimer):
    """Counts the loop-condition reads of `elapsed` (one per loop body started, one more when the loop runs out, one for
    the final print_info) and records what the NEXT body's best-cost test will compare."""
    last = None

    def __enter__(self):
        self.reads, self.best_margins, self.goal_costs = 0, [], []
        StarTimer.last = self
        return super().__enter__()

    @property
    def elapsed(self):
        f = sys._getframe(1)
        if f.f_code.co_name == '_run_optimization':
            self.reads += 1
            loc = f.f_locals
            g = loc.get('goal_n')
            if g is not None:
                self.goal_costs.append(float(g.cost))
                be = float(loc['best_cost_eps'])
                if np.isfinite(be):
                    self.best_margins.append(abs(float(g.cost) - (be - loc['self'].cost_eps)))
        return time.perf_counter() - self._t0


_ref.TimerCUDA = StarTimer


class StarTask(RefTask):
    """RefTask recording every decision input under (iteration, call site, neighbour index)."""

    def __init__(self, robot, field, dtype, prm):
        super().__init__(robot, field, dtype)
        self.prm = prm
        self.kd, self.kg = {}, {}                                 # key -> distances / hinge arguments
        self.m = dict(argmin=np.inf, count=np.inf, radius=np.inf, rewire=np.inf, nbr=np.inf, informed=np.inf, eps=np.inf)
        self.cost_ops = {}                                        # key -> (new.cost, n.cost) of a rewire test
        self.rewire_margins = {}                                  # key -> new.cost + d - n.cost
        self.e_eps = 0.0
        self.n_pass = self.n_rewires = self.n_rewires_children = self.n_dup = self.n_rejected = 0
        self._d1 = None
        self.rewire_keys = []                                     # (iteration, neighbour index) of every accepted rewire, in order

    @staticmethod
    def _key(f, site):
        loc = f.f_locals
        k = loc['self'].nodes.index(loc['n']) if site.startswith('rw') or site == 'rewire' else 0
        return (int(loc.get('iteration', -1)), site, k)

    def compute_collision(self, qs, **kwargs):
        f = _run_frame()
        g = self.hinge_argument(qs)
        self.kg[self._key(f, COLL_SITES[f.f_lineno])] = g.detach().reshape(-1).double().numpy().copy()
        return g > 0

    def _count_margin(self, d):
        x = d / self.prm['step_size']
        return min(x - np.floor(x), np.ceil(x) - x) * self.prm['step_size']

    def _eps_decision(self, q1, q2, d, eps):
        if d.dtype == torch.float32:
            d64 = float(torch.linalg.norm((q1 - q2).double()))
            if d64 > 0:
                self.e_eps = max(self.e_eps, abs(float(d) - d64) / d64)
            self.m['eps'] = min(self.m['eps'], abs(float(d) - eps) / max(float(d), eps))

    def distance_q(self, q1, q2):
        f = _run_frame()
        site = DIST_SITES[f.f_lineno]
        loc = f.f_locals
        d = torch.linalg.norm(q1 - q2, dim=-1)
        key = self._key(f, site)
        if site == 'informed':                                   # two calls: d(start, s), then d(s, goal)
            if self._d1 is None:
                self._d1, key = d, key[:2] + (0,)
            else:
                key = key[:2] + (1,)
                lhs, gc = self._d1 + d, loc['goal_n'].cost
                self.m['informed'] = min(self.m['informed'], abs(float(lhs) - float(gc)))
                self.n_rejected += int(bool(lhs >= gc))
                self._d1 = None
        dv = d.detach().reshape(-1).double().numpy().copy()
        self.kd[key] = dv
        if site == 'nearest' and len(dv) > 1:
            nodes = q1.detach().double().numpy()
            best = int(np.argmin(dv))
            other = (nodes != nodes[best]).any(axis=1)
            if other.any():
                self.m['argmin'] = min(self.m['argmin'], float(dv[other].min() - dv[best]))
        elif site == 'extend':
            self.m['count'] = min(self.m['count'], self._count_margin(dv[0]))
            self.m['radius'] = min(self.m['radius'], abs(dv[0] - self.prm['n_radius']))
        elif site == 'new_d':
            self.n_dup += int(dv[0] == 0.0)
        elif site == 'goal':
            if loc['do_goal']:
                self._eps_decision(q1, q2, d, loc['eps'])
        elif site == 'rw_d':
            new, n = loc['new'], loc['n']
            lhs = new.cost + d
            margin = float(lhs) - float(n.cost)
            self.rewire_margins[key] = margin
            self.cost_ops[key] = (float(new.cost), float(n.cost))
            if bool(lhs < n.cost):
                self.n_pass += 1
                self.m['nbr'] = min(self.m['nbr'], abs(dv[0] - self.prm['n_radius']), self._count_margin(dv[0]))
        elif site == 'rw_ndist':
            self._eps_decision(q1, q2, d, loc['eps'])
            if bool(d < loc['eps']):
                self.n_rewires += 1
                self.rewire_keys.append((key[0], key[2]))
                self.n_rewires_children += int(len(loc['n'].children) > 0)
        return d


class DrawRecorder:
    """torch.randperm (pool index) and torch.rand (goal draw) per iteration of the calling _run_optimization."""

    def __init__(self, n_iters, goal_prob):
        self.idx = np.zeros(n_iters + 1, np.int32)
        self.goal = np.zeros(n_iters + 1, np.int32)
        self.goal[0] = 1                                          # iteration 0 always aims at the goal (no draw)
        self.goal_prob = goal_prob
        self._randperm, self._rand = torch.randperm, torch.rand

    def __enter__(self):
        def randperm(n, *a, **k):
            p = self._randperm(n, *a, **k)
            self.idx[_run_frame().f_locals['iteration']] = int(p[0])
            return p

        def rand(*a, **k):
            r = self._rand(*a, **k)
            self.goal[_run_frame().f_locals['iteration']] = int(bool(r < self.goal_prob))
            return r
        torch.randperm, torch.rand = randperm, rand
        return self

    def __exit__(self, *a):
        torch.randperm, torch.rand = self._randperm, self._rand


def run_reference(robot, field, dtype, pool, start, goal, prm, seed):
    task = StarTask(robot, field, dtype, prm)
    ta = task.ta
    planner = RRTStar(task=task, n_iters=prm['n_iters'], start_state_pos=torch.as_tensor(start).to(**ta),
                      n_iters_after_success=prm['n_iters_after_success'], step_size=prm['step_size'], n_radius=prm['n_radius'],
                      max_time=1.0e9, goal_state_pos=torch.as_tensor(goal).to(**ta), tensor_args=ta,
                      n_pre_samples=pool.shape[0], pre_samples=torch.as_tensor(pool).to(**ta), informed=prm['informed'])
    torch.manual_seed(seed)
    with DrawRecorder(prm['n_iters'], planner.goal_prob) as rec, contextlib.redirect_stdout(io.StringIO()) as out:
        t0 = time.perf_counter()
        path = planner.optimize()
        seconds = time.perf_counter() - t0
    timer = StarTimer.last
    # print_info's last line carries the final `iteration`; the loop condition read `elapsed` once per body started, once
    # more when the loop ran out (not after a `break`), and print_info's argument once
    last = int(out.getvalue().strip().splitlines()[-1].split('Iteration:')[1].split('/')[0])
    bodies = last + 1
    broke = timer.reads == bodies + 1
    assert broke or timer.reads == bodies + 2, (timer.reads, bodies)
    # (max_best_cost_iters = 1000 > n_iters: the cost-converged rule cannot fire in these runs)
    assert planner.max_best_cost_iters > prm['n_iters']
    stop = STOP_AFTER if broke else STOP_ITERS
    found = isinstance(path, torch.Tensor) and path.ndim == 2 and path.shape[0] >= 2
    nodes = planner.nodes
    pos = {id(n): i for i, n in enumerate(nodes)}
    goal_idx = -1
    if found:
        hits = [i for i, n in enumerate(nodes) if n.solution and not any(c.solution for c in n.children)]
        assert len(hits) == 1, hits
        goal_idx = hits[0]
    gc = np.array(timer.goal_costs)
    return dict(found=found, path=path.double().numpy() if found else np.zeros((0, len(start))), idx=rec.idx, goal_draw=rec.goal,
                q=torch.stack([n.config for n in nodes]).double().numpy(),
                parent=np.array([-1 if n.parent is None else pos[id(n.parent)] for n in nodes], np.int32),
                d=np.array([float(n.d) for n in nodes]), cost=np.array([float(n.cost) for n in nodes]),
                goal_idx=goal_idx, iterations=bodies, stop=stop, pool_len=int(planner.pre_samples.shape[0]), seconds=seconds,
                task=task, best_margin=min(timer.best_margins) if timer.best_margins else np.inf,
                goal_cost_drops=int((np.diff(gc) < 0).sum()) if len(gc) > 1 else 0,
                first_cost=float(gc[0]) if len(gc) else np.nan)


def same_outcome(a, b):
    return (a['found'] == b['found'] and (a['idx'] == b['idx']).all() and (a['goal_draw'] == b['goal_draw']).all()
            and a['parent'].shape == b['parent'].shape and (a['parent'] == b['parent']).all() and a['pool_len'] == b['pool_len']
            and a['iterations'] == b['iterations'] and a['goal_idx'] == b['goal_idx'] and a['path'].shape == b['path'].shape
            and a['stop'] == b['stop'] and a['task'].rewire_keys == b['task'].rewire_keys
            and a['task'].n_rejected == b['task'].n_rejected)


def envelopes(r32, r64):
    t32, t64 = r32['task'], r64['task']
    e_gap = max(float(np.abs(t32.kg[k] - t64.kg[k]).max()) for k in t32.kg if k in t64.kg and t32.kg[k].shape == t64.kg[k].shape)
    e_dist = max(float(np.abs(t32.kd[k] - t64.kd[k]).max()) for k in t32.kd if k in t64.kd and t32.kd[k].shape == t64.kd[k].shape)
    e_cost = float(np.abs(r32['cost'] - r64['cost']).max())
    for k, (a, b) in t32.cost_ops.items():
        if k in t64.cost_ops:
            e_cost = max(e_cost, abs(a - t64.cost_ops[k][0]), abs(b - t64.cost_ops[k][1]))
    return e_gap, e_dist, e_cost, t32.e_eps


def margins(r32, r64):
    """(hinge, argmin, count, radius, rewire, nbr, informed, best, eps) and the number of structural ties."""
    t32, t64 = r32['task'], r64['task']
    hinge = min(float(np.abs(g).min()) for g in t64.kg.values())
    rewire, ties = np.inf, 0
    for k, m64 in t64.rewire_margins.items():
        if t32.rewire_margins.get(k) == 0.0 and abs(m64) < 1e-12:
            ties += 1
            continue
        rewire = min(rewire, abs(m64))
    m = t64.m
    return (hinge, m['argmin'], m['count'], m['radius'], rewire, m['nbr'], m['informed'], r64['best_margin'], t32.m['eps']), ties


def make_scene(name, robot, field, prm, n_candidates, lo, hi, seed, need, n_keep=N_KEEP):
    if ONLY and name not in ONLY:
        return
    rng = np.random.RandomState(seed)
    pool = free_configs(robot, field, prm['n_pre'], rng, lo, hi)
    ends = free_configs(robot, field, 2 * n_candidates, rng, lo, hi)
    cands = []
    for c in range(n_candidates):
        start, goal = ends[2 * c], ends[2 * c + 1]
        r32 = run_reference(robot, field, torch.float32, pool, start, goal, prm, seed=1000 + c)
        r64 = run_reference(robot, field, torch.float64, pool, start, goal, prm, seed=1000 + c)
        ok = same_outcome(r32, r64)
        t = r32['task']
        print(f'{name} candidate {c}: found {r32["found"]}, nodes {len(r32["parent"])}, iterations {r32["iterations"]}, stop {r32["stop"]}, '
              f'rewires {t.n_rewires} ({t.n_rewires_children} with children, {t.n_pass - t.n_rewires} edges rejected), duplicates {t.n_dup}, '
              f'informed rejections {t.n_rejected}, goal cost drops {r32["goal_cost_drops"]}, same fp32/fp64 outcome {ok}, '
              f'reference {r32["seconds"]:.3f} s', flush=True)
        cands.append(dict(start=start, goal=goal, r32=r32, r64=r64, eligible=ok))
    elig = [c for c in cands if c['eligible']]
    env = np.array([envelopes(c['r32'], c['r64']) for c in elig])
    e_gap, e_dist, e_cost, e_eps_measured = env.max(axis=0)
    e_eps = max(e_eps_measured, 2.0 ** -23)
    kept = []
    for c in elig:
        c['margins'], c['ties'] = margins(c['r32'], c['r64'])
        h, a, n, r, rw, nb, inf, best, eps = c['margins']
        c['kept'] = (h >= FACTOR * e_gap and min(a, n, r, nb) >= FACTOR * e_dist and min(rw, inf, best) >= FACTOR * e_cost
                     and eps >= FACTOR * e_eps)
        if c['kept'] and c['r32']['found']:
            kept.append(c)
    n_found = sum(c['r32']['found'] for c in cands)
    print(f'{name}: E_gap {e_gap:.3e}, E_dist {e_dist:.3e}, E_cost {e_cost:.3e}, E_eps {e_eps_measured:.3e}; {len(elig)}/{len(cands)} '
          f'eligible, {sum(c["kept"] for c in elig)} pass the {FACTOR:g} E screen, {n_found}/{len(cands)} found', flush=True)

    def cov(c):
        t = c['r32']['task']
        return dict(children=t.n_rewires_children, drops=c['r32']['goal_cost_drops'], rejected_edges=t.n_pass - t.n_rewires,
                    duplicates=t.n_dup, informed_rejections=t.n_rejected)
    # the problems that carry a coverage condition first, then the rest in candidate order
    chosen = []
    for key in need:
        hit = next((c for c in kept if cov(c)[key] > 0), None)
        assert hit is not None, f'{name}: no kept problem covers {key}: raise the number of candidates'
        if not any(hit is x for x in chosen):
            chosen.append(hit)
    chosen += [c for c in kept if not any(c is x for x in chosen)]
    kept = chosen[:n_keep]
    assert len(kept) >= 8, f'{name}: the screen keeps {len(kept)} found problems: raise the number of candidates'
    rs, fs = robot.spec(), field.spec()
    T = prm['n_iters'] + 1
    out = dict(robot_kind=np.int32(rs['kind']), n_dof=np.int32(rs['n_dof']), joint_tf=rs['joint_tf'], link_frame=rs['link_frame'],
               link_offset=rs['link_offset'], link_radius=rs['link_radius'], spheres=np.asarray(fs['spheres'], np.float32).reshape(-1, 4),
               boxes=np.asarray(fs['boxes'], np.float32).reshape(-1, 6), margin=np.float32(fs['margin']),
               pool=pool, step_size=np.float64(prm['step_size']), n_radius=np.float64(prm['n_radius']), n_iters=np.int32(prm['n_iters']),
               n_iters_after_success=np.int32(prm['n_iters_after_success']), informed=np.int32(prm['informed']),
               goal_prob=np.float64(0.1), cost_eps=np.float64(1e-2), eps=np.float64(1e-6), max_best_cost_iters=np.int32(1000),
               E_gap=np.float64(e_gap), E_dist=np.float64(e_dist), E_cost=np.float64(e_cost), E_eps=np.float64(e_eps),
               E_eps_measured=np.float64(e_eps_measured), factor=np.float64(FACTOR), n_candidates=np.int32(len(cands)),
               n_eligible=np.int32(len(elig)), n_screened=np.int32(sum(c['kept'] for c in elig)), n_found=np.int32(n_found),
               n_problems=np.int32(len(kept)), starts=np.stack([c['start'] for c in kept]), goals=np.stack([c['goal'] for c in kept]),
               margins=np.array([c['margins'] for c in kept], np.float64), structural_ties=np.array([c['ties'] for c in kept], np.int32),
               ref_seconds=np.array([c['r32']['seconds'] for c in kept], np.float64),
               n_iterations=np.array([c['r32']['iterations'] for c in kept], np.int32),
               stop_reason=np.array([c['r32']['stop'] for c in kept], np.int32),
               goal_idx=np.array([c['r32']['goal_idx'] for c in kept], np.int32),
               pool_len_after=np.array([c['r32']['pool_len'] for c in kept], np.int32),
               rewires=np.array([c['r32']['task'].n_rewires for c in kept], np.int32),
               informed_rejections=np.array([c['r32']['task'].n_rejected for c in kept], np.int32),
               first_cost=np.array([c['r32']['first_cost'] for c in kept], np.float64),
               cov_rewire_with_children=np.array([cov(c)['children'] for c in kept], np.int32),
               cov_goal_cost_drops=np.array([cov(c)['drops'] for c in kept], np.int32),
               cov_rejected_edges=np.array([cov(c)['rejected_edges'] for c in kept], np.int32),
               cov_duplicates=np.array([cov(c)['duplicates'] for c in kept], np.int32),
               sample_idx=np.stack([c['r32']['idx'] for c in kept]).reshape(len(kept), T),
               goal_draw=np.stack([c['r32']['goal_draw'] for c in kept]).reshape(len(kept), T))
    for k, c in enumerate(kept):
        r = c['r32']
        out[f'p{k}_q'] = r['q'].astype(np.float32)
        out[f'p{k}_parent'] = r['parent']
        out[f'p{k}_d'] = r['d'].astype(np.float32)
        out[f'p{k}_cost'] = r['cost'].astype(np.float32)
        out[f'p{k}_path'] = r['path'].astype(np.float32)
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path}: {len(kept)} problems, {os.path.getsize(path)} bytes', flush=True)


def main():
    pm = G.RobotPointMass(2, radius=0.01)
    lo2, hi2 = np.float32([-0.95, -0.95]), np.float32([0.95, 0.95])
    need2 = ('children', 'drops', 'rejected_edges', 'duplicates')
    for informed in (0, 1):
        prm = dict(step_size=0.1, n_radius=0.3, n_iters=400, n_iters_after_success=150, n_pre=1000, informed=informed)
        sfx = '_inf' if informed else ''
        need = need2 + (('informed_rejections',) if informed else ())
        make_scene('rrt_star_pm2d_grid' + sfx, pm, G.env_grid_circles_2d(), prm, 96, lo2, hi2, seed=21 + informed, need=need)
        make_scene('rrt_star_pm2d_dense' + sfx, pm, G.env_dense_2d(seed=3), prm, 96, lo2, hi2, seed=23 + informed, need=need)
    panda = G.RobotPanda()
    make_scene('rrt_star_panda_spheres', panda, G.env_spheres_3d(seed=0),
               dict(step_size=np.pi / 80, n_radius=np.pi / 2, n_iters=400, n_iters_after_success=150, n_pre=1000, informed=0),
               128, panda.q_min_np, panda.q_max_np, seed=25, need=('children',), n_keep=8)   # (8: the file stays under 100 KB)


if __name__ == '__main__':
    main()
