"""mpb_path_shortcut's definition (include/mpb.h) restated twice on the CPU (helper module, no tests; imported like
rrt_checks.py and collision_kinks.py).

restate32(p): fp32 throughout, in the operation order the definition gives -- numpy float32 scalars and arrays round after every
  operation, so mul-then-add reproduces the kernel's no-fma forms -- with the collision cost of the fp32 oracle
  (oracle/geometry_ref.py built in float32): a point is in collision iff that cost is positive.
replay64(p, log): the same point arithmetic in fp32 (the points are data), every dense point's clearance and hinge in fp64 from the
  oracle's geometry functions, and a `log` (the kernel's, or restate32's) to hold against them.  Per tested candidate, over the
  points the scan has to look at (all of them, or those up to the first one in collision in fp64):
      m_p   = max over fields and collision spheres of (margin + r_l - sd(x_l)), fp64: positive = in collision,
      E32   = max_p |m_p(fp32 oracle) - m_p(fp64)|, the fp32 restatement's own error ON THOSE POINTS,
      the decision is DECIDABLE when min_p |m_p| > bar(E32) = collision_kinks.bar(E32) = 4 max(E32, 2^-23).
  A decidable decision must equal the log (code and first-collision index); an undecidable one follows the log.  The decisions
  that involve no geometry (IDLE, SKIP, and OVERFLOW against ACCEPT once the candidate is free) must always equal the log.

Both return the final paths and lengths, a log and the stats; replay64 adds per candidate what a test wants to assert on.
"""
import functools
import types

import numpy as np
import torch

from collision_kinks import bar
from motion_planning_baselines_amd import ops
from oracle.geometry_ref import make_ref_geometry

# the log's codes and the shift of the first-collision index: the product's numbers (include/mpb.h MPB_SHORTCUT_*)
IDLE, SKIP, REJECT, OVERFLOW, ACCEPT = (getattr(ops, 'SHORTCUT_' + c) for c in ops.SHORTCUT_CODES)
SHIFT = ops.SHORTCUT_LOG_INDEX_SHIFT
MAX_PTS = 1 << 20
F32 = dict(device='cpu', dtype=torch.float32)
F64 = dict(device='cpu', dtype=torch.float64)
f32 = np.float32
ONE_BELOW = f32(1.0) - f32(2.0 ** -24)             # the largest fp32 below 1
# a zig-zag in the free space between four circles of env_grid_circles_2d() (centres 0.25 apart, radius 0.05)
ZIGZAG = np.array([[-0.64, -0.66], [-0.63, -0.59], [-0.625, -0.66], [-0.62, -0.59], [-0.61, -0.66]], f32)


# ------------------------------------------------------------------------------------------------
# the input sets
# ------------------------------------------------------------------------------------------------
def _second_field(kind):
    from motion_planning_baselines_amd import geometry as G
    if kind == 'pm2d':
        return G.CollisionField(boxes=np.array([[0.3, -0.4, 0.12, 0.07], [-0.5, 0.45, 0.06, 0.15]], np.float32),
                                spheres=np.array([[0.1, 0.55, 0.09]], np.float32), margin=0.02)
    return G.CollisionField(spheres=np.array([[0.4, 0.3, 0.5, 0.12], [-0.3, -0.4, 0.6, 0.1], [0.5, -0.2, 0.2, 0.15]], np.float32),
                            boxes=np.array([[0.0, 0.0, -0.1, 1.0, 1.0, 0.05]], np.float32), margin=0.03)


def _arm_field():
    """16 spheres around the 12-joint test arm, none within 0.3 of its base axis: about two thirds of its configurations are free (in
    test_gpu_generic_dof.make_field() none is)."""
    import math
    from motion_planning_baselines_amd import geometry as G
    rng, out = np.random.RandomState(21), []
    while len(out) < 16:
        c, r = rng.uniform(-0.9, 0.9, 3) + [0.0, 0.0, 0.6], rng.uniform(0.1, 0.2)
        if math.hypot(c[0], c[1]) - r > 0.3:
            out.append((*c, r))
    return G.CollisionField(spheres=np.array(out, np.float32), margin=0.06)


# name -> (robot kind, first field, N, Lmax, n_iters, check_step, node spacing, seed): N 3 .. 37, Lmax 4 .. 70, n_iters <= 64; odd
# sizes, Lmax no multiple of anything, more rows than one 64-lane trip of the tail shift moves (Lmax * Dp > 64)
_SETS = {
    'pm2d_grid': ('pm2d', 'grid', 37, 70, 64, 0.01, 0.30, 11),
    'pm2d_dense': ('pm2d', 'dense', 21, 33, 48, 0.004, 0.35, 12),        # segments of more than 64 points: several trips per scan
    'panda': ('panda', 's3d', 13, 23, 40, np.pi / 80, 1.0, 13),
    'arm12': ('arm12', 'arm', 5, 12, 32, 0.05, 1.6, 14),
}
BASE = tuple(_SETS)
SETS = BASE + tuple(n + '_chain' for n in BASE)                               # ... and each with two chained fields


@functools.lru_cache(maxsize=None)
def scene(name):
    """name -> (product robot, [product CollisionField, ...], [s_f, ...])"""
    from motion_planning_baselines_amd import geometry as G
    from test_gpu_generic_dof import make_arm
    kind, first = _SETS[name.replace('_chain', '')][:2]
    robot = {'pm2d': lambda: G.RobotPointMass(2, radius=0.02), 'panda': G.RobotPanda, 'arm12': lambda: make_arm(12)}[kind]()
    field = {'grid': G.env_grid_circles_2d, 'dense': G.env_dense_2d, 's3d': G.env_spheres_3d, 'arm': _arm_field}[first]()
    if name.endswith('_chain'):
        return robot, [field, _second_field(kind)], [0.5, 2.0]
    return robot, [field], [1.0]


@functools.lru_cache(maxsize=None)
def problem(name):
    """The input set `name`: zig-zag polylines (random walks within the joint limits, lengths 0 .. Lmax with the edge lengths among
    them), recorded draws, and the oracle geometry in both precisions.  Treat as read-only."""
    kind, _, N, Lmax, n_iters, step, spacing, seed = _SETS[name.replace('_chain', '')]
    robot, fields, scales = scene(name)
    D = robot.q_dim
    rng = np.random.RandomState(seed)
    lo, hi = 0.95 * robot.q_min_np, 0.95 * robot.q_max_np
    lengths = rng.randint(3, Lmax + 1, N)
    lengths[:3] = (Lmax, 3, Lmax)                                            # full paths (OVERFLOW can happen) and the shortest one
    if N > 5:
        lengths[3:6] = (0, 1, 2)
    rr64 = make_ref_geometry(robot, fields[0], F64)[0]
    rr32 = make_ref_geometry(robot, fields[0], F32)[0]
    rf64 = [make_ref_geometry(robot, f, F64)[1] for f in fields]

    def free(cands):                                                         # the first collision-free row of 16 (like a tree's nodes)
        ok = np.nonzero(hinge_max(rr64, rf64, torch.from_numpy(cands)).numpy() < -1e-3)[0]
        return cands[ok[0] if len(ok) else 0]
    paths = np.zeros((N, Lmax, D), f32)
    for b in range(N):
        q = free(rng.uniform(lo, hi, (16, D)))
        for j in range(lengths[b]):
            paths[b, j] = q
            d = rng.normal(size=(16, D))
            q = free(np.clip(q + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.3, 1.0, (16, 1)) * spacing, lo, hi))
    draws = rng.uniform(0.0, 1.0, (N, n_iters, 2)).astype(f32)
    draws[draws >= 1.0] = ONE_BELOW
    draws[0, 0] = (0.0, 0.5)                                                  # t == 0 at node 0
    return types.SimpleNamespace(name=name, robot=robot, fields=fields, scales=scales, D=D, N=N, Lmax=Lmax, n_iters=n_iters,
                                 step=f32(step), paths=paths, lengths=lengths.astype(np.int32), draws=draws,
                                 rr64=rr64, rf64=rf64,
                                 rr32=rr32, rf32=[make_ref_geometry(robot, f, F32)[1] for f in fields])


def with_inputs(p, paths, lengths, draws, Lmax=None, step=None):
    """The input set p with other paths / lengths / draws (the geometry shared)."""
    q = types.SimpleNamespace(**vars(p))
    q.paths, q.lengths, q.draws = np.ascontiguousarray(paths, f32), np.asarray(lengths, np.int32), np.ascontiguousarray(draws, f32)
    q.N, q.Lmax, q.n_iters = q.paths.shape[0], q.paths.shape[1] if Lmax is None else Lmax, q.draws.shape[1]
    q.step = p.step if step is None else f32(step)
    return q


# ------------------------------------------------------------------------------------------------
# geometry of the dense points
# ------------------------------------------------------------------------------------------------
def hinge_max(rr, rfs, q):
    """q (n, D) in the oracle's precision -> (n,) max over fields and collision spheres of margin + r_l - sd(x_l)."""
    x = rr.fk_map_collision(q)
    return torch.stack([(f.margin + f.link_radius - f.signed_distance(x)).max(-1)[0] for f in rfs]).max(0)[0]


def cost32(p, q):
    """q (n, D) float32 numpy -> (n,) float32: the fp32 oracle's collision cost sum_f s_f sum_l relu(margin + r_l - sd)."""
    qt = torch.from_numpy(np.ascontiguousarray(q, f32))
    x = p.rr32.fk_map_collision(qt)
    c = torch.zeros(len(q), dtype=torch.float32)
    for s, f in zip(p.scales, p.rf32):
        c = c + torch.tensor(s, dtype=torch.float32) * f.compute_cost(qt, x)
    return c.numpy()


# ------------------------------------------------------------------------------------------------
# the definition's fp32 arithmetic
# ------------------------------------------------------------------------------------------------
def unit(u):
    u = f32(u)
    if np.isnan(u):
        return f32(0.0)
    return min(max(u, f32(0.0)), ONE_BELOW)


def close(x, y):
    """torch.allclose(x, y) with the defaults, in fp32, as rrt_close states it (atol + rtol |y| is one fmaf)"""
    return bool(np.all(np.abs(x - y) <= fma32(f32(1e-5), np.abs(y), f32(1e-8))))


def dist32(x, y):
    d2 = f32(0.0)
    for k in range(len(x)):
        df = f32(x[k] - y[k])
        d2 = f32(d2 + f32(df * df))
    return f32(np.sqrt(d2))


def length32(path):
    s = f32(0.0)
    for j in range(1, len(path)):
        s = f32(s + dist32(path[j - 1], path[j]))
    return s


def position(u, L):
    s = f32(u * f32(L - 1))
    a = min(int(s), L - 2)
    return a, f32(s - f32(a))


def point(path, a, t):
    """-> (the point, the node it is or -1)"""
    q0, q1 = path[a], path[a + 1]
    pt = q0 + t * (q1 - q0)                                   # float32 arrays: rounded after the sub, the mul and the add
    if t == 0 or close(pt, q0):
        return q0.copy(), a
    if close(pt, q1):
        return q1.copy(), a + 1
    return pt, -1


def fma32(a, b, c):
    """fmaf of csrc/mpb_rrt.h (rrt_close, rrt_linspace_point): fl32(a * b + c) of float32 arrays.  The product of two float32 is exact in float64 (the sum is rounded twice, to 53 bits and
    to 24: it differs from the fused result only where the first rounding lands on a tie of the second)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def dense_points(p1, p2, n_pts):
    """extend_path's linspace (from the near end of each half) as rrt_linspace_point of csrc/mpb_rrt.h states it: 1 - lstep * j and
    q1 + dl * al are one fmaf each, the rest plain operators under #pragma clang fp contract(off).  The points are data to
    both restatements; a decision that fp64 can decide does not depend on their last bit."""
    dl = p2 - p1
    lstep = f32(1.0) / f32(n_pts - 1)
    i = np.arange(n_pts)
    al = np.where(i < n_pts // 2, lstep * i.astype(f32), fma32(-lstep, (n_pts - 1 - i).astype(f32), f32(1.0))).astype(f32)
    return fma32(dl[None, :], al[:, None], p1[None, :])


def candidate(path, u1, u2, step):
    """One iteration's draws on the polyline `path` (L >= 3 rows) -> None (SKIP) or (lo, hi, rows to insert, dense points)."""
    L = len(path)
    (a1, t1), (a2, t2) = sorted((position(unit(u1), L), position(unit(u2), L)))
    if a1 == a2:
        return None
    p1, n1 = point(path, a1, t1)
    p2, n2 = point(path, a2, t2)
    lo = a1 if n1 < 0 else n1
    hi = a2 + 1 if n2 < 0 else n2
    cntf = f32(dist32(p1, p2) / step)
    if hi - lo < 2 or close(p1, p2) or not cntf < f32(MAX_PTS - 1):
        return None
    rows = [q for q, n in ((p1, n1), (p2, n2)) if n < 0]
    return lo, hi, rows, dense_points(p1, p2, int(cntf) + 2)


def _walk(p, judge):
    """The definition over the input set p; judge(b, it, points) -> index of the first point in collision, -1 when none."""
    out_paths = np.zeros_like(p.paths)
    out_len = np.zeros(p.N, np.int32)
    log = np.zeros((p.N, p.n_iters), np.int32)
    stats = np.zeros((p.N, 4), f32)
    for b in range(p.N):
        L = int(p.lengths[b])
        if L < 0 or L > p.Lmax:
            stats[b] = np.nan
            continue
        path = p.paths[b, :L].copy()
        stats[b, 2] = length32(path)
        for it in range(p.n_iters):
            if len(path) < 3:
                continue                                       # IDLE
            log[b, it] = SKIP
            c = candidate(path, p.draws[b, it, 0], p.draws[b, it, 1], p.step)
            if c is None:
                continue
            lo, hi, rows, pts = c
            stats[b, 0] += 1
            first = judge(b, it, pts)
            if first >= 0:
                log[b, it] = REJECT | (first << SHIFT)
            elif lo + 1 + len(rows) + len(path) - hi > p.Lmax:
                log[b, it] = OVERFLOW
            else:
                log[b, it] = ACCEPT
                stats[b, 1] += 1
                path = np.concatenate([path[:lo + 1]] + [r[None] for r in rows] + [path[hi:]]).astype(f32)
        stats[b, 3] = length32(path)
        out_len[b] = len(path)
        out_paths[b, :len(path)] = path
    return out_paths, out_len, log, stats


def restate32(p):
    """-> SimpleNamespace(paths, lengths, log, stats): the definition in fp32 with the fp32 oracle's collision cost."""
    def judge(b, it, pts):
        hit = np.nonzero(cost32(p, pts) > 0)[0]
        return int(hit[0]) if len(hit) else -1
    paths, lengths, log, stats = _walk(p, judge)
    return types.SimpleNamespace(paths=paths, lengths=lengths, log=log, stats=stats)


def replay64(p, log):
    """-> SimpleNamespace(paths, lengths, log, stats, cands): `log` held against the fp64 oracle as the module docstring says (raises
    AssertionError naming the first decision that differs); cands: per tested candidate a SimpleNamespace(b, it, code, first,
    decidable, margin, E32, bar, m64_max: the largest m_p over ALL the candidate's points)."""
    log = np.asarray(log)
    cands = []

    def judge(b, it, pts):
        code, first = int(log[b, it]) & ((1 << SHIFT) - 1), int(log[b, it]) >> SHIFT
        assert code in (REJECT, OVERFLOW, ACCEPT), f'{p.name}: path {b} iteration {it}: the log says {code}, the definition tests a candidate'
        m64 = hinge_max(p.rr64, p.rf64, torch.from_numpy(pts).double()).numpy()
        m32 = hinge_max(p.rr32, p.rf32, torch.from_numpy(pts)).numpy().astype(np.float64)
        hit = np.nonzero(m64 > 0)[0]
        f64 = int(hit[0]) if len(hit) else -1
        n = f64 + 1 if f64 >= 0 else len(pts)
        E32 = float(np.abs(m32[:n] - m64[:n]).max())
        margin = float(np.abs(m64[:n]).min())
        c = types.SimpleNamespace(b=b, it=it, code=code, first=first, decidable=margin > bar(E32), margin=margin, E32=E32, bar=bar(E32),
                                  m64_max=float(m64.max()), n_pts=len(pts))
        cands.append(c)
        got = first if code == REJECT else -1
        if c.decidable:
            assert got == f64, (f'{p.name}: path {b} iteration {it}: decidable (margin {margin:.3e} > bar {c.bar:.3e}), fp64 says first '
                                f'collision {f64}, the log {got} (code {code})')
        return got

    paths, lengths, relog, stats = _walk(p, judge)
    assert np.array_equal(relog, log), f'{p.name}: the replayed log differs at (path, iteration) {np.argwhere(relog != log)[:5].tolist()}'
    return types.SimpleNamespace(paths=paths, lengths=lengths, log=relog, stats=stats, cands=cands)


@functools.lru_cache(maxsize=None)
def reference(name):
    """restate32 of the input set and its replay in fp64, computed once and shared.  Treat as read-only."""
    p = problem(name)
    r32 = restate32(p)
    return types.SimpleNamespace(p=p, r32=r32, r64=replay64(p, r32.log))


def undecidable_share(cands):
    return sum(not c.decidable for c in cands) / max(len(cands), 1)
