"""The world predicate by the fp64 oracle alone (helper module, no tests; imported like sdf_grid_checks.py).

A world is up to three parts -- obstacles (a CollisionField), an SDF grid (a GridSDFField whose node values are DATA), the robot against
itself (a SelfCollisionField's pair list as DATA) -- and a configuration is in collision iff one part says so.  Each part is restated
as an object with the three members rrt_checks.hinge_argument, rrt_checks.check_rrt_result and path_shortcut_checks.hinge_max /
replay64 ask of an oracle field: `margin`, `link_radius` and `signed_distance(x)` over the collision-sphere centres x, such that
max(margin + link_radius - signed_distance(x)) is the part's HINGE ARGUMENT, positive = in collision:
    obstacles   oracle.geometry_ref.RefCollisionField itself                                  max_l (margin + r_l - sd(x_l))
    grid        sdf_grid_checks.sample, thresholds                                            max_l (margin + r_l - s(x_l))
    self        self_collision_checks' pair distances and thresholds                          max_p (T_p - |x_a - x_b|)
in fp64, and the same expressions on fp32 tensors as the fp32 restatement whose own error E32 gives the bar (collision_kinks.bar).
Nothing here runs the code under test.

The scenes (each part alone puts some of the inputs in collision; the tests assert it):
    panda     RobotPanda; env_spheres_3d(); a 49 x 49 x 45 grid (sdf_grid_checks.DIMS['panda']) of a second, disjoint field -- four
              spheres that are in the grid alone; SelfCollisionField(robot) at the default gap
    pm2d      RobotPointMass(2); a small field of boxes and a circle; a planar 112 x 112 grid of env_grid_circles_2d(); no self field
    chain64   self_collision_checks.make_chain64(): 12 joints, run-time D, 64 collision spheres (the limit of the self block's LDS; the
              12-joint arm of test_gpu_generic_dof has 25); path_shortcut_checks' arm field; a 51^3 grid of three spheres; self field
"""
import functools
import types

import numpy as np
import torch

import path_shortcut_checks as K
import sdf_grid_checks as S
import self_collision_checks as C
from collision_kinks import bar
from oracle.geometry_ref import _safe_norm, make_ref_geometry

F32, F64 = S.F32, S.F64
f32 = np.float32
PARTS = ('obs', 'sdf', 'self')
CAP = 0.02                    # the project's cap of the share no fp64 oracle can decide (test_path_shortcut_cpu.py)
N_SMALL, N_LARGE = 21, 333     # ragged against 64 and 256
SCENES = ('panda', 'pm2d', 'chain64')


class GridPart:
    """An SDF grid as an oracle field over the sphere centres: hinge argument max_l (thr_l - s(x_l))."""

    def __init__(self, g, thr):
        self.g, self.link_radius, self.margin = g, thr, torch.zeros((), dtype=thr.dtype)

    def signed_distance(self, x):
        return S.sample(self.g, x)


class SelfPart:
    """A pair list as an oracle field over the sphere centres: hinge argument max_p (T_p - |x_a - x_b|)."""

    def __init__(self, a, b, T):
        self.a, self.b, self.link_radius, self.margin = a, b, T, torch.zeros((), dtype=T.dtype)

    def signed_distance(self, x):
        return _safe_norm(x[..., self.a, :] - x[..., self.b, :])


def _grid_only_field(name):
    from motion_planning_baselines_amd import geometry as G
    if name == 'panda':        # where env_spheres_3d() has nothing: the nearest of its spheres is 0.2 m from each surface
        return G.CollisionField(spheres=np.array([[0.45, 0.45, 0.75, 0.12], [-0.5, 0.35, 0.25, 0.13], [0.1, -0.6, 0.9, 0.11],
                                                  [-0.35, -0.45, 0.55, 0.1]], f32), margin=0.03)
    if name == 'pm2d':
        return G.env_grid_circles_2d()
    return G.CollisionField(spheres=np.array([[0.7, 0.2, 1.0, 0.2], [-0.5, -0.6, 0.5, 0.18], [0.0, 0.8, 1.4, 0.2]], f32), margin=0.04)


@functools.lru_cache(maxsize=None)
def scene(name):
    """name -> namespace(robot, field, grid (GridSDFField holding the fp64 oracle's node values rounded to fp32), self_field or None,
    rr64 / rr32 (RefRobot), parts64 / parts32 ([obstacles, grid, self or None] as oracle fields)).  Treat as read-only."""
    from motion_planning_baselines_amd import geometry as G
    if name == 'panda':
        robot, field, box, cell = G.RobotPanda(dt=0.04), G.env_spheres_3d(), ((-1.2, -1.2, -0.7), (1.2, 1.2, 1.5)), 0.05
        self_field = G.SelfCollisionField(robot)
    elif name == 'pm2d':
        robot, field, box, cell = G.RobotPointMass(2, radius=0.02), K._second_field('pm2d'), ((-1.1, -1.1), (1.1, 1.1)), 0.02
        self_field = None
    else:
        robot, field, box, cell = C.make_chain64(), K._arm_field(), ((-2.5, -2.5, -2.5), (2.5, 2.5, 2.5)), 0.1
        self_field = G.SelfCollisionField(robot, margin=0.01, min_frame_gap=5)
    src = _grid_only_field(name)
    layout = G.GridSDFField.from_field(src, box[0], box[1], cell)
    if name != 'chain64':
        assert layout.dims == S.DIMS['panda' if name == 'panda' else 'point2d'], layout.dims
    values = S.oracle_nodes(src, layout)
    grid = G.GridSDFField(values if not layout.planar else values[0], layout.lo if not layout.planar else layout.lo[:2], layout.cell,
                          margin=layout.margin)
    out = types.SimpleNamespace(name=name, robot=robot, field=field, grid_source=src, grid=grid, self_field=self_field, D=robot.q_dim)
    for tag, ta in (('64', F64), ('32', F32)):
        rr, rf = make_ref_geometry(robot, field, ta)
        parts = [rf, GridPart(S.grid_data(grid.values, grid.lo, grid.cell, grid.inv_cell, ta), S.thresholds(robot, f32(grid.margin), ta)),
                 None if self_field is None else SelfPart(*C.pair_data(self_field, ta))]
        setattr(out, 'rr' + tag, rr)
        setattr(out, 'parts' + tag, parts)
    return out


def fields(sc, tag='64'):
    """The parts that exist, as the list path_shortcut_checks.hinge_max and rrt_checks take."""
    return [p for p in getattr(sc, 'parts' + tag) if p is not None]


def hinges(sc, q, tag='64'):
    """q (n, D) numpy -> (n, 3) float64: every part's hinge argument in the oracle's precision `tag`, -inf for an absent part."""
    rr = getattr(sc, 'rr' + tag)
    qt = torch.from_numpy(np.ascontiguousarray(q, f32)).to(torch.float64 if tag == '64' else torch.float32)
    out = np.full((len(q), 3), -np.inf)
    for lo in range(0, len(q), 4096):
        x = rr.fk_map_collision(qt[lo:lo + 4096])
        for k, p in enumerate(getattr(sc, 'parts' + tag)):
            if p is not None:
                out[lo:lo + 4096, k] = (p.margin + p.link_radius - p.signed_distance(x)).max(-1)[0].double().numpy()
    return out


def decide(sc, q):
    """q (n, D) -> namespace(m64 (n, 3), flag64 (n,) the OR of the three fp64 predicates, E32 (3,) the fp32 restatement's own worst
    error per part on THESE inputs, bars (3,), excused (n,): some part's hinge argument lies within its bar of zero)."""
    m64, m32 = hinges(sc, q, '64'), hinges(sc, q, '32')
    have = np.array([p is not None for p in sc.parts64])
    E32 = np.abs(m32[:, have] - m64[:, have]).max(0)
    bars = np.array([bar(float(e)) for e in E32])
    excused = (np.abs(m64[:, have]) < bars).any(1)
    return types.SimpleNamespace(m64=m64, flag64=(m64 > 0).any(1), E32=E32, bars=bars, excused=excused)


def uniform_q(robot, n, seed):
    rng = np.random.RandomState(seed)
    return rng.uniform(robot.q_min_np.astype(np.float64), robot.q_max_np.astype(np.float64), (n, robot.q_dim)).astype(f32)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """{label: (n, D) fp32}: N_SMALL and N_LARGE uniform configurations, and `modules`: the configurations of the existing check modules
    for the scene's robot (sdf_grid_checks / self_collision_checks: their RandomState(11) rows; path_shortcut_checks: the nodes of its
    input paths; for the Panda also self_collision_checks.PANDA_HOME)."""
    sc = scene(name)
    out = {'u%d' % N_SMALL: uniform_q(sc.robot, N_SMALL, 101), 'u%d' % N_LARGE: uniform_q(sc.robot, N_LARGE, 102)}
    mod = [S.uniform_q(sc.robot, 64).numpy()]
    if name == 'panda':
        p = K.problem('panda')
        mod += [C.uniform_q(sc.robot, 64, seed=C.SEED + 1).numpy(), np.asarray([C.PANDA_HOME], f32)]
        mod += [p.paths[b, :p.lengths[b]] for b in range(p.N)]
    elif name == 'pm2d':
        p = K.problem('pm2d_grid')
        mod += [p.paths[b, :p.lengths[b]] for b in range(0, p.N, 4)]
    else:
        mod += [C.uniform_q(sc.robot, 64, seed=C.SEED + 1).numpy()]
    out['modules'] = np.ascontiguousarray(np.concatenate(mod), f32)
    return out


# ------------------------------------------------------------------------------------------------
# configurations and straight lines that ONE part alone refuses
# ------------------------------------------------------------------------------------------------
MARGIN = 2e-3      # how clearly (hinge argument, metres) a searched configuration is free of / inside a part: far above any bar


def free_q(sc, n, seed):
    """n configurations every part calls free by MARGIN (fp64), uniform in 95 % of the joint limits."""
    rng, out = np.random.RandomState(seed), []
    lo, hi = 0.95 * sc.robot.q_min_np.astype(np.float64), 0.95 * sc.robot.q_max_np.astype(np.float64)
    while sum(len(o) for o in out) < n:
        q = rng.uniform(lo, hi, (256, sc.D)).astype(f32)
        out.append(q[(hinges(sc, q) < -MARGIN).all(1)])
    return np.concatenate(out)[:n]


@functools.lru_cache(maxsize=None)
def only_line(name, part, seed=5):
    """(qa, qb, qm) fp32: the endpoints free of every part by MARGIN, and on the straight line between them (129 points, fp64) the
    part `part` alone is ever positive -- by more than MARGIN at qm --, every other part staying below -MARGIN."""
    sc, k = scene(name), PARTS.index(part)
    rng = np.random.RandomState(seed)
    lo, hi = sc.robot.q_min_np.astype(np.float64), sc.robot.q_max_np.astype(np.float64)
    al = np.linspace(0.0, 1.0, 129)[:, None]
    for _ in range(400):
        q = rng.uniform(lo, hi, (512, sc.D)).astype(f32)
        m = hinges(sc, q)
        others = np.delete(m, k, axis=1)
        for qm in q[(m[:, k] > 5 * MARGIN) & (others < -MARGIN).all(1)]:
            for scale in (0.15, 0.3, 0.6, 1.0):
                d = rng.normal(size=sc.D)
                d *= scale / np.linalg.norm(d)
                qa, qb = np.clip(qm - d, lo, hi).astype(f32), np.clip(qm + d, lo, hi).astype(f32)
                line = hinges(sc, (qa + (qb.astype(np.float64) - qa) * al).astype(f32))
                if (line[[0, -1]] < -MARGIN).all() and (np.delete(line, k, axis=1) < -MARGIN).all() and line[:, k].max() > MARGIN:
                    return qa, qb, qm.astype(f32)
    raise AssertionError(f'{name}: no straight line that the {part} part alone refuses')


# ------------------------------------------------------------------------------------------------
# input sets of the shortcut pass and of RRT-Connect
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shortcut_problem(name='panda', N=13, Lmax=23, n_iters=24, seed=17):
    """An input set as path_shortcut_checks.problem gives it (so _walk / replay64 serve it), with the world's parts as its fields:
    random-walk polylines whose nodes every part calls free, recorded draws; path 0 is a zig-zag whose ends see each other only
    through a grid-only obstacle, path 1 one whose ends see each other only through a folded (self-colliding) configuration, and
    iteration 0 of both draws (0, just below 1): the candidate is end to end."""
    sc = scene(name)
    rng = np.random.RandomState(seed)
    D = sc.D
    lo, hi = 0.95 * sc.robot.q_min_np, 0.95 * sc.robot.q_max_np
    step = f32(np.pi / 80 if name != 'pm2d' else 0.01)
    spacing = 1.0 if name != 'pm2d' else 0.3
    lengths = rng.randint(3, Lmax + 1, N)
    lengths[:5] = (3, 3, Lmax, 0, 2)

    def free(cands):
        ok = np.nonzero((hinges(sc, cands.astype(f32)) < -1e-3).all(1))[0]
        return cands[ok[0] if len(ok) else 0].astype(f32)
    paths = np.zeros((N, Lmax, D), f32)
    for b in range(N):
        q = free(rng.uniform(lo, hi, (32, D)))
        for j in range(lengths[b]):
            paths[b, j] = q
            d = rng.normal(size=(32, D))
            q = free(np.clip(q + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.3, 1.0, (32, 1)) * spacing, lo, hi))
    detour = free_q(sc, 2, seed + 1)
    parts = ('sdf', 'self') if sc.self_field is not None else ('sdf',)
    for b, part in enumerate(parts):
        qa, qb, _ = only_line(name, part)
        paths[b, :3] = (qa, detour[b], qb)
    draws = rng.uniform(0.0, 1.0, (N, n_iters, 2)).astype(f32)
    draws[draws >= 1.0] = K.ONE_BELOW
    draws[:len(parts), 0] = (0.0, K.ONE_BELOW)
    return types.SimpleNamespace(name='world_' + name, robot=sc.robot, fields=None, scales=None, D=D, N=N, Lmax=Lmax, n_iters=n_iters, step=step,
                                 paths=paths, lengths=lengths.astype(np.int32), draws=draws, rr64=sc.rr64, rf64=fields(sc, '64'),
                                 rr32=sc.rr32, rf32=fields(sc, '32'), only=parts)


@functools.lru_cache(maxsize=None)
def rrt_problem(name='panda', B=5, n_pre=192, total=601, seed=23):
    """B start / goal pairs and a pool every part calls free, recorded pool indices (B, total)."""
    sc = scene(name)
    q = free_q(sc, 2 * B + n_pre, seed)
    rng = np.random.RandomState(seed)
    step, radius = (np.pi / 80, np.pi / 4) if name != 'pm2d' else (0.01, 0.3)
    return types.SimpleNamespace(starts=q[:B], goals=q[B:2 * B], pool=q[2 * B:], idx=rng.randint(0, n_pre, (B, total)).astype(np.int32),
                                 step=step, radius=radius, total=total, B=B)


@functools.lru_cache(maxsize=None)
def trajectories(name='panda', N=7, H=9, seed=29):
    """(N, H, D) fp32: rows 0 .. N - 3 are random walks among free and colliding configurations; row N - 2 is a straight line only the
    grid refuses, row N - 1 one only the self part refuses (a scene without a self field: a line between two free configurations)."""
    sc = scene(name)
    rng = np.random.RandomState(seed)
    lo, hi = sc.robot.q_min_np.astype(np.float64), sc.robot.q_max_np.astype(np.float64)
    t = np.zeros((N, H, sc.D), f32)
    for n in range(N - 2):
        q = rng.uniform(lo, hi, sc.D)
        for h in range(H):
            t[n, h] = q
            q = np.clip(q + rng.normal(size=sc.D) * 0.25 * (hi - lo) / 6.0, lo, hi)
    al = np.linspace(0.0, 1.0, H)[:, None]
    for n, part in ((N - 2, 'sdf'), (N - 1, 'self')):
        if part == 'self' and sc.self_field is None:
            qa, qb = free_q(sc, 2, seed)
            qb = (qa + 0.02 * (qb - qa)).astype(f32)
        else:
            qa, qb, _ = only_line(name, part)
        t[n] = (qa + (qb.astype(np.float64) - qa) * al).astype(f32)
    return t


def why_rejected(sc, p, b, log):
    """The parts (fp64) that refuse the first point in collision of path b's iteration-0 candidate as `log` names it, joined by '+'."""
    lo, hi, rows, pts = K.candidate(p.paths[b, :p.lengths[b]], p.draws[b, 0, 0], p.draws[b, 0, 1], p.step)
    m = hinges(sc, pts[int(log[b, 0]) >> K.SHIFT][None])[0]
    return '+'.join(part for k, part in enumerate(PARTS) if m[k] > 0)
