"""Clearance and path certification (ops.clearance, ops.path_certify, csrc/mpb_certify.hip; definition: include/mpb.h)
restated on the CPU in fp64 (helper module, not collected): the scenes of the tests, the clearance eta_l on the oracle geometry
(oracle/geometry_ref.py), a chain walk that also gives the joint origins (for the reach bound), the bisection itself level by level, and
the dense resampling the soundness tests hold a certificate to.

    python tests/certify_checks.py        # measures E = max |eta fp32 restatement - eta fp64 oracle| over 10^5 uniform configurations
                                          # per scene: what certify_layout.CERT_E_MEASURED records
"""
import functools
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from motion_planning_baselines_amd import certify_layout as CL          # noqa: E402
from motion_planning_baselines_amd import geometry as G                # noqa: E402

FREE, COLLISION, UNDECIDED_DEPTH, UNDECIDED_QUEUE, BAD_INPUT, BUFFER_CHANGED = range(len(CL.STATUS))

# (a, d, alpha) rows in the modified-DH convention of geometry._mdh: a Panda-like arm continued to twelve joints
_MDH12 = [(0.0, 0.333, 0.0), (0.0, 0.0, -math.pi / 2), (0.0, 0.316, math.pi / 2), (0.0825, 0.0, math.pi / 2),
          (-0.0825, 0.384, -math.pi / 2), (0.0, 0.0, math.pi / 2), (0.088, 0.0, math.pi / 2), (0.0, 0.12, -math.pi / 2),
          (0.05, 0.0, math.pi / 2), (0.0, 0.15, -math.pi / 2), (0.04, 0.0, math.pi / 2), (0.0, 0.10, -math.pi / 2)]


def chain12():
    """A 12-joint table-driven chain: two collision spheres per link frame, one on the tool frame."""
    D = 12
    tfs = np.stack([G._mdh(alpha, a, d) for (a, d, alpha) in _MDH12])
    frames, offs, rad = [], [], []
    for f in range(1, D + 1):
        frames += [f, f]
        offs += [(0.0, 0.0, -0.05), (0.02, -0.03, 0.04)]
        rad += [0.07, 0.05]
    frames.append(D + 1)
    offs.append((0.0, 0.0, 0.05))
    rad.append(0.05)
    return G.RobotSerialChain(tfs, frames, offs, rad, q_min=[-2.5] * D, q_max=[2.5] * D)


def _boxes_3d(seed, n, margin):
    rng = np.random.RandomState(seed)
    box = []
    while len(box) < n:
        c, h = rng.uniform(-0.8, 0.8, 3) + [0.0, 0.0, 0.4], rng.uniform(0.04, 0.12, 3)
        if math.hypot(c[0], c[1]) - math.hypot(h[0], h[1]) > 0.25:
            box.append((*c, *h))
    return G.CollisionField(boxes=np.array(box, np.float32), margin=margin)


class Scene:
    """A robot, its obstacle field(s), the box configurations are drawn from, and the fp64 / fp32 oracle geometry."""

    def __init__(self, name, robot, fields, lo, hi):
        self.name, self.robot, self.fields = name, robot, list(fields)
        self.rs = robot.spec()
        self.D, self.L = int(self.rs['n_dof']), len(self.rs['link_radius'])
        self.lo, self.hi = float(lo), float(hi)
        self.rho = CL.reach_table(self.rs)

    @property
    def field(self):
        return self.fields[0] if len(self.fields) == 1 else self.fields

    @functools.lru_cache(maxsize=None)
    def ref(self, dtype):
        from oracle.geometry_ref import make_ref_geometry
        pairs = [make_ref_geometry(self.robot, f, dict(device='cpu', dtype=dtype)) for f in self.fields]
        return pairs[0][0], [p[1] for p in pairs]

    def eta_links(self, q, dtype=torch.float64):
        """eta_l (N, L) of configurations q (N, D) on the oracle geometry in `dtype`, returned as fp64 numpy."""
        rr, rfs = self.ref(dtype)
        x = rr.fk_map_collision(torch.as_tensor(np.asarray(q), dtype=dtype).reshape(-1, self.D))
        sd = torch.stack([rf.signed_distance(x) - rf.margin for rf in rfs]).min(0)[0]
        return (sd - rfs[0].link_radius).double().numpy()

    def eta(self, q, dtype=torch.float64):
        return self.eta_links(q, dtype).min(-1)

    def uniform(self, n, seed):
        return np.random.RandomState(seed).uniform(self.lo, self.hi, (n, self.D)).astype(np.float32)

    def motion_bound(self, a, b):
        return CL.motion_bound(self.rs, self.rho, a, b)


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == 'pm2d':            # 2-D point, spheres and boxes
        return Scene(name, G.RobotPointMass(2, radius=0.01), [G.env_dense_2d(seed=3)], -1.0, 1.0)
    if name == 'panda':           # Panda, 16 spheres: the scene of the rrt_panda_spheres golden
        return Scene(name, G.RobotPanda(), [G.env_spheres_3d(seed=0, n_spheres=16, margin=0.05)], -2.8, 2.8)
    if name == 'chain12':         # 12 joints, boxes, two chained fields of different margins
        return Scene(name, chain12(), [_boxes_3d(5, 10, 0.03), _boxes_3d(6, 6, 0.06)], -2.5, 2.5)
    raise KeyError(name)


SCENES = ('pm2d', 'panda', 'chain12')


def fk_with_origins(rs, q):
    """fp64 chain walk by the definition frame_{j+1} = frame_j P_j Rz(q_j): (sphere centres (N, L, 3), joint origins (N, D, 3)); the
    origin of joint i is where frame_i P_i puts its translation -- a point of the axis joint i turns about."""
    q = np.asarray(q, np.float64).reshape(-1, int(rs['n_dof']))
    tf = np.asarray(rs['joint_tf'], np.float64)
    N, D = q.shape
    R = np.broadcast_to(np.eye(3), (N, 3, 3)).copy()
    t = np.zeros((N, 3))
    frames, origins = [], []
    for j in range(tf.shape[0]):
        t = t + R @ tf[j, :, 3]
        R = R @ tf[j, :, :3]
        if j < D:
            origins.append(t.copy())
            c, s = np.cos(q[:, j]), np.sin(q[:, j])
            Rz = np.zeros((N, 3, 3))
            Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = c, -s, s, c, 1.0
            R = R @ Rz
        frames.append((R, t))
    off = np.asarray(rs['link_offset'], np.float64)
    x = np.stack([frames[int(f) - 1][0] @ off[l] + frames[int(f) - 1][1] for l, f in enumerate(rs['link_frame'])], 1)
    return x, np.stack(origins, 1)


def centres(sc, q):
    """Collision-sphere centres (N, L, 3) fp64 of any scene's robot (a point robot: the configuration, z = 0 in 2-D)."""
    q = np.asarray(q, np.float64).reshape(-1, sc.D)
    if int(sc.rs['kind']) == 0:
        return np.concatenate([q, np.zeros((len(q), 3 - sc.D))], 1)[:, None, :]
    return fk_with_origins(sc.rs, q)[0]


def certify_ref(sc, path, S, c_req=0.0, max_depth=CL.CERT_DEFAULT_MAX_DEPTH, max_intervals=CL.CERT_DEFAULT_MAX_INTERVALS):
    """The recursion of include/mpb.h on one path (Lp, D) in fp64: dict(status, witness = (segment, t, link, eta) or None, n_evals,
    depth_max, margin_cert)."""
    path = np.asarray(path, np.float64)
    out = dict(status=FREE, witness=None, n_evals=0, depth_max=-1, margin_cert=-np.inf)
    if len(path) < 1 or not np.isfinite(path).all():
        out['status'] = BAD_INPUT
        return out
    e = sc.eta_links(path)
    out['n_evals'] += len(path)
    hit = np.nonzero(e.min(1) - c_req < -S)[0]
    if len(hit):
        r = int(hit[0])
        out.update(status=COLLISION, witness=(r, 0.0, int(e[r].argmin()), float(e[r].min())))
        return out
    cert = float(e[0].min() - c_req) if len(path) == 1 else np.inf
    if len(path) - 1 > max_intervals:
        out['status'] = UNDECIDED_QUEUE
        return out
    seg, j = np.arange(len(path) - 1), np.zeros(len(path) - 1, np.int64)
    undecided = False
    for d in range(max_depth + 1):
        if not len(seg):
            break
        out['depth_max'] = d
        w = 2.0 ** -(d + 1)
        t = (2 * j + 1) * w
        a, b = path[seg], path[seg + 1]
        m = a + (b - a) * t[:, None]
        e = sc.eta_links(m)
        lam = sc.motion_bound(a, b)
        out['n_evals'] += len(seg)
        coll = e.min(1) - c_req < -S
        if coll.any():
            k = int(np.nonzero(coll)[0][0])
            out.update(status=COLLISION, witness=(int(seg[k]), float(t[k]), int(e[k].argmin()), float(e[k].min())))
            return out
        bound = (e - w * lam).min(1) - c_req
        free = bound > S
        if free.any():
            cert = min(cert, float(bound[free].min()))
        if d == max_depth:
            undecided = bool((~free).any())
            break
        if 2 * int((~free).sum()) > max_intervals:
            out['status'] = UNDECIDED_QUEUE
            return out
        seg, j = np.repeat(seg[~free], 2), (2 * np.repeat(j[~free], 2) + np.tile([0, 1], int((~free).sum())))
    out['status'] = UNDECIDED_DEPTH if undecided else FREE
    if out['status'] == FREE:
        out['margin_cert'] = cert
    return out


def dense_clearance(sc, path, n_per_segment):
    """min eta over the path's nodes and n_per_segment evenly spaced points inside every segment, fp64."""
    path = np.asarray(path, np.float64)
    if len(path) == 1:
        return float(sc.eta(path).min())
    t = (np.arange(n_per_segment + 1) / (n_per_segment + 1))[None, :, None]
    pts = path[:-1, None, :] + (path[1:, None, :] - path[:-1, None, :]) * t
    return float(min(sc.eta(pts.reshape(-1, sc.D)).min(), sc.eta(path[-1:]).min()))


def witness_q(path, seg, t):
    path = np.asarray(path, np.float64)
    return path[seg] if t == 0 else path[seg] + (path[seg + 1] - path[seg]) * t


def short_paths(sc, n, rows, short, seed, bump=0.03):
    """n polylines of `rows` rows (n, rows, D) fp32: a short straight line between two uniform draws plus a sine bump."""
    rng = np.random.RandomState(seed)
    span = sc.hi - sc.lo
    a = rng.uniform(sc.lo, sc.hi, (n, 1, sc.D))
    b = a + short * span * rng.uniform(-1, 1, (n, 1, sc.D))
    t = np.linspace(0, 1, rows)[None, :, None]
    return (a + (b - a) * t + bump * span * np.sin(np.pi * t) * rng.uniform(-1, 1, (n, 1, sc.D))).astype(np.float32)


def tunnel_scene():
    """The tunnelling scene: a 2-D point robot of radius 0.005, one circle of radius 0.01 on the straight segment (-0.5, 0) -> (0.5, 0)
    between two of its num_interpolation = 5 sample points (k / 6: the obstacle sits at parameter 0.25 = 1.5 / 6; the nearest samples are
    1/12 away, the margin + radii reach 0.02)."""
    field = G.CollisionField(spheres=np.array([[-0.25, 0.0, 0.01]], np.float32), margin=0.005)
    sc = Scene('tunnel', G.RobotPointMass(2, radius=0.005), [field], -1.0, 1.0)
    return sc, np.array([[-0.5, 0.0], [0.5, 0.0]], np.float32)


def rrt_paths():
    """The RRT-Connect paths stored in the rrt_panda_spheres golden: [(Lp, 7) fp32]."""
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'rrt_panda_spheres.npz'), allow_pickle=False)
    return [g[f'p{k}_path'].astype(np.float32) for k in range(int(g['n_problems']))]


def measure_E(n=100000):
    worst = 0.0
    for name in SCENES:
        sc = scene(name)
        q = sc.uniform(n, seed=20261021)
        e = float(np.abs(sc.eta(q, torch.float32) - sc.eta(q, torch.float64)).max())
        print(f'{name}: E = {e:.3e} over {n} uniform configurations')
        worst = max(worst, e)
    print(f'E = {worst:.3e}; S = 32 E = {32 * worst:.3e}')
    return worst


if __name__ == '__main__':
    measure_E()
