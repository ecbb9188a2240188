"""Geometry back-end specification: robots, collision primitives, packed device layout.

The reference delegates forward kinematics and signed-distance fields to the
un-vendored ``torch_robotics`` package (reference call sites:
mp_baselines/planners/costs/cost_functions.py:50-52 ``robot.get_position /
get_velocity / fk_map_collision`` and costs/factors/field_factor.py:39
``field.compute_cost``).  That package is not part of the reference tree, so the
geometry here is BUILD-DEFINED (parity with torch_robotics is unpinned, see
DESIGN.md).  This module holds only *data*: the analytic definitions are
evaluated on the GPU by csrc/mpb_collision.h and, for checking, on the CPU by
oracle/geometry_ref.py from the very same arrays.

Definitions (all fp32):
  * point robot, D in {2,3}: one collision sphere at (q0, q1, q2|0), radius r.
  * serial revolute chain (Panda): frame_0 = I; frame_{j+1} = frame_j * P_j * Rz(q_j)
    for j < D; an optional fixed tool frame_{D+1} = frame_D * P_D.  P_j are constant
    3x4 transforms (modified-DH: Rx(alpha_{j-1}) Tx(a_{j-1}) Tz(d_j)).
    Collision sphere l sits at frame_{link_frame[l]} * offset_l with radius r_l.
  * obstacle sphere: sdf(x) = |x - c| - r.
  * axis-aligned box: q = |x - c| - h; sdf = |max(q,0)| + min(max(qx,qy,qz), 0).
  * per-waypoint collision cost: sum_l relu(margin + r_l - min_o sdf_o(x_l)).
  * per-waypoint SELF-collision cost (serial chains, SelfCollisionField): sum over pairs (a, b) of
    relu(margin + r_a + r_b - |x_a - x_b|).
  * per-waypoint GRID cost (GridSDFField): sum_l relu(margin + r_l - s(x_l)), s the tri- / bilinear interpolant of a lattice of
    signed distances (its class says how).
"""
import math
import os

import numpy as np
import torch

# ----------------------------------------------------------------------------------------------
# The packed-geometry contract.  This block is its ONLY definition: model_gen.py emits include/mpb_geom_layout.h from it (C_LAYOUT
# below names what goes there, as MPB_<name>), which include/mpb.h and csrc/mpb_geom.h include; tests/test_host_logic.py pins the
# public numbers as literals so that an edit here cannot renumber the ABI unnoticed.
# ----------------------------------------------------------------------------------------------
GEOM_MAGIC = 0x4D504247  # 'MPBG'
GEOM_VERSION = 6         # the grid section is a COMPACT grid (or absent): cells on a lattice through the world origin
# geometry version 7 (round 6): fields whose obstacle set does not fit the compact grid (more than GRID_MAX_SPH spheres) carry a LIST
# grid -- a cell word holds (start, sphere count, box count) into a byte array of candidate indices that follows the cell words: any number
# of candidates per cell, boxes culled like spheres (csrc/mpb_geom.h, spheres_hinge_list).  Limits = what the persistent kernel keeps in LDS
GEOM_VERSION_LIST = 7
KIND_POINT = 0
KIND_CHAIN = 1
MAX_DOF = 12
MAX_FIELDS = 4           # collision fields chained in one buffer
GEOM_HEADER_WORDS = 32
GRID_MAX_CELLS = 4096    # cell words of a grid: 16 KB of LDS
GRID_PAD = 1024          # the grid section is padded to a multiple of this many words (one round of a 256-thread block's uint4 loads)
GRID_MAX_SPH = 63        # obstacle spheres a compact grid serves: the kernels' table in LDS holds 63 + one far-away dummy
LIST_MAX_SPH = 255       # 8-bit candidate indices; the kernels' sphere table holds 255 + the far dummy
LIST_MAX_BOX = 127       # ... and the box table 127 + the far dummy
LIST_MAX_CAND = 16384    # bytes of candidate indices (LDS)
LIST_CELL_MAX_SPH = 126  # per cell (7-bit field; 127 marks an overflowing cell: exhaustive loop)
LIST_CELL_MAX_BOX = 62   # per cell (6-bit field; 63 marks overflow)

# The header: GEOM_HEADER_WORDS 32-bit words, in this order -- (name, type, words).  Ints are stored bit-exact in the fp32 buffer.
HEADER_WORDS = (
    ('magic', 'i4', 1),        # GEOM_MAGIC
    ('version', 'i4', 1),      # GEOM_VERSION or GEOM_VERSION_LIST: the format of this field's grid section
    ('kind', 'i4', 1),         # KIND_POINT / KIND_CHAIN
    ('n_dof', 'i4', 1),
    ('n_tf', 'i4', 1),         # joint transforms: 0 (point robot) or n_dof + 1
    ('n_links', 'i4', 1),      # collision spheres of the robot in the link table
    ('n_sph', 'i4', 1),        # obstacle spheres
    ('n_box', 'i4', 1),        # obstacle boxes
    ('margin', 'f4', 1),       # hinge margin
    ('off_tf', 'i4', 1),       # word offsets of the sections from this header ...
    ('off_links', 'i4', 1),
    ('off_sph', 'i4', 1),
    ('off_box', 'i4', 1),
    ('total', 'i4', 1),        # words of this field, header included
    ('off_cull', 'i4', 1),
    ('off_fs', 'i4', 1),       # frame_start table
    ('off_grid', 'i4', 1),
    ('grid_dims', 'i4', 3),    # nx, ny, nz
    ('grid_lo', 'f4', 3),      # origin: (K - 1/2) h per axis with integer K
    ('grid_inv', 'f4', 3),     # 1 / cell size per axis
    ('n_cells', 'i4', 1),      # nx * ny * nz (0: no grid)
    ('next', 'i4', 1),         # words from this header to the next chained field (0: last)
    ('fscale', 'f4', 1),       # s_f: this field's share in sum_f s_f * cost_f
    ('model', 'i4', 1),        # compile-time robot model the tables equal bit for bit (model_gen.py; 0: none)
    ('keep_mask', 'u4', 1),    # bit l: the MODEL's collision sphere l is in the link table (static pruning)
    ('k_lin', 'i4', 1),        # linear index Kx + nx (Ky + ny Kz) of the lattice point the grid starts at
)
HEADER_DTYPE = np.dtype([(name, typ, (n,)) if n > 1 else (name, typ) for name, typ, n in HEADER_WORDS])
assert HEADER_DTYPE.itemsize == 4 * GEOM_HEADER_WORDS

# COMPACT grid cell word: GRID_SLOTS obstacle-sphere indices of GRID_SLOT_BITS each, filled from slot 0; an unused slot holds n_sph
# (the far dummy the kernels append to their table)
GRID_SLOTS = 4
GRID_SLOT_BITS = 8
GRID_SLOT_MASK = (1 << GRID_SLOT_BITS) - 1
GRID_OVERFLOW = (1 << 32) - 2   # more than GRID_SLOTS candidates in the cell: the kernels test every obstacle
# LIST grid cell word: start into the candidate bytes | sphere count | box count (a cell's boxes follow its spheres); bits 28-30 zero
LIST_START_BITS = 15
LIST_START_MASK = (1 << LIST_START_BITS) - 1
LIST_NSPH_SHIFT = LIST_START_BITS
LIST_NSPH_BITS = 7
LIST_NSPH_MASK = (1 << LIST_NSPH_BITS) - 1
LIST_NBOX_SHIFT = LIST_NSPH_SHIFT + LIST_NSPH_BITS
LIST_NBOX_BITS = 6
LIST_NBOX_MASK = (1 << LIST_NBOX_BITS) - 1
LIST_OVERFLOW = 1 << 31         # the cell overflows a count field: the kernels test every obstacle
LIST_RESERVED = LIST_OVERFLOW - (1 << (LIST_NBOX_SHIFT + LIST_NBOX_BITS))   # bits 28-30: must be zero

# geom_flags (mpb_geom_flags: what a launcher picks its kernel instantiation by; include/mpb.h says what each promises).  Bit 11 is unused.
GEOM_FLAG_MODEL_MASK = (1 << 8) - 1   # bits 0-7: compile-time robot model of EVERY chained field (0: table-driven kernels)
GEOM_FLAG_ALL_GRIDS = 1 << 8          # every chained field has a usable compact grid
GEOM_FLAG_POINT_SMALL = 1 << 9        # point robot, ONE field of at most 32 spheres and 8 boxes
GEOM_FLAG_POINT = 1 << 10             # point robot
GEOM_FLAG_ONE_FIELD = 1 << 12         # no chain
GEOM_FLAG_ALL_LISTS = 1 << 13         # every chained field carries a list grid
GEOM_FLAG_CELLS_SHIFT = 16            # bits 16-28: cells of the largest grid of the chain (with ALL_GRIDS or ALL_LISTS)
GEOM_FLAG_CELLS_MASK = (1 << 13) - 1

# what include/mpb_geom_layout.h carries besides the word indices: (heading, C literal form, names), each as MPB_<name>
C_LAYOUT = (
    ('magic, versions, robot kinds', '0x%X', ('GEOM_MAGIC',)),
    (None, '%d', ('GEOM_VERSION', 'GEOM_VERSION_LIST', 'KIND_POINT', 'KIND_CHAIN')),
    ('limits', '%d', ('MAX_DOF', 'MAX_FIELDS', 'GEOM_HEADER_WORDS', 'GRID_MAX_CELLS', 'GRID_PAD', 'GRID_MAX_SPH', 'LIST_MAX_SPH', 'LIST_MAX_BOX',
                      'LIST_MAX_CAND', 'LIST_CELL_MAX_SPH', 'LIST_CELL_MAX_BOX')),
    ('compact grid cell word', '%d', ('GRID_SLOTS', 'GRID_SLOT_BITS')),
    (None, '0x%Xu', ('GRID_SLOT_MASK', 'GRID_OVERFLOW')),
    ('list grid cell word', '%d', ('LIST_NSPH_SHIFT', 'LIST_NBOX_SHIFT')),
    (None, '0x%Xu', ('LIST_START_MASK', 'LIST_NSPH_MASK', 'LIST_NBOX_MASK', 'LIST_OVERFLOW', 'LIST_RESERVED')),
    ('geom_flags', '0x%X', ('GEOM_FLAG_MODEL_MASK', 'GEOM_FLAG_ALL_GRIDS', 'GEOM_FLAG_POINT_SMALL', 'GEOM_FLAG_POINT', 'GEOM_FLAG_ONE_FIELD',
                            'GEOM_FLAG_ALL_LISTS')),
    (None, '%d', ('GEOM_FLAG_CELLS_SHIFT',)),
    (None, '0x%X', ('GEOM_FLAG_CELLS_MASK',)),
)

# the grid builders' own tuning (not part of the layout)
GRID_MAX_DIM = 64       # cells per axis of the broad-phase grid
GRID_CELL = 0.14        # coarsest target cell edge [m]; refined by GRID_REFINE steps down to GRID_CELL_MIN while the grid fits
GRID_CELL_MIN = 0.05
GRID_REFINE = 0.97
BOX_2D_HALF_Z = 1.0e6  # 2-D boxes are 3-D boxes that are effectively infinite in z


def header(buf, offset=0):
    """The header of the field that starts at word `offset` of a packed buffer, as a numpy record over HEADER_WORDS: a VIEW -- reads
    and writes by name go to the buffer's own words (h['n_sph'], h['grid_dims'][0], h['next'] = 0)."""
    words = np.asarray(buf)[offset:offset + GEOM_HEADER_WORDS]
    assert words.dtype.itemsize == 4 and words.size == GEOM_HEADER_WORDS, 'a packed geometry buffer is an array of 32-bit words'
    return words.view(HEADER_DTYPE)[0]


def fields(buf):
    """The headers (as header() gives them) of the chained fields of a packed buffer, in order."""
    off = 0
    while True:
        h = header(buf, off)
        yield h
        if h['next'] == 0:
            return
        off += int(h['next'])


def grid_cell_slots(words):
    """Compact-grid cell words (..., ) -> their GRID_SLOTS obstacle indices (..., GRID_SLOTS); meaningless where words == GRID_OVERFLOW."""
    w = np.asarray(words, dtype=np.uint32)
    return np.stack([(w >> (GRID_SLOT_BITS * k)) & GRID_SLOT_MASK for k in range(GRID_SLOTS)], -1)


def list_cell_fields(words):
    """List-grid cell words -> (start, sphere count, box count, overflows) as the kernels decode them."""
    w = np.asarray(words, dtype=np.uint32)
    return (w & LIST_START_MASK, (w >> LIST_NSPH_SHIFT) & LIST_NSPH_MASK, (w >> LIST_NBOX_SHIFT) & LIST_NBOX_MASK, (w & LIST_OVERFLOW) != 0)


def _rot_x(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=np.float64)


def _rot_z(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float64)


def _mdh(alpha, a, d):
    """Modified-DH constant part: Rx(alpha) * Tx(a) * Tz(d) as a 3x4 matrix."""
    R = _rot_x(alpha)
    t = R @ np.array([a, 0.0, d])
    # Rx(alpha) Tx(a) Tz(d): translation = Rx * (a,0,d)  (Tx and Tz act in the rotated frame)
    out = np.zeros((3, 4), dtype=np.float64)
    out[:, :3] = R
    out[:, 3] = t
    # cos(+-pi/2) evaluates to 6.1e-17, not 0: the link twists of a modified-DH table are exact quarter turns, so such
    # residues are rounding noise of the table's construction -- snapped to exact zeros (the compile-time robot models
    # of model_gen.py then fold those terms away, and the generic kernels / the oracle see the same exact tables)
    out[np.abs(out) < 1e-12] = 0.0
    return out


class Robot:
    """Common robot interface mirroring what the reference consumes
    (cost_functions.py:21 ``q_dim``; :50-51 ``get_position``/``get_velocity``;
    :412-420 ``q_min``/``q_max``; :380 ``dt``)."""

    kind = None

    def __init__(self, q_dim, q_min, q_max, dt=None, dq_max=None, ddq_max=None):
        self.q_dim = int(q_dim)
        self.q_min_np = np.asarray(q_min, dtype=np.float32)
        self.q_max_np = np.asarray(q_max, dtype=np.float32)
        self.dt = dt
        # per-joint velocity / acceleration limits, symmetric about zero (None: the robot carries none): what retiming reads
        self.dq_max_np, self.ddq_max_np = (self._limit(v, name) for v, name in ((dq_max, 'dq_max'), (ddq_max, 'ddq_max')))

    def _limit(self, v, name):
        if v is None:
            return None
        v = np.asarray(v, dtype=np.float32)
        if v.shape != (self.q_dim,) or not (np.all(np.isfinite(v)) and np.all(v > 0)):
            raise ValueError(f'{name} must hold {self.q_dim} finite limits > 0 (got {v.tolist()})')
        return v

    @property
    def q_min(self):
        return torch.from_numpy(self.q_min_np)

    @property
    def q_max(self):
        return torch.from_numpy(self.q_max_np)

    @property
    def dq_max(self):
        return None if self.dq_max_np is None else torch.from_numpy(self.dq_max_np)

    @property
    def ddq_max(self):
        return None if self.ddq_max_np is None else torch.from_numpy(self.ddq_max_np)

    # state slicing -- same meaning as torch_robotics' RobotBase (positions first, velocities last)
    def get_position(self, x):
        return x[..., :self.q_dim]

    def get_velocity(self, x):
        return x[..., self.q_dim:2 * self.q_dim]

    def spec(self):
        raise NotImplementedError


class RobotPointMass(Robot):
    """Point-mass robot in 2-D or 3-D with one collision sphere of radius ``radius``."""

    kind = KIND_POINT

    def __init__(self, q_dim=2, radius=0.01, q_limits=(-1.0, 1.0), dt=None, dq_max=None, ddq_max=None):
        super().__init__(q_dim, [q_limits[0]] * q_dim, [q_limits[1]] * q_dim, dt=dt, dq_max=dq_max, ddq_max=ddq_max)
        assert q_dim in (2, 3)
        self.radius = float(radius)

    def spec(self):
        return dict(
            kind=KIND_POINT, n_dof=self.q_dim,
            joint_tf=np.zeros((0, 3, 4), np.float32),
            link_frame=np.zeros((1,), np.int32),
            link_offset=np.zeros((1, 3), np.float32),
            link_radius=np.array([self.radius], np.float32),
        )


class RobotSerialChain(Robot):
    """Serial chain of revolute joints with a fixed set of collision spheres."""

    kind = KIND_CHAIN

    def __init__(self, joint_tf, link_frame, link_offset, link_radius, q_min, q_max, dt=None, dq_max=None, ddq_max=None):
        joint_tf = np.asarray(joint_tf, dtype=np.float32)
        n_dof = len(q_min)
        assert joint_tf.shape in ((n_dof, 3, 4), (n_dof + 1, 3, 4))
        if joint_tf.shape[0] == n_dof:  # no tool frame: append identity
            eye = np.zeros((1, 3, 4), np.float32)
            eye[0, :, :3] = np.eye(3)
            joint_tf = np.concatenate([joint_tf, eye], 0)
        assert n_dof <= MAX_DOF
        super().__init__(n_dof, q_min, q_max, dt=dt, dq_max=dq_max, ddq_max=ddq_max)
        self.joint_tf = joint_tf
        self.link_frame = np.asarray(link_frame, dtype=np.int32)
        self.link_offset = np.asarray(link_offset, dtype=np.float32).reshape(-1, 3)
        self.link_radius = np.asarray(link_radius, dtype=np.float32)
        assert self.link_frame.min() >= 1 and self.link_frame.max() <= n_dof + 1
        # kernels walk the chain once and emit spheres frame by frame
        assert np.all(np.diff(self.link_frame) >= 0), "collision spheres must be sorted by frame"

    def spec(self):
        return dict(
            kind=KIND_CHAIN, n_dof=self.q_dim, joint_tf=self.joint_tf,
            link_frame=self.link_frame, link_offset=self.link_offset, link_radius=self.link_radius,
        )


# Franka Emika Panda, public modified-DH table (Franka Control Interface documentation):
#   joint : a_{i-1}   d_i    alpha_{i-1}
_PANDA_MDH = [
    (0.0, 0.333, 0.0),
    (0.0, 0.0, -math.pi / 2),
    (0.0, 0.316, math.pi / 2),
    (0.0825, 0.0, math.pi / 2),
    (-0.0825, 0.384, -math.pi / 2),
    (0.0, 0.0, math.pi / 2),
    (0.088, 0.0, math.pi / 2),
]
_PANDA_FLANGE_D = 0.107
_PANDA_Q_MIN = [-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973]
_PANDA_Q_MAX = [2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973]
# the data sheet's joint velocity (rad/s) and acceleration (rad/s^2) limits
_PANDA_DQ_MAX = [2.175, 2.175, 2.175, 2.175, 2.61, 2.61, 2.61]
_PANDA_DDQ_MAX = [15.0, 7.5, 10.0, 12.5, 15.0, 20.0, 20.0]

# Build-defined collision-sphere set: (frame, x, y, z, radius); frame j = link j (after joint j),
# frame 8 = flange + hand (Tz(0.107) Rz(-pi/4)).
_PANDA_SPHERES = [
    (1, 0.0, 0.0, -0.20, 0.08), (1, 0.0, 0.0, -0.10, 0.08), (1, 0.0, -0.03, 0.0, 0.08),
    (2, 0.0, 0.0, 0.03, 0.08), (2, 0.0, -0.07, 0.0, 0.07), (2, 0.0, -0.14, 0.0, 0.07),
    (3, 0.0, 0.0, -0.12, 0.07), (3, 0.0, 0.0, -0.05, 0.07), (3, 0.04, 0.0, -0.02, 0.07),
    (3, 0.0825, 0.03, 0.0, 0.07),
    (4, 0.0, 0.0, 0.03, 0.07), (4, -0.04, 0.02, 0.0, 0.07), (4, -0.0825, 0.06, 0.0, 0.07),
    (4, -0.0825, 0.10, 0.02, 0.06),
    (5, 0.0, 0.0, -0.26, 0.07), (5, 0.0, 0.04, -0.20, 0.06), (5, 0.0, 0.07, -0.14, 0.055),
    (5, 0.0, 0.08, -0.08, 0.055), (5, 0.0, 0.05, -0.02, 0.06), (5, 0.0, 0.0, 0.0, 0.07),
    (6, 0.0, 0.0, 0.01, 0.07), (6, 0.06, 0.0, 0.01, 0.06), (6, 0.088, 0.02, 0.0, 0.06),
    (7, 0.0, 0.0, 0.07, 0.06), (7, 0.03, 0.03, 0.09, 0.045), (7, -0.03, -0.03, 0.09, 0.045),
    (8, 0.0, 0.0, 0.03, 0.06), (8, 0.0, 0.06, 0.04, 0.045), (8, 0.0, -0.06, 0.04, 0.045),
    (8, 0.0, 0.04, 0.09, 0.03), (8, 0.0, -0.04, 0.09, 0.03),
]


class RobotPanda(RobotSerialChain):
    """7-DoF Franka Panda: public DH kinematics + a build-defined set of 31 collision spheres."""

    def __init__(self, dt=None):
        tfs = [_mdh(alpha, a, d) for (a, d, alpha) in _PANDA_MDH]
        tool = np.zeros((3, 4))
        tool[:, :3] = _rot_z(-math.pi / 4)
        tool[:, 3] = [0.0, 0.0, _PANDA_FLANGE_D]
        tfs.append(tool)
        sph = np.array(_PANDA_SPHERES, dtype=np.float64)
        super().__init__(
            joint_tf=np.stack(tfs), link_frame=sph[:, 0].astype(np.int32),
            link_offset=sph[:, 1:4], link_radius=sph[:, 4],
            q_min=_PANDA_Q_MIN, q_max=_PANDA_Q_MAX, dt=dt, dq_max=_PANDA_DQ_MAX, ddq_max=_PANDA_DDQ_MAX)


class CollisionField:
    """Set of sphere / axis-aligned-box obstacles plus the hinge margin.

    Stands in for torch_robotics' collision distance fields (reference call site
    field_factor.py:39 ``field.compute_cost(q_pos, link_pos, **kwargs)``).
    """

    def __init__(self, spheres=None, boxes=None, margin=0.05):
        def _arr(x, w):
            a = np.zeros((0, w), np.float32) if x is None else np.asarray(x, dtype=np.float32)
            return a.reshape(-1, w)
        sp = np.asarray(spheres, np.float32) if spheres is not None and len(spheres) else None
        bx_ = np.asarray(boxes, np.float32) if boxes is not None and len(boxes) else None
        # every primitive given in its 2-D form (circles, rectangles): what GridSDFField.from_field makes a planar grid of
        self.is_2d = all(a is None or a.shape[-1] == w for a, w in ((sp, 3), (bx_, 4)))
        if sp is not None and sp.shape[-1] == 3:  # 2-D circles (cx, cy, r)
            sp = np.concatenate([sp[:, :2], np.zeros((len(sp), 1), np.float32), sp[:, 2:3]], 1)
        bx = np.asarray(boxes, np.float32) if boxes is not None and len(boxes) else None
        if bx is not None and bx.shape[-1] == 4:  # 2-D boxes (cx, cy, hx, hy)
            n = len(bx)
            bx = np.concatenate([bx[:, :2], np.zeros((n, 1), np.float32), bx[:, 2:4],
                                 np.full((n, 1), BOX_2D_HALF_Z, np.float32)], 1)
        self.spheres = _arr(sp, 4)
        self.boxes = _arr(bx, 6)
        self.margin = float(margin)
        assert len(self.spheres) + len(self.boxes) > 0, "empty collision field"

    def spec(self):
        return dict(spheres=self.spheres, boxes=self.boxes, margin=np.float32(self.margin))

    def zero_grad(self):  # reference calls field.zero_grad() (field_factor.py:56); nothing to clear here
        pass


def fk_spheres_f64(rs, q):
    """Collision-sphere centres of a serial chain in fp64 on the host: robot spec, q (N, D) -> (N, L, 3), by the module docstring's
    definition (what the pair builder of SelfCollisionField judges "always in collision" with)."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, int(rs['n_dof']))
    tf = np.asarray(rs['joint_tf'], dtype=np.float64)
    N, D = q.shape
    R = np.broadcast_to(np.eye(3), (N, 3, 3)).copy()
    t = np.zeros((N, 3))
    frames = []
    for j in range(tf.shape[0]):
        t = t + R @ tf[j, :, 3]
        R = R @ tf[j, :, :3]
        if j < D:
            c, s = np.cos(q[:, j]), np.sin(q[:, j])
            Rz = np.zeros((N, 3, 3))
            Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = c, -s, s, c, 1.0
            R = R @ Rz
        frames.append((R, t))
    off = np.asarray(rs['link_offset'], dtype=np.float64)
    return np.stack([frames[int(f) - 1][0] @ off[l] + frames[int(f) - 1][1] for l, f in enumerate(rs['link_frame'])], 1)


class SelfCollisionField:
    """The robot against itself (build-defined; the reference's examples get this field from torch_robotics with
    use_self_collision_storm=True).  Serial chains only.

    Per-waypoint cost  c(q) = sum over pairs (a, b) of relu(T_ab - |x_a(q) - x_b(q)|),  T_ab = margin + r_a + r_b,  x_l the collision-
    sphere centres of fk_map_collision; a configuration collides with itself iff c(q) > 0.

    pairs=None builds the default list: all a < b with link_frame[b] - link_frame[a] >= min_frame_gap whose hinge is NOT positive at
    every one of ALWAYS_SAMPLES configurations drawn uniformly in the joint limits with np.random.RandomState(0), evaluated in fp64
    (MoveIt's "always in collision" rule: spheres of nearby links that overlap by construction), sorted by (a, b).  An explicit
    `pairs` is validated: a < b < n_links, no duplicates."""

    ALWAYS_SAMPLES = 1024

    def __init__(self, robot, margin=0.02, min_frame_gap=3, pairs=None):
        if getattr(robot, 'kind', None) != KIND_CHAIN:
            raise ValueError('SelfCollisionField serves serial chains only (a point robot has one collision sphere)')
        from .self_layout import SELF_MAX_LINKS, SELF_MAX_PAIRS
        self.robot = robot
        self.margin = float(margin)
        self.min_frame_gap = int(min_frame_gap)
        rs = robot.spec()
        n_links = len(rs['link_radius'])
        if n_links > SELF_MAX_LINKS:
            raise ValueError(f'{n_links} collision spheres exceed SELF_MAX_LINKS = {SELF_MAX_LINKS}')
        if pairs is None:
            pairs = self.default_pairs(robot, self.margin, self.min_frame_gap)
        else:
            pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
            if len(pairs) and not (np.all(pairs[:, 0] >= 0) and np.all(pairs[:, 0] < pairs[:, 1]) and np.all(pairs[:, 1] < n_links)):
                raise ValueError(f'every pair needs 0 <= a < b < n_links = {n_links}')
            if len(np.unique(pairs, axis=0)) != len(pairs):
                raise ValueError('duplicate pairs')
        if len(pairs) > SELF_MAX_PAIRS:
            raise ValueError(f'{len(pairs)} pairs exceed SELF_MAX_PAIRS = {SELF_MAX_PAIRS}')
        self.pairs = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)

    @classmethod
    def default_pairs(cls, robot, margin, min_frame_gap):
        rs = robot.spec()
        lf = np.asarray(rs['link_frame'], dtype=np.int64)
        a, b = np.triu_indices(len(lf), k=1)                   # a < b, sorted by (a, b)
        far = lf[b] - lf[a] >= min_frame_gap
        a, b = a[far], b[far]
        rng = np.random.RandomState(0)
        q = rng.uniform(robot.q_min_np.astype(np.float64), robot.q_max_np.astype(np.float64), (cls.ALWAYS_SAMPLES, robot.q_dim))
        x = fk_spheres_f64(rs, q)
        T = margin + np.asarray(rs['link_radius'], np.float64)[a] + np.asarray(rs['link_radius'], np.float64)[b]
        always = np.all(T[None, :] - np.linalg.norm(x[:, a] - x[:, b], axis=-1) > 0.0, axis=0)
        return np.stack([a[~always], b[~always]], -1)

    def thresholds(self):
        """T_ab of every pair, fp64: margin + r_a + r_b from the robot's fp32 radii."""
        r = np.asarray(self.robot.spec()['link_radius'], dtype=np.float64)
        return self.margin + r[self.pairs[:, 0]] + r[self.pairs[:, 1]]

    def zero_grad(self):
        pass


def pack_self_collision(robot, field):
    """Pack a chain + its SelfCollisionField into ONE self-contained fp32 word buffer (self_layout.py: header, joint_tf rows, links
    rows -- both in the row formats of pack_geometry, every link kept --, the pair table with T_ab rounded once from fp64)."""
    from . import self_layout as S
    if field.robot is not robot:
        rs0, rs1 = field.robot.spec(), robot.spec()
        if not all(np.array_equal(np.asarray(rs0[k]), np.asarray(rs1[k])) for k in ('joint_tf', 'link_frame', 'link_offset', 'link_radius')):
            raise ValueError('the SelfCollisionField was built for another robot')
    rs = robot.spec()
    n_tf, n_links, n_pairs = rs['joint_tf'].shape[0], len(rs['link_radius']), len(field.pairs)
    off_tf = S.SELF_HEADER_WORDS
    off_links = off_tf + 12 * n_tf
    off_pairs = off_links + 8 * n_links
    total = off_pairs + S.SELF_PAIR_WORDS * n_pairs
    buf = np.zeros((total,), dtype=np.float32)
    hdr = S.header(buf)
    for name, value in dict(magic=S.SELF_MAGIC, version=S.SELF_VERSION, n_dof=rs['n_dof'], n_tf=n_tf, n_links=n_links, n_pairs=n_pairs,
                            margin=field.margin, off_tf=off_tf, off_links=off_links, off_pairs=off_pairs, total=total).items():
        hdr[name] = value
    buf[off_tf:off_links] = rs['joint_tf'].astype(np.float32).reshape(-1)
    links = np.zeros((n_links, 8), np.float32)
    links.view(np.int32)[:, 0] = rs['link_frame']
    links[:, 1:4] = rs['link_offset']
    links[:, 4] = rs['link_radius']
    buf[off_links:off_pairs] = links.reshape(-1)
    pw = np.zeros((n_pairs, S.SELF_PAIR_WORDS), np.float32)
    pw.view(np.uint32)[:, 0] = (field.pairs[:, 0] | (field.pairs[:, 1] << S.SELF_PAIR_B_SHIFT)).astype(np.uint32)
    pw[:, 1] = field.thresholds().astype(np.float32)
    buf[off_pairs:total] = pw.reshape(-1)
    return buf


class MovingObstacleField:
    """Obstacles that move (build-defined): spheres and axis-aligned boxes whose centres follow keyframes, seen by
    row h of a trajectory at the time t_h of the field's clock.

    t_key (K,): K >= 1 keyframe times, strictly ascending.  sphere_centers (K, Os, 3) with sphere_radii (Os,); box_centers (K, Ob, 3)
    with box_half (Ob, 3): boxes translate and do not rotate.  Os + Ob >= 1.  Centres given with two coordinates get z = 0 (a planar
    point mass), box half extents given with two get BOX_2D_HALF_Z, as CollisionField's 2-D forms do.  Every refusal is a ValueError that
    names the argument.

    Motion: centres are piecewise linear between keyframes, held at the first keyframe before t_key[0] and at the last after
    t_key[-1], evaluated in fp64 on the host.
    Clock: a trajectory of R >= 2 rows spans [t_start, t_end] uniformly, row h at t_start + h (t_end - t_start) / (R - 1); a single
    row is at t_start.  The defaults are t_key[0] and t_key[-1].  The clock belongs to the field, not to a row count: the same field
    serves a planner's support points, an interpolated trajectory and MPPI's rollouts.

    Cost of row h:  c_h(q) = sum_l relu(margin + r_l - min_o sd_{o,h}(x_l(q)))  with CollisionField's signed distances and gradient
    conventions about the centres c_{o,h}; spheres in the given order, then boxes.  Time is fixed per row: the obstacles' velocity is no
    part of d c / d q.  A field whose keyframes are all equal means exactly the static CollisionField of at(t)."""

    def __init__(self, t_key, sphere_centers=None, sphere_radii=None, box_centers=None, box_half=None, margin=0.05, t_start=None, t_end=None):
        t = np.asarray(t_key, dtype=np.float64).reshape(-1)
        if t.size < 1 or not np.all(np.isfinite(t)) or np.any(np.diff(t) <= 0):
            raise ValueError('t_key must hold K >= 1 finite, strictly ascending keyframe times')
        self.t_key = t
        K = t.size

        def centres(c, name):
            if c is None:
                return np.zeros((K, 0, 3))
            c = np.asarray(c, dtype=np.float64)
            if c.ndim != 3 or c.shape[0] != K or c.shape[2] not in (2, 3):
                raise ValueError(f'{name} has shape {c.shape}, expected (K = {K}, O, 3) (or (K, O, 2): z = 0)')
            if not np.all(np.isfinite(c)):
                raise ValueError(f'{name} must be finite')
            if c.shape[2] == 2:
                c = np.concatenate([c, np.zeros(c.shape[:2] + (1,))], -1)
            return np.ascontiguousarray(c)

        def sizes(v, n, width, name, centres_name):
            if v is None:
                if n:
                    raise ValueError(f'{name} is required with {centres_name}')
                return np.zeros((0, width) if width > 1 else (0,))
            v = np.asarray(v, dtype=np.float64)
            if width == 3 and v.ndim == 2 and v.shape[1] == 2:
                v = np.concatenate([v, np.full((v.shape[0], 1), BOX_2D_HALF_Z)], -1)
            want = (n, width) if width > 1 else (n,)
            if v.shape != want:
                raise ValueError(f'{name} has shape {v.shape}, expected {want} to go with {centres_name}')
            if not (np.all(np.isfinite(v)) and np.all(v > 0)):
                raise ValueError(f'{name} must be finite and > 0')
            return np.ascontiguousarray(v)

        self.sphere_centers = centres(sphere_centers, 'sphere_centers')
        self.sphere_radii = sizes(sphere_radii, self.sphere_centers.shape[1], 1, 'sphere_radii', 'sphere_centers')
        self.box_centers = centres(box_centers, 'box_centers')
        self.box_half = sizes(box_half, self.box_centers.shape[1], 3, 'box_half', 'box_centers')
        if self.n_spheres + self.n_boxes < 1:
            raise ValueError('sphere_centers / box_centers: a MovingObstacleField needs at least one obstacle')
        self.margin = float(margin)
        if not np.isfinite(self.margin):
            raise ValueError('margin must be finite')
        self.t_start = float(t[0] if t_start is None else t_start)
        self.t_end = float(t[-1] if t_end is None else t_end)
        if not np.isfinite(self.t_start):
            raise ValueError('t_start must be finite')
        if not (np.isfinite(self.t_end) and self.t_end >= self.t_start):
            raise ValueError('t_end must be finite and >= t_start')

    @property
    def n_spheres(self):
        return self.sphere_centers.shape[1]

    @property
    def n_boxes(self):
        return self.box_centers.shape[1]

    def times(self, R):
        """(R,) fp64: the time of every row of a trajectory of R rows."""
        R = int(R)
        if R < 1:
            raise ValueError(f'R = {R}: a trajectory has at least one row')
        if R == 1:
            return np.array([self.t_start])
        return self.t_start + np.arange(R) * (self.t_end - self.t_start) / (R - 1)

    def _centres(self, t):
        """t (R,) -> ((R, Os, 3), (R, Ob, 3)) fp64: piecewise linear per component, held beyond the keyframes."""
        t = np.asarray(t, dtype=np.float64).reshape(-1)
        out = []
        for keys in (self.sphere_centers, self.box_centers):
            c = np.zeros((t.size,) + keys.shape[1:])
            for o in range(keys.shape[1]):
                for k in range(3):
                    c[:, o, k] = np.interp(t, self.t_key, keys[:, o, k])
            out.append(c)
        return tuple(out)

    def rows(self, R):
        """The centres of every obstacle at every row of a trajectory of R rows: ((R, Os, 3), (R, Ob, 3)) fp64."""
        return self._centres(self.times(R))

    def at(self, t):
        """The static CollisionField the obstacles form at time t, with the same margin (centres rounded once from fp64): for a
        frozen-time RRT, for drawing, and what the tests restate the definition with."""
        t = float(t)
        if not np.isfinite(t):
            raise ValueError('t must be finite')
        sc, bc = self._centres(np.array([t]))
        spheres = np.concatenate([sc[0], self.sphere_radii[:, None]], 1) if self.n_spheres else None
        boxes = np.concatenate([bc[0], self.box_half], 1) if self.n_boxes else None
        return CollisionField(spheres=spheres, boxes=boxes, margin=self.margin)

    def shifted(self, delta):
        """The same motion with the window [t_start, t_end] moved by `delta`: the receding-horizon step."""
        delta = float(delta)
        if not np.isfinite(delta):
            raise ValueError('delta must be finite')
        return MovingObstacleField(self.t_key, self.sphere_centers if self.n_spheres else None, self.sphere_radii if self.n_spheres else None,
                                   self.box_centers if self.n_boxes else None, self.box_half if self.n_boxes else None, margin=self.margin,
                                   t_start=self.t_start + delta, t_end=self.t_end + delta)

    def zero_grad(self):
        pass


def pack_moving_obstacles(robot, field, n_rows):
    """Pack a robot + a MovingObstacleField for trajectories of n_rows rows into ONE self-contained fp32 word buffer (moving_layout.py:
    header, joint_tf rows, links rows -- both in the row formats of pack_geometry, every link kept --, the radii and half-extent tables,
    then the centres as [obstacle][x|y|z][row], the row axis padded to a multiple of MOVING_ROW_PAD by repeating the last row; centres
    rounded once from fp64)."""
    from . import moving_layout as S
    if not isinstance(field, MovingObstacleField):
        raise TypeError('pack_moving_obstacles takes a MovingObstacleField')
    rs = robot.spec()
    n_rows = int(n_rows)
    n_tf, n_links, ns, nb = rs['joint_tf'].shape[0], len(rs['link_radius']), field.n_spheres, field.n_boxes
    for what, n, lo, name in (('n_rows', n_rows, 1, 'MOVING_MAX_ROWS'), ('moving spheres', ns, 0, 'MOVING_MAX_SPHERES'),
                              ('moving boxes', nb, 0, 'MOVING_MAX_BOXES'), ('collision spheres of the robot', n_links, 1, 'MOVING_MAX_LINKS')):
        if not lo <= n <= getattr(S, name):
            raise ValueError(f'{what}: {n} outside {lo}..{name} = {getattr(S, name)}')
    off = S.offsets(n_tf, n_links, n_rows, ns, nb)
    buf = np.zeros((off['total'],), dtype=np.float32)
    hdr = S.header(buf)
    for name, value in dict(magic=S.MOVING_MAGIC, version=S.MOVING_VERSION, n_dof=rs['n_dof'], n_tf=n_tf, n_links=n_links, n_rows=n_rows,
                            n_spheres=ns, n_boxes=nb, margin=field.margin, **off).items():
        hdr[name] = value
    sec = S.sections(buf)
    sec['joint_tf'][...] = rs['joint_tf'].astype(np.float32)
    sec['links'].view(np.int32)[:, 0] = rs['link_frame'] if rs['kind'] == KIND_CHAIN else 1
    sec['links'][:, 1:4] = rs['link_offset']
    sec['links'][:, 4] = rs['link_radius']
    sec['radii'][...] = field.sphere_radii.astype(np.float32)
    sec['half'][:, :3] = field.box_half.astype(np.float32)
    sc, bc = field.rows(n_rows)
    c = np.concatenate([sc, bc], 1).astype(np.float32)                 # (R, O, 3), spheres first
    sec['centres'][:, :, :n_rows] = c.transpose(1, 2, 0)
    sec['centres'][:, :, n_rows:] = sec['centres'][:, :, n_rows - 1:n_rows]
    return buf


class TriangleMesh:
    """A triangle mesh as the source of a GridSDFField (GridSDFField.from_mesh): `vertices` (nv, 3), `faces` (nt, 3) vertex indices,
    triangles counter-clockwise seen from outside.  The vertices are kept as the fp32 numbers the packed buffer carries; every check
    below is taken in fp64 on THOSE.  signed=True: a closed, consistently oriented surface, the grid's node value carries the sign
    (inside negative).  signed=False: any triangle soup -- open surfaces, scans --, node value distance - thickness.

    Refused, by ValueError: non-finite vertices; indices out of range; more than MESH_MAX_TRIS = 2^20 triangles; a triangle of zero
    area; for a signed mesh a directed edge that occurs twice (not consistently oriented) or whose reverse does not occur exactly once
    (not closed), and a negative total signed volume (oriented inside out)."""

    def __init__(self, vertices, faces, signed=True, thickness=0.0):
        from .mesh_layout import MESH_MAX_TRIS
        v = np.asarray(vertices, dtype=np.float64)
        f = np.asarray(faces)
        if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1:
            raise ValueError(f'TriangleMesh: vertices of shape {v.shape} and faces of shape {f.shape}, expected (nv, 3) and (nt >= 1, 3)')
        if not np.issubdtype(f.dtype, np.integer):
            raise ValueError('TriangleMesh: faces must be integer vertex indices')
        if not np.all(np.isfinite(v)) or not np.all(np.isfinite(v.astype(np.float32))):
            raise ValueError('TriangleMesh: non-finite vertices')
        f = f.astype(np.int64)
        if f.min() < 0 or f.max() >= v.shape[0]:
            raise ValueError(f'TriangleMesh: vertex indices out of range 0..{v.shape[0] - 1}')
        if f.shape[0] > MESH_MAX_TRIS:
            raise ValueError(f'TriangleMesh: {f.shape[0]} triangles exceed MESH_MAX_TRIS = {MESH_MAX_TRIS}')
        self.vertices = np.ascontiguousarray(v.astype(np.float32))
        self.faces = np.ascontiguousarray(f)
        self.signed = bool(signed)
        self.thickness = float(thickness)
        if not (np.isfinite(self.thickness) and self.thickness >= 0.0) or (self.signed and self.thickness != 0.0):
            raise ValueError('TriangleMesh: thickness must be finite and >= 0, and 0 for a signed mesh')
        a, b, c = (self.vertices.astype(np.float64)[f[:, m]] for m in range(3))
        cross = np.cross(b - a, c - a)
        area2 = np.linalg.norm(cross, axis=1)
        if np.any(area2 == 0.0):
            raise ValueError(f'TriangleMesh: triangle {int(np.argmax(area2 == 0.0))} is degenerate (zero area)')
        if self.signed:
            nv = v.shape[0]
            directed = np.concatenate([f[:, 0] * nv + f[:, 1], f[:, 1] * nv + f[:, 2], f[:, 2] * nv + f[:, 0]])
            reverse = np.concatenate([f[:, 1] * nv + f[:, 0], f[:, 2] * nv + f[:, 1], f[:, 0] * nv + f[:, 2]])
            if np.unique(directed).size != directed.size:
                raise ValueError('TriangleMesh: a directed edge occurs twice: a signed mesh must be consistently oriented')
            if not np.all(np.isin(reverse, directed)):
                raise ValueError('TriangleMesh: an edge without its reverse: a signed mesh must be closed')
            if float(np.einsum('ij,ij->', a, cross)) < 0.0:
                raise ValueError('TriangleMesh: negative signed volume: the triangles are oriented inside out')

    @property
    def n_tri(self):
        return self.faces.shape[0]

    def transformed(self, pose):
        """The mesh with every vertex taken through [R | t] (fp64, then rounded to fp32)."""
        P = np.asarray(pose, dtype=np.float64)
        return TriangleMesh(self.vertices.astype(np.float64) @ P[:3, :3].T + P[:3, 3], self.faces, signed=self.signed, thickness=self.thickness)


def mesh_pseudonormals(mesh):
    """(face (nt, 3), edge (nt, 3, 3), vertex (nt, 3, 3)) fp32 of a TriangleMesh: the unit face normals, per triangle the pseudonormals
    of its edges ab, bc, ca (sum of the unit normals of the faces on the edge) and of its vertices a, b, c (angle-weighted sum of the
    normals of the faces at the vertex; Baerentzen and Aanaes).  Computed in fp64 ONCE per edge and per vertex and rounded to fp32:
    every copy carries identical bits."""
    v, f = mesh.vertices.astype(np.float64), mesh.faces
    nv, nt = v.shape[0], f.shape[0]
    p = v[f]                                                         # (nt, 3, 3)
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    ends = np.stack([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=1)           # (nt, 3 edges, 2)
    key = ends.min(-1) * nv + ends.max(-1)
    uniq, inv = np.unique(key.reshape(-1), return_inverse=True)
    edge_sum = np.zeros((uniq.size, 3))
    np.add.at(edge_sum, inv.reshape(-1), np.repeat(n, 3, axis=0))
    vert_sum = np.zeros((nv, 3))
    for m in range(3):
        e1, e2 = p[:, (m + 1) % 3] - p[:, m], p[:, (m + 2) % 3] - p[:, m]
        cosang = np.einsum('ij,ij->i', e1, e2) / (np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1))
        np.add.at(vert_sum, f[:, m], np.arccos(np.clip(cosang, -1.0, 1.0))[:, None] * n)
    edge32, vert32 = edge_sum.astype(np.float32), vert_sum.astype(np.float32)
    return n.astype(np.float32), edge32[inv.reshape(nt, 3)], vert32[f]


def _morton30(u):
    """30-bit Morton codes of points u (n, 3) in [0, 1]^3: 10 bits per axis, x lowest."""
    q = np.minimum((u * 1024.0).astype(np.int64), 1023)
    code = np.zeros(q.shape[0], np.int64)
    for bit in range(10):
        for axis in range(3):
            code |= ((q[:, axis] >> bit) & 1) << (3 * bit + axis)
    return code


def pack_mesh(mesh):
    """Pack a TriangleMesh into ONE self-contained fp32 word buffer (mesh_layout.py: header, triangle records, group boxes).  The
    triangles are sorted by the Morton code of their centroid in the mesh's box (stable), so that a group of MESH_GROUP consecutive
    records is spatially compact; the last group is padded by repeating the last record (a repeat is never strictly nearer: it never
    wins).  A group's box is the minimum and maximum of its records' fp32 vertices -- exact in fp32, so it contains them."""
    from . import mesh_layout as M
    v, f = mesh.vertices, mesh.faces
    nt = f.shape[0]
    n_face, n_edge, n_vert = mesh_pseudonormals(mesh)
    v64 = v.astype(np.float64)
    lo, hi = v64[f].reshape(-1, 3).min(0), v64[f].reshape(-1, 3).max(0)
    cen = (v64[f].mean(1) - lo) / np.where(hi > lo, hi - lo, 1.0)
    order = np.argsort(_morton30(cen), kind='stable')
    rec = np.zeros((nt, M.MESH_TRI_WORDS), np.float32)
    rec[:, 0:9] = v[f].reshape(nt, 9)
    rec[:, 9:12] = n_face
    rec[:, 12:21] = n_edge.reshape(nt, 9)
    rec[:, 21:30] = n_vert.reshape(nt, 9)
    rec = rec[order]
    ng = (nt + M.MESH_GROUP - 1) // M.MESH_GROUP
    rec = np.concatenate([rec, np.repeat(rec[-1:], ng * M.MESH_GROUP - nt, axis=0)])
    corners = rec[:, 0:9].reshape(ng, M.MESH_GROUP * 3, 3)
    boxes = np.zeros((ng, M.MESH_BOX_WORDS), np.float32)
    boxes[:, 0:3], boxes[:, 4:7] = corners.min(1), corners.max(1)
    off_tris = M.MESH_HEADER_WORDS
    off_boxes = off_tris + ng * M.MESH_GROUP * M.MESH_TRI_WORDS
    total = off_boxes + ng * M.MESH_BOX_WORDS
    buf = np.zeros((total,), np.float32)
    hdr = M.header(buf)
    for name, value in dict(magic=M.MESH_MAGIC, version=M.MESH_VERSION, n_tri=nt, n_groups=ng, signed=int(mesh.signed), thickness=mesh.thickness,
                            bb_lo=boxes[:, 0:3].min(0), bb_hi=boxes[:, 4:7].max(0), off_tris=off_tris, off_boxes=off_boxes, total=total).items():
        hdr[name] = value
    buf[off_tris:off_boxes] = rec.reshape(-1)
    buf[off_boxes:total] = boxes.reshape(-1)
    return buf


def mesh_pose(pose, who):
    """A pose [R | t] (3 x 4 or 4 x 4, mesh frame to grid frame) as a contiguous fp32 (3, 4), or None; refused unless R is orthonormal
    with determinant +1 within 1e-5."""
    if pose is None:
        return None
    P = np.asarray(pose, dtype=np.float64)
    if P.shape == (4, 4):
        P = P[:3]
    if P.shape != (3, 4) or not np.all(np.isfinite(P)):
        raise ValueError(f'{who}: a pose is a finite 3 x 4 (or 4 x 4) matrix [R | t]')
    R = P[:, :3]
    if np.abs(R.T @ R - np.eye(3)).max() > 1e-5 or abs(np.linalg.det(R) - 1.0) > 1e-5:
        raise ValueError(f'{who}: the rotation of a pose must be orthonormal with determinant +1 within 1e-5')
    return np.ascontiguousarray(P.astype(np.float32))


class GridSDFField:
    """A precomputed grid of signed distances as a collision field (build-defined; the reference's examples build
    their environments with precompute_sdf_obj_fixed=True, sdf_cell_size=...).  Serves arbitrary geometry -- meshes, rounded boxes,
    scans: whatever the caller can tabulate -- at eight node loads per collision sphere whatever the scene holds.

    Grid: (nx, ny, nz) fp32 nodes, node (i, j, k) at lo + (i, j, k) * cell with ONE cell for all axes, stored at (k * ny + j) * nx + i:
    `values` is an array of shape (nz, ny, nx), or (ny, nx) for a planar grid (nz == 1: z is ignored, interpolation is bilinear -- the
    2-D point-mass examples).  Limits: every dimension in 2..SDF_MAX_DIM = 1024 (nz: or 1), at most SDF_MAX_NODES = 2^27 nodes.

    Sampling s(x), per axis: u = (x - lo) * inv_cell with inv_cell = fl32(1 / cell); u clamped to [0, n - 1]; i0 = min(floor(u), n - 2);
    f = u - i0; lerp form fmaf(f, v1 - v0, v0) along x, then y, then z: a point with f == 0 on every axis returns that node's bits.
    OUTSIDE the box the point is clamped: the value is that of the nearest boundary point and the gradient is zero along each clamped
    axis -- the grid is expected to COVER THE WORKSPACE (every position a collision sphere can take); nothing warns when it does not.

    Cost per waypoint c(q) = sum_l relu(margin + r_l - s(x_l(q))) over the robot's collision spheres; in collision iff c(q) > 0; an
    active sphere's gradient is -grad s(x_l) through J^T, grad s the exact derivative of the interpolant.

    GridSDFField(values, lo, cell, margin): the caller's node values (checked finite here).
    GridSDFField.from_field(collision_field, lo, hi, cell): min_o sdf_o of a CollisionField at every node, evaluated ON THE GPU when
    the field is put on a device (ops.DeviceSDFGrid, mpb_sdf_grid_build); `values` stays None on the host.
    GridSDFField.from_occupancy(occupancy, lo, cell): from an occupancy voxel map (a scan), by an exact Euclidean distance transform ON
    THE GPU (mpb_sdf_grid_build_occupancy, include/mpb.h has the definition); `values` stays None, the occupancy is the field's source.
    GridSDFField.from_mesh(mesh, lo, hi, cell): the exact signed distance to triangle meshes (TriangleMesh), each under a pose of its
    own, ON THE GPU (mpb_sdf_grid_build_mesh, include/mpb.h has the definition); `values` stays None, the source is the mesh list."""

    def __init__(self, values, lo, cell, margin=0.05):
        v = np.asarray(values, dtype=np.float32)
        if v.ndim == 2:
            v = v[None]
        if v.ndim != 3:
            raise ValueError(f'GridSDFField: values of shape {np.shape(values)}, expected (nz, ny, nx) or (ny, nx)')
        self.dims = self._check_dims(v.shape[2], v.shape[1], v.shape[0])
        if not np.all(np.isfinite(v)):
            raise ValueError('GridSDFField: non-finite node values')
        self.values = np.ascontiguousarray(v)
        self.source = None
        self._set_frame(lo, cell, margin)

    @staticmethod
    def _check_dims(nx, ny, nz):
        from .sdf_layout import SDF_MAX_DIM, SDF_MAX_NODES
        nx, ny, nz = int(nx), int(ny), int(nz)
        if nx < 2 or ny < 2 or nz < 1 or max(nx, ny, nz) > SDF_MAX_DIM:
            raise ValueError(f'GridSDFField: grid of {nx} x {ny} x {nz} nodes: every dimension must lie in 2..SDF_MAX_DIM = {SDF_MAX_DIM} '
                             f'(nz: or 1 for a planar grid)')
        if nx * ny * nz > SDF_MAX_NODES:
            raise ValueError(f'GridSDFField: {nx * ny * nz} nodes exceed SDF_MAX_NODES = {SDF_MAX_NODES}')
        return nx, ny, nz

    def _set_frame(self, lo, cell, margin):
        lo = np.asarray(lo, dtype=np.float64).reshape(-1)
        if lo.size == 2:
            lo = np.concatenate([lo, [0.0]])
        if lo.size != 3 or not np.all(np.isfinite(lo)):
            raise ValueError('GridSDFField: lo must be 2 or 3 finite coordinates')
        self.lo = lo.astype(np.float32)
        self.cell = np.float32(cell)
        if not (np.isfinite(self.cell) and self.cell > 0):
            raise ValueError('GridSDFField: cell must be positive and finite')
        self.inv_cell = np.float32(1.0) / self.cell
        self.margin = float(margin)

    @property
    def planar(self):
        return self.dims[2] == 1

    @classmethod
    def from_field(cls, collision_field, lo, hi, cell, margin=None, planar=None):
        """The grid of min_o sdf_o of `collision_field` over the box [lo, hi]: ceil((hi - lo) / cell) + 1 nodes per axis, cell as the fp32 number
        the header stores (the last node at or beyond hi).  planar (default: the field came from 2-D primitives) keeps ONE layer of nodes, at z = lo[2] (0 when lo has
        two coordinates).  margin defaults to the field's.  The nodes are evaluated on the GPU, when the field goes to a device."""
        if not isinstance(collision_field, CollisionField):
            raise TypeError('GridSDFField.from_field takes ONE CollisionField')
        self = cls.__new__(cls)
        planar = bool(collision_field.is_2d) if planar is None else bool(planar)
        lo = np.asarray(lo, dtype=np.float64).reshape(-1)
        hi = np.asarray(hi, dtype=np.float64).reshape(-1)
        if lo.size != hi.size or lo.size not in (2, 3) or (lo.size == 2 and not planar):
            raise ValueError('GridSDFField.from_field: lo and hi must both have 3 coordinates (2 for a planar grid)')
        n = [int(math.ceil((hi[a] - lo[a]) / float(np.float32(cell)))) + 1 for a in range(2 if planar else 3)]    # (the cell the header stores)
        self.dims = cls._check_dims(n[0], n[1], 1 if planar else n[2])
        self.values = None
        self.source = collision_field
        self._set_frame(lo, cell, collision_field.margin if margin is None else margin)
        return self

    @classmethod
    def from_occupancy(cls, occupancy, lo, cell, margin=0.05):
        """The grid of an occupancy voxel map: `occupancy` of shape (nz, ny, nx), or (ny, nx) for a planar grid, a numpy array or a torch
        tensor (on the CPU or already on the GPU) of any dtype, element != 0 meaning that the voxel of edge `cell` centred on the node is
        solid.  Node value: cell * (sqrt(D2) - 0.5) at a free node, minus that at an occupied one, D2 the smallest squared index distance
        to a node of the other class (include/mpb.h, mpb_sdf_grid_build_occupancy) -- evaluated on the GPU when the field goes to a
        device; ops.DeviceSDFGrid.update_occupancy rebuilds it there for the next scan.  The occupancy is kept as `source`: uint8 / bool
        arrays as they are, any other dtype as `!= 0` (never as fp32)."""
        occ = occupancy_bytes(occupancy, 'GridSDFField.from_occupancy')
        self = cls.__new__(cls)
        self.dims = cls._check_dims(occ.shape[2], occ.shape[1], occ.shape[0])
        self.values = None
        self.source = occ
        self._set_frame(lo, cell, margin)
        return self

    @classmethod
    def from_mesh(cls, mesh, lo, hi, cell, margin=0.05, pose=None, planar=False):
        """The grid of the exact signed distance to triangle meshes over the box [lo, hi] (dimensions as in from_field): `mesh` is a
        TriangleMesh, placed by `pose` ([R | t], mesh frame to grid frame; None: as it stands), or a list of (TriangleMesh, pose) whose
        union is taken (the minimum of their node values).  Node value: include/mpb.h, mpb_sdf_grid_build_mesh -- evaluated on the GPU
        when the field goes to a device; ops.DeviceSDFGrid.update_mesh rebuilds it there when an object moves.  `values` stays None;
        the field's `source` is the list of (TriangleMesh, pose as fp32 (3, 4) or None).  planar keeps ONE layer of nodes, at
        z = lo[2] (0 when lo has two coordinates)."""
        if isinstance(mesh, TriangleMesh):
            items = [(mesh, pose)]
        else:
            if pose is not None:
                raise ValueError('GridSDFField.from_mesh: a list of (TriangleMesh, pose) carries its poses, pose= must stay None')
            items = [tuple(it) for it in mesh]
        if not items or any(len(it) != 2 or not isinstance(it[0], TriangleMesh) for it in items):
            raise TypeError('GridSDFField.from_mesh takes a TriangleMesh or a non-empty list of (TriangleMesh, pose)')
        self = cls.__new__(cls)
        planar = bool(planar)
        lo = np.asarray(lo, dtype=np.float64).reshape(-1)
        hi = np.asarray(hi, dtype=np.float64).reshape(-1)
        if lo.size != hi.size or lo.size not in (2, 3) or (lo.size == 2 and not planar):
            raise ValueError('GridSDFField.from_mesh: lo and hi must both have 3 coordinates (2 for a planar grid)')
        n = [int(math.ceil((hi[a] - lo[a]) / float(np.float32(cell)))) + 1 for a in range(2 if planar else 3)]    # (the cell the header stores)
        self.dims = cls._check_dims(n[0], n[1], 1 if planar else n[2])
        self.values = None
        self.source = [(m, mesh_pose(p, 'GridSDFField.from_mesh')) for m, p in items]
        self._set_frame(lo, cell, margin)
        return self

    def zero_grad(self):
        pass


def occupancy_bytes(occupancy, who):
    """An occupancy map as a contiguous (nz, ny, nx) array of one byte per node, of the kind it came as (numpy array, or torch tensor on
    its device): uint8 / bool as they are, any other dtype as `!= 0`; (ny, nx) becomes (1, ny, nx)."""
    if isinstance(occupancy, torch.Tensor):
        occ = occupancy if occupancy.dtype in (torch.uint8, torch.bool) else occupancy != 0
        occ = occ[None] if occ.dim() == 2 else occ
        if occ.dim() == 3:
            occ = occ.contiguous()
    else:
        occ = np.asarray(occupancy)
        if occ.dtype == object:
            raise ValueError(f'{who}: occupancy must be a numeric or bool array')
        occ = occ if occ.dtype in (np.uint8, np.bool_) else occ != 0
        occ = occ[None] if occ.ndim == 2 else occ
        if occ.ndim == 3:
            occ = np.ascontiguousarray(occ)
    if len(occ.shape) != 3:
        raise ValueError(f'{who}: occupancy of shape {tuple(np.shape(occupancy))}, expected (nz, ny, nx) or (ny, nx)')
    return occ


def pack_sdf_grid(robot, field, with_nodes=True):
    """Pack a robot + a GridSDFField into ONE self-contained fp32 word buffer (sdf_layout.py: header, joint_tf rows, links rows -- both
    in the row formats of pack_geometry, every link kept --, then the node section, 16-byte aligned).  The node section holds the
    field's values; for a field made by from_field / from_occupancy / from_mesh it is left zero for the build kernels to fill on the device.  with_nodes=False
    returns the words BEFORE the node section only (the header's total still counts the nodes): what an upload needs when the nodes
    are built on the device."""
    from . import sdf_layout as S
    rs = robot.spec()
    if rs['kind'] == KIND_CHAIN and field.planar:
        raise ValueError('a planar GridSDFField (nz = 1) serves point robots only: a chain moves in three dimensions')
    n_tf, n_links = rs['joint_tf'].shape[0], len(rs['link_radius'])
    if n_links > S.SDF_MAX_LINKS:
        raise ValueError(f'{n_links} collision spheres exceed SDF_MAX_LINKS = {S.SDF_MAX_LINKS}')
    nx, ny, nz = field.dims
    off_tf = S.SDF_HEADER_WORDS
    off_links = off_tf + 12 * n_tf
    off_nodes = (off_links + 8 * n_links + S.SDF_NODE_ALIGN - 1) // S.SDF_NODE_ALIGN * S.SDF_NODE_ALIGN
    total = off_nodes + nx * ny * nz
    buf = np.zeros((total if with_nodes else off_nodes,), dtype=np.float32)
    hdr = S.header(buf)
    for name, value in dict(magic=S.SDF_MAGIC, version=S.SDF_VERSION, kind=rs['kind'], n_dof=rs['n_dof'], n_tf=n_tf, n_links=n_links,
                            margin=field.margin, dims=(nx, ny, nz), lo=field.lo, cell=field.cell, inv_cell=field.inv_cell, off_tf=off_tf,
                            off_links=off_links, off_nodes=off_nodes, total=total).items():
        hdr[name] = value
    buf[off_tf:off_links] = rs['joint_tf'].astype(np.float32).reshape(-1)
    links = np.zeros((n_links, 8), np.float32)
    links.view(np.int32)[:, 0] = rs['link_frame'] if rs['kind'] == KIND_CHAIN else 1
    links[:, 1:4] = rs['link_offset']
    links[:, 4] = rs['link_radius']
    buf[off_links:off_links + 8 * n_links] = links.reshape(-1)
    if with_nodes and field.values is not None:
        buf[off_nodes:total] = field.values.reshape(-1)
    return buf


def _fit_axis(a, b, edge):
    """(n, 1/h as fp32, K): fewest cells of a lattice-aligned edge <= `edge` that cover [a, b] (cells on a lattice through the world
    origin: cell ix of an axis is [(K + ix - 1/2) h, (K + ix + 1/2) h), geometry version 6)"""
    n = max(int(np.ceil((b - a) / edge)), 1)
    while n <= GRID_MAX_DIM:
        h = (b - a) / n
        while h <= edge * (1.0 + 1e-9):
            inv32 = np.float32(1.0 / h)
            he = 1.0 / float(inv32)                      # the edge the kernels effectively use
            K = int(np.floor(a / he + 0.5))              # (K - 1/2) he <= a
            if (K - 0.5 + n) * he >= b:
                return n, inv32, K
            h *= 1.0 + 2e-4
        n += 1
    return None


def build_list_grid(spheres, boxes, a_max, slack=1e-4, planar=False):
    """Broad-phase LIST grid (geometry version 7) over the inflated obstacle spheres AND boxes, for scenes beyond the compact grid's 63
    spheres: per cell the indices of every sphere / box a collision sphere of radius <= a_max - margin centred in the cell could be
    within its hinge threshold of (conservative, fp64).  Cell words: the LIST_* fields above (start into the candidate bytes, sphere
    count, box count -- boxes follow the spheres --, LIST_OVERFLOW where the cell overflows a count field).
    The finest lattice cell (from GRID_CELL_MIN up) whose grid fits GRID_MAX_CELLS words and LIST_MAX_CAND candidate bytes.
    None when the scene does not fit the kernels' tables (LIST_MAX_SPH / LIST_MAX_BOX) or no cell size fits."""
    ns, nb = len(spheres), len(boxes)
    if ns + nb == 0 or ns > LIST_MAX_SPH or nb > LIST_MAX_BOX:
        return None
    c = spheres[:, :3].astype(np.float64).reshape(-1, 3)
    R = spheres[:, 3].astype(np.float64).reshape(-1) + a_max + slack
    bc = boxes[:, 0:3].astype(np.float64).reshape(-1, 3)
    bh = boxes[:, 3:6].astype(np.float64).reshape(-1, 3)
    los = [c - R[:, None]] if ns else []
    his = [c + R[:, None]] if ns else []
    if nb:
        los.append(bc - bh - (a_max + slack))
        his.append(bc + bh + (a_max + slack))
    lo, hi = np.concatenate(los).min(0), np.concatenate(his).max(0)
    if planar:                                             # 2-D robots query z = 0 only: one layer of cells (2-D boxes are "infinite" in z)
        lo[2], hi[2] = -0.5 * GRID_CELL, 0.5 * GRID_CELL
    if np.any(hi - lo > 1.0e5):
        return None
    pad = 1e-5 + 1e-6 * float(np.abs(np.concatenate([lo, hi])).max())     # the kernels take the cell from fp32 arithmetic on x
    edge = GRID_CELL_MIN
    while edge < 4.0:
        fits = [(1, np.float32(1.0 / GRID_CELL), 0) if (planar and ax == 2) else _fit_axis(float(lo[ax]), float(hi[ax]), edge) for ax in range(3)]
        if all(f is not None for f in fits) and int(np.prod([f[0] for f in fits])) <= GRID_MAX_CELLS:
            dims = np.array([f[0] for f in fits], dtype=np.int64)
            inv32 = np.array([f[1] for f in fits], dtype=np.float32)
            K = np.array([f[2] for f in fits], dtype=np.int64)
            cell_eff = 1.0 / inv32.astype(np.float64)
            if not (np.abs(K).max() + dims.max() >= (1 << 16) or abs(int(K[0] + dims[0] * (K[1] + dims[1] * K[2]))) + int(dims.prod()) >= (1 << 21)):
                lo_s = (K - 0.5) * cell_eff
                ix = [np.arange(d) for d in dims]
                X, Y, Z = np.meshgrid(ix[0], ix[1], ix[2], indexing='ij')
                cmin = lo_s + np.stack([X, Y, Z], -1) * cell_eff          # (nx, ny, nz, 3)
                cmax = cmin + cell_eff
                hit_s = np.zeros((*dims, ns), dtype=bool)
                for o in range(ns):
                    d = np.maximum(np.maximum(cmin - c[o], c[o] - cmax), 0.0)
                    hit_s[..., o] = (d * d).sum(-1) < (R[o] + pad) ** 2
                hit_b = np.zeros((*dims, nb), dtype=bool)
                for o in range(nb):                                           # distance between the cell and the box, both axis aligned
                    d = np.maximum(np.maximum(cmin - (bc[o] + bh[o]), (bc[o] - bh[o]) - cmax), 0.0)
                    hit_b[..., o] = (d * d).sum(-1) < (a_max + slack + pad) ** 2
                cs, cb = hit_s.sum(-1), hit_b.sum(-1)
                over = (cs > LIST_CELL_MAX_SPH) | (cb > LIST_CELL_MAX_BOX)
                total = int((cs + cb)[~over].sum())
                if total <= LIST_MAX_CAND and total <= LIST_START_MASK:
                    # cell words in x-fastest order, candidates in ascending index order (spheres, then boxes)
                    order = (2, 1, 0)
                    ncl = int(dims.prod())
                    hs = np.ascontiguousarray(hit_s.transpose(*order, 3)).reshape(ncl, ns)
                    hbx = np.ascontiguousarray(hit_b.transpose(*order, 3)).reshape(ncl, nb)
                    ov = np.ascontiguousarray(over.transpose(*order)).reshape(-1)
                    words = np.zeros(hs.shape[0], dtype=np.uint32)
                    cand = []
                    pos = 0
                    for i in range(hs.shape[0]):
                        if ov[i]:
                            words[i] = LIST_OVERFLOW
                            continue
                        si, bi = np.nonzero(hs[i])[0], np.nonzero(hbx[i])[0]
                        words[i] = pos | (len(si) << LIST_NSPH_SHIFT) | (len(bi) << LIST_NBOX_SHIFT)
                        cand.extend(si.tolist())
                        cand.extend(bi.tolist())
                        pos += len(si) + len(bi)
                    cand = np.asarray(cand + [0] * ((-len(cand)) % 16 or (16 if not cand else 0)), dtype=np.uint8)
                    k_lin = int(K[0] + dims[0] * (K[1] + dims[1] * K[2]))
                    return dict(dims=dims.astype(np.int32), lo=lo_s.astype(np.float32), inv=inv32, words=words, cand=cand, k_lin=k_lin, K=K,
                                stats=dict(cell=float(cell_eff.max()), mean_sph=float(cs.mean()), max_sph=int(cs.max()), mean_box=float(cb.mean()),
                                           max_box=int(cb.max()), overflow=int(over.sum()), cand_bytes=total))
        edge /= GRID_REFINE
    return None


def build_grid(spheres, a_max, slack=1e-4, planar=False):
    """Uniform broad-phase grid over the inflated obstacle spheres (host, fp64).  None when there are no
    spheres or more than 254 of them (8-bit indices)."""
    n = len(spheres)
    if n == 0 or n > 254:
        return None
    c = spheres[:, :3].astype(np.float64)
    R = spheres[:, 3].astype(np.float64) + a_max + slack      # a sphere at x can matter only if |x - c| < R
    lo = (c - R[:, None]).min(0)
    hi = (c + R[:, None]).max(0)
    # Cells on a LATTICE through the world origin (geometry version 6): cell ix of an axis is [(K + ix - 1/2) h, (K + ix + 1/2) h)
    # with integer K, i.e. round-to-nearest(x / h) - K -- which a kernel gets from ONE fma(x, 1/h, 1.5 * 2^23) (the integer lands
    # in the low mantissa bits) where floor((x - lo) / h) took an fma with three register sources and a convert
    # (csrc/mpb_geom.h, grid_cell_rel).  Per axis the smallest cell count n whose lattice-aligned edge h (the smallest h >=
    # extent / n for which some lattice position covers [lo, hi]) does not exceed the target edge; the target goes from
    # GRID_CELL down to GRID_CELL_MIN while the grid still fits GRID_MAX_CELLS words of LDS: finer cells list fewer
    # obstacles each, and the kernels' candidate loop runs max-over-the-wave(candidates) times (C3: 17 x 15 x 16 cells of
    # ~0.12 m -> 1.27 trips per group of four collision spheres); planar problems get one layer of cells along z.
    flat = [planar and ax == 2 and np.ptp(c[:, ax]) == 0.0 for ax in range(3)]     # 2-D robots: every query point has z = 0

    def fit_axis(a, b, edge):
        """(n, h32, K): fewest cells of a lattice-aligned edge <= `edge` that cover [a, b]"""
        n = max(int(np.ceil((b - a) / edge)), 1)
        while n <= GRID_MAX_DIM:
            h = (b - a) / n
            while h <= edge * (1.0 + 1e-9):
                inv32 = np.float32(1.0 / h)
                he = 1.0 / float(inv32)                      # the edge the kernels effectively use
                K = int(np.floor(a / he + 0.5))              # (K - 1/2) he <= a
                if (K - 0.5 + n) * he >= b:
                    return n, inv32, K
                h *= 1.0 + 2e-4
            n += 1
        return None

    def lattice(edge):
        fits = []
        for ax in range(3):
            if flat[ax]:                                     # one layer of cells, the one that holds the plane z = 0
                fits.append((1, np.float32(1.0 / edge), 0))
                continue
            f = fit_axis(float(lo[ax]), float(hi[ax]), edge)
            if f is None:
                return None
            fits.append(f)
        return fits
    edge = GRID_CELL
    fits = lattice(edge)
    while edge * GRID_REFINE >= GRID_CELL_MIN:
        t = lattice(edge * GRID_REFINE)
        if t is None or int(np.prod([f[0] for f in t])) > GRID_MAX_CELLS:
            break
        edge *= GRID_REFINE
        fits = t
    while fits is None or int(np.prod([f[0] for f in fits])) > GRID_MAX_CELLS:      # (GRID_CELL itself too fine for a very large scene: coarsen)
        edge /= GRID_REFINE
        fits = lattice(edge)
    dims = np.array([f[0] for f in fits], dtype=np.int64)
    inv32 = np.array([f[1] for f in fits], dtype=np.float32)
    K = np.array([f[2] for f in fits], dtype=np.int64)
    cell_eff = 1.0 / inv32.astype(np.float64)
    # the kernels hold round(x / h) and the linear lattice index exactly in fp32 (integers below 2^22) and resolve a cell at
    # |x| / h only while fp32 does: a scene that far from the origin gets no grid (the exhaustive evaluators serve it)
    if np.abs(K).max() + dims.max() >= (1 << 16) or abs(int(K[0] + dims[0] * (K[1] + dims[1] * K[2]))) + int(dims.prod()) >= (1 << 21):
        return None
    lo_s = (K - 0.5) * cell_eff
    lo32 = lo_s.astype(np.float32)
    # the kernels take the cell from fp32 arithmetic on x: a point within ~1e-5 of a cell face may land in the neighbour --
    # added to R, with the fp32 rounding of large coordinates
    Rg = R + 1e-5 + 1e-6 * np.abs(np.concatenate([lo, hi])).max()
    ix = [np.arange(d) for d in dims]
    X, Y, Z = np.meshgrid(ix[0], ix[1], ix[2], indexing='ij')
    cmin = lo_s + np.stack([X, Y, Z], -1) * cell_eff          # (nx,ny,nz,3)
    cmax = cmin + cell_eff
    counts = np.zeros(dims, dtype=np.int64)
    lists = np.full((*dims, GRID_SLOTS), n, dtype=np.uint32)      # empty slot = n: the far dummy the kernels append to the table
    for o in range(n):
        d = np.maximum(np.maximum(cmin - c[o], c[o] - cmax), 0.0)
        hit = (d * d).sum(-1) < Rg[o] ** 2
        idx = np.nonzero(hit)
        k = counts[idx]
        ok = k < GRID_SLOTS
        sel = tuple(a[ok] for a in idx)
        lists[sel + (k[ok],)] = o
        counts[idx] += 1
    w = lists[..., 0]
    for k in range(1, GRID_SLOTS):
        w = w | (lists[..., k] << (GRID_SLOT_BITS * k))
    w = np.where(counts > GRID_SLOTS, np.uint32(GRID_OVERFLOW), w.astype(np.uint32))
    words = np.ascontiguousarray(w.transpose(2, 1, 0)).reshape(-1).astype(np.uint32)   # x fastest
    k_lin = int(K[0] + dims[0] * (K[1] + dims[1] * K[2]))     # linear index of the lattice point (Kx, Ky, Kz): header word k_lin
    return dict(dims=dims.astype(np.int32), lo=lo32, inv=inv32, words=words, k_lin=k_lin, K=K,
                stats=dict(mean=float(counts.mean()), max=int(counts.max()), overflow=int((counts > GRID_SLOTS).sum())))


def links_that_can_touch(rs, fs, slack=1e-4):
    """Static broad phase at pack time (serial chains): a collision sphere riding on frame 1 moves on a circle about the
    first joint axis whatever the trajectory does; when that circle keeps farther than margin + r_link (+ slack) from
    every obstacle its hinge is exactly zero for every configuration, and the sphere can be left out of the link table
    -- cost and gradient are unchanged bit for bit (x + 0).  Base links are the typical case (nothing is placed inside
    the robot's pedestal).  Returns a boolean keep-mask over the robot's collision spheres; spheres on later frames are
    always kept (their reach depends on several joints)."""
    n_links = len(rs['link_radius'])
    keep = np.ones(n_links, dtype=bool)
    if rs['kind'] != KIND_CHAIN:
        return keep
    P0 = np.asarray(rs['joint_tf'][0], dtype=np.float64)            # frame 1 = P0 * Rz(q0)
    R0, t0 = P0[:, :3], P0[:, 3]
    n = R0[:, 2]                                                     # joint axis in the world
    sph = np.asarray(fs['spheres'], dtype=np.float64).reshape(-1, 4)
    box = np.asarray(fs['boxes'], dtype=np.float64).reshape(-1, 6)
    cen = np.concatenate([sph[:, :3], box[:, :3]], 0)
    rad = np.concatenate([sph[:, 3], np.linalg.norm(box[:, 3:6], axis=1)], 0)     # boxes: bounding sphere
    for l in range(n_links):
        if int(rs['link_frame'][l]) != 1:
            continue
        o = np.asarray(rs['link_offset'][l], dtype=np.float64)
        a0 = t0 + R0 @ np.array([0.0, 0.0, o[2]])                   # centre of the circle
        rho = float(np.hypot(o[0], o[1]))
        v = cen - a0
        h = v @ n
        rperp = np.linalg.norm(v - h[:, None] * n[None, :], axis=1)
        dist = np.sqrt((rperp - rho) ** 2 + h ** 2)                 # obstacle centre to the circle
        thr = float(fs['margin']) + float(rs['link_radius'][l]) + slack
        if np.all(dist - rad > thr):
            keep[l] = False
    if not keep.any():
        keep[-1] = True                                              # the kernels want at least one link
    return keep


def hinge_bound(rs, fs):
    """Upper bound of a hinge margin + r_l - sdf of the scene: the signed distance to a sphere is >= -radius, to a box >= -(its
    smallest half extent)."""
    deepest = 0.0
    if len(fs['spheres']):
        deepest = max(deepest, float(np.max(np.asarray(fs['spheres'])[:, 3])))
    if len(fs['boxes']):
        deepest = max(deepest, float(np.max(np.min(np.asarray(fs['boxes'])[:, 3:6], axis=1))))
    return float(fs['margin']) + float(np.max(rs['link_radius'])) + deepest


def field_needs_list_grid(field):
    """The compact broad-phase grid (geometry version 6) serves up to GRID_MAX_SPH obstacle spheres; beyond that a field takes the
    list grid of version 7 where it fits."""
    return len(field.spec()['spheres']) > GRID_MAX_SPH


def pack_geometry(robot, field, scales=None, prune_static=True, use_model=True, list_grid=None):
    """Pack robot + collision field(s) into the flat fp32 word buffer the HIP kernels read.

    use_model: tag the buffer with the compile-time robot model its tables equal (model_gen.py), which lets the
    kernels take their unrolled chain walk; False keeps the generic table-driven walk (same bits; tests compare them).

    prune_static: leave out the collision spheres that can never come within their hinge threshold of this field's
    obstacles (links_that_can_touch); the per-sphere entry points (mpb_fk_collision_points, mpb_field_cost_points) need
    the full table: pack with prune_static=False for them.

    `field` may be a list of up to MAX_FIELDS CollisionFields (the reference builds one CostCollision per field,
    gpmp2.py:70-78, and sums them): the per-field buffers are chained, header word `next` of each holding the word
    offset to the next one (0 = last) and `fscale` a per-field scale s_f -- every kernel evaluates
    sum_f s_f * cost_f(q) (and its gradient) by walking the chain.

    Layout (32-bit words; ints stored bit-exact): the header is HEADER_WORDS at the top of this module (read one with header(), walk a
    chain with fields(); the C side has the same words as MPB_GW_* of include/mpb_geom_layout.h, generated from that table), `model` set
    only when the robot's tables equal the model's bit for bit.  The sections follow in this order:
      joint_tf    : n_frames_tf x 12   (row-major 3x4)
      links       : n_links x 8        (frame:int, ox, oy, oz, radius, 0, 0, 0)
      spheres     : n_spheres x 4      (cx, cy, cz, r)
      boxes       : n_boxes x 8        (cx, cy, cz, 0, hx, hy, hz, 0)
      cull        : ceil4(n_spheres) x 8 (-2cx, -2cy, -2cz, rhs, cx, cy, cz, r): a link sphere at x can
                    touch obstacle o only if |x|^2 - 2 x.c < rhs_o = (margin + max_l r_l + r_o)^2 - |c|^2 + slack
                    (3 fma + 1 compare per pair; the exact distance is evaluated only when a lane passes).
                    Padding entries never pass (rhs = -1e30).
      frame_start : n_frames + 1 ints (padded to 4): links [fs[j], fs[j+1]) ride on frame j+1
      grid        : nx*ny*nz uint32 words, x fastest (section zero-padded to a multiple of GRID_PAD words).  Broad phase for the obstacle spheres: a
                    word packs up to GRID_SLOTS obstacle indices (n_spheres = none: the far dummy) -- exactly the obstacles whose ball inflated
                    by (margin + max_l r_l + slack) touches the cell; GRID_OVERFLOW when more do.
                    A collision sphere at x can only be within its hinge threshold of the obstacles listed
                    in the cell containing x (none outside the grid), so per-LANE culling is exact.
                    version GEOM_VERSION_LIST: a LIST grid instead (build_list_grid), whose candidate bytes -- total - off_grid - the padded
                    cell words, in words -- follow the padded cell words.
    """
    if isinstance(field, (list, tuple)):
        fields = list(field)
        assert 1 <= len(fields) <= MAX_FIELDS, f'1..{MAX_FIELDS} collision fields per geometry buffer'
        scales = [1.0] * len(fields) if scales is None else [float(v) for v in scales]
        assert len(scales) == len(fields)
        # (the persistent kernel stages ONE grid format per launch: when any field needs the list grid, all of them take it)
        want_list = any(field_needs_list_grid(f) for f in fields) if list_grid is None else bool(list_grid)
        parts = [pack_geometry(robot, f, scales=[sc], prune_static=prune_static, use_model=use_model, list_grid=want_list)
                 for f, sc in zip(fields, scales)]
        for part in parts[:-1]:
            header(part)['next'] = part.size
        return np.concatenate(parts)
    if isinstance(field, MovingObstacleField):
        raise TypeError('a MovingObstacleField has no place in a geometry buffer (its centres carry a row axis): pack it with '
                        'pack_moving_obstacles / ops.DeviceMovingObstacles, or freeze it with field.at(t)')
    rs, fs = robot.spec(), field.spec()
    from . import model_gen
    model_id, keep_mask = 0, 0
    for name, mid in model_gen.MODEL_IDS.items():
        if use_model and model_gen.matches_model(rs, name):
            model_id, keep_mask = mid, (1 << len(rs['link_radius'])) - 1
    if model_id and hinge_bound(rs, fs) >= 1.0:
        # the model kernels take relu(hinge) as the [0, 1] clamp of the instruction encoding (csrc/mpb_geom.h, UNIT): a scene
        # whose hinges could reach 1 m keeps the table-driven walk
        model_id, keep_mask = 0, 0
    if prune_static and rs['kind'] == KIND_CHAIN:
        keep = links_that_can_touch(rs, fs)
        if model_id:
            keep_mask = int(sum(1 << l for l in range(len(keep)) if keep[l]))
            if np.any(np.asarray(rs['link_frame'])[~keep] != 1):      # the model kernels only expect frame-1 spheres to go
                model_id, keep_mask = 0, 0
        if not keep.all():
            rs = dict(rs, link_frame=np.asarray(rs['link_frame'])[keep], link_offset=np.asarray(rs['link_offset'])[keep],
                      link_radius=np.asarray(rs['link_radius'])[keep])
    n_tf = rs['joint_tf'].shape[0]
    n_links = len(rs['link_radius'])
    n_sph, n_box = len(fs['spheres']), len(fs['boxes'])
    n_sph_pad = (n_sph + 3) // 4 * 4
    n_frames = max(n_tf, 1)
    n_fs = (n_frames + 1 + 3) // 4 * 4
    off_tf = GEOM_HEADER_WORDS
    off_links = off_tf + 12 * n_tf
    off_sph = off_links + 8 * n_links
    off_box = off_sph + 4 * n_sph
    off_cull = off_box + 8 * n_box
    off_fs = off_cull + 8 * n_sph_pad
    off_grid = off_fs + n_fs
    planar = (rs['kind'] == KIND_POINT and rs['n_dof'] == 2 and (len(fs['spheres']) == 0 or bool(np.all(np.asarray(fs['spheres'])[:, 2] == 0.0))))
    a_max_g = float(fs['margin']) + float(np.max(rs['link_radius']))
    want_list = field_needs_list_grid(field) if list_grid is None else bool(list_grid)
    grid, version = None, GEOM_VERSION
    if want_list:
        grid = build_list_grid(np.asarray(fs['spheres']).reshape(-1, 4), np.asarray(fs['boxes']).reshape(-1, 6), a_max_g, planar=planar)
        if grid is not None:
            version = GEOM_VERSION_LIST
    if grid is None:
        grid = build_grid(fs['spheres'], a_max_g, planar=planar)
    n_cells = 0 if grid is None else int(grid['words'].size)
    n_cand_words = int(grid['cand'].size) // 4 if version == GEOM_VERSION_LIST else 0
    off_cand = off_grid + (n_cells + GRID_PAD - 1) // GRID_PAD * GRID_PAD   # the cell words are staged by the kernels in whole 16-byte rounds
    total = off_cand + n_cand_words
    buf = np.zeros((total,), dtype=np.float32)
    ibuf = buf.view(np.int32)
    written = dict(magic=GEOM_MAGIC, version=version, kind=rs['kind'], n_dof=rs['n_dof'], n_tf=n_tf, n_links=n_links, n_sph=n_sph, n_box=n_box,
                   margin=fs['margin'], off_tf=off_tf, off_links=off_links, off_sph=off_sph, off_box=off_box, total=total, off_cull=off_cull,
                   off_fs=off_fs, off_grid=off_grid, next=0, fscale=1.0 if scales is None else float(scales[0]), model=model_id,
                   keep_mask=keep_mask)
    if grid is not None:
        written.update(grid_dims=grid['dims'], grid_lo=grid['lo'], grid_inv=grid['inv'], n_cells=n_cells, k_lin=grid['k_lin'])
    hdr = header(buf)
    for name, value in written.items():
        hdr[name] = value
    if grid is not None:
        buf.view(np.uint32)[off_grid:off_grid + n_cells] = grid['words']
        if version == GEOM_VERSION_LIST:
            buf.view(np.uint8)[4 * off_cand:4 * off_cand + grid['cand'].size] = grid['cand']
    buf[off_tf:off_links] = rs['joint_tf'].astype(np.float32).reshape(-1)
    links = np.zeros((n_links, 8), np.float32)
    links.view(np.int32)[:, 0] = rs['link_frame'] if rs['kind'] == KIND_CHAIN else 1
    links[:, 1:4] = rs['link_offset']
    links[:, 4] = rs['link_radius']
    buf[off_links:off_sph] = links.reshape(-1)
    buf[off_sph:off_box] = fs['spheres'].reshape(-1)
    boxes = np.zeros((n_box, 8), np.float32)
    if n_box:
        boxes[:, 0:3] = fs['boxes'][:, 0:3]
        boxes[:, 4:7] = fs['boxes'][:, 3:6]
    buf[off_box:off_cull] = boxes.reshape(-1)
    # conservative cull table (fp64 on the host, rounded up)
    cull = np.zeros((n_sph_pad, 8), np.float32)
    cull[:, 3] = -1.0e30
    cull[:, 4:7] = -1.0e9   # (parked link slots sit at +1e9: never near a padding obstacle)
    if n_sph:
        c = fs['spheres'][:, :3].astype(np.float64)
        r = fs['spheres'][:, 3].astype(np.float64)
        a_max = float(fs['margin']) + float(np.max(rs['link_radius']))
        T = a_max + r
        cc = (c * c).sum(1)
        cmax = float(np.sqrt(cc.max()))
        slack = 2.0 ** -20 * (2.0 * cmax + float(T.max())) ** 2 + 1e-7   # 4x the fp32 error of the test value
        rhs = T * T - cc + slack
        cull[:n_sph, 0:3] = (-2.0 * c).astype(np.float32)
        cull[:n_sph, 3] = np.nextafter(rhs.astype(np.float32), np.float32(np.inf))
        cull[:n_sph, 4:7] = fs['spheres'][:, :3]
        cull[:n_sph, 7] = fs['spheres'][:, 3]
    buf[off_cull:off_fs] = cull.reshape(-1)
    fstart = np.zeros((n_fs,), np.int32)
    if rs['kind'] == KIND_CHAIN:
        lf = np.asarray(rs['link_frame'])
        for j in range(n_frames + 1):
            fstart[j] = int(np.searchsorted(lf, j + 1, side='left'))
        fstart[n_frames + 1:] = n_links
    else:
        fstart[0], fstart[1:] = 0, n_links
    ibuf[off_fs:off_grid] = fstart
    return buf


def count_fields(packed):
    """Number of chained fields in a packed geometry buffer."""
    return sum(1 for _ in fields(packed))


# ----------------------------------------------------------------------------------------------
# Synthetic environments for BASELINE.md configs (stand-ins for torch_robotics environments)
# ----------------------------------------------------------------------------------------------

def env_grid_circles_2d(margin=0.005, radius=0.05, n=7, extent=0.75):
    """C1: n x n grid of circles on [-extent, extent]^2 (stand-in for EnvGridCircles2D)."""
    xs = np.linspace(-extent, extent, n)
    c = np.array([(x, y, radius) for x in xs for y in xs], dtype=np.float32)
    return CollisionField(spheres=c, margin=margin)


def env_dense_2d(seed=3, n_circles=32, n_boxes=8, margin=0.01):
    """C2: random circles + boxes in [-1,1]^2, sizes U[0.05,0.15] (stand-in for EnvDense2D)."""
    rng = np.random.RandomState(seed)
    circles = np.concatenate([rng.uniform(-1, 1, (n_circles, 2)), rng.uniform(0.05, 0.15, (n_circles, 1))], 1)
    boxes = np.concatenate([rng.uniform(-1, 1, (n_boxes, 2)), rng.uniform(0.05, 0.15, (n_boxes, 2))], 1)
    return CollisionField(spheres=circles.astype(np.float32), boxes=boxes.astype(np.float32), margin=margin)


def env_spheres_3d(seed=0, n_spheres=16, margin=0.05):
    """C3/C4/C5: random spheres r U[0.05,0.15], centres U[-0.8,0.8]^3, none within 0.2 of the base axis."""
    rng = np.random.RandomState(seed)
    out = []
    while len(out) < n_spheres:
        c = rng.uniform(-0.8, 0.8, 3)
        r = rng.uniform(0.05, 0.15)
        if math.hypot(c[0], c[1]) - r < 0.2:
            continue
        out.append((c[0], c[1], c[2], r))
    return CollisionField(spheres=np.array(out, np.float32), margin=margin)


def env_spheres_boxes_3d(seed=0, n_spheres=200, n_boxes=32, margin=0.04):
    """A crowded 3-D scene (round 6): spheres r U[0.04, 0.12] and boxes with half extents U[0.03, 0.10], centres U[-0.8, 0.8]^3, none
    within 0.25 of the base axis -- beyond the compact broad-phase grid (63 spheres), so pack_geometry gives it the LIST grid of
    geometry version 7."""
    rng = np.random.RandomState(seed)
    sph, box = [], []
    while len(sph) < n_spheres:
        c, r = rng.uniform(-0.8, 0.8, 3), rng.uniform(0.04, 0.12)
        if math.hypot(c[0], c[1]) - r > 0.25:
            sph.append((*c, r))
    while len(box) < n_boxes:
        c, h = rng.uniform(-0.8, 0.8, 3), rng.uniform(0.03, 0.10, 3)
        if math.hypot(c[0], c[1]) - math.hypot(h[0], h[1]) > 0.25:
            box.append((*c, *h))
    return CollisionField(spheres=np.array(sph, np.float32), boxes=np.array(box, np.float32) if n_boxes else None, margin=margin)
