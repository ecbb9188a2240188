"""Tensor-level wrappers over the C-ABI: take PyTorch-ROCm tensors, pass raw device pointers + the
current HIP stream.  PyTorch is plumbing here (device memory, streams); all arithmetic is in
csrc/*.hip.  Every wrapper validates device / dtype / contiguity / shape on the host before
launching (a kernel that faults can reset the whole GPU host).
"""
import collections
import ctypes
import functools
import math
import warnings

import numpy as np
import torch

from . import _lib, blend_layout, certify_layout, path_timing_layout, rrt_layout, st_certify_layout, st_shortcut_layout, strrt_layout
from .geometry import KIND_CHAIN, MAX_FIELDS, CollisionField, TriangleMesh, count_fields, mesh_pose, occupancy_bytes, pack_geometry, pack_mesh, pack_moving_obstacles, pack_sdf_grid, pack_self_collision
from .geometry import header as geometry_header


# the raw handle of a device's current stream: torch.cuda.current_stream(dev).cuda_stream builds a Stream object per call (~2.5 us,
# a quarter of the host side of a persistent STOMP call); torch keeps the raw getter its own launchers use
_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def raw_stream(device_index):
    if _raw_stream is not None:
        return _raw_stream(device_index)
    return torch.cuda.current_stream(device_index).cuda_stream


def _stream():
    # called inside _on_tensor_device: the current device is the tensors' device
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _on_tensor_device(fn):
    """Every wrapper launches on the device its tensors live on, on THAT device's current stream: all GPU tensor
    arguments (a DeviceGeometry counts through its buffer) must share one device, which becomes the current device for
    the duration of the call.  Without this a planner built for cuda:1 while cuda:0 is current would launch on GPU 0
    with GPU-1 pointers."""
    @functools.wraps(fn)
    def run(*args, **kw):
        dev = None
        for a in list(args) + list(kw.values()):
            t = a.buf if isinstance(a, (DeviceGeometry, _DeviceMemberBuffer, DeviceWorld)) else a
            if isinstance(t, torch.Tensor) and t.is_cuda:
                if dev is None:
                    dev = t.device
                elif t.device != dev:
                    raise ValueError(f'{fn.__name__}: tensor arguments live on different devices ({dev} and {t.device})')
        if dev is None:
            return fn(*args, **kw)       # no GPU tensor: the shape / device checks of the wrapper raise
        with torch.cuda.device(dev):
            return fn(*args, **kw)
    return run


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _seed64(seed):
    return int(seed) & (2 ** 64 - 1)


def _chk(t, shape, name, allow_none=False, dtype=torch.float32):
    if t is None:
        if allow_none:
            return
        raise ValueError(f'{name} is required')
    if not t.is_cuda:
        raise ValueError(f'{name} must live on the GPU (got {t.device}); there is no CPU path')
    if t.dtype != dtype:
        raise ValueError(f'{name} must be {str(dtype).split(".")[-1]} (got {t.dtype})')
    if not t.is_contiguous():
        raise ValueError(f'{name} must be contiguous')
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f'{name} has shape {tuple(t.shape)}, expected {tuple(shape)}')


class DeviceGeometry:
    """Packed robot + field geometry resident in HBM (one small fp32 buffer)."""

    def __init__(self, robot, field, device, scales=None, keep_all_links=False, use_model=True):
        """`field`: one CollisionField or a list of up to 4 (evaluated as sum_f scales[f] * cost_f).
        keep_all_links: pack every collision sphere of the robot (needed by the per-sphere entry points
        fk_collision_points / field_cost_points); by default spheres that can never reach an obstacle of the field are
        left out of the link table (geometry.links_that_can_touch: exact, cost and gradient unchanged)."""
        self.robot, self.field = robot, field
        self._adopt(pack_geometry(robot, field, scales=scales, prune_static=not keep_all_links, use_model=use_model), device)
        self.all_links = self.n_links == len(robot.spec()['link_radius']) and (
            not isinstance(field, (list, tuple)) or keep_all_links or len(field) == 1)

    @classmethod
    def from_packed(cls, packed, device):
        self = cls.__new__(cls)
        self.robot = self.field = None
        self._adopt(np.ascontiguousarray(packed, dtype=np.float32), device)
        self.all_links = True
        return self

    def _adopt(self, host, device):
        """Check the packed buffer, read what the entry points ask of its (first) header once, and put it on the device."""
        _lib.geom_check(host)
        self.flags = _lib.geom_flags(host)
        self.host = host
        hdr = geometry_header(host)
        self.n_dof, self.n_links, self.kind = int(hdr['n_dof']), int(hdr['n_links']), int(hdr['kind'])
        self.n_fields = count_fields(host)
        self.buf = torch.from_numpy(host.copy()).to(device)


class _DeviceMemberBuffer:
    """What the buffers of the cost members with kernels of their own share: the packed robot + field in HBM as `buf`, the robot's `n_dof`,
    and the library's cached header dropped for the address on upload (INVALIDATE); MEMBER_OPS below says which wrappers serve which."""
    INVALIDATE = None

    def _adopt(self, buf):
        self.buf = buf
        # (the library reads such a buffer's header once per address: this address may have held another one before)
        _lib.check(getattr(_lib.lib(), self.INVALIDATE)(_ptr(buf)), self.INVALIDATE)


class DeviceSelfCollision(_DeviceMemberBuffer):
    """A chain + its SelfCollisionField as the packed self buffer (geometry.pack_self_collision) resident in HBM: packed, validated
    (mpb_self_check) and uploaded once."""
    INVALIDATE = 'mpb_self_invalidate'

    def __init__(self, robot, field, device):
        from .self_layout import header as self_header
        self.robot, self.field = robot, field
        self.host = pack_self_collision(robot, field)
        _lib.self_check(self.host)
        hdr = self_header(self.host)
        self.n_dof, self.n_links, self.n_pairs = int(hdr['n_dof']), int(hdr['n_links']), int(hdr['n_pairs'])
        self._adopt(torch.from_numpy(self.host.copy()).to(device))


def _cost_out(trajs, out, accumulate):
    """The (B,) sums a cost wrapper writes: the caller's `out`, checked, or a fresh one (which nothing can be accumulated onto)."""
    B = trajs.shape[0]
    if out is None:
        if accumulate:
            raise ValueError('accumulate needs an existing out buffer')
        return torch.empty(B, device=trajs.device, dtype=torch.float32)
    if out.numel() != B:
        raise ValueError(f'out has {out.numel()} elements, expected {B}')
    _chk(out, out.shape, 'out')
    return out


# the three wrappers over a packed robot buffer (a _DeviceMemberBuffer `mb`), by C entry point and the robot's noun
def _row_cost_eval(symbol, noun, trajs, mb, k_sigma, weight, h_begin, per_waypoint, out, accumulate):
    B, H, d = trajs.shape
    _chk(trajs, (B, H, d), 'trajs')
    if d < mb.n_dof:
        raise ValueError(f'trajs has {d} columns, the {noun} {mb.n_dof} degrees of freedom')
    out = _cost_out(trajs, out, accumulate)
    pw = torch.empty(B, H, device=trajs.device, dtype=torch.float32) if per_waypoint else None
    _lib.check(getattr(_lib.lib(), symbol)(_ptr(trajs), _ptr(mb.buf), _ptr(out), _ptr(pw), B, H, d, int(h_begin), float(k_sigma), float(weight),
                                           int(bool(accumulate)), _stream()), symbol)
    return (out, pw) if per_waypoint else out


def _row_cost_grad(symbol, noun, trajs, mb, k_sigma, weight, h_begin, out, grad, accumulate):
    B, H, d = trajs.shape
    _chk(trajs, (B, H, d), 'trajs')
    if d < mb.n_dof:
        raise ValueError(f'trajs has {d} columns, the {noun} {mb.n_dof} degrees of freedom')
    if accumulate and grad is None:
        raise ValueError('accumulate needs existing out and grad buffers')
    out = _cost_out(trajs, out, accumulate)
    if grad is None:
        grad = torch.empty_like(trajs)
    else:
        _chk(grad, (B, H, d), 'grad')
    _lib.check(getattr(_lib.lib(), symbol)(_ptr(trajs), _ptr(mb.buf), _ptr(out), _ptr(grad), B, H, d, int(h_begin), float(k_sigma), float(weight),
                                           int(bool(accumulate)), _stream()), symbol)
    return out, grad


def _config_predicate(symbol, noun, q, mb, with_gap, flag, gap):
    N, D = q.shape
    _chk(q, (N, D), 'q')
    if D != mb.n_dof:
        raise ValueError(f'q has {D} columns, the {noun} {mb.n_dof} degrees of freedom')
    or_into = flag is not None
    if or_into:
        _chk(flag, (N,), 'flag', dtype=torch.bool)
        _chk(gap, (N,), 'gap', allow_none=True)
        if with_gap and gap is None:
            raise ValueError('with_gap next to flag= needs the gap= to add onto (the gap of collision_check(..., with_gap=True))')
    else:
        flag = torch.empty(N, device=q.device, dtype=torch.bool)
        gap = torch.empty(N, device=q.device, dtype=torch.float32) if with_gap else None
    _lib.check(getattr(_lib.lib(), symbol)(_ptr(q), _ptr(mb.buf), _ptr(flag), _ptr(gap), N, D, int(or_into), _stream()), symbol)
    return (flag, gap) if (with_gap or gap is not None) else flag


@_on_tensor_device
def self_collision_eval(trajs, sc, k_sigma, weight=1.0, h_begin=1, per_waypoint=False, out=None, accumulate=False):
    """trajs (B, H, d) -> out (B,) (+)= weight * k_sigma * sum_{h >= h_begin} c(q_h) of a DeviceSelfCollision
    (mpb_self_collision_eval); per_waypoint also returns c (B, H), un-scaled, 0 below h_begin."""
    return _row_cost_eval('mpb_self_collision_eval', 'chain', trajs, sc, k_sigma, weight, h_begin, per_waypoint, out, accumulate)


@_on_tensor_device
def self_collision_grad(trajs, sc, k_sigma, weight=1.0, h_begin=1, out=None, grad=None, accumulate=False):
    """(out (B,), grad (B, H, d)) (+)= the self-collision cost and d out / d trajs (mpb_self_collision_grad); accumulate adds onto the
    given `out` AND `grad` (velocity channels left alone), otherwise both are written (velocity channels 0)."""
    return _row_cost_grad('mpb_self_collision_grad', 'chain', trajs, sc, k_sigma, weight, h_begin, out, grad, accumulate)


@_on_tensor_device
def self_collision_check(q, sc, with_gap=False, flag=None, gap=None):
    """(N, D) configurations -> bool (N,): the robot collides with itself (mpb_self_collision_check); with_gap also returns the hinge
    sum.  Given `flag` (and `gap`) -- the outputs of collision_check --, the answer is ORed into the flags and added onto the gap."""
    return _config_predicate('mpb_self_collision_check', 'chain', q, sc, with_gap, flag, gap)


class DeviceSDFGrid(_DeviceMemberBuffer):
    """A robot + a GridSDFField as the packed SDF buffer (geometry.pack_sdf_grid) resident in HBM: packed, validated (mpb_sdf_grid_check)
    and uploaded once -- or, for a field without host values, the header and the robot tables uploaded and the nodes built ON the
    device from the field's source: a CollisionField (GridSDFField.from_field, mpb_sdf_grid_build), an occupancy voxel map
    (GridSDFField.from_occupancy, mpb_sdf_grid_build_occupancy: the bytes uploaded once, a GPU tensor used in place) or triangle meshes
    (GridSDFField.from_mesh, mpb_sdf_grid_build_mesh: each mesh packed and uploaded once as a DeviceMesh in `.meshes`, update_mesh
    rebuilds the nodes under new poses).  `.nodes` is the node section as a (nz, ny, nx) view of the buffer."""
    INVALIDATE = 'mpb_sdf_grid_invalidate'

    def __init__(self, robot, field, device):
        from .sdf_layout import header as sdf_header
        self.robot, self.field = robot, field
        built = field.values is None
        self.host = pack_sdf_grid(robot, field, with_nodes=not built)      # (built: the words before the node section only)
        hdr = sdf_header(self.host)
        total, off_nodes = int(hdr['total']), int(hdr['off_nodes'])
        _lib.sdf_grid_check(self.host, n_words=total)
        self.kind, self.n_dof, self.n_links = int(hdr['kind']), int(hdr['n_dof']), int(hdr['n_links'])
        self.dims = tuple(int(v) for v in hdr['dims'])
        if built:
            buf = torch.empty(total, device=device, dtype=torch.float32)
            buf[:off_nodes].copy_(torch.from_numpy(self.host))
        else:
            buf = torch.from_numpy(self.host).to(device)
        self._adopt(buf)
        nx, ny, nz = self.dims
        self.nodes = self.buf[off_nodes:].view(nz, ny, nx)
        if built and isinstance(field.source, CollisionField):
            from .geometry import RobotPointMass
            geom = DeviceGeometry(RobotPointMass(3), field.source, device, use_model=False)
            sdf_grid_build(geom, self)
        elif built and isinstance(field.source, list):
            self.meshes = [DeviceMesh(m, device) for m, _ in field.source]
            self._build_meshes([p for _, p in field.source])
        elif built:
            self.update_occupancy(field.source)

    def _build_meshes(self, poses):
        for n, (mesh, pose) in enumerate(zip(self.meshes, poses)):
            sdf_grid_build_mesh(mesh, self, pose=pose, combine=n > 0)
        return self.nodes

    def update_mesh(self, poses):
        """Rebuild the node section in place with the objects of a field made by GridSDFField.from_mesh under new poses: `poses` is one
        pose per object in the field's order ([R | t], mesh frame to grid frame, or None: as the mesh stands), or a single pose (an
        array) when the field has one object.  Nothing is packed again and nothing is uploaded but the 12 floats per object: the DeviceMesh buffers
        made at construction are read in place.  The field then holds the new poses in its `source`, so a DeviceSDFGrid made from it
        later builds THIS placement.  Returns `.nodes`."""
        if getattr(self, 'meshes', None) is None:
            raise ValueError('update_mesh: this grid was not built from meshes (GridSDFField.from_mesh)')
        if poses is None or tuple(getattr(poses, 'shape', ())) in ((3, 4), (4, 4)):      # a single pose (an array, or None)
            poses = [poses]
        poses = list(poses)
        if len(poses) != len(self.meshes):
            raise ValueError(f'update_mesh: {len(poses)} poses for {len(self.meshes)} objects')
        poses = [mesh_pose(p, 'DeviceSDFGrid.update_mesh') for p in poses]
        self.field.source = [(m, p) for (m, _), p in zip(self.field.source, poses)]
        return self._build_meshes(poses)

    def update_occupancy(self, occupancy):
        """Rebuild the node section in place from the next scan: an occupancy map of the same dimensions, as GridSDFField.from_occupancy
        takes it (a GPU tensor of uint8 / bool on the buffer's device is used in place, anything else becomes bytes and is uploaded;
        the bytes are only read, a read-only numpy array -- a memory-mapped scan -- is fine).  The header does not change.  A field made
        by from_occupancy then holds the new scan as its `source`, so a DeviceSDFGrid made from it later (another device, a
        PlanningTask built afterwards) builds THIS scan; under a field with host `values` or one made by from_field only this device
        buffer changes, the field keeps what it held; so does one made by from_mesh.  Returns `.nodes`."""
        occ = occupancy_bytes(occupancy, 'DeviceSDFGrid.update_occupancy')
        nx, ny, nz = self.dims
        if tuple(occ.shape) != (nz, ny, nx):
            raise ValueError(f'update_occupancy: occupancy of shape {tuple(occ.shape)}, the grid has (nz, ny, nx) = {(nz, ny, nx)}')
        if self.field.values is None and not isinstance(self.field.source, (CollisionField, list)):     # (a list: from_mesh)
            self.field.source = occ
        if not isinstance(occ, torch.Tensor):
            with warnings.catch_warnings():        # (torch warns that a read-only array could be written through the tensor: it is only uploaded)
                warnings.filterwarnings('ignore', message='The given NumPy array is not writable', category=UserWarning)
                occ = torch.from_numpy(occ)
        return sdf_grid_build_occupancy(occ.to(self.buf.device), self)


@_on_tensor_device
def sdf_grid_build(geom, sdf):
    """Fill the node section of a DeviceSDFGrid with min_o sdf_o(node position) of the ONE CollisionField of a DeviceGeometry
    (mpb_sdf_grid_build; any robot: only the obstacle tables are read)."""
    if geom.n_fields != 1:
        raise ValueError(f'sdf_grid_build takes the geometry of ONE CollisionField, this one chains {geom.n_fields}')
    _chk(geom.buf, geom.buf.shape, 'geom.buf')
    _chk(sdf.buf, sdf.buf.shape, 'sdf.buf')
    _lib.check(_lib.lib().mpb_sdf_grid_build(_ptr(geom.buf), _ptr(sdf.buf), _stream()), 'mpb_sdf_grid_build')
    return sdf.nodes


@_on_tensor_device
def sdf_grid_build_occupancy(occupancy, sdf):
    """Fill the node section of a DeviceSDFGrid from an occupancy voxel map: a contiguous uint8 or bool GPU tensor of shape (nz, ny, nx) on
    the buffer's device, element != 0 = solid, read only (mpb_sdf_grid_build_occupancy: the exact Euclidean distance transform, in
    place in the node section; include/mpb.h has the definition).  Returns sdf.nodes."""
    if not isinstance(occupancy, torch.Tensor) or occupancy.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f'occupancy must be a uint8 or bool tensor (got {getattr(occupancy, "dtype", type(occupancy))})')
    nx, ny, nz = sdf.dims
    _chk(occupancy, (nz, ny, nx), 'occupancy', dtype=occupancy.dtype)
    _chk(sdf.buf, sdf.buf.shape, 'sdf.buf')
    _lib.check(_lib.lib().mpb_sdf_grid_build_occupancy(_ptr(occupancy), _ptr(sdf.buf), _stream()), 'mpb_sdf_grid_build_occupancy')
    return sdf.nodes


class DeviceMesh(_DeviceMemberBuffer):
    """A TriangleMesh as the packed mesh buffer (geometry.pack_mesh) resident in HBM: packed, validated (mpb_mesh_check) and uploaded
    once; what mpb_sdf_grid_build_mesh reads.  (The library forgets both kinds of buffer an address held through mpb_sdf_grid_invalidate.)"""
    INVALIDATE = 'mpb_sdf_grid_invalidate'

    def __init__(self, mesh, device):
        from .mesh_layout import header as mesh_header
        if not isinstance(mesh, TriangleMesh):
            raise TypeError('DeviceMesh takes a geometry.TriangleMesh')
        self.mesh = mesh
        self.host = pack_mesh(mesh)
        _lib.mesh_check(self.host)
        hdr = mesh_header(self.host)
        self.n_tri, self.n_groups = int(hdr['n_tri']), int(hdr['n_groups'])
        self._adopt(torch.from_numpy(self.host.copy()).to(device))


@_on_tensor_device
def sdf_grid_build_mesh(mesh, sdf, pose=None, combine=False, cull=True):
    """Fill the node section of a DeviceSDFGrid with the exact (signed) distance to a DeviceMesh placed by `pose` ([R | t], mesh frame to
    grid frame, 3 x 4 or 4 x 4; None: as the mesh stands) -- mpb_sdf_grid_build_mesh, include/mpb.h has the definition.  combine: the
    node becomes min(what it holds, the new value) (MPB_MESH_MIN: the union with what was built before); cull=False visits every
    group of triangles (MPB_MESH_NO_CULL: the same bits, slower).  Returns sdf.nodes."""
    from .mesh_layout import MESH_MIN, MESH_NO_CULL
    if not isinstance(mesh, DeviceMesh) or not isinstance(sdf, DeviceSDFGrid):
        raise TypeError('sdf_grid_build_mesh takes a DeviceMesh and a DeviceSDFGrid')
    _chk(mesh.buf, mesh.buf.shape, 'mesh.buf')
    _chk(sdf.buf, sdf.buf.shape, 'sdf.buf')
    flags = (0 if cull else MESH_NO_CULL) | (MESH_MIN if combine else 0)
    P = mesh_pose(pose, 'sdf_grid_build_mesh')
    _lib.check(_lib.lib().mpb_sdf_grid_build_mesh(_ptr(mesh.buf), None if P is None else P.ctypes.data_as(ctypes.c_void_p), _ptr(sdf.buf),
                                                  int(flags), _stream()), 'mpb_sdf_grid_build_mesh')
    return sdf.nodes


@_on_tensor_device
def sdf_grid_sample(points, sdf, with_grad=False):
    """points (N, 3) -> s (N,) of the grid's interpolant, with_grad also d s / d x (N, 3) (mpb_sdf_grid_sample).  No robot."""
    N = points.shape[0]
    _chk(points, (N, 3), 'points')
    s = torch.empty(N, device=points.device, dtype=torch.float32)
    g = torch.empty(N, 3, device=points.device, dtype=torch.float32) if with_grad else None
    _lib.check(_lib.lib().mpb_sdf_grid_sample(_ptr(points), _ptr(sdf.buf), _ptr(s), _ptr(g), N, _stream()), 'mpb_sdf_grid_sample')
    return (s, g) if with_grad else s


@_on_tensor_device
def sdf_grid_eval(trajs, sdf, k_sigma, weight=1.0, h_begin=1, per_waypoint=False, out=None, accumulate=False):
    """trajs (B, H, d) -> out (B,) (+)= weight * k_sigma * sum_{h >= h_begin} c(q_h) of a DeviceSDFGrid (mpb_sdf_grid_eval);
    per_waypoint also returns c (B, H), un-scaled, 0 below h_begin."""
    return _row_cost_eval('mpb_sdf_grid_eval', 'robot', trajs, sdf, k_sigma, weight, h_begin, per_waypoint, out, accumulate)


@_on_tensor_device
def sdf_grid_grad(trajs, sdf, k_sigma, weight=1.0, h_begin=1, out=None, grad=None, accumulate=False):
    """(out (B,), grad (B, H, d)) (+)= the grid cost and d out / d trajs (mpb_sdf_grid_grad); accumulate adds onto the given `out` AND
    `grad` (velocity channels left alone), otherwise both are written (velocity channels 0)."""
    return _row_cost_grad('mpb_sdf_grid_grad', 'robot', trajs, sdf, k_sigma, weight, h_begin, out, grad, accumulate)


@_on_tensor_device
def sdf_grid_check(q, sdf, with_gap=False, flag=None, gap=None):
    """(N, D) configurations -> bool (N,): the grid cost of the configuration is positive (mpb_sdf_grid_collision_check); with_gap also
    returns the hinge sum.  Given `flag` (and `gap`) -- the outputs of collision_check --, the answer is ORed into the flags and added
    onto the gap."""
    return _config_predicate('mpb_sdf_grid_collision_check', 'robot', q, sdf, with_gap, flag, gap)


class DeviceMovingObstacles(_DeviceMemberBuffer):
    """A robot + a MovingObstacleField for trajectories of `n_rows` rows as the packed moving-obstacle buffer
    (geometry.pack_moving_obstacles) resident in HBM: packed, validated (mpb_moving_check) and uploaded once.  The buffer serves
    exactly that row count: the centres are evaluated per row from the field's clock."""
    INVALIDATE = 'mpb_moving_invalidate'

    def __init__(self, robot, field, device, n_rows):
        from .moving_layout import header as moving_header
        self.robot, self.field = robot, field
        self.host = pack_moving_obstacles(robot, field, n_rows)
        _lib.moving_check(self.host)
        hdr = moving_header(self.host)
        self.n_dof, self.n_links, self.n_rows = int(hdr['n_dof']), int(hdr['n_links']), int(hdr['n_rows'])
        self.n_spheres, self.n_boxes, self.off_centres = int(hdr['n_spheres']), int(hdr['n_boxes']), int(hdr['off_centres'])
        self._adopt(torch.from_numpy(self.host.copy()).to(device))

    def update(self, field):
        """The obstacles of another field of the SAME shapes (counts, radii, half extents, margin) -- typically field.shifted(dt), the
        receding-horizon step -- into the same device buffer: packed again on the host, only the centre section is uploaded, and the
        library's cached header for the address is dropped.  Returns self."""
        host = pack_moving_obstacles(self.robot, field, self.n_rows)
        o = self.off_centres
        if host.size != self.host.size or not np.array_equal(host[:o].view(np.uint32), self.host[:o].view(np.uint32)):
            raise ValueError('update: the field must keep the obstacle counts, radii, half extents and margin the buffer was packed with')
        _lib.moving_check(host)
        self.field, self.host = field, host
        self.buf[o:].copy_(torch.from_numpy(host[o:].copy()))
        _lib.check(getattr(_lib.lib(), self.INVALIDATE)(_ptr(self.buf)), self.INVALIDATE)
        return self


@_on_tensor_device
def moving_collision_eval(trajs, mo, k_sigma, weight=1.0, h_begin=1, per_waypoint=False, out=None, accumulate=False):
    """trajs (B, H, d), H == mo.n_rows -> out (B,) (+)= weight * k_sigma * sum_{h >= h_begin} c_h(q_h) of a DeviceMovingObstacles
    (mpb_moving_collision_eval); per_waypoint also returns c (B, H), un-scaled, 0 below h_begin."""
    return _row_cost_eval('mpb_moving_collision_eval', 'robot', trajs, mo, k_sigma, weight, h_begin, per_waypoint, out, accumulate)


@_on_tensor_device
def moving_collision_grad(trajs, mo, k_sigma, weight=1.0, h_begin=1, out=None, grad=None, accumulate=False):
    """(out (B,), grad (B, H, d)) (+)= the moving-obstacle cost and d out / d trajs (mpb_moving_collision_grad); accumulate adds onto the
    given `out` AND `grad` (velocity channels left alone), otherwise both are written (velocity channels 0)."""
    return _row_cost_grad('mpb_moving_collision_grad', 'robot', trajs, mo, k_sigma, weight, h_begin, out, grad, accumulate)


@_on_tensor_device
def moving_collision_check(trajs, mo, with_gap=False, flag=None, gap=None):
    """trajs (B, H, d), H == mo.n_rows -> bool (B, H): row h collides with the obstacles as they stand at its time
    (mpb_moving_collision_check); with_gap also returns the hinge sums (B, H).  Given `flag` (and `gap`), both (B, H), the answer is ORed
    into the flags and added onto the gap."""
    B, H, d = trajs.shape
    _chk(trajs, (B, H, d), 'trajs')
    if d < mo.n_dof:
        raise ValueError(f'trajs has {d} columns, the robot {mo.n_dof} degrees of freedom')
    or_into = flag is not None
    if or_into:
        _chk(flag, (B, H), 'flag', dtype=torch.bool)
        _chk(gap, (B, H), 'gap', allow_none=True)
        if with_gap and gap is None:
            raise ValueError('with_gap next to flag= needs the gap= to add onto')
    else:
        flag = torch.empty(B, H, device=trajs.device, dtype=torch.bool)
        gap = torch.empty(B, H, device=trajs.device, dtype=torch.float32) if with_gap else None
    _lib.check(_lib.lib().mpb_moving_collision_check(_ptr(trajs), _ptr(mo.buf), _ptr(flag), _ptr(gap), B, H, d, int(or_into), _stream()),
               'mpb_moving_collision_check')
    return (flag, gap) if (with_gap or gap is not None) else flag


# the wrappers that serve each member buffer, for the callers that hold one without caring which (CostCollision.own_eval / own_grad,
# PlanningTask's predicate)
MemberOps = collections.namedtuple('MemberOps', 'eval grad check')
MEMBER_OPS = {DeviceSelfCollision: MemberOps(self_collision_eval, self_collision_grad, self_collision_check),
              DeviceSDFGrid: MemberOps(sdf_grid_eval, sdf_grid_grad, sdf_grid_check),
              DeviceMovingObstacles: MemberOps(moving_collision_eval, moving_collision_grad, moving_collision_check)}   # (check: per ROW of (B, H, d))


@_on_tensor_device
def cost_collision_eval(trajs, geom, k_sigma, weight=1.0, h_begin=1, per_waypoint=False):
    B, H, d = trajs.shape
    _chk(trajs, (B, H, d), 'trajs')
    out = torch.empty(B, device=trajs.device, dtype=torch.float32)
    pw = torch.empty(B, H, device=trajs.device, dtype=torch.float32) if per_waypoint else None
    _lib.check(_lib.lib().mpb_cost_collision_eval(_ptr(trajs), _ptr(geom.buf), _ptr(out), _ptr(pw), B, H, d, h_begin,
                                                 float(k_sigma), float(weight), _stream()), 'mpb_cost_collision_eval')
    return (out, pw) if per_waypoint else out


@_on_tensor_device
def cost_collision_grad(trajs, geom, k_sigma, weight=1.0, h_begin=1, grad=None):
    B, H, d = trajs.shape
    _chk(trajs, (B, H, d), 'trajs')
    out = torch.empty(B, device=trajs.device, dtype=torch.float32)
    if grad is None:
        grad = torch.empty_like(trajs)
    else:
        _chk(grad, (B, H, d), 'grad')
    _lib.check(_lib.lib().mpb_cost_collision_grad(_ptr(trajs), _ptr(geom.buf), int(geom.flags), _ptr(out), _ptr(grad), B, H, d, h_begin,
                                                 float(k_sigma), float(weight), _stream()), 'mpb_cost_collision_grad')
    return out, grad


TERM_GP, TERM_START, TERM_GOAL, TERM_SMOOTH, TERM_JLIM, TERM_VEL_FD = 1, 2, 4, 8, 16, 32   # include/mpb.h MPB_TERM_*


def _term_flags(terms, B, n_dof, vel_fd, start_state, goal_states, trajs_per_goal, q_min, q_max):
    """MPB_TERM_* flags of the named cost terms, with the tensors each enabled term reads checked (cost_terms_eval / _grad)."""
    terms = set(terms or ())
    unknown = terms - {'gp', 'start', 'goal', 'smooth', 'jlim'}
    if unknown:
        raise ValueError(f'unknown cost terms {sorted(unknown)}')
    flags = 0
    if 'gp' in terms:
        flags |= TERM_GP | (TERM_VEL_FD if vel_fd else 0)
    if 'start' in terms:
        flags |= TERM_START
        _chk(start_state, (2 * n_dof,), 'start_state')
    if 'goal' in terms:
        flags |= TERM_GOAL
        if goal_states is None or goal_states.ndim != 2:
            raise ValueError('goal_states (G, 2*n_dof) is required')
        _chk(goal_states, (goal_states.shape[0], 2 * n_dof), 'goal_states')
        if trajs_per_goal < 1 or goal_states.shape[0] * trajs_per_goal < B:
            raise ValueError(f'{goal_states.shape[0]} goals x {trajs_per_goal} trajectories do not cover B={B}')
    if 'smooth' in terms:
        flags |= TERM_SMOOTH
    if 'jlim' in terms:
        flags |= TERM_JLIM
        _chk(q_min, (n_dof,), 'q_min')
        _chk(q_max, (n_dof,), 'q_max')
    return flags


@_on_tensor_device
def cost_terms_eval(trajs, n_dof, dt=0.0, k_gp=0.0, vel_fd=False, k_start=0.0, start_state=None, k_goal=0.0,
                    goal_states=None, trajs_per_goal=1, k_smooth=0.0, k_jlim=0.0, q_min=None, q_max=None, jl_eps=0.0,
                    out=None, accumulate=False, broadcast_jlim=True, terms=None):
    """One pass over trajs (B,H,d) evaluating the enabled trajectory-only cost terms (mpb_cost_terms_eval).
    A term is enabled by naming it in `terms` (iterable of 'gp','start','goal','smooth','jlim').
    Returns (out (B,), jl_total 0-dim fp64 tensor or None)."""
    B, H, d = trajs.shape
    _chk(trajs, (B, H, d), 'trajs')
    flags = _term_flags(terms, B, n_dof, vel_fd, start_state, goal_states, trajs_per_goal, q_min, q_max)
    jl_total = torch.zeros((), device=trajs.device, dtype=torch.float64) if flags & TERM_JLIM else None
    if out is None:
        if accumulate:
            raise ValueError('accumulate needs an existing out buffer')
        out = torch.empty(B, device=trajs.device, dtype=torch.float32)
    else:
        if out.numel() != B:
            raise ValueError(f'out has {out.numel()} elements, expected {B}')
        _chk(out, out.shape, 'out')
    _lib.check(_lib.lib().mpb_cost_terms_eval(
        _ptr(trajs), _ptr(out), _ptr(jl_total), _ptr(start_state), _ptr(goal_states), _ptr(q_min), _ptr(q_max),
        B, H, d, int(n_dof), int(trajs_per_goal), flags, float(dt), float(k_gp), float(k_start), float(k_goal),
        float(k_smooth), float(k_jlim), float(jl_eps), int(bool(accumulate)), int(bool(broadcast_jlim)), _stream()),
        'mpb_cost_terms_eval')
    return out, jl_total


def _need_all_links(geom):
    if not getattr(geom, 'all_links', True):
        raise ValueError('this geometry leaves out collision spheres that cannot reach an obstacle; the per-sphere entry '
                         'points need DeviceGeometry(..., keep_all_links=True)')


@_on_tensor_device
def fk_collision_points(q, geom):
    """q (B,H,d) -> positions of the robot's collision spheres (B,H,L,3) (mpb_fk_collision_points)."""
    B, H, d = q.shape
    _chk(q, (B, H, d), 'q')
    _need_all_links(geom)
    L = geom.n_links
    pts = torch.empty(B, H, L, 3, device=q.device, dtype=torch.float32)
    _lib.check(_lib.lib().mpb_fk_collision_points(_ptr(q), _ptr(geom.buf), _ptr(pts), B, H, d, _stream()), 'mpb_fk_collision_points')
    return pts


@_on_tensor_device
def fk_collision_points_vjp(q, geom, grad_pts):
    B, H, d = q.shape
    _need_all_links(geom)
    L = geom.n_links
    _chk(q, (B, H, d), 'q')
    _chk(grad_pts, (B, H, L, 3), 'grad_pts')
    gq = torch.empty(B, H, geom.n_dof, device=q.device, dtype=torch.float32)
    _lib.check(_lib.lib().mpb_fk_collision_points_vjp(_ptr(q), _ptr(geom.buf), _ptr(grad_pts), _ptr(gq), B, H, d, _stream()),
               'mpb_fk_collision_points_vjp')
    return gq


@_on_tensor_device
def field_cost_points(pts, geom):
    """Collision-sphere positions (B,H,L,3) -> hinge cost per waypoint (B,H) (mpb_field_cost_points)."""
    B, H, L, _ = pts.shape
    _need_all_links(geom)
    _chk(pts, (B, H, geom.n_links, 3), 'pts')
    cost = torch.empty(B, H, device=pts.device, dtype=torch.float32)
    _lib.check(_lib.lib().mpb_field_cost_points(_ptr(pts), _ptr(geom.buf), _ptr(cost), B, H, _stream()), 'mpb_field_cost_points')
    return cost


@_on_tensor_device
def field_cost_points_vjp(pts, geom, grad_cost):
    B, H, L, _ = pts.shape
    _need_all_links(geom)
    _chk(pts, (B, H, geom.n_links, 3), 'pts')
    _chk(grad_cost, (B, H), 'grad_cost')
    gp = torch.empty_like(pts)
    _lib.check(_lib.lib().mpb_field_cost_points_vjp(_ptr(pts), _ptr(geom.buf), _ptr(grad_cost), _ptr(gp), B, H, _stream()),
               'mpb_field_cost_points_vjp')
    return gp


@_on_tensor_device
def gp_factor_error(x, D, dt):
    """(B,H,2D) -> (B,H-1,2D): x_{t+1} - Phi x_t (mpb_gp_factor_error)."""
    B, H, dim = x.shape
    _chk(x, (B, H, 2 * D), 'x')
    out = torch.empty(B, H - 1, dim, device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().mpb_gp_factor_error(_ptr(x), _ptr(out), B, H, D, float(dt), _stream()), 'mpb_gp_factor_error')
    return out


@_on_tensor_device
def cost_terms_grad(trajs, n_dof, grad_in=None, grad_out=None, apply=False, R=None, prior_bw=0.0, lr=0.0, grad_clip=0.0,
                    jl_scale=1.0, dt=0.0, k_gp=0.0, vel_fd=False, k_start=0.0, start_state=None, k_goal=0.0,
                    goal_states=None, trajs_per_goal=1, k_smooth=0.0, k_jlim=0.0, q_min=None, q_max=None, jl_eps=0.0,
                    terms=None):
    """Analytic gradient of the trajectory-only cost terms (+ CHOMP's smoothness prior, + an incoming gradient such as
    the collision one), written to grad_out or -- apply=True -- consumed by CHOMP's clamped, end-masked step on
    `trajs` in place (mpb_cost_terms_grad).  Term arguments as cost_terms_eval."""
    B, H, d = trajs.shape
    _chk(trajs, (B, H, d), 'trajs')
    flags = _term_flags(terms, B, n_dof, vel_fd, start_state, goal_states, trajs_per_goal, q_min, q_max)
    if grad_in is not None:
        _chk(grad_in, (B, H, d), 'grad_in')
    if not apply:
        if grad_out is None:
            grad_out = torch.empty(B, H, d, device=trajs.device, dtype=torch.float32)
        _chk(grad_out, (B, H, d), 'grad_out')
    if prior_bw != 0.0:
        _chk(R, (H, H), 'R')
    _lib.check(_lib.lib().mpb_cost_terms_grad(
        _ptr(trajs), _ptr(grad_in), _ptr(grad_out), _ptr(R), _ptr(start_state), _ptr(goal_states), _ptr(q_min), _ptr(q_max),
        B, H, d, int(n_dof), int(trajs_per_goal), flags, float(dt), float(k_gp), float(k_start), float(k_goal),
        float(k_smooth), float(k_jlim), float(jl_eps), float(jl_scale), float(prior_bw), float(lr), float(grad_clip),
        int(bool(apply)), _stream()), 'mpb_cost_terms_grad')
    return grad_out


@_on_tensor_device
def traj_interpolate(trajs, n_interp):
    """(B,H,d) -> (B,(H-1)(n+1)+1,d): n evenly spaced joint-space points per segment (mpb_traj_interpolate)."""
    B, H, d = trajs.shape
    _chk(trajs, (B, H, d), 'trajs')
    n = int(n_interp)
    out = torch.empty(B, (H - 1) * (n + 1) + 1, d, device=trajs.device, dtype=torch.float32)
    _lib.check(_lib.lib().mpb_traj_interpolate(_ptr(trajs), _ptr(out), B, H, d, n, _stream()), 'mpb_traj_interpolate')
    return out


@_on_tensor_device
def traj_resample(paths, lengths, H, dt):
    """N padded polylines (N,Lmax,D) with `lengths` (N,) int32 valid rows -> (N,H,2D) support points uniform in
    arc length + average-velocity channel (mpb_traj_resample)."""
    N, Lmax, D = paths.shape
    _chk(paths, (N, Lmax, D), 'paths')
    if not (lengths.is_cuda and lengths.dtype == torch.int32 and lengths.is_contiguous() and tuple(lengths.shape) == (N,)):
        raise ValueError('lengths must be a contiguous int32 GPU tensor of shape (N,)')
    out = torch.empty(N, H, 2 * D, device=paths.device, dtype=torch.float32)
    _lib.check(_lib.lib().mpb_traj_resample(_ptr(paths), _ptr(lengths), _ptr(out), N, Lmax, int(H), D, float(dt), _stream()),
               'mpb_traj_resample')
    return out


@_on_tensor_device
def traj_finite_difference(pos, dt):
    """(B,H,D) positions -> (B,H,2D) [pos, central-difference velocities] (mpb_traj_finite_difference)."""
    B, H, D = pos.shape
    _chk(pos, (B, H, D), 'pos')
    out = torch.empty(B, H, 2 * D, device=pos.device, dtype=torch.float32)
    _lib.check(_lib.lib().mpb_traj_finite_difference(_ptr(pos), _ptr(out), B, H, D, float(dt), _stream()),
               'mpb_traj_finite_difference')
    return out


def _stomp_shapes(means, samples, costs, weights, L, Sigma, S):
    """The buffers every whole-call STOMP entry point takes, checked against the means' (P, H, d); returns it."""
    P, H, d = means.shape
    _chk(means, (P, H, d), 'means')
    _chk(samples, (P, S, H, d), 'samples')
    _chk(costs, (P, S), 'costs')
    _chk(weights, (P, S), 'weights')
    _chk(L, (H, H), 'L')
    _chk(Sigma, (H, H), 'Sigma')
    return P, H, d


def _stomp_head(eps, means, samples, costs, weights, L, Sigma, geom, S, D, k_sigma, weight, lr, temperature, workspace=False):
    """The leading C arguments of a whole-call STOMP entry point, in the order of include/mpb.h: the buffers, geom_flags,
    [workspace, its bytes,] P S H d D and the four floats.  eps / workspace = False: the entry point has no such parameter
    (None: it has, and gets NULL)."""
    P, H, d = means.shape
    bufs = (means,) + (() if eps is False else (eps,)) + (samples, costs, weights, L, Sigma, geom.buf)
    ws = () if workspace is False else (_ptr(workspace), 0 if workspace is None else workspace.numel() * 4)
    return (*map(_ptr, bufs), int(geom.flags), *ws, P, S, H, d, D, float(k_sigma), float(weight), float(lr), float(temperature))


@_on_tensor_device
def stomp_step(means, eps, samples, costs, weights, L, Sigma, geom, S, D, k_sigma, weight, lr, temperature,
               n_iters=1, seed=0, iter0=0, particle_offset=0):
    P, H, d = _stomp_shapes(means, samples, costs, weights, L, Sigma, S)
    if eps is not None:
        _chk(eps, (n_iters, S, d, P, H), 'eps')
    _lib.check(_lib.lib().mpb_stomp_step(
        *_stomp_head(eps, means, samples, costs, weights, L, Sigma, geom, S, D, k_sigma, weight, lr, temperature),
        int(n_iters), _seed64(seed), int(iter0), int(particle_offset), _stream()), 'mpb_stomp_step')


def stomp_workspace(P, S, H, d, device):
    """Exchange buffer of the persistent STOMP kernel (mpb_stomp_run): header zeroed (mpb_stomp_workspace_init), the
    rest need not be initialised.  One workspace serves one call at a time."""
    n = int(_lib.lib().mpb_stomp_workspace_bytes(int(P), int(S), int(H), int(d)))
    ws = torch.empty((n + 3) // 4, device=device, dtype=torch.float32)
    with torch.cuda.device(ws.device):
        _lib.check(_lib.lib().mpb_stomp_workspace_init(_ptr(ws), ws.numel() * 4, _stream()), 'mpb_stomp_workspace_init')
    return ws


STOMP_PATH_TWO_KERNEL, STOMP_PATH_PERSISTENT_EXCHANGE, STOMP_PATH_PERSISTENT = 0, 1, 2


def stomp_run_path(geom, workspace, P, S, H, d):
    """Which form of the loop mpb_stomp_run takes for this call (STOMP_PATH_*), without launching anything."""
    nbytes = 0 if workspace is None else workspace.numel() * 4
    with torch.cuda.device(geom.buf.device):
        return int(_lib.lib().mpb_stomp_run_path(int(geom.flags), nbytes, int(P), int(S), int(H), int(d)))


class StompRunStatus:
    """Host-visible status block of mpb_stomp_run_checked: 8 words of pinned host memory the kernel writes directly
    ([0] tag of the last completed call, [1] tag of the last LOST call, [2] why, [4..7] device real-time stamps of the
    launch's begin / end), read here without synchronising."""

    def __init__(self):
        self.buf = torch.zeros(8, dtype=torch.int32).pin_memory()
        self._view = self.buf.numpy().view(np.uint32)
        self.issued = []             # tags of the persistent launches not yet known to be complete, in launch order
        self.tag_c = ctypes.c_uint32(0)

    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr())

    def note_launch(self):
        tag = int(self.tag_c.value)
        if tag:
            self.issued.append(tag)
        return tag

    def lost(self):
        """(tag, why) of a lost call among the ones issued through this block, else None.  Reads host memory only."""
        lost, done = int(self._view[1]), int(self._view[0])
        if lost and lost in self.issued:
            return lost, int(self._view[2])
        if done in self.issued:      # calls complete in launch order: everything up to `done` is over, and was fine
            del self.issued[:self.issued.index(done) + 1]
        return None

    def device_span_ms(self):
        """Duration of the last COMPLETED persistent launch as the device saw it (100 MHz real-time counter: first unit
        started -> last workgroup left), in milliseconds; None if no launch has completed.  Host memory only."""
        v = self._view
        if int(v[0]) == 0:
            return None
        t0, t1 = int(v[4]) | (int(v[5]) << 32), int(v[6]) | (int(v[7]) << 32)
        return (t1 - t0) * 1e-5 if t1 > t0 else None

    def acknowledge(self, tag):
        """Forget a lost call (after it has been reported)."""
        if tag in self.issued:
            del self.issued[:self.issued.index(tag) + 1]


@_on_tensor_device
def stomp_run(means, eps, samples, costs, weights, L, Sigma, geom, S, D, k_sigma, weight, lr, temperature, workspace,
              n_iters=1, seed=0, iter0=0, particle_offset=0, status=None, means_copy=None):
    """stomp_step as ONE persistent launch where the shape allows it (H = 64, S <= 64, grid-backed fields), the
    two-kernel loop otherwise (the C side decides).  status: a StompRunStatus the kernel reports a lost call to
    (include/mpb.h, "Failure contract"); means_copy: a second (P,H,d) destination of the final means, written by the same
    launch.  Returns the call's tag (0: two-kernel loop)."""
    P, H, d = _stomp_shapes(means, samples, costs, weights, L, Sigma, S)
    if eps is not None:
        _chk(eps, (n_iters, S, d, P, H), 'eps')
    if workspace is not None:
        _chk(workspace, tuple(workspace.shape), 'workspace')
    if means_copy is not None:
        _chk(means_copy, (P, H, d), 'means_copy')
    _lib.check(_lib.lib().mpb_stomp_run_checked(
        *_stomp_head(eps, means, samples, costs, weights, L, Sigma, geom, S, D, k_sigma, weight, lr, temperature, workspace),
        int(n_iters), _seed64(seed), int(iter0), int(particle_offset),
        None if status is None else status.ptr(), None if status is None else ctypes.byref(status.tag_c), _ptr(means_copy),
        _stream()), 'mpb_stomp_run')
    return 0 if status is None else status.note_launch()


class StompRunPlan:
    """The arguments of stomp_run for a planner whose buffers do not change between optimize() calls, validated ONCE and
    kept on the library's side (mpb_stomp_plan_*): launch() hands over four values per call.  (stomp_run's per-call
    checks and conversions are ~15 us of host time -- 4 % of a 20-iteration call at C3.)  Device-noise calls only."""

    def __init__(self, means, samples, costs, weights, L, Sigma, geom, S, D, k_sigma, weight, lr, temperature, workspace,
                 seed, particle_offset, status):
        P, H, d = _stomp_shapes(means, samples, costs, weights, L, Sigma, S)
        _chk(workspace, tuple(workspace.shape), 'workspace')
        devs = {t.device for t in (means, samples, costs, weights, L, Sigma, geom.buf, workspace)}
        if len(devs) != 1:
            raise ValueError(f'StompRunPlan: tensors live on different devices ({devs})')
        self.device = means.device
        self.shape = (P, H, d)
        self.key = (means.data_ptr(), samples.data_ptr(), costs.data_ptr(), weights.data_ptr(), L.data_ptr(),
                    Sigma.data_ptr(), geom.buf.data_ptr(), workspace.data_ptr(), S, D, float(k_sigma), float(weight),
                    float(lr), float(temperature), int(seed), int(particle_offset))
        # launch_timed's arguments (it builds the long form when called); they also keep the plan's pointers valid
        self._call = (means, samples, costs, weights, L, Sigma, geom, S, D, k_sigma, weight, lr, temperature, workspace)
        self._seed, self._poff = _seed64(seed), int(particle_offset)
        self._status = status
        self._status_ptr = status.ptr()
        self._tag_ref = ctypes.byref(status.tag_c)
        h = ctypes.c_void_p(0)
        _lib.check(_lib.lib().mpb_stomp_plan_create(
            ctypes.byref(h), *_stomp_head(False, *self._call), self._seed, self._poff, self._status_ptr),
            'mpb_stomp_plan_create')
        self._handle = h
        self._launch = _lib.lib().mpb_stomp_plan_launch
        self._destroy = _lib.lib().mpb_stomp_plan_destroy

    def __del__(self):
        h = getattr(self, '_handle', None)
        if h is not None and h.value:
            self._destroy(h)
            self._handle = None

    def launch_timed(self, n_iters, iter0, means_copy=None):
        """launch() with the kernel's own duration measured on the dispatch (mpb_stomp_run_timed): synchronises; returns ms."""
        ms = ctypes.c_float(0.0)
        rc = _lib.lib().mpb_stomp_run_timed(*_stomp_head(None, *self._call), int(n_iters), self._seed,
                                            int(iter0), self._poff, self._status_ptr,
                                            self._tag_ref, None if means_copy is None else means_copy.data_ptr(),
                                            torch.cuda.current_stream(self.device).cuda_stream, ctypes.byref(ms))
        if rc != 0:
            _lib.check(rc, 'mpb_stomp_run_timed')
        self._status.note_launch()
        return float(ms.value)

    def launch(self, n_iters, iter0, means_copy=None):
        """Enqueue the call on the current stream of the plan's device (which must be the current device)."""
        rc = self._launch(self._handle, n_iters, iter0, None if means_copy is None else means_copy.data_ptr(),
                          raw_stream(self.device.index), self._tag_ref)
        if rc != 0:
            _lib.check(rc, 'mpb_stomp_run')
        return self._status.note_launch()


def stomp_run_state(workspace):
    """State of the last persistent stomp_run on this workspace (synchronises): 0 fine, 1 a workgroup gave up waiting
    for its partner (the call is lost), 2 the workspace header was not zeroed."""
    out = ctypes.c_int(0)
    with torch.cuda.device(workspace.device):
        _lib.check(_lib.lib().mpb_stomp_run_status(_ptr(workspace), _stream(), ctypes.cast(ctypes.pointer(out), ctypes.c_void_p)),
                   'mpb_stomp_run_status')
    return int(out.value)


def stomp_run_timed_out(workspace):
    """Was the last persistent stomp_run on this workspace lost?  (synchronises)"""
    return stomp_run_state(workspace) != 0


def debug_philox(ctr, key, rounds):
    """Test aid: raw Philox4x32-`rounds` words for (n,4) int64/uint32 counters and (n,2) keys (host arrays) -> (n,4) uint32."""
    ctr = np.ascontiguousarray(np.asarray(ctr, dtype=np.uint32).reshape(-1, 4))
    key = np.ascontiguousarray(np.asarray(key, dtype=np.uint32).reshape(-1, 2))
    n = ctr.shape[0]
    dev = torch.device('cuda', torch.cuda.current_device())
    c = torch.from_numpy(ctr.view(np.int32)).to(dev)
    k = torch.from_numpy(key.view(np.int32)).to(dev)
    out = torch.empty(n, 4, dtype=torch.int32, device=dev)
    _lib.debug_check(_lib.debug_lib().mpb_debug_philox(_ptr(c), _ptr(k), _ptr(out), n, int(rounds), _stream()), 'mpb_debug_philox')
    return out.cpu().numpy().view(np.uint32)


def debug_stomp_normals(P, S, d, n_iters, device, seed=0, iter0=0, particle_offset=0, H=64):
    """Test aid: the standard normals the STOMP kernels draw in throughput mode, (n_iters, P, S, d, 64 * ceil(H / 64)) fp32
    (columns k >= H are drawn by the kernels as well and meet zero columns of L)."""
    Hp = 64 * ((int(H) + 63) // 64)
    out = torch.empty(n_iters, P, S, d, Hp, device=device, dtype=torch.float32)
    with torch.cuda.device(out.device):
        _lib.debug_check(_lib.debug_lib().mpb_debug_stomp_normals_h(_ptr(out), int(P), int(S), int(d), int(H), int(n_iters),
                                                                    _seed64(seed), int(iter0), int(particle_offset), _stream()),
                         'mpb_debug_stomp_normals_h')
    return out


def debug_mppi_normals(NP, S, T, c, n_iters, device, seed=0, iter0=0):
    """Test aid: the standard normals mppi_step draws in throughput mode, in the layout of its injected eps (n_iters, NP, c, S, T)."""
    out = torch.empty(n_iters, NP, c, S, T, device=device, dtype=torch.float32)
    with torch.cuda.device(out.device):
        _lib.debug_check(_lib.debug_lib().mpb_debug_mppi_normals(_ptr(out), int(NP), int(S), int(T), int(c), int(n_iters),
                                                                 _seed64(seed), int(iter0), _stream()), 'mpb_debug_mppi_normals')
    return out


def debug_occupy(n_blocks, usec, device):
    """Test aid: n_blocks workgroups that each take a CU's LDS and idle for `usec` microseconds on the current stream."""
    sink = torch.zeros(1, dtype=torch.int32, device=device)
    with torch.cuda.device(sink.device):
        _lib.debug_check(_lib.debug_lib().mpb_debug_occupy(int(n_blocks), int(usec), _ptr(sink), _stream()), 'mpb_debug_occupy')
    return sink


@_on_tensor_device
def stomp_step_profile(means, samples, costs, weights, L, Sigma, geom, S, D, k_sigma, weight, lr, temperature,
                       n_iters=50, seed=0, iter0=0, particle_offset=0):
    """Measurement aid: n_iters iterations of stomp_step (device noise) with per-dispatch HIP events; returns the average
    duration in ms of (sample+cost kernel, update kernel) inside that loop.  Synchronises the stream."""
    _stomp_shapes(means, samples, costs, weights, L, Sigma, S)
    ka, kb = ctypes.c_float(0.0), ctypes.c_float(0.0)
    _lib.check(_lib.lib().mpb_stomp_step_profile(
        *_stomp_head(False, means, samples, costs, weights, L, Sigma, geom, S, D, k_sigma, weight, lr, temperature),
        int(n_iters), _seed64(seed), int(iter0), int(particle_offset), _stream(),
        ctypes.cast(ctypes.pointer(ka), ctypes.c_void_p), ctypes.cast(ctypes.pointer(kb), ctypes.c_void_p)),
        'mpb_stomp_step_profile')
    return float(ka.value), float(kb.value)


@_on_tensor_device
def stomp_sample(means, eps, samples, L, S, seed=0, it=0, particle_offset=0, geom=None, costs=None, k_sigma=0.0,
                 weight=1.0):
    """First kernel of an iteration: draw + write samples; with geom/costs also the fused collision cost."""
    P, H, d = means.shape
    _chk(means, (P, H, d), 'means')
    _chk(samples, (P, S, H, d), 'samples')
    _chk(L, (H, H), 'L')
    if eps is not None:
        _chk(eps, (S, d, P, H), 'eps')
    if (geom is None) != (costs is None):
        raise ValueError('geom and costs must be given together')
    if costs is not None:
        _chk(costs, (P, S), 'costs')
    _lib.check(_lib.lib().mpb_stomp_sample(_ptr(means), _ptr(eps), _ptr(samples), _ptr(L),
                                          _ptr(None if geom is None else geom.buf),
                                          0 if geom is None else int(geom.flags), _ptr(costs), P, S, H, d,
                                          float(k_sigma), float(weight), _seed64(seed), int(it),
                                          int(particle_offset), _stream()), 'mpb_stomp_sample')


@_on_tensor_device
def stomp_update(means, samples, costs, weights, Sigma, lr, temperature):
    P, S, H, d = samples.shape
    _chk(means, (P, H, d), 'means')
    _chk(samples, (P, S, H, d), 'samples')
    _chk(costs, (P, S), 'costs')
    _chk(weights, (P, S), 'weights')
    _chk(Sigma, (H, H), 'Sigma', allow_none=True)   # None: update without the covariance product (StochGPMP)
    _lib.check(_lib.lib().mpb_stomp_update(_ptr(means), _ptr(samples), _ptr(costs), _ptr(weights), _ptr(Sigma),
                                          P, S, H, d, float(lr), float(temperature), _stream()), 'mpb_stomp_update')


@_on_tensor_device
def chomp_step(means, R, geom, D, k_sigma, weight, w_prior, lr, grad_clip, n_iters=1, B_global=None, costs_out=None):
    B, H, d = means.shape
    _chk(means, (B, H, d), 'means')
    _chk(R, (H, H), 'R')
    _chk(costs_out, (B,), 'costs_out', allow_none=True)
    _lib.check(_lib.lib().mpb_chomp_step(_ptr(means), _ptr(R), _ptr(geom.buf), int(geom.flags), _ptr(costs_out), B,
                                        B if B_global is None else int(B_global), H, d, D, float(k_sigma), float(weight),
                                        float(w_prior), float(lr), float(grad_clip), int(n_iters), _stream()),
               'mpb_chomp_step')


@_on_tensor_device
def gpmp2_workspace(B, H, D, device):
    n = int(_lib.lib().mpb_gpmp2_workspace_bytes(B, H, D))
    if n == 0:
        raise ValueError(f'unsupported GPMP2 shape B={B} H={H} D={D}')
    return torch.empty(n, dtype=torch.uint8, device=device)


@_on_tensor_device
def gpmp2_step(x, start, goal, geom, workspace, sigmas, dt, delta, trust_region, step_size, n_iters=1, costs_out=None,
               n_interp=0):
    """n_iters Gauss-Newton iterations on one GPU.  sigmas = (start, gp, goal, coll)."""
    B, H, dim = x.shape
    D = dim // 2
    _chk(x, (B, H, dim), 'x')
    _chk(start, (B, dim), 'start')
    _chk(goal, (B, dim), 'goal')
    _chk(costs_out, (B,), 'costs_out', allow_none=True)
    assert workspace.numel() >= _lib.lib().mpb_gpmp2_workspace_bytes(B, H, D)
    _lib.check(_lib.lib().mpb_gpmp2_step(
        _ptr(x), _ptr(start), _ptr(goal), _ptr(geom.buf), int(geom.flags), _ptr(workspace), _ptr(costs_out), B, H, D, float(dt),
        float(sigmas[0]), float(sigmas[1]), float(sigmas[2]), float(sigmas[3]), float(delta), int(bool(trust_region)),
        float(step_size), int(n_iters), int(n_interp or 0), int(geom.n_fields), _stream()), 'mpb_gpmp2_step')


@_on_tensor_device
def gpmp2_linearize(x, geom, workspace, n_interp=0):
    B, H, dim = x.shape
    _chk(x, (B, H, dim), 'x')
    _lib.check(_lib.lib().mpb_gpmp2_linearize(_ptr(x), _ptr(geom.buf), int(geom.flags), _ptr(workspace), B, H, dim // 2,
                                              int(n_interp or 0), _stream()), 'mpb_gpmp2_linearize')


@_on_tensor_device
def gpmp2_collision_rows(x, geom, n_interp=0):
    """The collision factor's rows as the GPMP2 solve consumes them: (F, B, H, D+1) fp32 with [..., :D] = h_t =
    -d c_t / d q_t (with n_interp > 0: of the INTERPOLATED trajectory's summed cost, cost_functions.py:115-119,
    field_factor.py:42-54) and [..., D] = c_t, one set per chained field, each scaled by sqrt(s_f); row 0 takes no
    collision factor (traj_range [1, None]): its c is zero, and so is its h unless n_interp > 0.  Runs mpb_gpmp2_linearize into a scratch buffer that holds only the Jacobian section of
    the GPMP2 workspace (the kernel writes nothing else)."""
    B, H, dim = x.shape
    D = dim // 2
    _chk(x, (B, H, dim), 'x')
    if _lib.lib().mpb_gpmp2_workspace_bytes(B, H, D) == 0:
        raise ValueError(f'unsupported GPMP2 shape B={B} H={H} D={D}')
    jac = torch.zeros(MAX_FIELDS, B, H, D + 1, device=x.device, dtype=torch.float32)     # (the section is laid out for MAX_FIELDS fields)
    _lib.check(_lib.lib().mpb_gpmp2_linearize(_ptr(x), _ptr(geom.buf), int(geom.flags), _ptr(jac), B, H, D, int(n_interp or 0), _stream()),
               'mpb_gpmp2_linearize')
    return jac[:geom.n_fields]


@_on_tensor_device
def gpmp2_diag(workspace, B, H, D, sigmas, dt, n_fields=1):
    """Local SUM over particles of diag(A^T K A) as an (H*2D,) fp64 tensor."""
    out = torch.empty(H * 2 * D, dtype=torch.float64, device=workspace.device)
    _lib.check(_lib.lib().mpb_gpmp2_diag(_ptr(workspace), _ptr(out), B, H, D, int(n_fields), float(dt), float(sigmas[0]),
                                        float(sigmas[1]), float(sigmas[2]), float(sigmas[3]), _stream()), 'mpb_gpmp2_diag')
    return out


@_on_tensor_device
def gpmp2_solve(x, start, goal, diag_mean, workspace, sigmas, dt, delta, trust_region, step_size, costs_out=None,
                n_fields=1):
    B, H, dim = x.shape
    _chk(x, (B, H, dim), 'x')
    _chk(start, (B, dim), 'start')
    _chk(goal, (B, dim), 'goal')
    _chk(diag_mean, (H * dim,), 'diag_mean', allow_none=True, dtype=torch.float64)
    _lib.check(_lib.lib().mpb_gpmp2_solve(
        _ptr(x), _ptr(start), _ptr(goal), _ptr(diag_mean), _ptr(workspace), _ptr(costs_out), B, H, dim // 2, int(n_fields),
        float(dt), float(sigmas[0]), float(sigmas[1]), float(sigmas[2]), float(sigmas[3]), float(delta), int(bool(trust_region)),
        float(step_size), _stream()), 'mpb_gpmp2_solve')


@_on_tensor_device
def mppi_step(mean, eps, scale_tril, cov_inv, state0, goal, ctrl_min, ctrl_max, discount, c_weights, geom, controls,
              states, costs, weights, dt, k_sigma=0.0, weight=1.0, temp=1.0, step_size=1.0, n_iters=1, seed=0, iter0=0,
              best_cost=None, best_states=None):
    NP, T, c = mean.shape
    S = controls.shape[1]
    _chk(mean, (NP, T, c), 'mean')
    if eps is not None:
        _chk(eps, (n_iters, NP, c, S, T), 'eps')
    _chk(scale_tril, (c, T, T), 'scale_tril')
    _chk(cov_inv, (c, T, T), 'cov_inv')
    _chk(state0, (NP, c), 'state0')
    _chk(goal, (NP, c), 'goal')
    _chk(ctrl_min, (c,), 'ctrl_min')
    _chk(ctrl_max, (c,), 'ctrl_max')
    _chk(discount, (T,), 'discount')
    _chk(c_weights, (4,), 'c_weights')
    _chk(controls, (NP, S, T, c), 'controls')
    _chk(states, (NP, S, T, c), 'states')
    _chk(costs, (NP, S), 'costs')
    _chk(weights, (NP, S), 'weights')
    if (best_cost is None) != (best_states is None):
        raise ValueError('best_cost and best_states must be given together')
    _chk(best_cost, (NP,), 'best_cost', allow_none=True)
    _chk(best_states, (NP, T, c), 'best_states', allow_none=True)
    _lib.check(_lib.lib().mpb_mppi_step(
        _ptr(mean), _ptr(eps), _ptr(scale_tril), _ptr(cov_inv), _ptr(state0), _ptr(goal), _ptr(ctrl_min), _ptr(ctrl_max),
        _ptr(discount), _ptr(c_weights), _ptr(None if geom is None else geom.buf), 0 if geom is None else int(geom.flags),
        _ptr(controls), _ptr(states),
        _ptr(costs), _ptr(weights), _ptr(best_cost), _ptr(best_states), NP, S, T, c, 0, float(dt), float(k_sigma),
        float(weight), float(temp),
        float(step_size), int(n_iters), _seed64(seed), int(iter0), _stream()), 'mpb_mppi_step')


MPPI_NOISE_GLOBAL, MPPI_NOISE_LDS, MPPI_NOISE_MATRIX = 0, 1, 2
MppiPlan = collections.namedtuple('MppiPlan', 'noise_mode waves grid_words lds_bytes')


def mppi_plan(geom, NP, S, T, c, has_eps=False, n_cu=0):
    """How mppi_step would launch this shape (mpb_mppi_plan: the launcher's own decision, nothing is launched): MppiPlan(noise_mode
    MPPI_NOISE_*, waves per problem, grid_words staged in LDS -- 0: exhaustive collision walk --, dynamic LDS bytes).  geom: a
    DeviceGeometry, None, or the mpb_geom_flags (int) of a packed scene; n_cu: compute units to plan for, 0 asks the device.
    Raises MPBError where mppi_step would."""
    out = (ctypes.c_int * 4)()
    flags = 0 if geom is None else int(geom.flags if isinstance(geom, DeviceGeometry) else geom)
    args = (flags, int(geom is not None), int(NP), int(S), int(T), int(c), int(bool(has_eps)), int(n_cu), ctypes.cast(out, ctypes.c_void_p))
    if isinstance(geom, DeviceGeometry):         # (n_cu = 0 asks the CURRENT device: the geometry's)
        with torch.cuda.device(geom.buf.device):
            rc = _lib.lib().mpb_mppi_plan(*args)
    else:
        rc = _lib.lib().mpb_mppi_plan(*args)
    _lib.check(rc, 'mpb_mppi_plan')
    return MppiPlan(*[int(v) for v in out])


@_on_tensor_device
def point_dynamics(x, u, ctrl_min, ctrl_max, dt, dyn_std=None, noise=None):
    """PointParticleDynamics.dynamics (point.py:102-140): x, u (..., dim) contiguous fp32 of the same shape -> x_next."""
    dim = x.shape[-1]
    _chk(x, tuple(x.shape), 'x')
    _chk(u, tuple(x.shape), 'u')
    _chk(ctrl_min, (dim,), 'ctrl_min')
    _chk(ctrl_max, (dim,), 'ctrl_max')
    if noise is not None:
        _chk(noise, tuple(x.shape), 'noise')
        _chk(dyn_std, (dim,), 'dyn_std')
    out = torch.empty_like(x)
    _lib.check(_lib.lib().mpb_point_dynamics(_ptr(x), _ptr(u), _ptr(ctrl_min), _ptr(ctrl_max), _ptr(dyn_std if noise is not None else None),
                                            _ptr(noise), _ptr(out), x.numel() // dim, dim, float(dt), _stream()), 'mpb_point_dynamics')
    return out


@_on_tensor_device
def point_traj_cost(X, U, goal, discount, w_pos, w_vel, w_ctrl, w_pos_T, energy=0.0):
    """PointParticleDynamics.traj_cost (point.py:154-226): X (T,B,sd), U (T,B,cd), goal (sd), discount (T) -> costs (B)."""
    T, B, sd = X.shape
    cd = U.shape[-1]
    _chk(X, (T, B, sd), 'X')
    _chk(U, (T, B, cd), 'U')
    _chk(goal, (sd,), 'goal')
    _chk(discount, (T,), 'discount')
    out = torch.empty(B, device=X.device, dtype=torch.float32)
    _lib.check(_lib.lib().mpb_point_traj_cost(_ptr(X), _ptr(U), _ptr(goal), _ptr(discount), float(w_pos), float(w_vel), float(w_ctrl),
                                             float(w_pos_T), float(energy), _ptr(out), T, B, sd, cd, _stream()), 'mpb_point_traj_cost')
    return out


@_on_tensor_device
def mvn_sample_dense(means, eps, tril_t, n, seed=0):
    """x = mean + L eps from a dense scale_tril handed over transposed (mpb_mvn_sample_dense): means (G,M) fp64, eps None or
    (n,G,M) fp64, tril_t (M,M) fp64 with tril_t[k,m] = L[m,k] -> (G*n, M) fp32, row mode * n + sample."""
    G, M = means.shape
    _chk(means, (G, M), 'means', dtype=torch.float64)
    _chk(tril_t, (M, M), 'tril_t', dtype=torch.float64)
    _chk(eps, (n, G, M), 'eps', allow_none=True, dtype=torch.float64)
    out = torch.empty(G * n, M, device=means.device, dtype=torch.float32)
    _lib.check(_lib.lib().mpb_mvn_sample_dense(_ptr(out), _ptr(means), _ptr(eps), _ptr(tril_t), G, n, M,
                                              _seed64(seed), _stream()), 'mpb_mvn_sample_dense')
    return out


@_on_tensor_device
def gp_prior_sample(means, eps, Udiag, Uoff, n, D, seed=0, scale_tril=None, out=None):
    """Initial particles from the GP prior: means (G,H,2D) fp64, eps None or (n,G,H*2D) fp64 -> (G*n,H,2D) fp32.
    With `scale_tril` (2H,2H fp64, planners.base.gp_prior_scale_tril) and H <= 128 the product runs as a GEMM on
    the matrix cores; otherwise as the per-chain forward substitution."""
    G, H, dim = means.shape
    _chk(means, (G, H, 2 * D), 'means', dtype=torch.float64)
    _chk(Udiag, (H, 3), 'Udiag', dtype=torch.float64)
    _chk(Uoff, (H - 1, 4), 'Uoff', dtype=torch.float64)
    _chk(eps, (n, G, H * dim), 'eps', allow_none=True, dtype=torch.float64)
    if out is None:
        out = torch.empty(G * n, H, dim, device=means.device, dtype=torch.float32)
    else:
        _chk(out, (G * n, H, dim), 'out')
    if scale_tril is not None and H <= 128:
        _chk(scale_tril, (2 * H, 2 * H), 'scale_tril', dtype=torch.float64)
        _lib.check(_lib.lib().mpb_gp_prior_sample_dense(_ptr(out), _ptr(means), _ptr(eps), _ptr(scale_tril), G, n, H, D,
                                                       _seed64(seed), _stream()), 'mpb_gp_prior_sample_dense')
        return out
    _lib.check(_lib.lib().mpb_gp_prior_sample(_ptr(out), _ptr(means), _ptr(eps), _ptr(Udiag), _ptr(Uoff), G, n, H, D,
                                             _seed64(seed), _stream()), 'mpb_gp_prior_sample')
    return out


@_on_tensor_device
def stoch_gpmp_step(means, means64, samples, costs, weights, Udiag, Uoff, scale_tril, start, goal, geom, S, sig_cost,
                    sig_sample, dt, temperature, step_size, n_iters=1, seed=0):
    """n_iters StochGPMP iterations (device noise) enqueued by one C call: sample -> costs -> update."""
    P, H, dim = means.shape
    _chk(means, (P, H, dim), 'means')
    _chk(samples, (P * S, H, dim), 'samples')
    _chk(costs, (P, S), 'costs')
    _chk(weights, (P, S), 'weights')
    _chk(start, (P, dim), 'start')
    _chk(goal, (P, dim), 'goal')
    _chk(means64, (P, H, dim), 'means64', dtype=torch.float64)
    _chk(Udiag, (H, 3), 'Udiag', dtype=torch.float64)
    _chk(Uoff, (H - 1, 4), 'Uoff', dtype=torch.float64)
    _chk(scale_tril, (2 * H, 2 * H), 'scale_tril', allow_none=True, dtype=torch.float64)
    _lib.check(_lib.lib().mpb_stoch_gpmp_step(
        _ptr(means), _ptr(means64), _ptr(samples), _ptr(costs), _ptr(weights), _ptr(Udiag), _ptr(Uoff), _ptr(scale_tril),
        _ptr(start), _ptr(goal), _ptr(geom.buf), P, S, H, dim // 2, float(dt), float(sig_cost[0]), float(sig_cost[1]),
        float(sig_cost[2]), float(sig_cost[3]), float(sig_sample[0]), float(sig_sample[1]), float(sig_sample[2]),
        float(temperature), float(step_size), int(n_iters), _seed64(seed), _stream()), 'mpb_stoch_gpmp_step')


@_on_tensor_device
def stoch_gpmp_costs(samples, means, start, goal, geom, costs, S, sig_cost, sig_sample, dt, temperature):
    """costs (P,S) of StochGPMP samples (P*S,H,2D): composite cost + importance term.
    sig_cost = (start, gp, goal_prior, coll); sig_sample = (start, gp, goal)."""
    B, H, dim = samples.shape
    P = B // S
    _chk(samples, (P * S, H, dim), 'samples')
    _chk(means, (P, H, dim), 'means')
    _chk(start, (P, dim), 'start')
    _chk(goal, (P, dim), 'goal')
    _chk(costs, (P, S), 'costs')
    _lib.check(_lib.lib().mpb_stoch_gpmp_costs(
        _ptr(samples), _ptr(means), _ptr(start), _ptr(goal), _ptr(geom.buf), _ptr(costs), P, S, H, dim // 2, float(dt),
        float(sig_cost[0]), float(sig_cost[1]), float(sig_cost[2]), float(sig_cost[3]), float(sig_sample[0]),
        float(sig_sample[1]), float(sig_sample[2]), float(temperature), _stream()), 'mpb_stoch_gpmp_costs')


# ---- torch's CPU generator on the device (noise = 'mt19937') ---------------------------------------------------------------------
class _MTTables:
    """The device copy of a draw shape's jump tables (mt19937.jump_tables); read-only, shared by every stream."""

    def __init__(self, n, n_calls, device, uniform):
        from . import mt19937 as MT
        spc = MT.segments_per_call(n, n_calls)
        polys, rows, self.total, self.host_s = MT.jump_tables(n, n_calls, spc, uniform)
        idx, cnt = MT.jump_lists(polys)
        self.n_segs = len(rows)
        self.stride = idx.shape[1]
        self.idx = torch.from_numpy(idx.view(np.int16)).to(device)
        self.cnt = torch.from_numpy(cnt).to(device)
        self.segs = torch.from_numpy(rows[:, 1:].astype(np.int32)).contiguous().to(device)
        self.work_words = 20608 + MT.N * (self.n_segs + 1)


_MT_TABLES = {}
_MT_WORK = {}


def _mt_device(device):
    """A device with its index: torch.device('cuda') is the current device (planners accept that spelling)."""
    device = torch.device(device)
    if device.type != 'cuda':
        raise _lib.MPBError(f'torch_cpu_normal_: the draw runs on a GPU, not on {device}')
    return device if device.index is not None else torch.device('cuda', torch.cuda.current_device())


def _mt_tables(n, n_calls, device, uniform=False):
    key = (int(n), int(n_calls), _mt_device(device), bool(uniform))
    t = _MT_TABLES.get(key)
    if t is None:
        if len(_MT_TABLES) >= 16:
            _MT_TABLES.pop(next(iter(_MT_TABLES)))
        t = _MT_TABLES[key] = _MTTables(n, n_calls, key[2], uniform)
    return t


def _mt_work(tb, device):
    """The prefix + windows scratch of a draw: written by every draw, so one buffer per (device, current stream) -- two
    generators drawing on different streams never share one.  Grown to the largest draw seen."""
    device = _mt_device(device)
    key = (device, raw_stream(device.index))
    w = _MT_WORK.get(key)
    if w is None or w.numel() < tb.work_words:
        w = _MT_WORK[key] = torch.empty(tb.work_words, dtype=torch.int32, device=device)
    return w


def _mt_check_out(out, n_calls):
    if not isinstance(out, torch.Tensor) or not out.is_cuda:
        raise _lib.MPBError('torch_cpu_normal_: out must be a GPU tensor (the CPU generator draws CPU tensors itself)')
    if out.dtype != torch.float32:
        raise _lib.MPBError(f'torch_cpu_normal_: only float32 draws are served (got {out.dtype}; fp64 takes 53-bit uniforms '
                            f'from two words)')
    if not out.is_contiguous():
        raise _lib.MPBError('torch_cpu_normal_: out must be contiguous (torch draws a non-contiguous tensor another way)')
    n_calls = int(n_calls)
    if n_calls < 1 or out.dim() < 1 or out.shape[0] != n_calls:
        raise _lib.MPBError(f'torch_cpu_normal_: out must have shape (n_calls = {n_calls}, *block), got {tuple(out.shape)}')
    n = out.numel() // n_calls
    if n < 16:
        raise _lib.MPBError(f'torch_cpu_normal_: a block of {n} < 16 elements takes torch\'s scalar normal_ path, not served')
    if n >= 2 ** 31 - 16:
        raise _lib.MPBError('torch_cpu_normal_: block too large')
    return n


class TorchCpuGeneratorOnDevice:
    """A torch CPU generator's mt19937 state held on a device across several draws: the constructor copies it in (2.5 KB),
    every `normal_` draws on the device and keeps the state there, `store` writes it back to the generator.  `stage` queues
    the copy back behind the draws made so far, so that `store` waits for them only, not for work queued after `stage`.
    Between the constructor and `store` the generator must not be used by anything else."""

    def __init__(self, device, generator=None):
        from . import mt19937 as MT
        self.gen = generator if generator is not None else torch.default_generator
        if self.gen.device.type != 'cpu':
            raise _lib.MPBError('TorchCpuGeneratorOnDevice: the generator must be a CPU generator')
        self.device = _mt_device(device)
        self.host = MT.MTState.from_bytes(self.gen.get_state())
        self.pos = self.host.pos
        self.words = 0
        self.state = torch.from_numpy(self.host.arr.view(np.int32).copy()).to(self.device)
        self._staged = None              # (pinned host copy of the state, its event, pos, words) queued by stage()

    def normal_(self, out, n_calls, events=None):
        """out (n_calls, *block) on this object's device: n_calls successive normal_() draws of the block.
        events: four torch.cuda.Event(enable_timing=True) recorded around the three launches (a measurement aid: the draw is
        then made through the test-aid library's timed entry)."""
        from . import mt19937 as MT
        n = _mt_check_out(out, n_calls)
        if out.device != self.device:
            raise _lib.MPBError(f'torch_cpu_normal_: out lives on {out.device}, the state on {self.device}')
        tb = _mt_tables(n, n_calls, self.device)
        with torch.cuda.device(self.device):
            work = _mt_work(tb, self.device)
            args = (_ptr(out), n, int(n_calls), _ptr(self.state), self.pos, MT.final_index(self.pos, tb.total), _ptr(self.state),
                    _ptr(tb.idx), _ptr(tb.cnt), tb.stride, _ptr(tb.segs), tb.n_segs, _ptr(work))
            if events is None:
                _lib.check(_lib.lib().mpb_mt19937_normals(*args, _stream()), 'mpb_mt19937_normals')
            else:
                for e in events:
                    e.record()                   # (torch creates an event's handle at its first record)
                ev = (ctypes.c_void_p * 4)(*[e.cuda_event for e in events])
                _lib.debug_check(_lib.debug_lib().mpb_debug_mt19937_normals_timed(*args, ctypes.cast(ev, ctypes.c_void_p), _stream()),
                                 'mpb_debug_mt19937_normals_timed')
        self.pos = MT.pos_after(self.pos, tb.total)
        self.words += tb.total
        self._staged = None
        return out

    def stage(self):
        """Queue the copy of the state after the draws so far to pinned host memory (no wait)."""
        if self.words:
            host = torch.empty(self.state.shape, dtype=self.state.dtype).pin_memory()
            with torch.cuda.device(self.device):
                host.copy_(self.state, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
            self._staged = (host, ev, self.pos, self.words)

    def store(self):
        """Write the state after every draw so far back to the generator (waits for the draws, or for the staged copy)."""
        from . import mt19937 as MT
        if not self.words:
            return
        if self._staged is None:
            self.stage()
        host, ev, pos, words = self._staged
        ev.synchronize()
        st = self.host.copy()
        st.arr, st.next, st.left = host.numpy().view(np.uint32).copy(), pos, MT.N + 1 - pos
        self.gen.set_state(st.to_tensor())
        self.host, self.words, self._staged = st, 0, None


def torch_cpu_normal_(out, n_calls, generator=None):
    """Fill the GPU tensor out (n_calls, *block) with what n_calls successive `torch.empty(block).normal_(generator=g)` on the
    CPU produce, and advance g (default: the global CPU generator) as those draws do.  The uniforms and the generator state
    are torch's bit for bit; the normals agree within a few ULP (torch's vectorised log / sincos are not restated).
    fp32, contiguous, blocks of >= 16 elements only (torch takes other paths for the rest): anything else raises MPBError."""
    _mt_check_out(out, n_calls)
    g = TorchCpuGeneratorOnDevice(out.device, generator)
    g.normal_(out, n_calls)
    g.store()
    return out


def debug_mt19937_uniforms(n, n_calls, device, generator=None):
    """Test aid: n_calls successive `torch.empty(n).uniform_()` draws on the device (the generator of torch_cpu_normal_ with
    uniform_()'s n words a call); returns (out (n_calls, n), the state after them as MTState).  The generator is not advanced."""
    from . import mt19937 as MT
    gen = generator if generator is not None else torch.default_generator
    host = MT.MTState.from_bytes(gen.get_state())
    out = torch.empty(n_calls, n, device=device, dtype=torch.float32)
    tb = _mt_tables(n, n_calls, device, uniform=True)
    st_in = torch.from_numpy(host.arr.view(np.int32).copy()).to(device)
    st_out = torch.empty_like(st_in)
    with torch.cuda.device(out.device):
        _lib.debug_check(_lib.debug_lib().mpb_debug_mt19937_uniforms(
            _ptr(out), int(n), int(n_calls), _ptr(st_in), host.pos, MT.final_index(host.pos, tb.total), _ptr(st_out),
            _ptr(tb.idx), _ptr(tb.cnt), tb.stride, _ptr(tb.segs), tb.n_segs, _ptr(_mt_work(tb, out.device)), _stream()),
            'mpb_debug_mt19937_uniforms')
    return out, MT.state_after(host, tb.total, st_out.cpu().numpy().view(np.uint32))


# ---- collision predicate, batched RRT-Connect (csrc/mpb_rrt_connect.hip), batched RRT* / informed RRT* (csrc/mpb_rrt_star.hip) ---
# statuses, stop reasons, the pool limit and the layout of the two workspaces: rrt_layout.py, their one definition
RRT_STATUS_NAMES, RRT_STOP_NAMES, RRT_MAX_PRE_SAMPLES = rrt_layout.STATUS, rrt_layout.STOP, rrt_layout.MAX_PRE_SAMPLES
(RRT_RUNNING, RRT_FOUND, RRT_EXHAUSTED_ITERS, RRT_START_OR_GOAL_IN_COLLISION, RRT_POOL_EMPTY, RRT_TREE_FULL,
 RRT_PATH_TOO_LONG) = map(RRT_STATUS_NAMES.index, ('RUNNING', 'FOUND', 'EXHAUSTED_ITERS', 'START_OR_GOAL_IN_COLLISION', 'POOL_EMPTY',
                                                   'TREE_FULL', 'PATH_TOO_LONG'))
(RRT_STOP_RUNNING, RRT_STOP_ITERS, RRT_STOP_COST_CONVERGED, RRT_STOP_AFTER_SUCCESS, RRT_STOP_TREE_FULL,
 RRT_STOP_POOL_EMPTY) = map(RRT_STOP_NAMES.index, ('RUNNING', 'ITERS', 'COST_CONVERGED', 'AFTER_SUCCESS', 'TREE_FULL', 'POOL_EMPTY'))


@_on_tensor_device
def collision_check(q, geom, with_gap=False):
    """(N, D) configurations -> bool (N,): the collision cost of the configuration is positive (mpb_collision_check);
    with_gap also returns that cost (the hinge sum)."""
    N, D = q.shape
    _chk(q, (N, D), 'q')
    if D != geom.n_dof:
        raise ValueError(f'q has {D} columns, the geometry {geom.n_dof} degrees of freedom')
    flag = torch.empty(N, device=q.device, dtype=torch.bool)
    gap = torch.empty(N, device=q.device, dtype=torch.float32) if with_gap else None
    _lib.check(_lib.lib().mpb_collision_check(_ptr(q), _ptr(geom.buf), int(geom.flags), _ptr(flag), _ptr(gap), N, D, _stream()),
               'mpb_collision_check')
    return (flag, gap) if with_gap else flag


# ---- the world: one in-kernel predicate over obstacles, SDF grid and the robot against itself (csrc/mpb_world.h) --------------------
def _robot_tables(host, hdr):
    """(kind, n_dof, joint_tf words, link rows (n_links, 5): frame, offset, radius) of a packed buffer's robot, from its host words."""
    f = np.asarray(host).view(np.float32)
    n_tf, n_links, o_tf, o_l = int(hdr['n_tf']), int(hdr['n_links']), int(hdr['off_tf']), int(hdr['off_links'])
    return (int(hdr['kind']) if 'kind' in hdr.dtype.names else KIND_CHAIN, int(hdr['n_dof']),
            f[o_tf:o_tf + 12 * n_tf].view(np.uint32), f[o_l:o_l + 8 * n_links].reshape(n_links, 8)[:, :5].view(np.uint32))


def check_world_parts(geom_host, sdf_host=None, self_host=None):
    """The robot-consistency check of DeviceWorld on HOST words (packed geometry, packed SDF-grid buffer or its words before the node
    section, packed self buffer): every part given must have been packed for the same robot -- kind, n_dof, the joint transforms bit
    for bit, and link rows (frame, offset, radius) that agree: the SDF and self buffers hold the whole link table and must hold the
    same one, the geometry's (statically pruned) rows must all be rows of it.  Raises ValueError naming the part."""
    from .sdf_layout import header as sdf_header
    from .self_layout import header as self_header
    kind, n_dof, tf, links = _robot_tables(geom_host, geometry_header(geom_host))
    whole = None
    for noun, host, hdr_of in (('SDF-grid', sdf_host, sdf_header), ('self-collision', self_host, self_header)):
        if host is None:
            continue
        k2, d2, tf2, links2 = _robot_tables(host, hdr_of(host))
        if d2 != n_dof:
            raise ValueError(f'DeviceWorld: the {noun} buffer was packed for a robot of n_dof = {d2}, the geometry for n_dof = {n_dof}')
        if k2 != kind:
            raise ValueError(f'DeviceWorld: the {noun} buffer was packed for another kind of robot (point / chain) than the geometry')
        if tf2.shape != tf.shape or not np.array_equal(tf2, tf):
            raise ValueError(f'DeviceWorld: the {noun} buffer was packed for another robot than the geometry (joint transforms differ)')
        if whole is not None and (links2.shape != whole.shape or not np.array_equal(links2, whole)):
            raise ValueError(f'DeviceWorld: the {noun} buffer was packed for another robot than the SDF-grid buffer (link tables differ)')
        whole = links2
    if whole is not None:
        rows = {r.tobytes() for r in whole}
        if any(r.tobytes() not in rows for r in links):
            raise ValueError('DeviceWorld: the geometry was packed for another robot than the other parts (a link row of its table is '
                             'not in theirs)')


class DeviceWorld:
    """What the in-kernel world predicate reads (csrc/mpb_world.h): a DeviceGeometry and, each optional, a DeviceSDFGrid
    and a DeviceSelfCollision, all packed for the same robot (check_world_parts).  A configuration is in collision iff one of the
    three stand-alone predicates says so.  Accepted wherever world_collision_check, rrt_init / rrt_connect_run on an RRT-Connect
    workspace, path_shortcut and traj_collision_stats accept a DeviceGeometry: they then call the *_world entries.  With neither
    optional part those entries launch the old kernels."""

    def __init__(self, geom, sdf=None, self_collision=None):
        if not isinstance(geom, DeviceGeometry):
            raise TypeError('DeviceWorld(geom, ...): geom must be a DeviceGeometry')
        if sdf is not None and not isinstance(sdf, DeviceSDFGrid):
            raise TypeError('DeviceWorld(..., sdf=): a DeviceSDFGrid or None')
        if self_collision is not None and not isinstance(self_collision, DeviceSelfCollision):
            raise TypeError('DeviceWorld(..., self_collision=): a DeviceSelfCollision or None')
        check_world_parts(geom.host, None if sdf is None else sdf.host, None if self_collision is None else self_collision.host)
        for part in (sdf, self_collision):
            if part is not None and part.buf.device != geom.buf.device:
                raise ValueError(f'DeviceWorld: its parts live on different devices ({geom.buf.device} and {part.buf.device})')
        self.geom, self.sdf, self.self_collision = geom, sdf, self_collision
        # (a DeviceWorld stands in for its geometry: the wrappers read these three of either)
        self.buf, self.flags, self.n_dof = geom.buf, geom.flags, geom.n_dof

    def extra(self):
        """(sdfb, selfb) as the *_world entries take them: null where a part is absent."""
        return _ptr(None if self.sdf is None else self.sdf.buf), _ptr(None if self.self_collision is None else self.self_collision.buf)


def _need_geometry(geom, what):
    if isinstance(geom, DeviceWorld):
        raise NotImplementedError(f'{what} reads the obstacle geometry alone and does not take a DeviceWorld; the world is served by '
                                  f'world_collision_check, rrt_connect_run, path_shortcut and traj_collision_stats')


@_on_tensor_device
def world_collision_check(q, world, with_parts=False):
    """(N, D) configurations -> bool (N,): in collision with the world -- obstacles, SDF grid or the robot itself -- in ONE launch
    (mpb_world_collision_check); with_parts also returns (N, 3) fp32 = (c_obs, c_sdf, c_self), the gaps of collision_check,
    sdf_grid_check and self_collision_check bit for bit, 0 where a part is absent."""
    if not isinstance(world, DeviceWorld):
        raise TypeError('world_collision_check takes an ops.DeviceWorld')
    N, D = q.shape
    _chk(q, (N, D), 'q')
    if D != world.n_dof:
        raise ValueError(f'q has {D} columns, the world {world.n_dof} degrees of freedom')
    flag = torch.empty(N, device=q.device, dtype=torch.bool)
    parts = torch.empty(N, 3, device=q.device, dtype=torch.float32) if with_parts else None
    sdfb, selfb = world.extra()
    _lib.check(_lib.lib().mpb_world_collision_check(_ptr(q), _ptr(world.buf), int(world.flags), sdfb, selfb, _ptr(flag), _ptr(parts), N, D,
                                                    _stream()), 'mpb_world_collision_check')
    return (flag, parts) if with_parts else flag


# ---- end effector: pose, Jacobian, batched inverse kinematics (csrc/mpb_ik.hip) ----------------------------------------------------
IK_MAX_ITERS, IK_MIN_DAMPING = 1024, 1e-2          # include/mpb.h MPB_IK_MAX_ITERS, MPB_IK_MIN_DAMPING


def _need_chain(geom, what):
    if geom.kind != KIND_CHAIN:
        raise ValueError(f'{what}: a point robot has no end effector (serial chains only)')


@_on_tensor_device
def fk_ee_pose(q, geom, with_jacobian=False):
    """(N, D) configurations -> the end-effector pose (N, 3, 4) = [R | t], the last frame of the chain walk; with_jacobian also
    returns the geometric Jacobian (N, 6, D): rows 0-2 z_j x (t - p_j), rows 3-5 z_j (mpb_fk_ee_pose)."""
    if q.dim() != 2:
        raise ValueError(f'q has shape {tuple(q.shape)}, expected (N, D)')
    N, D = q.shape
    _chk(q, (N, D), 'q')
    _need_chain(geom, 'fk_ee_pose')
    if D != geom.n_dof:
        raise ValueError(f'q has {D} columns, the geometry {geom.n_dof} degrees of freedom')
    pose = torch.empty(N, 3, 4, device=q.device, dtype=torch.float32)
    jac = torch.empty(N, 6, D, device=q.device, dtype=torch.float32) if with_jacobian else None
    _lib.check(_lib.lib().mpb_fk_ee_pose(_ptr(q), _ptr(geom.buf), _ptr(pose), _ptr(jac), N, D, _stream()), 'mpb_fk_ee_pose')
    return (pose, jac) if with_jacobian else pose


@_on_tensor_device
def ik_solve(target, q_seed, geom, q_min=None, q_max=None, n_iters=64, damping=0.1, pos_tol=1e-3, rot_tol=1e-2, position_only=False):
    """Damped-least-squares inverse kinematics of N targets from S seeds each (mpb_ik_solve): target (N, 3, 4) = [R* | t*], q_seed
    (N, S, D), q_min / q_max (D,) both or neither -> q (N, S, D), pos_err (N, S), rot_err (N, S), converged bool (N, S), iters int32
    (N, S), all at the returned q.  A fixed budget of n_iters steps per problem; a converged problem is frozen."""
    if q_seed.dim() != 3:
        raise ValueError(f'q_seed has shape {tuple(q_seed.shape)}, expected (N, S, D)')
    N, S, D = q_seed.shape
    _chk(q_seed, (N, S, D), 'q_seed')
    _chk(target, (N, 3, 4), 'target')
    _need_chain(geom, 'ik_solve')
    if D != geom.n_dof:
        raise ValueError(f'q_seed has {D} columns, the geometry {geom.n_dof} degrees of freedom')
    if (q_min is None) != (q_max is None):
        raise ValueError('q_min and q_max: both or neither')
    _chk(q_min, (D,), 'q_min', allow_none=True)
    _chk(q_max, (D,), 'q_max', allow_none=True)
    n_iters, damping, pos_tol, rot_tol = int(n_iters), float(damping), float(pos_tol), float(rot_tol)
    if not 0 <= n_iters <= IK_MAX_ITERS:
        raise ValueError(f'n_iters = {n_iters} outside 0..{IK_MAX_ITERS}')
    if not damping >= IK_MIN_DAMPING:
        raise ValueError(f'damping = {damping} below {IK_MIN_DAMPING}: the unpivoted fp32 Cholesky needs the floor')
    if not (pos_tol >= 0.0 and rot_tol >= 0.0):
        raise ValueError('pos_tol and rot_tol must not be negative')
    dev = q_seed.device
    q = torch.empty(N, S, D, device=dev, dtype=torch.float32)
    pos_err = torch.empty(N, S, device=dev, dtype=torch.float32)
    rot_err = torch.empty(N, S, device=dev, dtype=torch.float32)
    conv = torch.empty(N, S, device=dev, dtype=torch.bool)
    iters = torch.empty(N, S, device=dev, dtype=torch.int32)
    _lib.check(_lib.lib().mpb_ik_solve(_ptr(target), _ptr(q_seed), _ptr(geom.buf), _ptr(q_min), _ptr(q_max), _ptr(q), _ptr(pos_err),
                                       _ptr(rot_err), _ptr(conv), _ptr(iters), N, S, D, n_iters, damping, pos_tol, rot_tol,
                                       1 if position_only else 0, _stream()), 'mpb_ik_solve')
    return q, pos_err, rot_err, conv, iters


# ---- Cartesian end-effector moves: batched straight-line tracking (csrc/mpb_cartesian.hip) -----------------------------------------
# include/mpb.h MPB_CART_*
CART_OK, CART_LOST, CART_JUMP, CART_BAD_TARGET, CART_COLLISION = 0, 1, 2, 3, 4
CART_MAX_STEPS, CART_MAX_WORK, CART_MAX_TURN = 4096, 65536, 3.04159265


@_on_tensor_device
def cartesian_path(target, q_start, geom, n_steps, n_inner=8, damping=0.1, pos_tol=1e-3, rot_tol=1e-2, jump_max=0.5, position_only=False,
                   q_min=None, q_max=None):
    """Straight-line end-effector moves from S start configurations per target (mpb_cartesian_path): target (N, 3, 4) = [R* | t*],
    q_start (N, S, D), q_min / q_max (D,) both or neither -> q_path (N, S, K+1, D), pos_err, rot_err (N, S, K+1), n_ok int32 (N, S),
    status int32 (N, S) (CART_OK / CART_LOST / CART_JUMP / CART_BAD_TARGET), K = n_steps.  Step k follows the pose interpolated between
    the start's own pose and the target at k / K (straight line, geodesic), at most n_inner iterations of ik_solve from the last accepted
    configuration; a problem stops where tracking is lost or a joint would move by more than jump_max in one step, and holds still from
    there: rows beyond n_ok repeat row n_ok."""
    if q_start.dim() != 3:
        raise ValueError(f'q_start has shape {tuple(q_start.shape)}, expected (N, S, D)')
    N, S, D = q_start.shape
    _chk(q_start, (N, S, D), 'q_start')
    _chk(target, (N, 3, 4), 'target')
    _need_chain(geom, 'cartesian_path')
    if D != geom.n_dof:
        raise ValueError(f'q_start has {D} columns, the geometry {geom.n_dof} degrees of freedom')
    if (q_min is None) != (q_max is None):
        raise ValueError('q_min and q_max: both or neither')
    _chk(q_min, (D,), 'q_min', allow_none=True)
    _chk(q_max, (D,), 'q_max', allow_none=True)
    K, n_inner, damping, pos_tol, rot_tol, jump_max = int(n_steps), int(n_inner), float(damping), float(pos_tol), float(rot_tol), float(jump_max)
    if not 1 <= K <= CART_MAX_STEPS:
        raise ValueError(f'n_steps = {K} outside 1..{CART_MAX_STEPS}')
    if not 0 <= n_inner <= IK_MAX_ITERS:
        raise ValueError(f'n_inner = {n_inner} outside 0..{IK_MAX_ITERS}')
    if K * n_inner > CART_MAX_WORK:
        raise ValueError(f'n_steps * n_inner = {K * n_inner} beyond {CART_MAX_WORK}')
    if not damping >= IK_MIN_DAMPING:
        raise ValueError(f'damping = {damping} below {IK_MIN_DAMPING}: the unpivoted fp32 Cholesky needs the floor')
    if not (pos_tol >= 0.0 and rot_tol >= 0.0):
        raise ValueError('pos_tol and rot_tol must not be negative')
    if not jump_max > 0.0:
        raise ValueError(f'jump_max = {jump_max}: must be positive (inf turns the check off)')
    dev = q_start.device
    q_path = torch.empty(N, S, K + 1, D, device=dev, dtype=torch.float32)
    pos_err = torch.empty(N, S, K + 1, device=dev, dtype=torch.float32)
    rot_err = torch.empty(N, S, K + 1, device=dev, dtype=torch.float32)
    n_ok = torch.empty(N, S, device=dev, dtype=torch.int32)
    status = torch.empty(N, S, device=dev, dtype=torch.int32)
    _lib.check(_lib.lib().mpb_cartesian_path(_ptr(target), _ptr(q_start), _ptr(geom.buf), _ptr(q_min), _ptr(q_max), _ptr(q_path),
                                             _ptr(pos_err), _ptr(rot_err), _ptr(n_ok), _ptr(status), N, S, D, K, n_inner, damping, pos_tol,
                                             rot_tol, jump_max, 1 if position_only else 0, _stream()), 'mpb_cartesian_path')
    return q_path, pos_err, rot_err, n_ok, status


def _ee_cost_args(trajs, geom, target, k_pos, k_rot, axis, h_begin, h_end, target_per_waypoint, what):
    """The checks ee_cost_eval / ee_cost_grad share -> the C arguments after the pointers: (B, H, d, D, h_begin, h_end, group, stride_g,
    stride_h, k_pos, k_rot, use_axis, ax, ay, az)."""
    if trajs.dim() != 3:
        raise ValueError(f'trajs has shape {tuple(trajs.shape)}, expected (B, H, d)')
    B, H, d = trajs.shape
    _chk(trajs, (B, H, d), 'trajs')
    _need_chain(geom, what)
    D = geom.n_dof
    if d < D:
        raise ValueError(f'trajs has {d} columns, the chain {D} degrees of freedom')
    h_end = H if h_end is None else int(h_end)
    h_begin = int(h_begin)
    if not 0 <= h_begin < h_end <= H:
        raise ValueError(f'bad range [{h_begin}, {h_end}) of H = {H} waypoints')
    per = (H, 3, 4) if target_per_waypoint else (3, 4)
    if target is None or target.dim() not in (len(per), len(per) + 1) or tuple(target.shape[-len(per):]) != per:
        raise ValueError(f'target has shape {None if target is None else tuple(target.shape)}, expected {per} or (G,) + {per}')
    G = target.shape[0] if target.dim() == len(per) + 1 else 1
    _chk(target, target.shape, 'target')
    if G < 1 or B % G != 0:
        raise ValueError(f'{G} targets do not divide the batch of {B} trajectories')
    k_pos, k_rot = float(k_pos), float(k_rot)
    if not (0.0 <= k_pos < math.inf and 0.0 <= k_rot < math.inf):
        raise ValueError('k_pos and k_rot must be finite and not negative')
    if k_pos == 0.0 and k_rot == 0.0:
        raise ValueError('both terms are off (k_pos = k_rot = 0)')
    a = (0.0, 0.0, 0.0)
    if axis is not None:
        a = tuple(float(x) for x in np.asarray(axis, dtype=np.float64).reshape(-1))
        if len(a) != 3 or not abs(math.sqrt(sum(x * x for x in a)) - 1.0) <= 1e-3:
            raise ValueError(f'axis {a} is not a unit 3-vector (within 1e-3)')
        if k_rot == 0.0:
            raise ValueError('an axis needs the rotation term (k_rot > 0)')
    stride_h = 1 if target_per_waypoint else 0
    stride_g = 0 if G == 1 else (H if target_per_waypoint else 1)
    return (B, H, d, D, h_begin, h_end, max(B // G, 1), stride_g, stride_h, k_pos, k_rot, int(axis is not None)) + a


@_on_tensor_device
def ee_cost_eval(trajs, geom, target, k_pos=0.0, k_rot=0.0, axis=None, weight=1.0, h_begin=1, h_end=None, target_per_waypoint=False,
                 per_waypoint=False, out=None, accumulate=False):
    """trajs (B, H, d) -> out (B,) (+)= weight * sum_{h_begin <= h < h_end} c_h, the end-effector pose cost of a DeviceGeometry's chain
    (mpb_ee_cost_eval; include/mpb.h has the definition): c_h = k_pos |t* - t|^2 + k_rot (|e_w|^2, or |R a - R* a|^2 with `axis` = a, a
    unit vector of the tool frame).  target (3, 4) or (G, 3, 4) -- trajectory b reads target b // (B / G) --, with target_per_waypoint
    (H, 3, 4) or (G, H, 3, 4).  per_waypoint also returns c (B, H), un-scaled by weight, 0 outside the range."""
    args = _ee_cost_args(trajs, geom, target, k_pos, k_rot, axis, h_begin, h_end, target_per_waypoint, 'ee_cost_eval')
    B, H = args[0], args[1]
    out = _cost_out(trajs, out, accumulate)
    pw = torch.empty(B, H, device=trajs.device, dtype=torch.float32) if per_waypoint else None
    _lib.check(_lib.lib().mpb_ee_cost_eval(_ptr(trajs), _ptr(geom.buf), _ptr(target), _ptr(out), _ptr(pw), *args, float(weight),
                                          int(bool(accumulate)), _stream()), 'mpb_ee_cost_eval')
    return (out, pw) if per_waypoint else out


@_on_tensor_device
def ee_cost_grad(trajs, geom, target, k_pos=0.0, k_rot=0.0, axis=None, weight=1.0, h_begin=1, h_end=None, target_per_waypoint=False,
                 out=None, grad=None, accumulate=False):
    """(out (B,), grad (B, H, d)) (+)= the end-effector pose cost and d out / d trajs by the closed forms through the geometric Jacobian
    (mpb_ee_cost_grad); accumulate adds onto the given `out` AND onto the position channels of the range's rows of `grad` (nothing else
    is touched), otherwise every element of both is written (velocity channels and rows outside the range 0)."""
    args = _ee_cost_args(trajs, geom, target, k_pos, k_rot, axis, h_begin, h_end, target_per_waypoint, 'ee_cost_grad')
    B, H, d = args[0], args[1], args[2]
    if accumulate and grad is None:
        raise ValueError('accumulate needs existing out and grad buffers')
    out = _cost_out(trajs, out, accumulate)
    if grad is None:
        grad = torch.empty_like(trajs)
    else:
        _chk(grad, (B, H, d), 'grad')
    _lib.check(_lib.lib().mpb_ee_cost_grad(_ptr(trajs), _ptr(geom.buf), _ptr(target), _ptr(out), _ptr(grad), *args, float(weight),
                                          int(bool(accumulate)), _stream()), 'mpb_ee_cost_grad')
    return out, grad


@_on_tensor_device
def traj_collision_stats(trajs, geom, n_interp=5, with_flags=False):
    """(N, H, W) trajectories, W >= the geometry's degrees of freedom, read in place (the first D columns of a row are the
    joint positions, the others are never touched) -> per trajectory, over its P = (H-1)(n_interp+1)+1 dense points (the
    points of traj_interpolate, never stored): n_in_collision int32 (N,), first_in_collision int32 (N,) (-1: none),
    max_gap fp32 (N,) (the largest hinge sum, 0 when free); with_flags adds the per-point answers, bool (N, P)
    (mpb_traj_collision_stats)."""
    if not (isinstance(trajs, torch.Tensor) and trajs.is_cuda):
        raise _lib.MPBError('traj_collision_stats: trajs must be a GPU tensor; there is no CPU fallback')
    if trajs.dim() != 3:
        raise ValueError(f'trajs has shape {tuple(trajs.shape)}, expected (N, H, W)')
    N, H, W = trajs.shape
    _chk(trajs, (N, H, W), 'trajs')
    D, n = geom.n_dof, int(n_interp)
    if W < D:
        raise ValueError(f'trajs has {W} columns, the geometry {D} degrees of freedom')
    P = (H - 1) * (n + 1) + 1
    count = torch.empty(N, device=trajs.device, dtype=torch.int32)
    first = torch.empty(N, device=trajs.device, dtype=torch.int32)
    gap = torch.empty(N, device=trajs.device, dtype=torch.float32)
    flags = torch.empty(N, max(P, 0), device=trajs.device, dtype=torch.bool) if with_flags else None
    if isinstance(geom, DeviceWorld):
        # (the world predicate on the dense points; max_gap: the largest sum of the three parts)
        _lib.check(_lib.lib().mpb_traj_collision_stats_world(_ptr(trajs), W, _ptr(geom.buf), int(geom.flags), *geom.extra(), n, _ptr(count),
                                                             _ptr(first), _ptr(gap), _ptr(flags), N, H, D, _stream()),
                   'mpb_traj_collision_stats_world')
        return (count, first, gap, flags) if with_flags else (count, first, gap)
    _lib.check(_lib.lib().mpb_traj_collision_stats(_ptr(trajs), W, _ptr(geom.buf), int(geom.flags), n, _ptr(count), _ptr(first),
                                                   _ptr(gap), _ptr(flags), N, H, D, _stream()), 'mpb_traj_collision_stats')
    return (count, first, gap, flags) if with_flags else (count, first, gap)


class RRTWorkspace:
    """The caller-allocated state of a batch of RRT-Connect problems: trees, pool lists, status words (layout: rrt_layout.py)."""
    kind = 'connect'

    def __init__(self, B, max_nodes, n_pre, D, device):
        sym = f'mpb_rrt_{self.kind}_workspace_bytes'
        nbytes = int(getattr(_lib.lib(), sym)(int(B), int(max_nodes), int(n_pre), int(D)))
        if nbytes == 0:
            msg = _lib.lib().mpb_last_error()
            raise _lib.MPBError(f'{sym}: {msg.decode() if msg else "?"}')
        self.B, self.max_nodes, self.n_pre, self.D = int(B), int(max_nodes), int(n_pre), int(D)
        self.nbytes = nbytes
        self.buf = torch.zeros(nbytes // 4, device=device, dtype=torch.int32)


class RRTStarWorkspace(RRTWorkspace):
    """The caller-allocated state of a batch of RRT* problems: one tree per problem with parents, d and cost, the
    neighbour scratch, pool lists and the per-problem header of counters (layout: rrt_layout.py)."""
    kind = 'star'


@_on_tensor_device
def rrt_init(ws_buf, ws, start, goal, geom):
    """Roots (RRT*: the root and the goal), counts, pool lists, status words and the start / goal collision check of every problem, by
    the workspace's kind (mpb_rrt_connect_init, mpb_rrt_star_init).  `ws_buf` is ws.buf (passed so that the launch lands on its device)."""
    _chk(start, (ws.B, ws.D), 'start')
    _chk(goal, (ws.B, ws.D), 'goal')
    if ws.D != geom.n_dof:
        raise ValueError(f'the problems have {ws.D} columns, the geometry {geom.n_dof} degrees of freedom')
    if isinstance(geom, DeviceWorld):
        if ws.kind != 'connect':
            _need_geometry(geom, f'mpb_rrt_{ws.kind}_init')
        _lib.check(_lib.lib().mpb_rrt_connect_init_world(_ptr(ws_buf), ws.nbytes, _ptr(start), _ptr(goal), _ptr(geom.buf), int(geom.flags),
                                                         *geom.extra(), ws.B, ws.max_nodes, ws.n_pre, ws.D, _stream()),
                   'mpb_rrt_connect_init_world')
        return
    sym = f'mpb_rrt_{ws.kind}_init'
    _lib.check(getattr(_lib.lib(), sym)(_ptr(ws_buf), ws.nbytes, _ptr(start), _ptr(goal), _ptr(geom.buf), int(geom.flags), ws.B,
                                        ws.max_nodes, ws.n_pre, ws.D, _stream()), sym)


rrt_connect_init = rrt_star_init = rrt_init


def _rrt_run_shapes(ws, pre_samples, paths, lengths, status):
    """The checks both *_run wrappers make of the pool and of the outputs: (pre_stride, Lmax)."""
    if pre_samples.ndim == 2:
        _chk(pre_samples, (ws.n_pre, ws.D), 'pre_samples')
        stride = 0
    else:
        _chk(pre_samples, (ws.B, ws.n_pre, ws.D), 'pre_samples')
        stride = ws.n_pre * ws.D
    Lmax = paths.shape[1]
    _chk(paths, (ws.B, Lmax, ws.D), 'paths')
    _chk(lengths, (ws.B,), 'lengths', dtype=torch.int32)
    _chk(status, (ws.B,), 'status', dtype=torch.int32)
    return stride, Lmax


@_on_tensor_device
def rrt_connect_run(ws_buf, ws, geom, pre_samples, sample_idx, paths, lengths, status, iter0, n_iters, total_iters, step_size,
                    n_radius, seed=0, problem_offset=0):
    """Iterations iter0 .. min(iter0 + n_iters, total_iters) - 1 of every problem still RUNNING (mpb_rrt_connect_run).
    pre_samples (n_pre, D) shared or (B, n_pre, D) one pool per problem; sample_idx None (device Philox) or (B, total_iters) int32."""
    B, D = ws.B, ws.D
    stride, Lmax = _rrt_run_shapes(ws, pre_samples, paths, lengths, status)
    _chk(sample_idx, (B, total_iters), 'sample_idx', allow_none=True, dtype=torch.int32)
    if isinstance(geom, DeviceWorld):
        _lib.check(_lib.lib().mpb_rrt_connect_run_world(
            _ptr(ws_buf), ws.nbytes, _ptr(geom.buf), int(geom.flags), *geom.extra(), _ptr(pre_samples), stride, _ptr(sample_idx),
            _ptr(paths), _ptr(lengths), _ptr(status), B, ws.max_nodes, ws.n_pre, D, Lmax, int(iter0), int(n_iters), int(total_iters),
            float(step_size), float(n_radius), _seed64(seed), int(problem_offset) & 0xFFFFFFFF, _stream()), 'mpb_rrt_connect_run_world')
        return
    _lib.check(_lib.lib().mpb_rrt_connect_run(
        _ptr(ws_buf), ws.nbytes, _ptr(geom.buf), int(geom.flags), _ptr(pre_samples), stride, _ptr(sample_idx), _ptr(paths),
        _ptr(lengths), _ptr(status), B, ws.max_nodes, ws.n_pre, D, Lmax, int(iter0), int(n_iters), int(total_iters),
        float(step_size), float(n_radius), _seed64(seed), int(problem_offset) & 0xFFFFFFFF, _stream()), 'mpb_rrt_connect_run')


@_on_tensor_device
def rrt_star_run(ws_buf, ws, geom, pre_samples, sample_idx, goal_draw, paths, lengths, costs, status, iter0, n_iters, total_iters,
                 step_size, n_radius, max_best_cost_iters=1000, n_iters_after_success=None, informed=False, goal_prob=0.1,
                 cost_eps=1e-2, eps=1e-6, seed=0, problem_offset=0):
    """Loop bodies iter0 .. min(iter0 + n_iters, total_iters) - 1 of every problem still RUNNING (mpb_rrt_star_run).
    pre_samples (n_pre, D) shared or (B, n_pre, D); sample_idx and goal_draw both None (device Philox) or both
    (B, total_iters) int32.  paths / lengths / costs hold the current best path of every problem with a goal node after
    every call."""
    _need_geometry(geom, 'mpb_rrt_star_run')
    B, D = ws.B, ws.D
    stride, Lmax = _rrt_run_shapes(ws, pre_samples, paths, lengths, status)
    if (sample_idx is None) != (goal_draw is None):
        raise ValueError('sample_idx and goal_draw are given together or not at all')
    _chk(sample_idx, (B, total_iters), 'sample_idx', allow_none=True, dtype=torch.int32)
    _chk(goal_draw, (B, total_iters), 'goal_draw', allow_none=True, dtype=torch.int32)
    _chk(costs, (B,), 'costs')
    _lib.check(_lib.lib().mpb_rrt_star_run(
        _ptr(ws_buf), ws.nbytes, _ptr(geom.buf), int(geom.flags), _ptr(pre_samples), stride, _ptr(sample_idx), _ptr(goal_draw),
        _ptr(paths), _ptr(lengths), _ptr(costs), _ptr(status), B, ws.max_nodes, ws.n_pre, D, Lmax, int(iter0), int(n_iters),
        int(total_iters), int(max_best_cost_iters), -1 if n_iters_after_success is None else int(n_iters_after_success),
        1 if informed else 0, float(step_size), float(n_radius), float(goal_prob), float(cost_eps), float(eps), _seed64(seed),
        int(problem_offset) & 0xFFFFFFFF, _stream()), 'mpb_rrt_star_run')


def _rrt_read(kind, ws, hidden=()):
    """A workspace of `kind` as a dict of views, by walking rrt_layout's table: every header word and every section by its
    name there (fp32 words viewed as fp32, node rows cut to D columns, the pool words unpacked to one index per entry),
    less the names in `hidden`."""
    K, lay = rrt_layout.KINDS[kind], rrt_layout.offsets(kind, ws.B, ws.max_nodes, ws.n_pre, ws.D)
    w = ws.buf
    glob = dict(zip(rrt_layout.GLOBAL, w[:len(rrt_layout.GLOBAL)].tolist()))
    if glob != dict(magic=K.magic, B=ws.B, max_nodes=ws.max_nodes, n_pre=ws.n_pre, D=ws.D, Dp=lay.Dp):
        raise ValueError(f'the workspace was not initialised for these shapes (rrt_{kind}_init)')
    out = {}
    for name, (o, typ, shape) in lay.sections.items():
        t = w[o:o + math.prod(shape)]
        out[name] = (t.view(torch.float32) if typ == 'f4' else t).reshape(shape)
    hdr = out.pop('hdr')
    for name, (i, typ, n) in rrt_layout.header_index(kind).items():
        t = hdr[:, i:i + n] if n > 1 else hdr[:, i]
        out[name] = t.view(torch.float32) if typ == 'f4' else t
    out['nodes'] = out['nodes'][..., :ws.D]
    per, mask = rrt_layout.POOL_PER_WORD, (1 << rrt_layout.POOL_INDEX_BITS) - 1
    out['pool'] = torch.stack([(out['pool'] >> (rrt_layout.POOL_INDEX_BITS * k)) & mask for k in range(per)],
                              dim=-1).reshape(ws.B, per * lay.pool_words)[:, :ws.n_pre]
    return {name: t for name, t in out.items() if name not in hidden}


def rrt_connect_trees(ws):
    """The trees of a workspace, for tests and rendering: dict of `nodes` (B, 2, max_nodes, D) fp32, `parents`
    (B, 2, max_nodes) int32 (-1: root), `counts` (B, 2), `iters` (B,) iterations used, `status` (B,), `swap` (B,) and
    `pool_len` (B,), `pool` (B, n_pre) int32 (entries beyond pool_len are stale).  Tree 0 is rooted at the start, tree 1 at the goal."""
    return _rrt_read('connect', ws)


def rrt_star_tree(ws):
    """The trees of an RRT* workspace, for tests and rendering: dict of `nodes` (B, max_nodes, D) fp32, `parents`
    (B, max_nodes) int32 (-1: root), `d`, `cost` (B, max_nodes) fp32, `count`, `goal` (index, -1: none), `status`,
    `stop_reason`, `iters` (loop bodies started), `pool` (B, n_pre) int32 (entries beyond pool_len are stale), `pool_len`,
    `rewires`, `informed_rejections`, `best_cost_iters`, `iters_after_first_success`, and the first success: `first_cost`,
    `first_iter`, `first_count` (all (B,))."""
    return _rrt_read('star', ws, hidden=('goal_q', 'cand', 'best_cost_eps'))


# ---- space-time RRT-Connect among moving obstacles (csrc/mpb_strrt.hip; layout: strrt_layout.py) ------------------------------------
STRRT_STATUS_NAMES = strrt_layout.STATUS
(STRRT_RUNNING, STRRT_FOUND, STRRT_EXHAUSTED_ITERS, STRRT_START_OR_GOAL_IN_COLLISION, STRRT_HORIZON_TOO_SHORT, STRRT_TREE_FULL,
 STRRT_PATH_TOO_LONG) = range(len(STRRT_STATUS_NAMES))
STRRT_MIN_ROWS, STRRT_MAX_ROWS, STRRT_MAX_PRE_SAMPLES = strrt_layout.STRRT_MIN_ROWS, strrt_layout.STRRT_MAX_ROWS, strrt_layout.STRRT_MAX_PRE_SAMPLES
STRRT_LOG_WORDS, STRRT_LOG_NONE = strrt_layout.STRRT_LOG_WORDS, strrt_layout.STRRT_LOG_NONE


class STRRTWorkspace:
    """The caller-allocated state of a batch of space-time RRT-Connect problems: two trees per problem (configuration, row, parent), counts,
    status words (layout: strrt_layout.py)."""

    def __init__(self, B, max_nodes, D, n_rows, device):
        nbytes = int(_lib.lib().mpb_strrt_workspace_bytes(int(B), int(max_nodes), int(D)))
        if nbytes == 0:
            msg = _lib.lib().mpb_last_error()
            raise _lib.MPBError(f'mpb_strrt_workspace_bytes: {msg.decode() if msg else "?"}')
        self.B, self.max_nodes, self.D, self.n_rows = int(B), int(max_nodes), int(D), int(n_rows)
        self.nbytes = nbytes
        self.buf = torch.zeros(nbytes // 4, device=device, dtype=torch.int32)


def _strrt_scene(ws, geom, mo, w):
    """The checks both STRRT wrappers make of the scene: the static geometry, the moving buffer's rows, the per-row step limits."""
    if ws.D != geom.n_dof or ws.D != mo.n_dof:
        raise ValueError(f'the problems have {ws.D} columns, the geometry {geom.n_dof} and the moving-obstacle buffer {mo.n_dof} degrees of freedom')
    if ws.n_rows != mo.n_rows:
        raise ValueError(f'n_rows = {ws.n_rows}, the moving-obstacle buffer was packed for n_rows = {mo.n_rows}')
    _chk(w, (ws.D,), 'w')


@_on_tensor_device
def strrt_init(ws_buf, ws, start, goal, w, geom, mo):
    """Roots (start at row 0, goal at row n_rows - 1), counts and the first status word of every problem (mpb_strrt_init):
    START_OR_GOAL_IN_COLLISION by the predicate of those two rows, HORIZON_TOO_SHORT when max_k |goal - start|_k / w_k > n_rows - 1.
    w (D,) fp32: the most a joint may move per row.  `ws_buf` is ws.buf (passed so that the launch lands on its device)."""
    _chk(start, (ws.B, ws.D), 'start')
    _chk(goal, (ws.B, ws.D), 'goal')
    _strrt_scene(ws, geom, mo, w)
    _lib.check(_lib.lib().mpb_strrt_init(_ptr(ws_buf), ws.nbytes, _ptr(start), _ptr(goal), _ptr(w), _ptr(geom.buf), int(geom.flags),
                                         _ptr(mo.buf), ws.B, ws.max_nodes, ws.D, ws.n_rows, _stream()), 'mpb_strrt_init')


@_on_tensor_device
def strrt_run(ws_buf, ws, geom, mo, w, pre_samples, sample_idx, sample_row, trajs, vertex_q, vertex_row, n_vertices, status, iter0, n_iters,
              total_iters, max_step_rows, seed=0, problem_offset=0, log=None):
    """Iterations iter0 .. min(iter0 + n_iters, total_iters) - 1 of every problem still RUNNING (mpb_strrt_run).  pre_samples (n_pre, D)
    shared or (B, n_pre, D); sample_idx and sample_row both None (device Philox) or both (B, total_iters) int32; trajs (B, n_rows, D);
    vertex_q (B, Lmax, D), vertex_row (B, Lmax) and n_vertices (B,) int32; log None or (B, total_iters, STRRT_LOG_WORDS) int32 filled with
    STRRT_LOG_NONE by the caller."""
    B, D = ws.B, ws.D
    _strrt_scene(ws, geom, mo, w)
    n_pre = pre_samples.shape[-2]
    if pre_samples.ndim == 2:
        _chk(pre_samples, (n_pre, D), 'pre_samples')
        stride = 0
    else:
        _chk(pre_samples, (B, n_pre, D), 'pre_samples')
        stride = n_pre * D
    if (sample_idx is None) != (sample_row is None):
        raise ValueError('sample_idx and sample_row are given together or not at all')
    _chk(sample_idx, (B, total_iters), 'sample_idx', allow_none=True, dtype=torch.int32)
    _chk(sample_row, (B, total_iters), 'sample_row', allow_none=True, dtype=torch.int32)
    Lmax = vertex_q.shape[1]
    _chk(trajs, (B, ws.n_rows, D), 'trajs')
    _chk(vertex_q, (B, Lmax, D), 'vertex_q')
    _chk(vertex_row, (B, Lmax), 'vertex_row', dtype=torch.int32)
    _chk(n_vertices, (B,), 'n_vertices', dtype=torch.int32)
    _chk(status, (B,), 'status', dtype=torch.int32)
    _chk(log, (B, total_iters, STRRT_LOG_WORDS), 'log', allow_none=True, dtype=torch.int32)
    _lib.check(_lib.lib().mpb_strrt_run(
        _ptr(ws_buf), ws.nbytes, _ptr(geom.buf), int(geom.flags), _ptr(mo.buf), _ptr(w), _ptr(pre_samples), stride, _ptr(sample_idx),
        _ptr(sample_row), _ptr(trajs), _ptr(vertex_q), _ptr(vertex_row), _ptr(n_vertices), _ptr(status), _ptr(log), B, ws.max_nodes, n_pre, D,
        ws.n_rows, Lmax, int(max_step_rows), int(iter0), int(n_iters), int(total_iters), _seed64(seed), int(problem_offset) & 0xFFFFFFFF,
        _stream()), 'mpb_strrt_run')


def strrt_trees(ws):
    """The trees of a workspace, for tests and rendering: dict of `nodes` (B, 2, max_nodes, D) fp32, `rows` and `parents`
    (B, 2, max_nodes) int32 (-1: root), `counts` (B, 2), `iters` (B,) iterations used, `status` (B,) and `rejected_joins` (B,).  Tree 0 is
    rooted at (start, row 0), tree 1 at (goal, row n_rows - 1)."""
    lay = strrt_layout.offsets(ws.B, ws.max_nodes, ws.D)
    w = ws.buf
    glob = dict(zip(strrt_layout.GLOBAL, w[:len(strrt_layout.GLOBAL)].tolist()))
    if glob != dict(magic=strrt_layout.STRRT_MAGIC, B=ws.B, max_nodes=ws.max_nodes, D=ws.D, Dp=lay.Dp, n_rows=ws.n_rows):
        raise ValueError('the workspace was not initialised for these shapes (strrt_init)')
    out = {}
    for name, (o, typ, shape) in lay.sections.items():
        t = w[o:o + math.prod(shape)]
        out[name] = (t.view(torch.float32) if typ == 'f4' else t).reshape(shape)
    hdr = out.pop('hdr')
    for name, (i, typ, n) in strrt_layout.header_index().items():
        out[name] = hdr[:, i:i + n] if n > 1 else hdr[:, i]
    out['nodes'] = out['nodes'][..., :ws.D]
    return out


# ---- timing of geometric paths among moving obstacles (csrc/mpb_path_timing.hip; numbers: path_timing_layout.py) ----------------------
PT_STATUS_NAMES = path_timing_layout.STATUS
PT_FOUND, PT_START_BLOCKED, PT_GOAL_NOT_HOLDABLE, PT_SEGMENT_TOO_LONG, PT_NO_TIMING, PT_BUFFER_CHANGED = range(len(PT_STATUS_NAMES))
PathTiming = collections.namedtuple('PathTiming', 'trajs found status arrival_row idx free_table')


@_on_tensor_device
def path_time_plan(paths, mo, w, blocked=None, with_table=False):
    """paths (N, S, D) fp32 -- sample 0 the start, sample S - 1 the goal -- timed on the row grid of a DeviceMovingObstacles `mo`
    (mpb_path_time_plan; include/mpb.h has the definition): at which row to stand on which sample, advancing or waiting, so that every
    row is free at its own time.  w (D,) fp32: the most a joint may move per row.  blocked: None or (N, S) bool / uint8, True = the sample
    is refused by a static predicate of the caller's.  Returns a PathTiming: trajs (N, n_rows, D) (zero where no timing was found), found
    (N,) bool, status (N,) int32 (PT_*), arrival_row (N,) int32 and idx (N, n_rows) int32 (-1 where none was found), free_table
    (N, n_rows, S) bool with with_table, else None."""
    if not isinstance(mo, DeviceMovingObstacles):
        raise TypeError('path_time_plan takes a DeviceMovingObstacles')
    if paths.dim() != 3:
        raise ValueError(f'paths has shape {tuple(paths.shape)}, expected (N, S, D)')
    N, S, D = paths.shape
    _chk(paths, (N, S, D), 'paths')
    R = mo.n_rows
    if D != mo.n_dof:
        raise ValueError(f'paths has D = {D} columns, the moving-obstacle buffer\'s robot {mo.n_dof} degrees of freedom')
    L = path_timing_layout
    if not L.PT_MIN_SAMPLES <= S <= L.PT_MAX_SAMPLES:
        raise ValueError(f'n_samples = {S} outside {L.PT_MIN_SAMPLES} .. PT_MAX_SAMPLES = {L.PT_MAX_SAMPLES}')
    if not L.PT_MIN_ROWS <= R <= L.PT_MAX_ROWS:
        raise ValueError(f'n_rows = {R} outside {L.PT_MIN_ROWS} .. PT_MAX_ROWS = {L.PT_MAX_ROWS}')
    need = L.lds_bytes(mo.n_links, S, R)
    if need > L.PT_MAX_LDS_BYTES:
        raise ValueError(f'{mo.n_links} collision spheres x {S} samples over {R} rows need {need} bytes of LDS, above PT_MAX_LDS_BYTES = '
                         f'{L.PT_MAX_LDS_BYTES}: fewer samples or a robot with fewer spheres')
    _chk(w, (D,), 'w')
    if blocked is not None:
        if blocked.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f'blocked must be bool or uint8 (got {blocked.dtype})')
        _chk(blocked, (N, S), 'blocked', dtype=blocked.dtype)
    dev = paths.device
    trajs = torch.empty(N, R, D, device=dev, dtype=torch.float32)
    idx = torch.empty(N, R, device=dev, dtype=torch.int32)
    arrival, status = torch.empty(N, device=dev, dtype=torch.int32), torch.empty(N, device=dev, dtype=torch.int32)
    table = torch.empty(N, R, S, device=dev, dtype=torch.bool) if with_table else None
    _lib.check(_lib.lib().mpb_path_time_plan(_ptr(paths), _ptr(mo.buf), _ptr(w), _ptr(blocked), _ptr(trajs), _ptr(idx), _ptr(arrival),
                                             _ptr(status), _ptr(table), N, S, D, R, _stream()), 'mpb_path_time_plan')
    return PathTiming(trajs, status == PT_FOUND, status, arrival, idx, table)


# ---- space-time shortcutting of timed trajectories among moving obstacles (csrc/mpb_st_shortcut.hip; numbers: st_shortcut_layout.py) --
STS_STATUS_NAMES = st_shortcut_layout.STATUS
STS_OK, STS_NOT_VALID, STS_BUFFER_CHANGED, STS_INPUT_IN_COLLISION, STS_INPUT_TOO_FAST = range(len(STS_STATUS_NAMES))
STS_LOG_CODES = st_shortcut_layout.LOG_CODES
STS_LOG_IDLE, STS_LOG_SKIP_SHORT, STS_LOG_SKIP_FAST, STS_LOG_SKIP_STRAIGHT, STS_LOG_REJECT, STS_LOG_ACCEPT = range(len(STS_LOG_CODES))
STS_LOG_INDEX_SHIFT, STS_MAX_ITERS = st_shortcut_layout.STS_LOG_INDEX_SHIFT, st_shortcut_layout.STS_MAX_ITERS
STShortcut = collections.namedtuple('STShortcut', 'trajs ok status first_bad stats log')


@_on_tensor_device
def st_shortcut(trajs, geom, mo, w, n_iters, draws=None, seed=0, problem_offset=0, valid=None, max_span=0, with_log=False, out=None):
    """Shortcut N dense trajectories (N, R, D) fp32 on the clock of a DeviceMovingObstacles `mo` packed for R rows in one launch
    (mpb_st_shortcut; include/mpb.h has the definition): n_iters times per trajectory two rows a < b are drawn and the rows between them
    are replaced by the constant-velocity straight piece when that piece moves no joint k by more than w_k per row and every new row is
    free at its own time -- of geom's static obstacles and of mo's obstacles of that row.  The row count, and so the clock, never changes.
    geom: the DeviceGeometry of the static scene.  w (D,) fp32: the most a joint may move per row.  draws: None (device Philox;
    trajectory n draws from stream problem_offset + n of `seed`) or (N, n_iters, 2) int32 recorded rows.  valid: None or (N,) bool /
    uint8, False = pass the trajectory through.  max_span: 0 (no limit) or the most rows a piece may span.  out: None (a new tensor) or
    the (N, R, D) tensor to write into; it may be `trajs` itself (in place).
    Returns an STShortcut: trajs (N, R, D); ok (N,) bool; status (N,) int32 (STS_*: only OK trajectories are edited, every other one
    comes out with its input bits); first_bad (N,) int32, the first row the input gate refuses or -1; stats (N, 4) fp32: candidates
    checked, accepted, length before, length after (NaN where not OK); log (N, n_iters) int32 with with_log (STS_LOG_* | first colliding
    row << STS_LOG_INDEX_SHIFT), else None."""
    if not isinstance(geom, DeviceGeometry):
        raise TypeError('st_shortcut takes the DeviceGeometry of the static scene')
    if not isinstance(mo, DeviceMovingObstacles):
        raise TypeError('st_shortcut takes a DeviceMovingObstacles')
    if not (isinstance(trajs, torch.Tensor) and trajs.dim() == 3):
        raise ValueError(f'trajs has shape {tuple(getattr(trajs, "shape", ()))}, expected (N, R, D)')
    N, R, D = trajs.shape
    _chk(trajs, (N, R, D), 'trajs')
    L = st_shortcut_layout
    if D != geom.n_dof or D != mo.n_dof:
        raise ValueError(f'trajs has D = {D} columns, the geometry {geom.n_dof} and the moving-obstacle buffer {mo.n_dof} degrees of freedom')
    if R != mo.n_rows:
        raise ValueError(f'trajs has n_rows = {R}, the moving-obstacle buffer was packed for n_rows = {mo.n_rows}')
    if not L.STS_MIN_ROWS <= R <= L.STS_MAX_ROWS:
        raise ValueError(f'n_rows = {R} outside {L.STS_MIN_ROWS} .. STS_MAX_ROWS = {L.STS_MAX_ROWS}')
    n_iters, max_span = int(n_iters), int(max_span)
    if not 0 <= n_iters <= L.STS_MAX_ITERS:
        raise ValueError(f'n_iters = {n_iters} outside 0 .. STS_MAX_ITERS = {L.STS_MAX_ITERS}')
    if max_span < 0:
        raise ValueError(f'max_span = {max_span}: 0 (no limit) or a positive row count')
    need = L.lds_bytes(R, D)
    if need > L.STS_MAX_LDS_BYTES:
        raise ValueError(f'{R} rows of D = {D} need {need} bytes of LDS, above STS_MAX_LDS_BYTES = {L.STS_MAX_LDS_BYTES}: fewer rows')
    _chk(w, (D,), 'w')
    _chk(draws, (N, n_iters, 2), 'draws', allow_none=True, dtype=torch.int32)
    if valid is not None:
        if valid.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f'valid must be bool or uint8 (got {valid.dtype})')
        _chk(valid, (N,), 'valid', dtype=valid.dtype)
    if out is None:
        out = torch.empty_like(trajs)
    else:
        _chk(out, (N, R, D), 'out')
    dev = trajs.device
    status, first_bad = torch.empty(N, device=dev, dtype=torch.int32), torch.empty(N, device=dev, dtype=torch.int32)
    stats = torch.empty(N, 4, device=dev, dtype=torch.float32)
    log = torch.empty(N, n_iters, device=dev, dtype=torch.int32) if with_log else None
    _lib.check(_lib.lib().mpb_st_shortcut(_ptr(trajs), _ptr(out), _ptr(geom.buf), int(geom.flags), _ptr(mo.buf), _ptr(w), _ptr(valid),
                                          _ptr(draws), _ptr(status), _ptr(first_bad), _ptr(stats), _ptr(log), N, R, D, n_iters, max_span,
                                          _seed64(seed), int(problem_offset) & 0xFFFFFFFF, _stream()), 'mpb_st_shortcut')
    return STShortcut(out, status == STS_OK, status, first_bad, stats, log)


# ---- path shortcutting between the tree and the optimiser (csrc/mpb_path_shortcut.hip) ---------------------------------------------
# include/mpb.h MPB_SHORTCUT_*: the codes of the log's low bits, the shift of the first-collision index, the bound of n_iters
SHORTCUT_CODES = ('IDLE', 'SKIP', 'REJECT', 'OVERFLOW', 'ACCEPT')
SHORTCUT_IDLE, SHORTCUT_SKIP, SHORTCUT_REJECT, SHORTCUT_OVERFLOW, SHORTCUT_ACCEPT = range(5)
SHORTCUT_LOG_INDEX_SHIFT, SHORTCUT_MAX_ITERS = 8, 1 << 20
SHORTCUT_PHILOX_TAG = 0x53484354                # word 2 of the Philox counter (csrc/mpb_path_shortcut.hip SC_TAG)


@_on_tensor_device
def path_shortcut(paths, lengths, geom, n_iters, check_step, draws=None, seed=0, problem_offset=0, with_log=False, out=None):
    """Shortcut N padded polylines (paths (N, Lmax, D), lengths (N,) int32 -- what optimize_batched of the RRT planners returns) in
    one launch (mpb_path_shortcut; include/mpb.h has the definition): n_iters times per path two draws pick two points on the
    polyline, and the nodes between them are replaced by the straight segment when that is collision-free at spacing check_step.
    draws: None (device Philox; path b draws from stream problem_offset + b of `seed`) or (N, n_iters, 2) fp32 recorded uniforms.
    out: None (new tensors) or (paths, lengths) to write into; out[0] may be `paths` itself (in place).
    Returns (paths, lengths, stats (N, 4) fp32: candidates checked, accepted, length before, length after[, log (N, n_iters) int32:
    SHORTCUT_* | first index in collision << SHORTCUT_LOG_INDEX_SHIFT])."""
    if not (isinstance(paths, torch.Tensor) and paths.dim() == 3):
        raise ValueError(f'paths has shape {tuple(getattr(paths, "shape", ()))}, expected (N, Lmax, D)')
    N, Lmax, D = paths.shape
    _chk(paths, (N, Lmax, D), 'paths')
    _chk(lengths, (N,), 'lengths', dtype=torch.int32)
    if D != geom.n_dof:
        raise ValueError(f'paths has {D} columns, the geometry {geom.n_dof} degrees of freedom')
    n_iters = int(n_iters)
    _chk(draws, (N, n_iters, 2), 'draws', allow_none=True)
    if out is None:
        paths_out, lengths_out = torch.empty_like(paths), torch.empty_like(lengths)
    else:
        paths_out, lengths_out = out
        _chk(paths_out, (N, Lmax, D), 'out[0]')
        _chk(lengths_out, (N,), 'out[1]', dtype=torch.int32)
    stats = torch.empty(N, 4, device=paths.device, dtype=torch.float32)
    log = torch.empty(N, max(n_iters, 0), device=paths.device, dtype=torch.int32) if with_log else None
    if isinstance(geom, DeviceWorld):
        _lib.check(_lib.lib().mpb_path_shortcut_world(_ptr(paths), _ptr(lengths), _ptr(paths_out), _ptr(lengths_out), _ptr(stats), _ptr(log),
                                                      _ptr(geom.buf), int(geom.flags), *geom.extra(), _ptr(draws), N, Lmax, D, n_iters,
                                                      float(check_step), _seed64(seed), int(problem_offset) & 0xFFFFFFFF, _stream()),
                   'mpb_path_shortcut_world')
        return (paths_out, lengths_out, stats, log) if with_log else (paths_out, lengths_out, stats)
    _lib.check(_lib.lib().mpb_path_shortcut(_ptr(paths), _ptr(lengths), _ptr(paths_out), _ptr(lengths_out), _ptr(stats), _ptr(log),
                                            _ptr(geom.buf), int(geom.flags), _ptr(draws), N, Lmax, D, n_iters, float(check_step),
                                            _seed64(seed), int(problem_offset) & 0xFFFFFFFF, _stream()), 'mpb_path_shortcut')
    return (paths_out, lengths_out, stats, log) if with_log else (paths_out, lengths_out, stats)


# ---- batched PRM: one roadmap, many start / goal queries (csrc/mpb_prm.hip) ------------------------------------------------------------
# include/mpb.h MPB_PRM_*: the limits, the edge flags, the query statuses, the shortest edge a roadmap keeps
PRM_MAX_NODES, PRM_MAX_K, PRM_MAX_PATH_ROWS, PRM_MIN_EDGE = 16384, 32, 1 << 20, 1e-4
PRM_EDGE_FLAGS = ('FREE', 'BLOCKED', 'BAD_INDEX', 'TOO_LONG')
PRM_EDGE_FREE, PRM_EDGE_BLOCKED, PRM_EDGE_BAD_INDEX, PRM_EDGE_TOO_LONG = range(4)
PRM_STATUS = ('OK', 'NO_START', 'NO_GOAL', 'DISCONNECTED', 'PATH_TOO_LONG', 'DEGENERATE')
PRM_OK, PRM_NO_START, PRM_NO_GOAL, PRM_DISCONNECTED, PRM_PATH_TOO_LONG, PRM_DEGENERATE = range(6)


def _rows(t, name):
    if not (isinstance(t, torch.Tensor) and t.dim() == 2):
        raise ValueError(f'{name} has shape {tuple(getattr(t, "shape", ()))}, expected two dimensions')
    return t.shape


@_on_tensor_device
def prm_knn(queries, nodes, K, exclude_self=False):
    """The K nearest rows of nodes (M, D) to every row of queries (Q, D) in one launch (mpb_prm_knn): -> (idx (Q, K) int32, dist (Q, K)
    fp32), each row in ascending order of (squared distance, index); the distance is the sequential fp32 sum of the shortcut pass.
    exclude_self: the queries are the nodes, and node i is left out of row i."""
    Q, D = _rows(queries, 'queries')
    M = _rows(nodes, 'nodes')[0]
    _chk(queries, (Q, D), 'queries')
    _chk(nodes, (M, D), 'nodes')
    K = int(K)
    idx = torch.empty(Q, max(K, 0), device=queries.device, dtype=torch.int32)
    dist = torch.empty(Q, max(K, 0), device=queries.device, dtype=torch.float32)
    if Q == 0 and 1 <= K <= PRM_MAX_K:                          # (an empty tensor has no address to hand over)
        return idx, dist
    _lib.check(_lib.lib().mpb_prm_knn(_ptr(queries), _ptr(nodes), _ptr(idx), _ptr(dist), Q, M, D, K, 1 if exclude_self else 0, _stream()),
               'mpb_prm_knn')
    return idx, dist


@_on_tensor_device
def prm_edge_check(pts, pairs, geom, check_step):
    """The straight segments between rows of pts (P, D) that pairs (E, 2) int32 name, scanned as the shortcut pass scans a candidate at
    spacing check_step, one wave per edge in one launch (mpb_prm_edge_check): -> (flag (E,) int32 PRM_EDGE_*, first (E,) int32: the index
    of the first point in collision of a BLOCKED edge, else -1)."""
    P, D = _rows(pts, 'pts')
    E = _rows(pairs, 'pairs')[0]
    _chk(pts, (P, D), 'pts')
    _chk(pairs, (E, 2), 'pairs', dtype=torch.int32)
    if D != geom.n_dof:
        raise ValueError(f'pts has {D} columns, the geometry {geom.n_dof} degrees of freedom')
    flag = torch.empty(E, device=pts.device, dtype=torch.int32)
    first = torch.empty(E, device=pts.device, dtype=torch.int32)
    if E == 0:                                                   # (an empty tensor has no address to hand over)
        return flag, first
    _lib.check(_lib.lib().mpb_prm_edge_check(_ptr(pts), _ptr(pairs), _ptr(flag), _ptr(first), _ptr(geom.buf), int(geom.flags), P, E, D,
                                             float(check_step), _stream()), 'mpb_prm_edge_check')
    return flag, first


@_on_tensor_device
def prm_query(nodes, nbr, w, starts, goals, cs, ws, cg, wg, direct, max_path_nodes):
    """Q start / goal queries against one roadmap in one launch, one workgroup per query (mpb_prm_query; include/mpb.h has the
    definition).  The roadmap: nodes (M, D), nbr (M, K) int32, w (M, K) (+inf: no edge); per query the connection tables cs, cg (Q, Kc)
    int32 with ws, wg (Q, Kc) and direct (Q,) (the start-goal distance where that segment is free, else +inf).
    -> (paths (Q, max_path_nodes, D), lengths (Q,) int32, costs (Q,), status (Q,) int32 PRM_*)."""
    M, D = _rows(nodes, 'nodes')
    K = _rows(nbr, 'nbr')[1]
    Q = _rows(starts, 'starts')[0]
    Kc = _rows(cs, 'cs')[1]
    _chk(nodes, (M, D), 'nodes')
    _chk(nbr, (M, K), 'nbr', dtype=torch.int32)
    _chk(w, (M, K), 'w')
    _chk(starts, (Q, D), 'starts')
    _chk(goals, (Q, D), 'goals')
    for t, name in ((cs, 'cs'), (cg, 'cg')):
        _chk(t, (Q, Kc), name, dtype=torch.int32)
    for t, name in ((ws, 'ws'), (wg, 'wg')):
        _chk(t, (Q, Kc), name)
    _chk(direct, (Q,), 'direct')
    Lmax = int(max_path_nodes)
    paths = torch.empty(Q, max(Lmax, 0), D, device=nodes.device, dtype=torch.float32)
    lengths = torch.empty(Q, device=nodes.device, dtype=torch.int32)
    costs = torch.empty(Q, device=nodes.device, dtype=torch.float32)
    status = torch.empty(Q, device=nodes.device, dtype=torch.int32)
    if Q == 0 and Lmax >= 2:                                     # (an empty tensor has no address to hand over)
        return paths, lengths, costs, status
    _lib.check(_lib.lib().mpb_prm_query(_ptr(nodes), _ptr(nbr), _ptr(w), _ptr(starts), _ptr(goals), _ptr(cs), _ptr(ws), _ptr(cg), _ptr(wg),
                                        _ptr(direct), _ptr(paths), _ptr(lengths), _ptr(costs), _ptr(status), Q, M, K, Kc, D, Lmax, _stream()),
               'mpb_prm_query')
    return paths, lengths, costs, status


# ---- time parameterisation under joint limits (csrc/mpb_retime.hip) --------------------------------------------------------------------
# include/mpb.h MPB_RETIME_*: the per-trajectory status of the timing and of the sampler
RETIME_STATUS = ('OK', 'STALLED', 'TOO_LONG')
RETIME_OK, RETIME_STALLED, RETIME_TOO_LONG = range(3)

TrajTiming = collections.namedtuple('TrajTiming', 'x u t qd status duration')
TrajTiming.__doc__ = """What traj_retime returns: x (N, H) = sdot^2 at the waypoints, u (N, H-1) = sddot on the intervals, t (N, H) the
times of the waypoints, qd (N, H, D) the joint velocities there, status (N,) int32 RETIME_OK / RETIME_STALLED, duration (N,) = t[:, -1]
(a view)."""


def _retime_trajs(trajs, what):
    if not (isinstance(trajs, torch.Tensor) and trajs.is_cuda):
        raise _lib.MPBError(f'{what}: trajs must be a GPU tensor; there is no CPU fallback')
    if trajs.dim() != 3:
        raise ValueError(f'trajs has shape {tuple(trajs.shape)}, expected (N, H, W)')
    _chk(trajs, tuple(trajs.shape), 'trajs')
    return trajs.shape


@_on_tensor_device
def traj_retime(trajs, v_max, a_max, sdot_max=1e3, t_max=1e4):
    """The time-optimal rest-to-rest timing along each of N waypoint trajectories under per-joint velocity / acceleration limits, in one
    launch (mpb_traj_retime; include/mpb.h has the definition: TOPP-RA for limits symmetric about zero).  trajs (N, H, W) is read in
    place, the first D = len(v_max) columns of a row are the joint positions (a planner's (N, H, 2D) state output is read as it is).
    v_max, a_max: (D,) finite and > 0 (rad/s, rad/s^2); sdot_max caps the path speed (waypoints/s) where the path does not move; a
    trajectory longer than t_max seconds is STALLED -- repeated waypoints do that, purge them.

    GUARANTEE: the limits hold AT the waypoints, to rounding.  Between them they do not: a cubic through smooth Panda trajectories
    sampled at 1 ms oversteps the velocity limit by 0.9 % at H = 64 and 10 % at H = 16, the acceleration limit by 28 % / 70 %, and a
    polyline with corners by a factor 3.9 in acceleration.  The answer is a denser input (traj_interpolate) or scaled limits; nothing
    is clamped here.  Returns a TrajTiming."""
    N, H, W = _retime_trajs(trajs, 'traj_retime')
    lim = []
    for t, name in ((v_max, 'v_max'), (a_max, 'a_max')):
        t = torch.as_tensor(t, dtype=torch.float32)
        if t.dim() != 1 or not bool(torch.isfinite(t).all()) or not bool((t > 0).all()):
            raise ValueError(f'{name} must be a vector of finite limits > 0 (got {t.tolist() if t.dim() == 1 else tuple(t.shape)})')
        lim.append(t.to(trajs.device).contiguous())
    D = lim[0].numel()
    if lim[1].numel() != D or not 1 <= D <= W:
        raise ValueError(f'v_max has {D} entries, a_max {lim[1].numel()}, the rows of trajs {W} columns')
    dev = trajs.device
    x, t = torch.empty(N, H, device=dev), torch.empty(N, H, device=dev)
    u = torch.empty(N, max(H - 1, 0), device=dev)
    qd = torch.empty(N, H, D, device=dev)
    status = torch.empty(N, device=dev, dtype=torch.int32)
    if N > 0:                                                    # (an empty tensor has no address to hand over)
        _lib.check(_lib.lib().mpb_traj_retime(_ptr(trajs), W, _ptr(lim[0]), _ptr(lim[1]), _ptr(x), _ptr(u), _ptr(t), _ptr(qd), _ptr(status),
                                              N, H, D, float(sdot_max), float(t_max), _stream()), 'mpb_traj_retime')
    return TrajTiming(x, u, t, qd, status, t[:, -1] if H else t.reshape(N))


@_on_tensor_device
def traj_retime_sample(trajs, timing, dt, n_rows=None):
    """trajs (N, H, W) and their TrajTiming -> the trajectories at the fixed control period dt, in one launch (mpb_traj_retime_sample):
    (out (N, n_rows, 2D) positions and velocities, rows (N,) int32, status (N,) int32).  Row k is the state at k dt: a cubic Hermite of the
    two waypoints around it; rows at and past a trajectory's own rows[n] = ceil(T / dt) + 1 hold its last waypoint at rest.  n_rows=None
    reads the longest duration back (one synchronisation) and sizes the output to it.  A trajectory with more rows than n_rows is
    RETIME_TOO_LONG (the rows that fit are written); a STALLED one has rows 0 and holds its first waypoint."""
    N, H, W = _retime_trajs(trajs, 'traj_retime_sample')
    D = timing.qd.shape[-1]
    _chk(timing.x, (N, H), 'timing.x')
    _chk(timing.u, (N, max(H - 1, 0)), 'timing.u')
    _chk(timing.t, (N, H), 'timing.t')
    _chk(timing.status, (N,), 'timing.status', dtype=torch.int32)
    if D > W:
        raise ValueError(f'the timing is of {D} joints, the rows of trajs have {W} columns')
    dt = float(dt)
    if n_rows is None:
        if not (dt > 0 and math.isfinite(dt)):
            raise ValueError(f'dt = {dt}: a finite period > 0')
        ok = (timing.status == RETIME_OK) & torch.isfinite(timing.duration)
        T = float(torch.where(ok, timing.duration, torch.zeros_like(timing.duration)).max()) if N else 0.0
        n_rows = int(math.ceil(T / float(np.float32(dt)))) + 1
    n_rows = int(n_rows)
    out = torch.empty(N, max(n_rows, 0), 2 * D, device=trajs.device)
    rows = torch.empty(N, device=trajs.device, dtype=torch.int32)
    status = torch.empty(N, device=trajs.device, dtype=torch.int32)
    if N > 0:
        _lib.check(_lib.lib().mpb_traj_retime_sample(_ptr(trajs), W, _ptr(timing.x), _ptr(timing.u), _ptr(timing.t), _ptr(timing.status),
                                                     _ptr(out), _ptr(rows), _ptr(status), N, H, D, dt, n_rows, _stream()),
                   'mpb_traj_retime_sample')
    return out, rows, status


# ---- linear segments with parabolic blends (csrc/mpb_path_blend.hip; the definition: include/mpb.h; blend_layout.py) ------
BLEND_STATUS = blend_layout.STATUS
BLEND_OK, BLEND_NOT_CONVERGED, BLEND_DEGENERATE_SEGMENT, BLEND_BAD_INPUT, BLEND_TOO_LONG = range(len(BLEND_STATUS))

BlendTiming = collections.namedtuple('BlendTiming', 'T tb tw dev duration sweeps status first_bad lengths max_deviation n_dof')
BlendTiming.__doc__ = """What path_blend returns: T (N, H-1) the segment durations, tb (N, H) the blend durations, tw (N, H) the times of
the waypoints, dev (N, H) = max_k |dv_ik| tb_i / 8 how far the blend of waypoint i leaves the polyline (joint-space infinity-norm),
duration (N,), sweeps (N,) int32 rescalings made, status (N,) int32 BLEND_OK / BLEND_NOT_CONVERGED / BLEND_DEGENERATE_SEGMENT /
BLEND_BAD_INPUT, first_bad (N,) int32 the segment of a DEGENERATE_SEGMENT (-1 otherwise); lengths (N,) int32 or None, max_deviation
and n_dof = D as the launch took them.  A path that is not OK has zeros everywhere, an OK one at and past its length."""


def _blend_paths(paths, lengths, what):
    if not (isinstance(paths, torch.Tensor) and paths.is_cuda):
        raise _lib.MPBError(f'{what}: paths must be a GPU tensor; there is no CPU fallback')
    if paths.dim() != 3:
        raise ValueError(f'paths has shape {tuple(paths.shape)}, expected (N, H, W)')
    _chk(paths, tuple(paths.shape), 'paths')
    _chk(lengths, (paths.shape[0],), 'lengths', allow_none=True, dtype=torch.int32)
    return paths.shape


@_on_tensor_device
def path_blend(paths, v_max, a_max, lengths=None, max_deviation=None, max_sweeps=blend_layout.BLEND_DEFAULT_MAX_SWEEPS):
    """N joint-space polylines -> linear segments with parabolic blends under per-joint velocity / acceleration limits, in one launch
    (mpb_path_blend; include/mpb.h has the definition, DESIGN.md 10 the proofs).  paths (N, H, W) is read in place, the first
    D = len(v_max) columns of a row are the joint positions; lengths (N,) int32 or None: path n is the polyline through its first
    lengths[n] rows (what the RRT planners, shortcut_paths and path_certify take).  v_max, a_max: (D,) finite and > 0.  max_deviation:
    how far a blend may leave its corner, a joint-space infinity-norm in rad; None or inf: no cap.

    GUARANTEES: the limits hold for EVERY t, not at samples; the trajectory is C1, rest to rest, starts and ends on the end waypoints;
    inside the blend of waypoint i joint k is within |dv_ik| tb_i / 8 <= max_deviation of the polyline, on the segments it is ON the
    polyline.  The result is NOT time-optimal (traj_retime's is, at the waypoints).  Duplicate waypoints are DEGENERATE_SEGMENT: purge
    them.  Returns a BlendTiming."""
    N, H, W = _blend_paths(paths, lengths, 'path_blend')
    lim = []
    for t, name in ((v_max, 'v_max'), (a_max, 'a_max')):
        t = torch.as_tensor(t, dtype=torch.float32)
        if t.dim() != 1 or not bool(torch.isfinite(t).all()) or not bool((t > 0).all()):
            raise ValueError(f'{name} must be a vector of finite limits > 0 (got {t.tolist() if t.dim() == 1 else tuple(t.shape)})')
        lim.append(t.to(paths.device).contiguous())
    D = lim[0].numel()
    if lim[1].numel() != D or not 1 <= D <= W:
        raise ValueError(f'v_max has {D} entries, a_max {lim[1].numel()}, the rows of paths {W} columns')
    delta = math.inf if max_deviation is None else float(max_deviation)
    if not delta > 0:
        raise ValueError(f'max_deviation = {max_deviation}: a distance > 0 in rad, or None / inf for no cap')
    if int(max_sweeps) < 1:
        raise ValueError(f'max_sweeps = {max_sweeps}: at least one sweep')
    dev = paths.device
    T = torch.empty(N, max(H - 1, 0), device=dev)
    tb, tw, dv = (torch.empty(N, H, device=dev) for _ in range(3))
    duration = torch.empty(N, device=dev)
    sweeps, status, first_bad = (torch.empty(N, device=dev, dtype=torch.int32) for _ in range(3))
    if N > 0:                                                    # (an empty tensor has no address to hand over)
        _lib.check(_lib.lib().mpb_path_blend(_ptr(paths), W, _ptr(lengths), _ptr(lim[0]), _ptr(lim[1]), delta, int(max_sweeps), _ptr(T), _ptr(tb),
                                             _ptr(tw), _ptr(dv), _ptr(duration), _ptr(sweeps), _ptr(status), _ptr(first_bad), N, H, D, _stream()),
                   'mpb_path_blend')
    return BlendTiming(T, tb, tw, dv, duration, sweeps, status, first_bad, lengths, delta, D)


@_on_tensor_device
def path_blend_sample(paths, timing, dt, n_rows=None):
    """paths (N, H, W) and their BlendTiming -> the blended trajectories at the fixed control period dt, in one launch
    (mpb_path_blend_sample): (out (N, n_rows, 3D) positions, velocities and accelerations, rows (N,) int32, status (N,) int32).  Row k
    is the state at k dt; rows at and past a path's own rows[n] = ceil(duration / dt) + 1 hold its last waypoint at rest.  n_rows=None
    reads the longest duration back (one synchronisation) and sizes the output to it.  A path with more rows than n_rows is
    BLEND_TOO_LONG (the rows that fit are written); one whose timing is not BLEND_OK keeps that status, has rows 0 and holds its first
    waypoint."""
    N, H, W = _blend_paths(paths, timing.lengths, 'path_blend_sample')
    _chk(timing.T, (N, max(H - 1, 0)), 'timing.T')
    for name in ('tb', 'tw', 'dev'):
        _chk(getattr(timing, name), (N, H), 'timing.' + name)
    _chk(timing.duration, (N,), 'timing.duration')
    _chk(timing.status, (N,), 'timing.status', dtype=torch.int32)
    D = int(timing.n_dof)
    if not 1 <= D <= W:
        raise ValueError(f'the timing is of {D} joints, the rows of paths have {W} columns')
    dt = float(dt)
    if n_rows is None:
        if not (dt > 0 and math.isfinite(dt)):
            raise ValueError(f'dt = {dt}: a finite period > 0')
        ok = (timing.status == BLEND_OK) & torch.isfinite(timing.duration)
        Tmax = float(torch.where(ok, timing.duration, torch.zeros_like(timing.duration)).max()) if N else 0.0
        n_rows = int(math.ceil(Tmax / float(np.float32(dt)))) + 1
    n_rows = int(n_rows)
    out = torch.empty(N, max(n_rows, 0), 3 * D, device=paths.device)
    rows = torch.empty(N, device=paths.device, dtype=torch.int32)
    status = torch.empty(N, device=paths.device, dtype=torch.int32)
    if N > 0:
        _lib.check(_lib.lib().mpb_path_blend_sample(_ptr(paths), W, _ptr(timing.lengths), _ptr(timing.T), _ptr(timing.tb), _ptr(timing.tw),
                                                    _ptr(timing.duration), _ptr(timing.status), _ptr(out), _ptr(rows), _ptr(status), N, H, D, dt,
                                                    n_rows, _stream()), 'mpb_path_blend_sample')
    return out, rows, status


# ---- clearance and path certification (csrc/mpb_certify.hip; the definition: include/mpb.h) ---------------------------
CERT_STATUS_NAMES = certify_layout.STATUS
CERT_FREE, CERT_COLLISION, CERT_UNDECIDED_DEPTH, CERT_UNDECIDED_QUEUE, CERT_BAD_INPUT, CERT_BUFFER_CHANGED = range(len(CERT_STATUS_NAMES))
CERT_DEFAULT_SLACK = certify_layout.CERT_DEFAULT_SLACK


class DeviceReach:
    """The reach buffer of a robot (certify_layout.pack_reach: how far each collision sphere can be from each joint that moves it)
    resident in HBM: what path_certify forms its motion bounds from."""

    def __init__(self, robot, device):
        rs = robot.spec()
        self.robot, self.host = robot, certify_layout.pack_reach(rs)
        self.n_dof, self.n_links, self.kind = int(rs['n_dof']), len(rs['link_radius']), int(rs['kind'])
        self.buf = torch.from_numpy(self.host.copy()).to(device)


def _need_whole_link_table(geom, what):
    if not geom.all_links:
        raise ValueError(f'{what} needs every collision sphere of the robot in every chained field: build the DeviceGeometry with '
                         f'keep_all_links=True')


@_on_tensor_device
def clearance(q, geom, with_link=False):
    """(N, D) configurations -> eta fp32 (N,): the clearance min_l (min_f (sd_f(x_l) - margin_f) - r_l) over the obstacle geometry,
    every obstacle of every chained field walked exhaustively (mpb_clearance); eta < 0 is collision_check's predicate.  with_link
    also returns the arg-min collision sphere, int32 (N,), the lowest index on a tie."""
    if not (isinstance(q, torch.Tensor) and q.is_cuda):
        raise _lib.MPBError('clearance: q must be a GPU tensor; there is no CPU fallback')
    if q.dim() != 2:
        raise ValueError(f'q has shape {tuple(q.shape)}, expected (N, D)')
    N, D = q.shape
    _chk(q, (N, D), 'q')
    if D != geom.n_dof:
        raise ValueError(f'q has {D} columns, the geometry {geom.n_dof} degrees of freedom')
    _need_whole_link_table(geom, 'clearance')
    eta = torch.empty(N, device=q.device, dtype=torch.float32)
    link = torch.empty(N, device=q.device, dtype=torch.int32) if with_link else None
    _lib.check(_lib.lib().mpb_clearance(_ptr(q), _ptr(geom.buf), _ptr(eta), _ptr(link), N, D, _stream()), 'mpb_clearance')
    return (eta, link) if with_link else eta


class PathCertificate:
    """What path_certify returns, per path (N,): status int32 (CERT_FREE / CERT_COLLISION / CERT_UNDECIDED_DEPTH / CERT_UNDECIDED_QUEUE /
    CERT_BAD_INPUT / CERT_BUFFER_CHANGED), free / collision / undecided bool; the witness of a COLLISION -- witness_segment int32,
    witness_t fp32 (a node: its index and t = 0), witness_link int32, witness_eta fp32; -1, 0, -1, 0 without one --; n_evals int32
    configurations evaluated, depth_max int32 the deepest level evaluated (-1: nodes only), margin_cert fp32 a certified lower bound
    of the path's clearance minus c_req, up to the slack (-inf unless FREE); slack, c_req as the launch took them.  The certificate
    covers the joint-space POLYLINE through the rows, not a spline through them."""

    def __init__(self, out_i, out_f, slack, c_req):
        self.status, self.witness_segment, self.witness_link, self.n_evals, self.depth_max = (out_i[:, k] for k in range(5))
        self.witness_t, self.witness_eta, self.margin_cert = (out_f[:, k] for k in range(3))
        self.free, self.collision = self.status == CERT_FREE, self.status == CERT_COLLISION
        self.undecided = (self.status == CERT_UNDECIDED_DEPTH) | (self.status == CERT_UNDECIDED_QUEUE)
        self.slack, self.c_req = float(slack), float(c_req)

    def witness_q(self, paths):
        """(N, D) the witness configurations on paths (N, H, W): fmaf(b - a, t, a) on the witness segment, the node itself for t = 0;
        rows without a witness hold row 0."""
        H = paths.shape[1]
        s = self.witness_segment.clamp_min(0).long()
        idx = torch.arange(paths.shape[0], device=paths.device)
        a, b = paths[idx, s], paths[idx, (s + 1).clamp_max(H - 1)]
        t = self.witness_t[:, None]
        return torch.where(t == 0, a, torch.addcmul(a, b - a, t))


@_on_tensor_device
def path_certify(paths, geom, reach, lengths=None, slack=None, c_req=0.0, max_depth=certify_layout.CERT_DEFAULT_MAX_DEPTH,
                 max_intervals=certify_layout.CERT_DEFAULT_MAX_INTERVALS):
    """(N, H, W) paths, W >= the geometry's degrees of freedom, read in place (the first D columns of a row) -> a PathCertificate: is
    the joint-space polyline through the first lengths[n] rows (every row without lengths) free of the obstacle geometry over its
    whole continuum, with clearance above c_req?  Bisection with the motion bound of `reach` (a DeviceReach of the same robot),
    mpb_path_certify: include/mpb.h has the definition.  slack: the S of the definition, CERT_DEFAULT_SLACK (measured: certify_layout.py)
    when None.  UNDECIDED_DEPTH: raise max_depth (<= 20); UNDECIDED_QUEUE: raise max_intervals (<= 4096)."""
    if not (isinstance(paths, torch.Tensor) and paths.is_cuda):
        raise _lib.MPBError('path_certify: paths must be a GPU tensor; there is no CPU fallback')
    if paths.dim() != 3:
        raise ValueError(f'paths has shape {tuple(paths.shape)}, expected (N, H, W)')
    N, H, W = paths.shape
    _chk(paths, (N, H, W), 'paths')
    D = geom.n_dof
    if W < D:
        raise ValueError(f'paths has {W} columns, the geometry {D} degrees of freedom')
    _need_whole_link_table(geom, 'path_certify')
    if (reach.n_dof, reach.n_links, reach.kind) != (geom.n_dof, geom.n_links, geom.kind):
        raise ValueError(f'path_certify: the reach buffer is of a robot with {reach.n_dof} joints and {reach.n_links} collision spheres '
                         f'(kind {reach.kind}), the geometry of one with {geom.n_dof} and {geom.n_links} (kind {geom.kind})')
    if reach.buf.device != paths.device or geom.buf.device != paths.device:
        raise ValueError('path_certify: paths, the geometry and the reach buffer must live on one device')
    _chk(lengths, (N,), 'lengths', allow_none=True, dtype=torch.int32)
    if H > certify_layout.CERT_MAX_ROWS:
        raise ValueError(f'path_certify: H = {H} exceeds CERT_MAX_ROWS = {certify_layout.CERT_MAX_ROWS} (the segment field of the interval word)')
    if not 0 <= int(max_depth) <= certify_layout.CERT_MAX_DEPTH:
        raise ValueError(f'path_certify: max_depth = {max_depth} outside 0 .. CERT_MAX_DEPTH = {certify_layout.CERT_MAX_DEPTH} (the j field of the interval word)')
    if not 1 <= int(max_intervals) <= certify_layout.CERT_MAX_INTERVALS:
        raise ValueError(f'path_certify: max_intervals = {max_intervals} outside 1 .. CERT_MAX_INTERVALS = {certify_layout.CERT_MAX_INTERVALS} (the queue lives in LDS)')
    slack = CERT_DEFAULT_SLACK if slack is None else float(slack)
    if not (math.isfinite(slack) and slack >= 0.0 and math.isfinite(float(c_req))):
        raise ValueError(f'path_certify: slack = {slack} must be finite and >= 0, c_req = {c_req} finite')
    out_i = torch.empty(N, certify_layout.CERT_OUT_INTS, device=paths.device, dtype=torch.int32)
    out_f = torch.empty(N, certify_layout.CERT_OUT_FLOATS, device=paths.device, dtype=torch.float32)
    _lib.check(_lib.lib().mpb_path_certify(_ptr(paths), W, _ptr(lengths), _ptr(geom.buf), _ptr(reach.buf), int(reach.n_links), slack,
                                           float(c_req), int(max_depth), int(max_intervals), _ptr(out_i), _ptr(out_f), N, H, D, _stream()),
               'mpb_path_certify')
    return PathCertificate(out_i, out_f, slack, c_req)


# ---- clearance and certification of timed trajectories among moving obstacles (csrc/mpb_certify_moving.hip; st_certify_layout.py) ------
STC_STATUS_NAMES = st_certify_layout.STATUS
STC_NOT_VALID = len(CERT_STATUS_NAMES)                 # (the values before it are CERT_FREE .. CERT_BUFFER_CHANGED)
STC_NO_OBSTACLE = st_certify_layout.STC_NO_OBSTACLE
STC_DEFAULT_SLACK = st_certify_layout.STC_DEFAULT_SLACK


def _moving_certify_args(what, trajs, geom, mo):
    """The shape checks moving_clearance and traj_certify_moving share: (N, R, W, D)."""
    if not isinstance(geom, DeviceGeometry):
        raise TypeError(f'{what} takes the DeviceGeometry of the static scene')
    if not isinstance(mo, DeviceMovingObstacles):
        raise TypeError(f'{what} takes a DeviceMovingObstacles')
    if not (isinstance(trajs, torch.Tensor) and trajs.is_cuda):
        raise _lib.MPBError(f'{what}: trajs must be a GPU tensor; there is no CPU fallback')
    if trajs.dim() != 3:
        raise ValueError(f'trajs has shape {tuple(trajs.shape)}, expected (N, R, W)')
    N, R, W = trajs.shape
    _chk(trajs, (N, R, W), 'trajs')
    D = geom.n_dof
    if W < D:
        raise ValueError(f'trajs has {W} columns, the geometry {D} degrees of freedom')
    if (mo.n_dof, mo.n_links) != (geom.n_dof, geom.n_links):
        raise ValueError(f'{what}: the moving-obstacle buffer is of a robot with {mo.n_dof} joints and {mo.n_links} collision spheres, the '
                         f'geometry of one with {geom.n_dof} and {geom.n_links}')
    if R != mo.n_rows:
        raise ValueError(f'{what}: trajs has n_rows = {R}, the moving-obstacle buffer was packed for n_rows = {mo.n_rows}')
    _need_whole_link_table(geom, what)
    if geom.buf.device != trajs.device or mo.buf.device != trajs.device:
        raise ValueError(f'{what}: trajs, the geometry and the moving-obstacle buffer must live on one device')
    return N, R, W, D


@_on_tensor_device
def moving_clearance(trajs, geom, mo, with_args=False):
    """trajs (N, R, W), R == mo.n_rows, read in place (the first D columns of a row) -> eta fp32 (N, R): the clearance of every row AT ITS
    OWN TIME against the static geometry and the obstacles of a DeviceMovingObstacles as they stand at that row (mpb_moving_clearance;
    include/mpb.h has the definition): the quantitative counterpart of moving_collision_check OR collision_check.  with_args also returns
    the arg-min robot sphere int32 (N, R) and the arg-min obstacle int32 (N, R): o >= 0 a moving obstacle (spheres first, then boxes),
    -1 - f the static field f."""
    N, R, W, D = _moving_certify_args('moving_clearance', trajs, geom, mo)
    eta = torch.empty(N, R, device=trajs.device, dtype=torch.float32)
    link = torch.empty(N, R, device=trajs.device, dtype=torch.int32) if with_args else None
    obst = torch.empty(N, R, device=trajs.device, dtype=torch.int32) if with_args else None
    _lib.check(_lib.lib().mpb_moving_clearance(_ptr(trajs), W, _ptr(geom.buf), _ptr(mo.buf), _ptr(eta), _ptr(link), _ptr(obst), N, R, D, _stream()),
               'mpb_moving_clearance')
    return (eta, link, obst) if with_args else eta


class TrajCertificate:
    """What traj_certify_moving returns, per trajectory (N,): status int32 (CERT_FREE / CERT_COLLISION / CERT_UNDECIDED_DEPTH /
    CERT_UNDECIDED_QUEUE / CERT_BAD_INPUT / CERT_BUFFER_CHANGED, and STC_NOT_VALID for a trajectory a caller did not submit), free /
    collision / undecided bool; the witness of a COLLISION -- witness_row int32 (the segment h; a node: its row and s = 0), witness_s
    fp32, witness_time fp64 = t_start + (h + s) dt_row formed on the host, witness_link int32, witness_obstacle int32 (o >= 0 a moving
    obstacle, -1 - f the static field f), witness_eta fp32; -1, 0, NaN, -1, STC_NO_OBSTACLE, 0 without one --; n_evals int32, depth_max
    int32 (-1: nodes only), margin_cert fp32 a certified lower bound of the continuum's clearance minus c_req, up to the slack (-inf
    unless FREE); slack and c_req as the launch took them (c_req: the EFFECTIVE one), and the scalar chord_deviation the caller
    reports (0.0 from ops.traj_certify_moving, which certifies the chord motion)."""

    def __init__(self, out_i, out_f, slack, c_req, t_start, dt_row, chord_deviation=0.0):
        self.status, self.witness_row, self.witness_link, self.witness_obstacle, self.n_evals, self.depth_max = (out_i[:, k] for k in range(6))
        self.witness_s, self.witness_eta, self.margin_cert = (out_f[:, k] for k in range(3))
        self.free, self.collision = self.status == CERT_FREE, self.status == CERT_COLLISION
        self.undecided = (self.status == CERT_UNDECIDED_DEPTH) | (self.status == CERT_UNDECIDED_QUEUE)
        time = float(t_start) + (self.witness_row.double() + self.witness_s.double()) * float(dt_row)
        self.witness_time = torch.where(self.collision, time, torch.full_like(time, float('nan')))
        self.slack, self.c_req, self.chord_deviation = float(slack), float(c_req), float(chord_deviation)


@_on_tensor_device
def traj_certify_moving(trajs, geom, mo, reach, slack=None, c_req=0.0, max_depth=certify_layout.CERT_DEFAULT_MAX_DEPTH,
                        max_intervals=certify_layout.CERT_DEFAULT_MAX_INTERVALS):
    """trajs (N, R, W), R == mo.n_rows, read in place -> a TrajCertificate: is the timed trajectory free of the static geometry AND of
    the moving obstacles over the whole continuum of its clock -- the robot on the joint-space polyline through the rows, every obstacle
    on the chord between its centres of consecutive rows -- with clearance above c_req?  Bisection with a motion bound in which the
    obstacles move too (mpb_traj_certify_moving; include/mpb.h has the definition).  This call certifies the CHORD motion and takes
    c_req as given; PlanningTask.certify_trajs_moving raises it by the field's chord deviation.  slack: the S of the definition,
    STC_DEFAULT_SLACK (measured: st_certify_layout.py) when None.  The witness time is formed from mo.field's clock."""
    what = 'traj_certify_moving'
    N, R, W, D = _moving_certify_args(what, trajs, geom, mo)
    if (reach.n_dof, reach.n_links, reach.kind) != (geom.n_dof, geom.n_links, geom.kind):
        raise ValueError(f'{what}: the reach buffer is of a robot with {reach.n_dof} joints and {reach.n_links} collision spheres '
                         f'(kind {reach.kind}), the geometry of one with {geom.n_dof} and {geom.n_links} (kind {geom.kind})')
    if reach.buf.device != trajs.device:
        raise ValueError(f'{what}: trajs and the reach buffer must live on one device')
    if not 0 <= int(max_depth) <= certify_layout.CERT_MAX_DEPTH:
        raise ValueError(f'{what}: max_depth = {max_depth} outside 0 .. CERT_MAX_DEPTH = {certify_layout.CERT_MAX_DEPTH} (the j field of the interval word)')
    if not 1 <= int(max_intervals) <= certify_layout.CERT_MAX_INTERVALS:
        raise ValueError(f'{what}: max_intervals = {max_intervals} outside 1 .. CERT_MAX_INTERVALS = {certify_layout.CERT_MAX_INTERVALS} (the queue lives in LDS)')
    slack = STC_DEFAULT_SLACK if slack is None else float(slack)
    if not (math.isfinite(slack) and slack >= 0.0 and math.isfinite(float(c_req))):
        raise ValueError(f'{what}: slack = {slack} must be finite and >= 0, c_req = {c_req} finite')
    out_i = torch.empty(N, st_certify_layout.STC_OUT_INTS, device=trajs.device, dtype=torch.int32)
    out_f = torch.empty(N, st_certify_layout.STC_OUT_FLOATS, device=trajs.device, dtype=torch.float32)
    _lib.check(_lib.lib().mpb_traj_certify_moving(_ptr(trajs), W, _ptr(geom.buf), _ptr(mo.buf), _ptr(reach.buf), int(reach.n_links), slack,
                                                  float(c_req), int(max_depth), int(max_intervals), _ptr(out_i), _ptr(out_f), N, R, D, _stream()),
               'mpb_traj_certify_moving')
    f = mo.field
    dt_row = (float(f.t_end) - float(f.t_start)) / (R - 1) if R > 1 else 0.0
    return TrajCertificate(out_i, out_f, slack, c_req, f.t_start, dt_row)
