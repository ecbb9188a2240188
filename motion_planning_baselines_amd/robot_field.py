"""Duck-typed `robot` / `field` objects on the GPU with the API the reference's cost layer consumes from torch_robotics
(SURVEY 8b): robot.q_dim / q_min / q_max / dt / get_position / get_velocity / fk_map_collision (cost_functions.py:21,
:50-52, :380, :412-420), field.compute_cost / zero_grad (field_factor.py:39, :52, :56).

With these the reference's own, unmodified CostCollision / FieldFactor / CostComposite run on GPU tensors against this
package's geometry; forward kinematics and the field cost are HIP kernels (csrc/mpb_points.hip) and torch.autograd
differentiates through them by their hand-written vector-Jacobian products.  The planners of this package do NOT go
through these objects: they use the fused evaluators.
"""
import numpy as np
import torch

from . import ops


class _FKPoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, geom):
        q3 = q.reshape(-1, q.shape[-2], q.shape[-1]).to(torch.float32).contiguous()
        ctx.geom, ctx.q_shape = geom, q.shape
        ctx.save_for_backward(q3)
        pts = ops.fk_collision_points(q3, geom)
        return pts.reshape(*q.shape[:-1], pts.shape[-2], 3)

    @staticmethod
    def backward(ctx, grad_pts):
        (q3,) = ctx.saved_tensors
        g = grad_pts.reshape(q3.shape[0], q3.shape[1], -1, 3).to(torch.float32).contiguous()
        gq = ops.fk_collision_points_vjp(q3, ctx.geom, g)                     # (B,H,n_dof)
        out = torch.zeros(q3.shape, device=q3.device, dtype=torch.float32)
        out[..., :gq.shape[-1]] = gq
        return out.reshape(ctx.q_shape), None


class _FieldCost(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pts, geom):
        p4 = pts.reshape(-1, pts.shape[-3], pts.shape[-2], 3).to(torch.float32).contiguous()
        ctx.geom, ctx.p_shape = geom, pts.shape
        ctx.save_for_backward(p4)
        return ops.field_cost_points(p4, geom).reshape(pts.shape[:-2])

    @staticmethod
    def backward(ctx, grad_cost):
        (p4,) = ctx.saved_tensors
        g = grad_cost.reshape(p4.shape[0], p4.shape[1]).to(torch.float32).contiguous()
        return ops.field_cost_points_vjp(p4, ctx.geom, g).reshape(ctx.p_shape), None


class _EEPose(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, geom):
        q2 = q.reshape(-1, q.shape[-1]).to(torch.float32).contiguous()
        pose, jac = ops.fk_ee_pose(q2, geom, with_jacobian=True)
        ctx.save_for_backward(pose, jac)
        ctx.q_shape = q.shape
        return pose.reshape(*q.shape[:-1], 3, 4)

    @staticmethod
    def backward(ctx, grad_pose):
        pose, jac = ctx.saved_tensors
        g = grad_pose.reshape(-1, 3, 4).to(torch.float32)
        # d t / d q_j = Jv_j; d R[:, c] / d q_j = z_j x R[:, c], so  grad_q_j = Jv_j . G_t + z_j . sum_c (R[:, c] x G_R[:, c])
        m = torch.linalg.cross(pose[:, :, :3], g[:, :, :3], dim=1).sum(-1)                    # (N, 3)
        gq = torch.einsum('nkj,nk->nj', jac[:, :3], g[:, :, 3]) + torch.einsum('nkj,nk->nj', jac[:, 3:], m)
        return gq.reshape(ctx.q_shape), None


def ee_pose(q, geom):
    """(..., D) configurations -> the end-effector pose (..., 3, 4) = [R | t] of an ops.DeviceGeometry's chain (mpb_fk_ee_pose),
    differentiable w.r.t. q: the backward is formed in torch from the kernel's own Jacobian.  An end-effector cost can thus be a
    caller-supplied cost of CHOMP or a member of an MPPI cost."""
    return _EEPose.apply(q, geom)


class DeviceRobot:
    """robot API of the reference's cost layer, evaluated on the GPU."""

    def __init__(self, robot, geom, device):
        self._robot, self._geom = robot, geom
        self.q_dim = robot.q_dim
        self.dt = robot.dt
        self.q_min = robot.q_min.to(device)
        self.q_max = robot.q_max.to(device)

    def get_position(self, x):
        return x[..., :self.q_dim]

    def get_velocity(self, x):
        return x[..., self.q_dim:2 * self.q_dim]

    def fk_map_collision(self, q_pos, **kwargs):
        """(..., H, >=q_dim) joint positions -> (..., H, L, 3) collision-sphere positions (differentiable)."""
        return _FKPoints.apply(q_pos, self._geom)

    def get_EE_pose(self, q):
        """(..., >=q_dim) joint positions -> (..., 3, 4) end-effector pose [R | t] (differentiable); leading dimensions are kept."""
        return ee_pose(q[..., :self.q_dim], self._geom)

    def get_EE_position(self, q):
        """(..., >=q_dim) joint positions -> (..., 3) end-effector position (differentiable): the reference's robot.get_EE_position
        (panda_spheres_GPMP.py:63-64)."""
        return self.get_EE_pose(q)[..., :, 3]


class DeviceField:
    """field API of the reference's cost layer: hinge cost of the robot's collision spheres, evaluated on the GPU."""

    def __init__(self, field, geom):
        self._field, self._geom = field, geom

    def compute_cost(self, q_pos, link_pos, **kwargs):
        """link_pos (..., H, L, 3) -> (..., H) cost per waypoint (differentiable w.r.t. link_pos); extra keyword arguments
        (`obstacle_spheres`, `trajs_interp`, ...) are accepted and ignored like the call sites require."""
        return _FieldCost.apply(link_pos, self._geom)

    def zero_grad(self):
        pass


class _SDFSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pts, sdf):
        p2 = pts.reshape(-1, 3).to(torch.float32).contiguous()
        s, g = ops.sdf_grid_sample(p2, sdf, with_grad=True)          # (value and gradient come from the same node loads)
        ctx.save_for_backward(g)
        ctx.p_shape = pts.shape
        return s.reshape(pts.shape[:-1])

    @staticmethod
    def backward(ctx, grad_s):
        (g,) = ctx.saved_tensors
        return (grad_s.reshape(-1, 1).to(torch.float32) * g).reshape(ctx.p_shape), None


def sdf_grid_sample(points, sdf):
    """points (..., 3) -> s (...) of the interpolant of an ops.DeviceSDFGrid (mpb_sdf_grid_sample), differentiable w.r.t. the points:
    torch.autograd multiplies by the kernel's own d s / d x."""
    return _SDFSample.apply(points, sdf)


class DeviceGridField:
    """`field` of the reference's cost layer over a geometry.GridSDFField: compute_cost(q_pos, link_pos) = sum_l relu(margin + r_l -
    s(x_l)) with s from sdf_grid_sample above (differentiable w.r.t. link_pos)."""

    def __init__(self, sdf):
        self._sdf = sdf
        self._thr = torch.as_tensor(sdf.robot.spec()['link_radius'], dtype=torch.float32, device=sdf.buf.device) + float(sdf.field.margin)

    def compute_cost(self, q_pos, link_pos, **kwargs):
        return torch.relu(self._thr - sdf_grid_sample(link_pos, self._sdf)).sum(-1)

    def zero_grad(self):
        pass


def device_robot_field(robot, field, device):
    """(DeviceRobot, DeviceField) for one robot / collision field pair (geometry.Robot*, geometry.CollisionField)."""
    geom = ops.DeviceGeometry(robot, field, device, keep_all_links=True)
    return DeviceRobot(robot, geom, device), DeviceField(field, geom)


class PlanningTask:
    """The slice of torch_robotics' planning task that the reference's sample-based planners call (rrt_base.py:56-57,
    :100-110): compute_collision, random_coll_free_q, random_q, distance_q -- on the GPU -- and what its examples ask after
    a planner has run (panda_spheres_CHOMP.py:126, :146-148): get_trajs_collision_and_free, compute_fraction_free_trajs,
    compute_collision_intensity_trajs, compute_success_free_trajs (one launch of mpb_traj_collision_stats each).

    The collision predicate is build-defined (torch_robotics is absent): a configuration is in collision iff the
    package's per-waypoint collision cost  sum_f s_f sum_l relu(margin + r_l - min_o sdf_o(x_l))  is positive
    (mpb_collision_check; the same evaluators as every cost kernel).  `field` may be a list of up to four fields.

    self_field: a geometry.SelfCollisionField (the reference's use_self_collision_storm=True).  compute_collision and
    random_coll_free_q then OR the self predicate in (a second launch, mpb_self_collision_check with or_into); without
    world_predicate the trajectory validation below and the RRT planners built on the task read `geom` alone and raise
    NotImplementedError rather than ignore it.

    sdf_field: a geometry.GridSDFField (a precomputed grid of signed distances: geometry the obstacle list cannot hold).  Its predicate
    (mpb_sdf_grid_collision_check with or_into) is ORed in the same way, and the same callers refuse such a task by name.

    world_predicate=True (opt-in): the task builds `world`, an ops.DeviceWorld of geom, sdf_geom and self_geom, and the
    in-kernel world predicate -- obstacles OR grid OR self, one launch -- serves _in_collision, RRTConnect (and through it
    MultiSampleBasedPlanner and HybridPlanner), shortcut_paths / RRTConnect.shortcut and the four validation calls.  RRTStar,
    InfRRTStar, PRM, STRRTConnect, shortcut_trajs_moving, certify_* and compute_clearance(_moving) keep refusing a task with a self_field or an
    sdf_field by name.

    A geometry.MovingObstacleField is none of these: it is refused by name as field, self_field or sdf_field (the predicates and the
    sample-based planners have no time axis).  check_trajs_moving(trajs, moving_field) validates trajectories against the task's static
    predicates AND such a field, row by row at the field's clock.

    End-effector goals (serial chains): get_EE_pose / get_EE_position (the reference's robot.get_EE_position,
    panda_spheres_GPMP.py:63-64) and inverse_kinematics -- a pose in, many goal configurations out, filtered by the predicates above
    (mpb_fk_ee_pose, mpb_ik_solve) --, and cartesian_path: straight-line end-effector moves from those configurations, cropped at the
    first row one of the predicates above refuses (mpb_cartesian_path; unlike validation and shortcutting it serves a task with a
    self_field or an sdf_field)."""

    def __init__(self, robot, field, self_field=None, tensor_args=None, seed=0, sdf_field=None, world_predicate=False):
        from .planners.base import require_cuda
        self.tensor_args = tensor_args
        self.device = require_cuda(tensor_args)
        from .geometry import MovingObstacleField
        for name, f in (('field', field), ('self_field', self_field), ('sdf_field', sdf_field)):
            if any(isinstance(x, MovingObstacleField) for x in (f if isinstance(f, (list, tuple)) else [f])):
                raise TypeError(f'PlanningTask({name}=...): a MovingObstacleField is no static field -- the task\'s predicates, samplers and '
                                f'the RRT / PRM / shortcut kernels have no time axis.  Plan among it with planners.STRRTConnect(task, moving_field, n_rows, ...), '
                                f'freeze it with field.at(t), give it to the optimisers '
                                f'as CostCollision(field=...), validate trajectories with check_trajs_moving(trajs, moving_field) and certify them between the '
                                f'rows with certify_trajs_moving(trajs, moving_field) (certify_paths / certify_trajs have no clock)')
        self.robot, self.field = robot, field
        self.geom = ops.DeviceGeometry(robot, field, self.device)
        self.self_field = self_field
        self.self_geom = None if self_field is None else ops.DeviceSelfCollision(robot, self_field, self.device)
        self.sdf_field = sdf_field
        self.sdf_geom = None if sdf_field is None else ops.DeviceSDFGrid(robot, sdf_field, self.device)
        self.world_predicate = bool(world_predicate)
        self.world = ops.DeviceWorld(self.geom, sdf=self.sdf_geom, self_collision=self.self_geom) if self.world_predicate else None
        self.q_dim = robot.q_dim
        self.q_min = robot.q_min.to(self.device)
        self.q_max = robot.q_max.to(self.device)
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(int(seed))

    def compute_collision(self, qs, **kwargs):
        """(..., D) configurations -> bool (...): in collision."""
        q2 = torch.as_tensor(qs, dtype=torch.float32, device=self.device).reshape(-1, self.q_dim).contiguous()
        return self._in_collision(q2).reshape(qs.shape[:-1])

    def _in_collision(self, q2):
        """(N, D) contiguous fp32 on the device -> bool (N,): collides with the world, (self_field) with itself or (sdf_field) with
        what the grid holds (world_predicate: the one fused launch)."""
        if self.world is not None:
            return ops.world_collision_check(q2, self.world)
        flag = ops.collision_check(q2, self.geom)
        for own in (self.self_geom, self.sdf_geom):
            if own is not None:
                ops.MEMBER_OPS[type(own)].check(q2, own, flag=flag)
        return flag

    def check_trajs_moving(self, trajs, moving_field):
        """trajs (..., H, W), W >= q_dim, against the task's own static predicates AND a geometry.MovingObstacleField: returns
        (in_collision (...), rows (..., H)), both bool.  rows[..., h] = the task's predicate on row h (_in_collision: obstacles,
        self_field, sdf_field) ORed with the moving predicate of row h at the time t_h of the field's clock over H rows
        (mpb_moving_collision_check); in_collision = any row.  The check is made AT THE ROWS only.  For a denser check interpolate the
        trajectory first (ops.traj_interpolate) and call again: the clock follows the row count, so the denser rows are seen at their own
        times.  One packed buffer per (field, H) is kept on the task."""
        from .geometry import MovingObstacleField
        if not isinstance(moving_field, MovingObstacleField):
            raise TypeError('check_trajs_moving takes a geometry.MovingObstacleField')
        t = torch.as_tensor(trajs, dtype=torch.float32, device=self.device)
        if t.dim() < 2 or t.shape[-1] < self.q_dim:
            raise ValueError(f'trajs has shape {tuple(t.shape)}, expected (..., H, W) with W >= {self.q_dim}')
        lead, H = tuple(t.shape[:-2]), t.shape[-2]
        t = t.reshape(-1, H, t.shape[-1]).contiguous()
        mo = self._moving_geom(moving_field, H)
        rows = self._in_collision(t[..., :self.q_dim].reshape(-1, self.q_dim).contiguous()).reshape(t.shape[0], H).contiguous()
        if t.shape[0]:
            ops.moving_collision_check(t, mo, flag=rows)
        return rows.any(-1).reshape(lead), rows.reshape(*lead, H)

    def _moving_geom(self, moving_field, n_rows):
        """The packed buffer of (moving_field, n_rows), one per pair kept on the task (check_trajs_moving, time_paths_moving)."""
        cache = self.__dict__.setdefault('_moving_geoms', {})
        key = (id(moving_field), int(n_rows))
        if key not in cache or cache[key].field is not moving_field:
            cache[key] = ops.DeviceMovingObstacles(self.robot, moving_field, self.device, int(n_rows))
        return cache[key]

    # ---- timing of geometric paths among moving obstacles (build-defined: DESIGN.md 10) ------------------------------------------------
    def time_paths_moving(self, paths, moving_field, n_rows, lengths=None, n_samples=None, dq_max=None):
        """Path-velocity decomposition: geometric paths -- from RRTConnect on this task or on field.at(t), shortcut_paths -- keep their
        shape and get their timing among a geometry.MovingObstacleField on a clock of n_rows rows (ops.path_time_plan, which has the
        definition): when to advance along the path and when to wait, so that every row is free at its own time.
        paths (N, S, D) samples, sample 0 the start and sample S - 1 the goal; or, with lengths (N,) int32, padded polylines (N, Lmax, D)
        that are first resampled uniformly in arc length to n_samples samples (ops.traj_resample, its position half).  A sample this
        task's own predicate refuses (_in_collision: obstacles, self_field, sdf_field) is never stood on.  dq_max (D,) rad/s defaults to
        the robot's; a row may move joint k by dq_max_k * (t_end - t_start) / (n_rows - 1).  Returns an ops.PathTiming; its trajs
        (N, n_rows, D) are accepted by check_trajs_moving(trajs, moving_field) wherever found is set.  One packed buffer per
        (field, n_rows) is kept on the task."""
        from .geometry import MovingObstacleField
        if not isinstance(moving_field, MovingObstacleField):
            raise TypeError('time_paths_moving takes a geometry.MovingObstacleField')
        if not moving_field.t_end > moving_field.t_start:
            raise ValueError(f'time_paths_moving: the MovingObstacleField has t_end = {moving_field.t_end} <= t_start = {moving_field.t_start}: '
                             f'a clock needs a positive span')
        n_rows = int(n_rows)
        if n_rows < 2:
            raise ValueError(f'time_paths_moving: n_rows = {n_rows}, the clock needs at least 2 rows')
        dq = getattr(self.robot, 'dq_max_np', None) if dq_max is None else dq_max
        if dq is None:
            raise ValueError('time_paths_moving: no dq_max given and the robot carries none')
        dq = np.asarray(dq.detach().cpu().numpy() if isinstance(dq, torch.Tensor) else dq, np.float64).reshape(-1)
        if dq.size != self.q_dim or not (np.isfinite(dq).all() and (dq > 0).all()):
            raise ValueError(f'time_paths_moving: dq_max must hold {self.q_dim} finite positive entries')
        dt_row = (float(moving_field.t_end) - float(moving_field.t_start)) / (n_rows - 1)
        w = torch.from_numpy((dq * dt_row).astype(np.float32)).to(self.device)
        p = torch.as_tensor(paths, dtype=torch.float32, device=self.device)
        if p.dim() != 3 or p.shape[-1] != self.q_dim:
            raise ValueError(f'paths has shape {tuple(p.shape)}, expected (N, S, D) with D = {self.q_dim}')
        p = p.contiguous()
        if lengths is not None:
            if n_samples is None:
                raise ValueError('time_paths_moving: lengths needs n_samples, the samples to resample every polyline to')
            ln = torch.as_tensor(lengths, device=self.device).to(torch.int32).contiguous()
            p = ops.traj_resample(p, ln, int(n_samples), 1.0)[..., :self.q_dim].contiguous() if p.shape[0] else p[:, :0]
        elif n_samples is not None and int(n_samples) != p.shape[1]:
            raise ValueError(f'time_paths_moving: n_samples = {n_samples} without lengths, and paths holds {p.shape[1]} samples')
        N, S = p.shape[0], p.shape[1]
        mo = self._moving_geom(moving_field, n_rows)
        blocked = self._in_collision(p.reshape(-1, self.q_dim).contiguous()).reshape(N, S).contiguous()
        return ops.path_time_plan(p, mo, w, blocked=blocked)

    # ---- space-time shortcutting of timed trajectories (build-defined: DESIGN.md 10) ---------------------------------------------------
    def shortcut_trajs_moving(self, trajs, moving_field, n_iters=64, dq_max=None, valid=None, **kw):
        """The pass between a planner on the moving-obstacle clock and the optimiser: trajs (N, R, D) -- STRRTConnect plans, or the
        trajs of time_paths_moving -- are shortcut on their own clock of R rows among the task's static obstacles AND a
        geometry.MovingObstacleField (ops.st_shortcut, which has the definition): rows between two drawn rows are replaced by the
        constant-velocity straight piece when it is free at every row's own time and within the per-row velocity bound.  dq_max (D,)
        rad/s defaults to the robot's; a row may move joint k by dq_max_k * (t_end - t_start) / (R - 1), formed as time_paths_moving
        forms it.  valid: None or (N,) bool, False = pass the trajectory through (the `found` of either producer).  **kw: draws, seed,
        problem_offset, max_span, with_log, out of ops.st_shortcut.  Returns an ops.STShortcut; its trajs are accepted by
        check_trajs_moving(trajs, moving_field) wherever ok is set.  One packed buffer per (field, R) is kept on the task."""
        from .geometry import MovingObstacleField
        what = 'shortcut_trajs_moving (the space-time shortcut kernel)'
        self.require_no_self_field(what)
        self.require_no_sdf_field(what)
        if not isinstance(moving_field, MovingObstacleField):
            raise TypeError('shortcut_trajs_moving takes a geometry.MovingObstacleField')
        if not moving_field.t_end > moving_field.t_start:
            raise ValueError(f'shortcut_trajs_moving: the MovingObstacleField has t_end = {moving_field.t_end} <= t_start = '
                             f'{moving_field.t_start}: a clock needs a positive span')
        t = torch.as_tensor(trajs, dtype=torch.float32, device=self.device)
        if t.dim() != 3 or t.shape[-1] != self.q_dim:
            raise ValueError(f'trajs has shape {tuple(t.shape)}, expected (N, R, D) with D = {self.q_dim}')
        n_rows = int(t.shape[1])
        if n_rows < 3:
            raise ValueError(f'shortcut_trajs_moving: n_rows = {n_rows}, a trajectory needs at least 3 rows')
        dq = getattr(self.robot, 'dq_max_np', None) if dq_max is None else dq_max
        if dq is None:
            raise ValueError('shortcut_trajs_moving: no dq_max given and the robot carries none')
        dq = np.asarray(dq.detach().cpu().numpy() if isinstance(dq, torch.Tensor) else dq, np.float64).reshape(-1)
        if dq.size != self.q_dim or not (np.isfinite(dq).all() and (dq > 0).all()):
            raise ValueError(f'shortcut_trajs_moving: dq_max must hold {self.q_dim} finite positive entries')
        dt_row = (float(moving_field.t_end) - float(moving_field.t_start)) / (n_rows - 1)
        w = torch.from_numpy((dq * dt_row).astype(np.float32)).to(self.device)
        if valid is not None:
            valid = torch.as_tensor(valid, device=self.device)
            valid = (valid if valid.dtype in (torch.bool, torch.uint8) else valid != 0).contiguous()
        mo = self._moving_geom(moving_field, n_rows)
        return ops.st_shortcut(t.contiguous(), self.geom, mo, w, n_iters, valid=valid, **kw)

    # what serves a task with an sdf_field / a self_field instead of the caller that refuses it
    _SERVED = ('PlanningTask(..., world_predicate=True) serves RRTConnect, MultiSampleBasedPlanner, HybridPlanner, shortcut_paths and the '
               'trajectory validation on such a task')

    def require_no_sdf_field(self, what):
        if self.sdf_field is not None:
            raise NotImplementedError(f'{what} reads the obstacle geometry alone: it does not serve a task with an sdf_field '
                                      f'(GridSDFField) yet; {self._SERVED}')

    def require_no_self_field(self, what):
        if self.self_field is not None:
            raise NotImplementedError(f'{what} reads the obstacle geometry alone: it does not serve a task with a self_field '
                                      f'(SelfCollisionField) yet; {self._SERVED}')

    def world_or_geom(self, what):
        """What a kernel with the world predicate is launched on: `world` where the task was built with world_predicate=True, else
        `geom` -- after refusing, by name, a task whose self_field or sdf_field that kernel would then ignore."""
        if self.world is not None:
            return self.world
        self.require_no_self_field(what)
        self.require_no_sdf_field(what)
        return self.geom

    def random_q(self, n_samples=1):
        """n_samples configurations uniform within the joint limits, (n_samples, D)."""
        u = torch.rand(int(n_samples), self.q_dim, device=self.device, dtype=torch.float32, generator=self._gen)
        return self.q_min + (self.q_max - self.q_min) * u

    def random_coll_free_q(self, n_samples=1, max_samples=1000, max_tries=1000):
        """n_samples collision-free configurations (n_samples, D), drawn max_samples at a time (at least n_samples) and
        filtered by mpb_collision_check; raises when max_tries rounds do not yield them."""
        n_samples = int(n_samples)
        if n_samples <= 0:
            return torch.empty(0, self.q_dim, device=self.device, dtype=torch.float32)
        found, have = [], 0
        for _ in range(int(max_tries)):
            q = self.random_q(max(int(max_samples), n_samples)).contiguous()
            free = q[~self._in_collision(q)]
            found.append(free)
            have += free.shape[0]
            if have >= n_samples:
                return torch.cat(found)[:n_samples].contiguous()
        raise RuntimeError(f'random_coll_free_q: {have} of {n_samples} collision-free configurations after {max_tries} rounds')

    def distance_q(self, q1, q2):
        return torch.linalg.norm(q1 - q2, dim=-1)

    # ---- end-effector goals (build-defined: DESIGN.md 10) ---------------------------------------------------------------------
    def get_EE_pose(self, q):
        """(..., D) configurations -> (..., 3, 4) end-effector pose [R | t] (differentiable, robot_field.ee_pose)."""
        return ee_pose(torch.as_tensor(q, dtype=torch.float32, device=self.device), self.geom)

    def get_EE_position(self, q):
        """(..., D) configurations -> (..., 3) end-effector position."""
        return self.get_EE_pose(q)[..., :, 3]

    def inverse_kinematics(self, ee_pose, n_seeds=32, n_iters=64, damping=0.1, pos_tol=1e-3, rot_tol=1e-2, position_only=False,
                           q_seed=None, q_ref=None, collision_free=True):
        """Goal configurations for end-effector targets: damped-least-squares IK from many seeds per target (mpb_ik_solve, within
        the joint limits), then the task's own collision predicate on every solution.
        ee_pose: (N, 3, 4) = [R* | t*], or (N, 3) positions with position_only.  Seeds: q_seed (N, S, D) when given, else n_seeds per
        target from random_q (the task's generator: reproducible per `seed`); with q_ref (D,) or (N, D), seed 0 of every target is
        q_ref.  collision_free=False skips the predicate (free = converged).  Returns an IKResult."""
        t = torch.as_tensor(ee_pose, dtype=torch.float32, device=self.device)
        if position_only and t.dim() == 2 and t.shape[-1] == 3:
            eye = torch.eye(3, device=self.device, dtype=torch.float32).expand(t.shape[0], 3, 3)
            t = torch.cat([eye, t[:, :, None]], -1)
        if t.dim() != 3 or tuple(t.shape[1:]) != (3, 4):
            raise ValueError(f'ee_pose has shape {tuple(t.shape)}, expected (N, 3, 4)' + (' or (N, 3)' if position_only else ''))
        N, D = t.shape[0], self.q_dim
        if q_seed is None:
            S = int(n_seeds)
            if S < 1:
                raise ValueError(f'n_seeds = {n_seeds}: at least one seed per target')
            seeds = self.random_q(N * S).reshape(N, S, D)
        else:
            seeds = torch.as_tensor(q_seed, dtype=torch.float32, device=self.device).clone()
            if seeds.dim() != 3 or seeds.shape[0] != N or seeds.shape[2] != D:
                raise ValueError(f'q_seed has shape {tuple(seeds.shape)}, expected ({N}, S, {D})')
        if q_ref is not None:
            q_ref = torch.as_tensor(q_ref, dtype=torch.float32, device=self.device)
            if tuple(q_ref.shape) not in ((D,), (N, D)):
                raise ValueError(f'q_ref has shape {tuple(q_ref.shape)}, expected ({D},) or ({N}, {D})')
            q_ref = q_ref.expand(N, D).contiguous()
            if seeds.shape[1] > 0:
                seeds[:, 0] = q_ref
        q, pos_err, rot_err, conv, iters = ops.ik_solve(t.contiguous(), seeds.contiguous(), self.geom, q_min=self.q_min.contiguous(),
                                                        q_max=self.q_max.contiguous(), n_iters=n_iters, damping=damping, pos_tol=pos_tol,
                                                        rot_tol=rot_tol, position_only=position_only)
        free = conv.clone()
        if collision_free and q.numel():
            free &= ~self._in_collision(q.reshape(-1, D)).reshape(conv.shape)
        return IKResult(q, conv, free, pos_err, rot_err, iters, q_ref)

    def cartesian_path(self, q_start, ee_goal, n_steps=32, n_inner=8, damping=0.1, pos_tol=1e-3, rot_tol=1e-2, jump_max=0.5,
                       position_only=False, collision_free=True):
        """Straight-line end-effector moves (the approach to a grasp, the retreat, a lift): from every start configuration follow the
        pose interpolated between the start's own pose and the goal pose in n_steps steps, each warm-started from the last
        (ops.cartesian_path, within the joint limits), then the task's own collision predicates -- obstacles, self_field, sdf_field --
        ONCE over all rows; a path is cropped before its first colliding row (status CART_COLLISION).
        q_start: (N, S, D), or (N, D) meaning S = 1.  ee_goal: (N, 3, 4) = [R* | t*], one per target and shared by its S starts, or
        (N, 3) positions with position_only.  Returns a CartesianPathResult whose fields keep q_start's leading dimensions."""
        q0 = torch.as_tensor(q_start, dtype=torch.float32, device=self.device)
        if q0.dim() not in (2, 3) or q0.shape[-1] != self.q_dim:
            raise ValueError(f'q_start has shape {tuple(q0.shape)}, expected (N, S, {self.q_dim}) or (N, {self.q_dim})')
        lead = tuple(q0.shape[:-1])
        q0 = q0.reshape(q0.shape[0], -1, self.q_dim).contiguous()
        N, S, D = q0.shape
        t = torch.as_tensor(ee_goal, dtype=torch.float32, device=self.device)
        if position_only and t.dim() == 2 and t.shape[-1] == 3:
            eye = torch.eye(3, device=self.device, dtype=torch.float32).expand(t.shape[0], 3, 3)
            t = torch.cat([eye, t[:, :, None]], -1)
        if t.dim() != 3 or tuple(t.shape) != (N, 3, 4):
            raise ValueError(f'ee_goal has shape {tuple(t.shape)}, expected ({N}, 3, 4)' + (f' or ({N}, 3)' if position_only else ''))
        q, pos_err, rot_err, n_ok, status = ops.cartesian_path(t.contiguous(), q0, self.geom, n_steps, n_inner=n_inner, damping=damping,
                                                               pos_tol=pos_tol, rot_tol=rot_tol, jump_max=jump_max,
                                                               position_only=position_only, q_min=self.q_min.contiguous(),
                                                               q_max=self.q_max.contiguous())
        K = q.shape[2] - 1
        if collision_free and q.numel():
            hit = self._in_collision(q.reshape(-1, D)).reshape(N, S, K + 1)
            rows = torch.arange(K + 1, device=self.device, dtype=torch.int32)
            first = torch.where(hit, rows, K + 1).amin(-1).to(torch.int32)           # the first colliding row, K + 1 when there is none
            crop = first <= n_ok
            keep = (first - 1).clamp_min(0)                                            # (r = 0: n_ok = 0, the rows are kept)
            held = torch.gather(q, 2, keep.long()[:, :, None, None].expand(N, S, 1, D))
            over = (crop & (first > 0))[:, :, None] & (rows >= first[:, :, None])
            q = torch.where(over[..., None], held, q)
            n_ok = torch.where(crop, keep, n_ok)
            status = torch.where(crop, torch.full_like(status, ops.CART_COLLISION), status)
        return CartesianPathResult(q.reshape(*lead, K + 1, D), n_ok.reshape(lead), status.reshape(lead), pos_err.reshape(*lead, K + 1),
                                   rot_err.reshape(*lead, K + 1), K)


    # ---- validation of a trajectory batch (build-defined like the predicate: DESIGN.md 10) -----------------------------------
    def _trajs_stats(self, trajs, num_interpolation, with_flags=False):
        """trajs (..., H, W), W >= q_dim, leading dimensions flattened -> (trajs (N, H, W), the outputs of
        ops.traj_collision_stats).  A contiguous fp32 GPU tensor is read in place, velocity columns and all."""
        geom = self.world_or_geom('trajectory validation (mpb_traj_collision_stats)')
        t = torch.as_tensor(trajs, dtype=torch.float32, device=self.device)
        if t.dim() < 2 or t.shape[-1] < self.q_dim:
            raise ValueError(f'trajs has shape {tuple(t.shape)}, expected (..., H, W) with W >= {self.q_dim}')
        t = t.reshape(-1, t.shape[-2], t.shape[-1]).contiguous()
        return t, ops.traj_collision_stats(t, geom, n_interp=int(num_interpolation), with_flags=with_flags)

    def get_trajs_collision_and_free(self, trajs, return_indices=False, num_interpolation=5, **kwargs):
        """(trajs_coll, trajs_free): the trajectories with a dense point in collision and those without, each (n, H, W) in
        input order, None for a set without members (the examples test `is not None`).  The dense points are the waypoints
        and num_interpolation evenly spaced joint-space points per segment; the predicate is compute_collision's (margin
        included).  return_indices: (trajs_coll, coll_idxs, trajs_free, free_idxs, waypoints_in_collision (N, P) bool)."""
        t, out = self._trajs_stats(trajs, num_interpolation, with_flags=return_indices)
        in_coll = out[0] > 0
        coll_idxs = torch.nonzero(in_coll).flatten()
        free_idxs = torch.nonzero(~in_coll).flatten()
        trajs_coll = t[coll_idxs] if coll_idxs.numel() else None
        trajs_free = t[free_idxs] if free_idxs.numel() else None
        if return_indices:
            return trajs_coll, coll_idxs, trajs_free, free_idxs, out[3]
        return trajs_coll, trajs_free

    def compute_fraction_free_trajs(self, trajs, **kwargs):
        """Share of the trajectories without a dense point in collision (Python float)."""
        _, (count, _, _) = self._trajs_stats(trajs, kwargs.get('num_interpolation', 5))
        return int((count == 0).sum()) / max(count.numel(), 1)

    def compute_collision_intensity_trajs(self, trajs, **kwargs):
        """Share of all N * P dense points that are in collision (Python float)."""
        n = int(kwargs.get('num_interpolation', 5))
        t, (count, _, _) = self._trajs_stats(trajs, n)
        return int(count.sum(dtype=torch.int64)) / max(count.numel() * ((t.shape[1] - 1) * (n + 1) + 1), 1)

    def compute_success_free_trajs(self, trajs, **kwargs):
        """1 if any trajectory is free of collisions, else 0."""
        _, (count, _, _) = self._trajs_stats(trajs, kwargs.get('num_interpolation', 5))
        return 1 if bool((count == 0).any()) else 0

    # ---- clearance and the certificate between the samples (build-defined: DESIGN.md 10) ----------------------------------------------
    def _certify_buffers(self, what):
        """(geometry with the whole link table in every field, reach buffer) of this task's robot and obstacle field(s), built on first
        use and kept.  The clearance walk knows the obstacle geometry alone: a self_field or an sdf_field is refused by name."""
        self.require_no_self_field(what)
        self.require_no_sdf_field(what)
        if '_certify_geom' not in self.__dict__:
            self._certify_geom = (ops.DeviceGeometry(self.robot, self.field, self.device, keep_all_links=True, use_model=False),
                                  ops.DeviceReach(self.robot, self.device))
        return self._certify_geom

    def compute_clearance(self, qs, return_link=False):
        """(..., D) configurations -> eta (...): the signed clearance of the robot's collision spheres from the obstacles, margins taken
        off (ops.clearance): eta < 0 is compute_collision's answer, eta is how far it is from flipping.  return_link adds the arg-min
        collision sphere, int32 (...)."""
        geom, _ = self._certify_buffers('compute_clearance (mpb_clearance)')
        q = torch.as_tensor(qs, dtype=torch.float32, device=self.device)
        if q.dim() < 1 or q.shape[-1] != self.q_dim:
            raise ValueError(f'qs has shape {tuple(q.shape)}, expected (..., {self.q_dim})')
        lead = tuple(q.shape[:-1])
        eta, link = ops.clearance(q.reshape(-1, self.q_dim).contiguous(), geom, with_link=True)
        return (eta.reshape(lead), link.reshape(lead)) if return_link else eta.reshape(lead)

    def certify_paths(self, paths, lengths=None, **kwargs):
        """(paths (N, Lmax, D), lengths (N,) int32 or None) -- what the RRT planners and shortcut_paths emit -> an ops.PathCertificate:
        which joint-space polylines are free of the obstacles over their whole continuum, not only at check_step samples
        (ops.path_certify, which also takes slack, c_req, max_depth, max_intervals).  The certificate covers the polyline, not a spline
        through it."""
        geom, reach = self._certify_buffers('certify_paths (mpb_path_certify)')
        p = torch.as_tensor(paths, dtype=torch.float32, device=self.device)
        if p.dim() != 3 or p.shape[-1] < self.q_dim:
            raise ValueError(f'paths has shape {tuple(p.shape)}, expected (N, Lmax, W) with W >= {self.q_dim}')
        if lengths is not None:
            lengths = torch.as_tensor(lengths, device=self.device).to(torch.int32).contiguous()
        return ops.path_certify(p.contiguous(), geom, reach, lengths=lengths, **kwargs)

    def certify_trajs(self, trajs, **kwargs):
        """trajs (..., H, W), W >= q_dim, leading dimensions flattened as in get_trajs_collision_and_free and read in place -> an
        ops.PathCertificate over the N flattened trajectories: free BETWEEN the waypoints too, where get_trajs_collision_and_free
        looks at num_interpolation points per segment.  The certificate covers the polyline through the waypoints, not a spline."""
        geom, reach = self._certify_buffers('certify_trajs (mpb_path_certify)')
        t = torch.as_tensor(trajs, dtype=torch.float32, device=self.device)
        if t.dim() < 2 or t.shape[-1] < self.q_dim:
            raise ValueError(f'trajs has shape {tuple(t.shape)}, expected (..., H, W) with W >= {self.q_dim}')
        return ops.path_certify(t.reshape(-1, t.shape[-2], t.shape[-1]).contiguous(), geom, reach, **kwargs)

    # ---- clearance and the certificate of a timed trajectory among moving obstacles (build-defined: DESIGN.md 10) -----------------------
    def _moving_certify_args(self, what, trajs, moving_field):
        """(flat trajs (N, R, W), leading shape, geometry with the whole link table, reach buffer, the packed buffer of (field, R))."""
        from .geometry import MovingObstacleField
        geom, reach = self._certify_buffers(what)
        if not isinstance(moving_field, MovingObstacleField):
            raise TypeError(f'{what.split(" ")[0]} takes a geometry.MovingObstacleField')
        t = torch.as_tensor(trajs, dtype=torch.float32, device=self.device)
        if t.dim() < 2 or t.shape[-1] < self.q_dim:
            raise ValueError(f'trajs has shape {tuple(t.shape)}, expected (..., R, W) with W >= {self.q_dim}')
        lead = tuple(t.shape[:-2])
        t = t.reshape(-1, t.shape[-2], t.shape[-1]).contiguous()
        return t, lead, geom, reach, self._moving_geom(moving_field, t.shape[1])

    def compute_clearance_moving(self, trajs, moving_field, return_args=False):
        """trajs (..., R, W), W >= q_dim -> eta (..., R): the signed clearance of every row at ITS OWN TIME of the field's clock over R
        rows, from the task's static obstacles and the moving ones, margins taken off (ops.moving_clearance): eta < 0 is
        check_trajs_moving's answer for the row, eta is how far it is from flipping.  return_args adds the arg-min collision sphere and
        the arg-min obstacle (o >= 0 a moving obstacle, -1 - f the static field f), int32 (..., R)."""
        t, lead, geom, _, mo = self._moving_certify_args('compute_clearance_moving (mpb_moving_clearance)', trajs, moving_field)
        eta, link, obst = ops.moving_clearance(t, geom, mo, with_args=True)
        R = t.shape[1]
        return (eta.reshape(*lead, R), link.reshape(*lead, R), obst.reshape(*lead, R)) if return_args else eta.reshape(*lead, R)

    def certify_trajs_moving(self, trajs, moving_field, c_req=0.0, max_depth=None, max_intervals=None, slack=None):
        """trajs (..., R, W), W >= q_dim, leading dimensions flattened -> an ops.TrajCertificate over the N flattened trajectories: which
        timed plans are free of the task's static obstacles AND of a geometry.MovingObstacleField over the whole continuum of the clock
        of R rows, with clearance above c_req -- where check_trajs_moving looks at the rows only (ops.traj_certify_moving, which has the
        definition).  The kernel certifies the chord motion between the rows' centres; the field's own motion is piecewise linear
        between keyframes, and a keyframe strictly inside a row interval makes the two differ by at most chord_deviation
        (st_certify_layout.chord_deviation, fp64): the required clearance is raised by it, c_req_eff = c_req + chord_deviation, so that
        FREE is a statement about the field's own motion.  The result reports chord_deviation and, as c_req, the effective value."""
        from . import certify_layout, st_certify_layout
        t, lead, geom, reach, mo = self._moving_certify_args('certify_trajs_moving (mpb_traj_certify_moving)', trajs, moving_field)
        dev = st_certify_layout.chord_deviation(moving_field, t.shape[1])
        cert = ops.traj_certify_moving(t, geom, mo, reach, slack=slack, c_req=float(c_req) + dev,
                                       max_depth=certify_layout.CERT_DEFAULT_MAX_DEPTH if max_depth is None else max_depth,
                                       max_intervals=certify_layout.CERT_DEFAULT_MAX_INTERVALS if max_intervals is None else max_intervals)
        cert.chord_deviation = dev
        return cert

    # ---- shortcutting of a path batch (build-defined: DESIGN.md 10) ------------------------------------------------------------
    def shortcut_paths(self, paths, lengths, n_iters=64, check_step=0.05, **kwargs):
        """(paths (N, Lmax, D), lengths (N,) int32) device tensors -> (paths, lengths, stats (N, 4)): n_iters shortcut attempts
        per path against this task's obstacle geometry, checked at spacing check_step (ops.path_shortcut, which also takes the
        keyword arguments draws, seed, problem_offset, with_log, out).  Without world_predicate the in-kernel predicate knows
        obstacles only and a task with a self_field or an sdf_field is refused by name; with it the candidates are checked against the
        world (mpb_path_shortcut_world)."""
        return ops.path_shortcut(paths, lengths, self.world_or_geom('path shortcutting (mpb_path_shortcut)'), n_iters, check_step, **kwargs)

    # ---- time parameterisation of a trajectory batch (build-defined: DESIGN.md 10) -------------------------------------------------
    def retime_trajs(self, trajs, dt=None, v_max=None, a_max=None, scale=1.0, **kwargs):
        """trajs (..., H, W), W >= q_dim, leading dimensions flattened as in get_trajs_collision_and_free -> a TrajsRetimed: the
        time-optimal rest-to-rest timing of every trajectory under per-joint velocity / acceleration limits (ops.traj_retime, which also
        takes the keyword arguments sdot_max, t_max) and, with a control period dt, the batch sampled at it (ops.traj_retime_sample).
        v_max, a_max default to the robot's dq_max, ddq_max; both are multiplied by `scale` (0 < scale: run slower than the data sheet
        allows).  The limits hold AT the waypoints, not between them: ops.traj_retime says by how much."""
        lim = {}
        for name, given, own in (('v_max', v_max, 'dq_max'), ('a_max', a_max, 'ddq_max')):
            v = getattr(self.robot, own, None) if given is None else given
            if v is None:
                raise ValueError(f'retime_trajs: no {name} given and the robot carries no {own}')
            lim[name] = torch.as_tensor(v, dtype=torch.float32).reshape(-1)
            if lim[name].numel() != self.q_dim:
                raise ValueError(f'retime_trajs: {name} has {lim[name].numel()} entries, the robot {self.q_dim} joints')
        scale = float(scale)
        if not (scale > 0 and scale < float('inf')):
            raise ValueError(f'retime_trajs: scale = {scale}, a finite factor > 0')
        t = torch.as_tensor(trajs, dtype=torch.float32, device=self.device)
        if t.dim() < 2 or t.shape[-1] < self.q_dim:
            raise ValueError(f'trajs has shape {tuple(t.shape)}, expected (..., H, W) with W >= {self.q_dim}')
        lead = tuple(t.shape[:-2])
        t = t.reshape(-1, t.shape[-2], t.shape[-1]).contiguous()
        timing = ops.traj_retime(t, lim['v_max'] * scale, lim['a_max'] * scale, **kwargs)
        trajs_dt = n_rows = sample_status = None
        if dt is not None:
            out, rows, st = ops.traj_retime_sample(t, timing, dt)
            trajs_dt, n_rows, sample_status = out.reshape(*lead, *out.shape[1:]), rows.reshape(lead), st.reshape(lead)
        return TrajsRetimed(timing.duration.reshape(lead), timing.status.reshape(lead), timing, trajs_dt, n_rows, sample_status)

    # ---- polylines into executable trajectories: linear segments with parabolic blends (build-defined: DESIGN.md 10) ---------------------
    def blend_paths(self, paths, lengths=None, dt=None, v_max=None, a_max=None, scale=1.0, max_deviation=None, certificate=None, **kwargs):
        """paths (..., H, W), W >= q_dim, leading dimensions kept, lengths (...) int32 or None -- what the RRT planners, PRM and
        shortcut_paths emit -> a PathsBlended: every polyline run at constant velocity along its segments with a constant-acceleration
        blend around every waypoint (ops.path_blend, which has the guarantees and also takes max_sweeps) and, with a control period dt,
        sampled at it (ops.path_blend_sample).  v_max, a_max default to the robot's dq_max, ddq_max; both are multiplied by `scale`.
        Unlike retime_trajs the limits hold for EVERY t and the trajectory stays within a known distance of the polyline; it is not
        time-optimal.

        certificate: the ops.PathCertificate of certify_paths ON THE SAME paths and lengths.  The result then carries
        deviation_workspace (...): no collision sphere of the blended trajectory is farther than that from where it is on the polyline
        (the reach table of the certifier applied to the per-joint deviations), and certified (...) bool: status OK, certificate FREE and
        deviation_workspace < margin_cert -- the blended trajectory is then free of the obstacles over its whole continuum, with
        nothing checked again.  max_deviation (rad, joint-space infinity-norm; None: no cap) is the knob that buys `certified` at the
        price of duration: a smaller cap keeps the blends closer to the corners and makes them slower."""
        lim = {}
        for name, given, own in (('v_max', v_max, 'dq_max'), ('a_max', a_max, 'ddq_max')):
            v = getattr(self.robot, own, None) if given is None else given
            if v is None:
                raise ValueError(f'blend_paths: no {name} given and the robot carries no {own}')
            lim[name] = torch.as_tensor(v, dtype=torch.float32).reshape(-1)
            if lim[name].numel() != self.q_dim:
                raise ValueError(f'blend_paths: {name} has {lim[name].numel()} entries, the robot {self.q_dim} joints')
        scale = float(scale)
        if not (scale > 0 and scale < float('inf')):
            raise ValueError(f'blend_paths: scale = {scale}, a finite factor > 0')
        p = torch.as_tensor(paths, dtype=torch.float32, device=self.device)
        if p.dim() < 2 or p.shape[-1] < self.q_dim:
            raise ValueError(f'paths has shape {tuple(p.shape)}, expected (..., H, W) with W >= {self.q_dim}')
        lead = tuple(p.shape[:-2])
        p = p.reshape(-1, p.shape[-2], p.shape[-1]).contiguous()
        if lengths is not None:
            lengths = torch.as_tensor(lengths, device=self.device).to(torch.int32).reshape(-1).contiguous()
        timing = ops.path_blend(p, lim['v_max'] * scale, lim['a_max'] * scale, lengths=lengths, max_deviation=max_deviation, **kwargs)
        res = PathsBlended(timing.duration.reshape(lead), timing.status.reshape(lead), timing)
        if dt is not None:
            out, rows, st = ops.path_blend_sample(p, timing, dt)
            res.trajs_dt, res.n_rows, res.sample_status = out.reshape(*lead, *out.shape[1:]), rows.reshape(lead), st.reshape(lead)
        if certificate is not None:
            _, reach = self._certify_buffers('blend_paths with a certificate (mpb_path_certify)')
            if certificate.status.numel() != p.shape[0]:
                raise ValueError(f'blend_paths: the certificate is of {certificate.status.numel()} paths, paths holds {p.shape[0]}')
            dev_w = self._blend_workspace_deviation(p, timing, reach)
            res.deviation_workspace = dev_w.reshape(lead)
            res.certified = ((timing.status == ops.BLEND_OK) & (certificate.status == ops.CERT_FREE)
                             & (dev_w < certificate.margin_cert.to(torch.float64))).reshape(lead)
        return res

    def _blend_workspace_deviation(self, p, timing, reach):
        """(N,) fp64 on the device: max over waypoints i and collision spheres l of sum_k rho_kl dev_ik, dev_ik = |dv_ik| tb_i / 8 formed
        from the timing's T and tb (blend_layout.joint_deviation / workspace_deviation are the same on the host)."""
        from . import certify_layout
        N, H, _ = p.shape
        D = self.q_dim
        q, T, tb = p[:, :, :D].to(torch.float64), timing.T.to(torch.float64), timing.tb.to(torch.float64)
        L = torch.full((N,), H, device=p.device, dtype=torch.int64) if timing.lengths is None else timing.lengths.to(torch.int64)
        seg = (torch.arange(H - 1, device=p.device)[None, :] < (L - 1)[:, None]) & (T > 0)
        v = torch.where(seg[:, :, None], (q[:, 1:] - q[:, :-1]) / torch.where(seg, T, torch.ones_like(T))[:, :, None], torch.zeros((), dtype=torch.float64, device=p.device))
        v = torch.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0)
        zero = torch.zeros(N, 1, D, dtype=torch.float64, device=p.device)
        dv = torch.cat([v, zero], 1) - torch.cat([zero, v], 1)
        way = torch.arange(H, device=p.device)[None, :] < L[:, None]
        dev = torch.where(way[:, :, None], dv.abs() * tb[:, :, None] / 8.0, torch.zeros((), dtype=torch.float64, device=p.device))
        rho = torch.from_numpy(reach.host[certify_layout.REACH_HEADER_WORDS:].reshape(D, reach.n_links).astype('float64')).to(p.device)
        return (dev @ rho).amax(dim=(1, 2)) if N else torch.zeros(0, dtype=torch.float64, device=p.device)


class PathsBlended:
    """What PlanningTask.blend_paths returns, the leading dimensions of its input kept: durations (...) seconds, status (...) int32
    (ops.BLEND_OK / BLEND_NOT_CONVERGED / BLEND_DEGENERATE_SEGMENT / BLEND_BAD_INPUT), timing (the flat ops.BlendTiming: T, tb, tw, dev, ...);
    with a control period also trajs_dt (..., n_rows, 3D) positions, velocities and accelerations at k dt, n_rows (...) int32 the rows
    each path needs, sample_status (...) int32; with a certificate also deviation_workspace (...) fp64 metres and certified (...) bool;
    else None."""

    def __init__(self, durations, status, timing):
        self.durations, self.status, self.timing = durations, status, timing
        self.trajs_dt = self.n_rows = self.sample_status = self.deviation_workspace = self.certified = None


class TrajsRetimed:
    """What PlanningTask.retime_trajs returns, the leading dimensions of its input kept: durations (...) seconds, status (...) int32
    (ops.RETIME_OK / RETIME_STALLED), timing (the flat ops.TrajTiming: x, u, t, qd); with a control period also trajs_dt (..., n_rows, 2D)
    positions and velocities at k dt, n_rows (...) int32 the rows each trajectory needs, sample_status (...) int32; else None."""

    def __init__(self, durations, status, timing, trajs_dt=None, n_rows=None, sample_status=None):
        self.durations, self.status, self.timing = durations, status, timing
        self.trajs_dt, self.n_rows, self.sample_status = trajs_dt, n_rows, sample_status


class CartesianPathResult:
    """What PlanningTask.cartesian_path returns, q_start's leading dimensions (...) kept: q (..., K+1, D) -- row 0 the start, rows beyond
    n_ok repeat row n_ok: always a valid trajectory --, n_ok (...) int32 steps accepted, fraction (...) = n_ok / K, status (...) int32
    (ops.CART_OK / CART_LOST / CART_JUMP / CART_BAD_TARGET / CART_COLLISION), complete (...) bool = status is CART_OK, pos_err / rot_err
    (..., K+1) the tracking error of every row against its step's target as the tracker left it (the rejected step's in row n_ok + 1 of
    a LOST or JUMP problem).  q[complete] is a trajectory batch for retime_trajs and the validation calls."""

    def __init__(self, q, n_ok, status, pos_err, rot_err, n_steps):
        self.q, self.n_ok, self.status, self.pos_err, self.rot_err, self.n_steps = q, n_ok, status, pos_err, rot_err, int(n_steps)
        self.fraction = n_ok.to(torch.float32) / float(n_steps)
        self.complete = status == ops.CART_OK


class IKResult:
    """What PlanningTask.inverse_kinematics returns: q (N, S, D), converged / free bool (N, S) (free = converged and not in collision
    by the task's predicates), pos_err / rot_err (N, S) at q, iters int32 (N, S) steps taken."""

    def __init__(self, q, converged, free, pos_err, rot_err, iters, q_ref=None):
        self.q, self.converged, self.free, self.pos_err, self.rot_err, self.iters, self.q_ref = q, converged, free, pos_err, rot_err, iters, q_ref

    def select(self, k=1):
        """(q (N, k, D), valid bool (N, k)): per target its first k free solutions -- ordered by distance to q_ref when one was given
        (stable: ties by seed index), otherwise by seed index; rows beyond a target's free solutions are invalid (and hold the
        solutions that follow in that order)."""
        N, S, D = self.q.shape
        k = int(k)
        if not 1 <= k <= S:
            raise ValueError(f'k = {k} outside 1..{S}')
        order = torch.arange(S, device=self.q.device).expand(N, S)
        if self.q_ref is not None:
            order = torch.argsort(torch.linalg.norm(self.q - self.q_ref[:, None, :], dim=-1), dim=1, stable=True)
        free = torch.gather(self.free, 1, order)
        pick = torch.gather(order, 1, torch.argsort((~free).to(torch.uint8), dim=1, stable=True)[:, :k])      # free ones first, order kept
        return torch.gather(self.q, 1, pick[:, :, None].expand(N, k, D)), torch.gather(self.free, 1, pick)
