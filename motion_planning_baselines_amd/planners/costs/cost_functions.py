"""Cost-function objects with the reference's API surface (mp_baselines/planners/costs/cost_functions.py)
whose evaluation runs in the HIP library.

``Cost.__call__(trajs) -> (B,)`` / ``eval`` / ``get_linear_system`` keep the reference's meaning
(cost_functions.py:18-53).  The planners recognise these objects and fuse their arithmetic into the
planner kernels (no per-term launches); called on their own, ``eval`` launches the stand-alone HIP
collision-cost kernel (mpb_cost_collision_eval) or the trajectory-terms kernel (mpb_cost_terms_eval:
GP prior, start / goal priors, CHOMP smoothness, joint limits -- any subset of them in one pass, which
is how CostComposite evaluates them).  There is no CPU path: trajectories must be CUDA tensors.
"""
from abc import ABC, abstractmethod

import numpy as np
import torch

from ... import ops
from ...geometry import GridSDFField, MovingObstacleField, SelfCollisionField


class Cost(ABC):
    """cost_functions.py:18-53."""

    def __init__(self, robot, n_support_points, tensor_args=None, **kwargs):
        self.robot = robot
        self.n_dof = robot.q_dim
        self.dim = 2 * self.n_dof
        self.n_support_points = n_support_points
        self.tensor_args = tensor_args

    def set_cost_factors(self):
        pass

    def __call__(self, trajs, **kwargs):
        return self.eval(trajs, **kwargs)

    @abstractmethod
    def eval(self, trajs, **kwargs):
        pass

    @abstractmethod
    def get_linear_system(self, trajs, **kwargs):
        pass

    def get_q_pos_vel_and_fk_map(self, trajs, **kwargs):
        """cost_functions.py:41-53: (trajs (B,H,d), q_pos, q_vel, H_positions) with H_positions = positions of the
        robot's collision spheres (B,H,L,3), computed by the FK kernel (mpb_fk_collision_points)."""
        trajs = self._as_3d(trajs)
        q_pos = self.robot.get_position(trajs)
        q_vel = self.robot.get_velocity(trajs)
        geom = self.__dict__.get('_fk_geom')
        if geom is None or geom.buf.device != trajs.device:
            import numpy as np
            from ...geometry import CollisionField
            far = CollisionField(spheres=np.array([[1.0e6, 1.0e6, 1.0e6, 1.0]], np.float32))     # FK only: the field is unused
            geom = self.__dict__['_fk_geom'] = ops.DeviceGeometry(self.robot, far, trajs.device, keep_all_links=True)
        return trajs, q_pos, q_vel, ops.fk_collision_points(trajs, geom)

    @staticmethod
    def _as_3d(trajs):
        """Accept (B,H,d) or (N,B,H,d) like get_q_pos_vel_and_fk_map (cost_functions.py:41-48)."""
        assert trajs.ndim == 3 or trajs.ndim == 4
        if trajs.ndim == 4:
            trajs = trajs.reshape(-1, trajs.shape[-2], trajs.shape[-1])
        return trajs.contiguous()


class CostCollision(Cost):
    """Hinge collision cost over one collision field (cost_functions.py:147-231).

    eval: ``1/sigma_coll^2 * sum_{h>=1} field_cost(q_h)`` (traj_range [1, None], field_factor.py:31-39).

    `field` may be a geometry.SelfCollisionField (the robot against itself; the reference's examples get that field from
    task.get_collision_fields() with use_self_collision_storm=True): eval / eval_with_grad / get_linear_system then go to the
    self-collision kernels (mpb_self_collision_*).  Such a member is never fused into a planner kernel.

    `field` may also be a geometry.GridSDFField (a precomputed grid of signed distances, the reference's precompute_sdf_obj_fixed=True):
    the same three go to the SDF-grid kernels (mpb_sdf_grid_*).

    `field` may also be a geometry.MovingObstacleField (obstacles whose centres follow keyframes; row h of whatever trajectory the member
    is handed sees them at the time t_h of the field's clock): the same three go to the moving-obstacle kernels (mpb_moving_collision_*),
    through one packed buffer per row count (device_own(device, rows)).

    All three kinds are "members with kernels of their own" (own_kernels): never an obstacle member, never fused, served by own_eval /
    own_grad -- which is all a planner's device path needs to know of them.
    """

    def __init__(self, robot, n_support_points, field=None, sigma_coll=None, **kwargs):
        super().__init__(robot, n_support_points, **kwargs)
        self.field = field
        self.sigma_coll = sigma_coll
        self._geom = None
        self._own = None

    @property
    def k_sigma(self):
        return 1.0 / (self.sigma_coll ** 2)          # FieldFactor.K (field_factor.py:15)

    @property
    def is_self(self):
        return isinstance(self.field, SelfCollisionField)

    @property
    def is_grid(self):
        return isinstance(self.field, GridSDFField)

    @property
    def is_moving(self):
        return isinstance(self.field, MovingObstacleField)

    @property
    def own_kernels(self):
        """The member's field is no static obstacle list: it has eval / gradient kernels of its own (own_eval, own_grad)."""
        return self.is_self or self.is_grid or self.is_moving

    def device_own(self, device, rows=None):
        """The packed buffer of a member with kernels of its own on `device` -- an ops.DeviceSelfCollision, an ops.DeviceSDFGrid or an
        ops.DeviceMovingObstacles: packed, checked and uploaded (the grid, where it has no host values, built there) once.  `rows`: the
        rows of the trajectories a MovingObstacleField member is to serve -- one buffer per row count is kept (the support points, an
        interpolated trajectory and MPPI's rollouts each have their own); the other kinds ignore it."""
        assert self.own_kernels
        if self.is_moving:
            if rows is None:
                raise TypeError('device_own of a MovingObstacleField member needs the row count: its buffer holds the centres per row')
            cache = self.__dict__.setdefault('_own_rows', {})
            key = (str(torch.device(device)), int(rows))
            if key not in cache or cache[key].field is not self.field:
                cache[key] = ops.DeviceMovingObstacles(self.robot, self.field, device, int(rows))
            return cache[key]
        if self._own is None or self._own.buf.device != torch.device(device):
            self._own = (ops.DeviceSelfCollision if self.is_self else ops.DeviceSDFGrid)(self.robot, self.field, device)
        return self._own

    def device_self(self, device):
        """device_own of a SelfCollisionField member."""
        assert self.is_self
        return self.device_own(device)

    def device_sdf(self, device):
        """device_own of a GridSDFField member."""
        assert self.is_grid
        return self.device_own(device)

    def own_eval(self, trajs, weight=1.0, k_sigma=None, **kw):
        """ops.self_collision_eval / ops.sdf_grid_eval / ops.moving_collision_eval of this member on (B, H, d) trajectories: h_begin,
        per_waypoint, out, accumulate as those take them; k_sigma defaults to the member's.  A MovingObstacleField member takes the row
        count, hence the times, from trajs.shape[1]."""
        own = self.device_own(trajs.device, trajs.shape[1])
        return ops.MEMBER_OPS[type(own)].eval(trajs, own, self.k_sigma if k_sigma is None else k_sigma, weight=weight, **kw)

    def own_grad(self, trajs, weight=1.0, k_sigma=None, **kw):
        """ops.self_collision_grad / ops.sdf_grid_grad / ops.moving_collision_grad of this member: h_begin, out, grad, accumulate as
        those take them."""
        own = self.device_own(trajs.device, trajs.shape[1])
        return ops.MEMBER_OPS[type(own)].grad(trajs, own, self.k_sigma if k_sigma is None else k_sigma, weight=weight, **kw)

    def device_geometry(self, device):
        if self.is_self:
            raise TypeError('a SelfCollisionField has no obstacle geometry: use device_self()')
        if self.is_grid:
            raise TypeError('a GridSDFField has no obstacle geometry: use device_sdf()')
        if self.is_moving:
            raise TypeError('a MovingObstacleField has no static obstacle geometry: use device_own(device, rows)')
        if self._geom is None or self._geom.buf.device != torch.device(device):
            self._geom = ops.DeviceGeometry(self.robot, self.field, device)
        return self._geom

    def eval(self, trajs, **observation):
        if self.field is None:
            return 0
        trajs = self._as_3d(trajs)
        if self.own_kernels:
            return self.own_eval(trajs)
        return ops.cost_collision_eval(trajs, self.device_geometry(trajs.device), self.k_sigma)

    def eval_with_grad(self, trajs, weight=1.0):
        """(cost (B,), d cost / d trajs (B,H,d)): what the reference gets from autograd (chomp.py:139)."""
        trajs = self._as_3d(trajs)
        if self.own_kernels:
            return self.own_grad(trajs, weight=weight)
        return ops.cost_collision_grad(trajs, self.device_geometry(trajs.device), self.k_sigma, weight=weight)

    def get_linear_system(self, trajs, n_interpolated_points=None, **observation):
        """Dense (A, b, K) rows of the collision factor (cost_functions.py:191-231): row i has H_obst = -d err / d q at
        columns (i+1)*dim .. +n_dof, b = the support points' errors, K = I / sigma^2.  With `n_interpolated_points`
        (forwarded by CostComposite.get_linear_system, cost_functions.py:112-119) the Jacobian is that of the
        INTERPOLATED trajectory's error w.r.t. the support points (field_factor.py:42-54) while b stays the support
        points' own error.  Values come from the kernel GPMP2 itself uses (mpb_gpmp2_linearize); the dense form is
        an inspection aid -- GPMP2 never materialises it."""
        trajs = self._as_3d(trajs)
        B, H, d = trajs.shape
        assert d == self.dim, 'get_linear_system works on (B, H, 2*n_dof) trajectories'
        if self.own_kernels:
            return self._self_linear_system(trajs)
        rows = ops.gpmp2_collision_rows(trajs, self.device_geometry(trajs.device), n_interp=n_interpolated_points or 0)[0]
        N, D = self.dim * H, self.n_dof
        A = torch.zeros(B, H - 1, N, device=trajs.device, dtype=trajs.dtype)
        for i in range(H - 1):
            A[:, i, (i + 1) * self.dim:(i + 1) * self.dim + D] = rows[:, i + 1, :D]
        b = rows[:, 1:, D].unsqueeze(-1).clone()
        K = self.k_sigma * torch.eye(H - 1, device=trajs.device, dtype=trajs.dtype).repeat(B, 1, 1)
        return A, b, K

    def _self_linear_system(self, trajs):
        """(A, b, K) of a self-collision or SDF-grid member in the obstacle member's convention: row i holds -d c / d q of waypoint i + 1 at
        that waypoint's position columns, b the waypoint costs, K = I / sigma^2.  ONE gradient launch gives every row of A (c_h
        depends on q_h alone: the gradient of sum_h c_h IS the per-waypoint Jacobian); b takes a cost launch of its own, since
        mpb_self_collision_grad has no per-waypoint output.  The support points only: a self member has no interpolated
        Jacobian."""
        B, H, d = trajs.shape
        D = self.n_dof
        _, grad = self.own_grad(trajs, k_sigma=1.0, h_begin=1)
        _, pw = self.own_eval(trajs, k_sigma=1.0, h_begin=1, per_waypoint=True)
        A = torch.zeros(B, H - 1, self.dim * H, device=trajs.device, dtype=trajs.dtype)
        for i in range(H - 1):
            A[:, i, (i + 1) * self.dim:(i + 1) * self.dim + D] = -grad[:, i + 1, :D]
        b = pw[:, 1:].unsqueeze(-1).clone()
        K = self.k_sigma * torch.eye(H - 1, device=trajs.device, dtype=trajs.dtype).repeat(B, 1, 1)
        return A, b, K


class _TrajectoryTermCost(Cost):
    """A cost that depends on the trajectory alone (no FK / field): served by mpb_cost_terms_eval.
    ``term_spec(device)`` returns the keyword arguments of ops.cost_terms_eval for this term with unit
    composite weight; CostComposite merges the specs of its members into one launch."""

    def term_spec(self, device):
        raise NotImplementedError

    def _dev(self, name, value, device):
        """float32 device copy of a small constant, cached per device."""
        cache = self.__dict__.setdefault('_dev_cache', {})
        key = (name, str(device))
        if key not in cache:
            cache[key] = torch.as_tensor(np.asarray(value.detach().cpu() if torch.is_tensor(value) else value),
                                         dtype=torch.float32).to(device).contiguous()
        return cache[key]

    def eval(self, trajs, **observation):
        trajs = self._as_3d(trajs)
        out, _ = ops.cost_terms_eval(trajs, self.n_dof, **self.term_spec(trajs.device))
        return out

    def get_linear_system(self, trajs, **observation):
        return None                                   # the reference's `pass` (cost_functions.py:356-357, :389, :428)


class CostGPTrajectory(_TrajectoryTermCost):
    """GP-prior smoothness cost sum_t e_t^T Q^-1 e_t (cost_functions.py:317-357; GPFactor gp_factor.py:4-65)."""

    def __init__(self, robot, n_support_points, dt, sigma_gp=None, **kwargs):
        super().__init__(robot, n_support_points, **kwargs)
        self.dt = dt
        self.sigma_gp = sigma_gp

    def term_spec(self, device):
        return dict(terms={'gp'}, dt=self.dt, k_gp=1.0 / self.sigma_gp ** 2)


class CostGPTrajectoryPositionOnlyWrapper(CostGPTrajectory):
    """Same cost on position-only trajectories: velocities by central differences inside the kernel
    (cost_functions.py:360-368)."""

    def term_spec(self, device):
        return dict(terms={'gp'}, dt=self.dt, k_gp=1.0 / self.sigma_gp ** 2, vel_fd=True)


class CostGP(_TrajectoryTermCost):
    """Start prior + GP prior (cost_functions.py:234-314)."""

    def __init__(self, robot, n_support_points, start_state, dt, sigma_params, **kwargs):
        super().__init__(robot, n_support_points, **kwargs)
        self.start_state = start_state
        self.dt = dt
        self.sigma_start = sigma_params['sigma_start']
        self.sigma_gp = sigma_params['sigma_gp']

    def term_spec(self, device):
        return dict(terms={'gp', 'start'}, dt=self.dt, k_gp=1.0 / self.sigma_gp ** 2,
                    k_start=1.0 / self.sigma_start ** 2, start_state=self._dev('start', self.start_state, device))

    def get_linear_system(self, trajs, **observation):
        """Dense (A, b, K) of the start + GP factors (cost_functions.py:291-314).  Inspection aid (torch
        assembly on the device): GPMP2 never materialises it, it works on the block-tridiagonal form."""
        trajs = self._as_3d(trajs)
        B, H, dim = trajs.shape
        D, dt, dev = self.n_dof, self.dt, trajs.device
        kw = dict(device=dev, dtype=trajs.dtype)
        N = dim * H
        A, b, K = torch.zeros(B, N, N, **kw), torch.zeros(B, N, 1, **kw), torch.zeros(B, N, N, **kw)
        I, Z = torch.eye(D, **kw), torch.zeros(D, D, **kw)
        Phi = torch.cat((torch.cat((I, dt * I), 1), torch.cat((Z, I), 1)), 0)
        Qc = I / self.sigma_gp ** 2
        Qi = torch.cat((torch.cat((12. * dt ** -3. * Qc, -6. * dt ** -2. * Qc), 1),
                        torch.cat((-6. * dt ** -2. * Qc, 4. * dt ** -1. * Qc), 1)), 0)
        A[:, :dim, :dim] = torch.eye(dim, **kw)                                                # unary_factor.py:28
        b[:, :dim, 0] = self.start_state.to(**kw) - trajs[:, 0]
        K[:, :dim, :dim] = torch.eye(dim, **kw) / self.sigma_start ** 2
        for t in range(H - 1):
            r = slice(dim * (t + 1), dim * (t + 2))
            A[:, r, dim * t:dim * (t + 1)] = Phi                                               # H1 (gp_factor.py:28)
            A[:, r, r] += -torch.eye(dim, **kw)                                                # H2 (gp_factor.py:29-31)
            K[:, r, r] += Qi
        b[:, dim:, 0] = (trajs[:, 1:] - trajs[:, :-1] @ Phi.t()).reshape(B, -1)
        return A, b, K


class CostSmoothnessCHOMP(_TrajectoryTermCost):
    """x^T R x with CHOMP's precision R (cost_functions.py:371-390; chomp.py:81-101).  The reference
    returns whatever torch_robotics' batched_weighted_dot_prod returns (external); this build defines
    the cost as the sum over state columns -> (B,)."""

    def __init__(self, robot, n_support_points, **kwargs):
        super().__init__(robot, n_support_points, **kwargs)
        self.dt = robot.dt
        assert self.dt is not None, 'CostSmoothnessCHOMP reads robot.dt (cost_functions.py:380)'

    def term_spec(self, device):
        return dict(terms={'smooth'}, dt=self.dt, k_smooth=1.0)


class CostJointLimits(_TrajectoryTermCost):
    """Squared violation of q_min + eps / q_max - eps (cost_functions.py:393-429).  As in the reference the
    result is ONE scalar for the whole batch (its `.sum(-1)` acts on a 1-D gather); CostComposite adds
    it to every trajectory's cost."""

    def __init__(self, robot, n_support_points, eps=np.deg2rad(3), **kwargs):
        super().__init__(robot, n_support_points, **kwargs)
        self.eps = float(eps)

    def term_spec(self, device):
        return dict(terms={'jlim'}, k_jlim=1.0, jl_eps=self.eps, q_min=self._dev('q_min', self.robot.q_min, device),
                    q_max=self._dev('q_max', self.robot.q_max, device))

    def eval(self, trajs, **observation):
        assert trajs.ndim == 3                                                                  # cost_functions.py:407
        trajs = trajs.contiguous()
        _, total = ops.cost_terms_eval(trajs, self.n_dof, broadcast_jlim=False, **self.term_spec(trajs.device))
        return total.to(torch.float32)


class CostGoalPrior(_TrajectoryTermCost):
    """Unary prior on the last state, one goal per block of num_particles_per_goal * num_samples
    trajectories (cost_functions.py:488-554)."""

    def __init__(self, robot, n_support_points, multi_goal_states=None, num_particles_per_goal=None,
                 num_samples=None, sigma_goal_prior=None, **kwargs):
        super().__init__(robot, n_support_points, **kwargs)
        self.multi_goal_states = multi_goal_states
        self.num_goals = multi_goal_states.shape[0]
        self.num_particles_per_goal = num_particles_per_goal
        self.num_particles = num_particles_per_goal * self.num_goals
        self.num_samples = num_samples
        self.sigma_goal_prior = sigma_goal_prior

    def term_spec(self, device):
        return dict(terms={'goal'}, k_goal=1.0 / self.sigma_goal_prior ** 2,
                    goal_states=self._dev('goals', self.multi_goal_states, device),
                    trajs_per_goal=self.num_particles_per_goal * self.num_samples)

    def eval(self, trajs, **observation):
        trajs = self._as_3d(trajs)
        assert trajs.shape[0] == self.num_goals * self.num_particles_per_goal * self.num_samples  # the reshape at :525
        return super().eval(trajs, **observation)

    def get_linear_system(self, trajs, **observation):
        """(A, b, K) of the goal factor (cost_functions.py:538-554); one row block per particle."""
        trajs = self._as_3d(trajs)
        B, H, dim = trajs.shape
        kw = dict(device=trajs.device, dtype=trajs.dtype)
        A = torch.zeros(B, dim, dim * H, **kw)
        A[:, :, -dim:] = torch.eye(dim, **kw)
        goals = self.multi_goal_states.to(**kw).repeat_interleave(self.num_particles_per_goal, 0)
        b = (goals - trajs[:, -1]).unsqueeze(-1)
        K = (torch.eye(dim, **kw) / self.sigma_goal_prior ** 2).repeat(B, 1, 1)
        return A, b, K


class CostGoal(Cost):
    """Field cost of the LAST waypoint only (FieldFactor with traj_range [-1, None]; cost_functions.py:432-485);
    0 without a field.  With a CollisionField it is the collision kernel restricted to h = H-1."""

    def __init__(self, robot, n_support_points, field=None, sigma_goal=None, **kwargs):
        super().__init__(robot, n_support_points, **kwargs)
        self.field = field
        self.sigma_goal = sigma_goal
        self._geom = None

    def eval(self, trajs, x_trajs=None, **observation):
        if self.field is None:
            return 0
        trajs = self._as_3d(trajs)
        if self._geom is None or self._geom.buf.device != trajs.device:
            self._geom = ops.DeviceGeometry(self.robot, self.field, trajs.device)
        return ops.cost_collision_eval(trajs, self._geom, 1.0 / self.sigma_goal ** 2, h_begin=trajs.shape[1] - 1)

    def get_linear_system(self, trajs, x_trajs=None, **observation):
        if self.field is None:
            return None, None, None
        trajs = self._as_3d(trajs)
        B, H, d = trajs.shape
        if self._geom is None or self._geom.buf.device != trajs.device:
            self._geom = ops.DeviceGeometry(self.robot, self.field, trajs.device)
        _, pw = ops.cost_collision_eval(trajs, self._geom, 1.0, h_begin=H - 1, per_waypoint=True)
        _, grad = ops.cost_collision_grad(trajs, self._geom, 1.0, h_begin=H - 1)
        A = torch.zeros(B, 1, self.dim * H, device=trajs.device, dtype=trajs.dtype)
        A[:, 0, (H - 1) * self.dim:(H - 1) * self.dim + self.n_dof] = -grad[:, -1, :self.n_dof]
        b = pw[:, -1:].unsqueeze(-1)
        K = (1.0 / self.sigma_goal ** 2) * torch.ones(B, 1, 1, device=trajs.device, dtype=trajs.dtype)
        return A, b, K


class CostEEPose(Cost):
    """End-effector pose cost (build-defined; kernels of its own: mpb_ee_cost_eval / _grad): over the waypoints h of
    `traj_range`, with (R, t) the end-effector pose of q_h and [R* | t*] the target,

        c_h = |t* - t|^2 / sigma_pos^2 + (|e_w|^2  or  |R a - R* a|^2) / sigma_rot^2,        cost = sum_h c_h

    - sigma_pos given: the position term.  sigma_rot given: the rotation term -- e_w the rotation error of the inverse kinematics
      (angle * axis of R* R^T), or, with `axis` = a (a unit vector of the TOOL frame), the distance of the world directions R a and R* a:
      the rotation about a is free ("keep the cup upright"; `target_for_axis` builds such a target).  At least one sigma.
    - traj_range: 'goal' (the last waypoint), 'path' (waypoints 1 .. H-1, the collision members' range) or (h_begin, h_end).
    - target: (3, 4) for all, or (G, 3, 4), one per goal: trajectory b of a flat batch of B reads target b // (B / G) (the reshape of
      CostGoalPrior.eval; B % G != 0 is a ValueError).  With target_per_waypoint (H, 3, 4) or (G, H, 3, 4): a Cartesian path to track.

    The gradient is the closed form through the geometric Jacobian (include/mpb.h).  theta = pi is a cut locus of the full rotation
    term; the axis term has none.  A member with kernels of its own (own_kernels), like the self-collision and SDF-grid members: never
    fused, served by own_eval / own_grad on CHOMP's and STOMP's planned paths, by CostComposite.eval for MPPI, and by
    get_linear_system as one of GPMP2's extra_costs.  CHOMP zeroes the gradient rows of both endpoints, so a 'goal' member does nothing
    there: it acts wherever the last waypoint is free to move."""

    own_kernels = True
    is_self = False
    is_grid = False
    is_moving = False

    def __init__(self, robot, n_support_points, target, sigma_pos=None, sigma_rot=None, axis=None, traj_range='goal',
                 target_per_waypoint=False, tensor_args=None, **kwargs):
        super().__init__(robot, n_support_points, tensor_args=tensor_args, **kwargs)
        from ...geometry import KIND_CHAIN
        if getattr(robot, 'kind', None) != KIND_CHAIN:
            raise ValueError('CostEEPose: a point robot has no end effector (serial chains only)')
        if sigma_pos is None and sigma_rot is None:
            raise ValueError('CostEEPose: give sigma_pos, sigma_rot or both')
        for name, sg in (('sigma_pos', sigma_pos), ('sigma_rot', sigma_rot)):
            if sg is not None and not (float(sg) > 0.0 and np.isfinite(float(sg))):
                raise ValueError(f'CostEEPose: {name} must be positive and finite')
        if axis is not None:
            if sigma_rot is None:
                raise ValueError('CostEEPose: an axis needs sigma_rot')
            axis = tuple(float(x) for x in np.asarray(axis, dtype=np.float64).reshape(-1))
            if len(axis) != 3 or not abs(float(np.linalg.norm(axis)) - 1.0) <= 1e-3:
                raise ValueError(f'CostEEPose: axis {axis} is not a unit 3-vector (within 1e-3)')
        H = int(n_support_points)
        if isinstance(traj_range, str):
            if traj_range not in ('goal', 'path'):
                raise ValueError("CostEEPose: traj_range is 'goal', 'path' or (h_begin, h_end)")
        else:
            h0, h1 = (int(x) for x in traj_range)
            if not 0 <= h0 < h1 <= H:
                raise ValueError(f'CostEEPose: bad range [{h0}, {h1}) of {H} support points')
            traj_range = (h0, h1)
        target = torch.as_tensor(target)
        per = (H, 3, 4) if target_per_waypoint else (3, 4)
        if target.dim() not in (len(per), len(per) + 1) or tuple(target.shape[-len(per):]) != per:
            raise ValueError(f'CostEEPose: target has shape {tuple(target.shape)}, expected {per} or (G,) + {per}')
        self.target = target.detach().to(torch.float32)
        self.num_goals = int(target.shape[0]) if target.dim() == len(per) + 1 else 1
        self.sigma_pos, self.sigma_rot, self.axis = sigma_pos, sigma_rot, axis
        self.traj_range, self.target_per_waypoint = traj_range, bool(target_per_waypoint)
        self._geom = None
        self._target_dev = None

    @property
    def k_pos(self):
        return 0.0 if self.sigma_pos is None else 1.0 / float(self.sigma_pos) ** 2

    @property
    def k_rot(self):
        return 0.0 if self.sigma_rot is None else 1.0 / float(self.sigma_rot) ** 2

    @staticmethod
    def target_for_axis(axis, direction, position=(0.0, 0.0, 0.0)):
        """A target (3, 4) = [R* | position] whose R* takes the tool axis `axis` to the world direction `direction` (R* a = d, the
        smallest such rotation): the target of an `axis` member that keeps the tool axis pointing along d."""
        a = np.asarray(axis, dtype=np.float64).reshape(3)
        d = np.asarray(direction, dtype=np.float64).reshape(3)
        a, d = a / np.linalg.norm(a), d / np.linalg.norm(d)
        v, c = np.cross(a, d), float(a @ d)
        if c < -1.0 + 1e-12:                                    # opposite: half a turn about any axis perpendicular to a
            p = np.cross(a, np.eye(3)[int(np.argmin(np.abs(a)))])
            p /= np.linalg.norm(p)
            R = 2.0 * np.outer(p, p) - np.eye(3)
        else:
            V = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
            R = np.eye(3) + V + V @ V / (1.0 + c)
        return torch.as_tensor(np.concatenate([R, np.asarray(position, dtype=np.float64).reshape(3, 1)], 1), dtype=torch.float32)

    def device_geometry(self, device):
        """The chain on `device` (the end-effector kernels read the header and the joint transforms alone: the field is unused)."""
        if self._geom is None or self._geom.buf.device != torch.device(device):
            from ...geometry import CollisionField
            far = CollisionField(spheres=np.array([[1.0e6, 1.0e6, 1.0e6, 1.0]], np.float32))
            self._geom = ops.DeviceGeometry(self.robot, far, device)
        return self._geom

    def device_target(self, device):
        if self._target_dev is None or self._target_dev.device != torch.device(device):
            self._target_dev = self.target.to(device).contiguous()
        return self._target_dev

    def range_of(self, H):
        """[h_begin, h_end) on trajectories of H waypoints."""
        if self.traj_range == 'goal':
            return H - 1, H
        if self.traj_range == 'path':
            return 1, H
        return self.traj_range

    def _kernel_kw(self, trajs, k_sigma, kw):
        h0, h1 = self.range_of(trajs.shape[1])
        kw = dict(kw)
        kw.setdefault('h_begin', h0)
        kw.setdefault('h_end', h1)
        on = lambda k: k if (k_sigma is None or k == 0.0) else float(k_sigma)
        return dict(k_pos=on(self.k_pos), k_rot=on(self.k_rot), axis=self.axis, target_per_waypoint=self.target_per_waypoint, **kw)

    def own_eval(self, trajs, weight=1.0, k_sigma=None, **kw):
        """ops.ee_cost_eval of this member on (B, H, d) trajectories, in the collision members' contract: h_begin, per_waypoint, out,
        accumulate as that takes them (the range defaults to the member's); k_sigma replaces 1 / sigma^2 of every term that is on."""
        return ops.ee_cost_eval(trajs, self.device_geometry(trajs.device), self.device_target(trajs.device), weight=weight,
                                **self._kernel_kw(trajs, k_sigma, kw))

    def own_grad(self, trajs, weight=1.0, k_sigma=None, **kw):
        """ops.ee_cost_grad of this member: h_begin, out, grad, accumulate as that takes them."""
        return ops.ee_cost_grad(trajs, self.device_geometry(trajs.device), self.device_target(trajs.device), weight=weight,
                                **self._kernel_kw(trajs, k_sigma, kw))

    def eval(self, trajs, **observation):
        return self.own_eval(self._as_3d(trajs))

    def eval_with_grad(self, trajs, weight=1.0):
        """(cost (B,), d cost / d trajs (B, H, d))."""
        return self.own_grad(self._as_3d(trajs), weight=weight)

    def get_linear_system(self, trajs, **observation):
        """Dense (A, b, K) in the reference's convention: per waypoint of the range one block of rows at that waypoint's position
        columns -- three rows of the position term (A = J_v, b = e_p, K = I / sigma_pos^2), then three of the rotation term (full:
        A = J_w, b = e_w; axis: A = -[u]x J_w, b = u* - u; K = I / sigma_rot^2) -- so that A = -d b / d q and A^T K b is minus half the
        gradient.  For the full term the Jacobian of the rotation logarithm is dropped: J_r^{-T} e_w = e_w, the product stays exact.
        The slow inspection path, like every dense route: mpb_fk_ee_pose with its Jacobian, the error in torch."""
        trajs = self._as_3d(trajs)
        B, H, d = trajs.shape
        D = self.n_dof
        h0, h1 = self.range_of(H)
        n = h1 - h0
        kw = dict(device=trajs.device, dtype=trajs.dtype)
        q = trajs[:, h0:h1, :D].reshape(-1, D).to(torch.float32).contiguous()
        pose, J = ops.fk_ee_pose(q, self.device_geometry(trajs.device), with_jacobian=True)
        tgt = self.device_target(trajs.device)
        if self.num_goals == 1:
            tgt = tgt.unsqueeze(0)
        if B % self.num_goals != 0:
            raise ValueError(f'{self.num_goals} targets do not divide the batch of {B} trajectories')
        tgt = tgt.repeat_interleave(B // self.num_goals, 0)                                       # (B, [H,] 3, 4)
        tgt = (tgt[:, h0:h1] if self.target_per_waypoint else tgt.unsqueeze(1).expand(B, n, 3, 4)).reshape(-1, 3, 4).to(pose.dtype)
        R, t, Rs, ts = pose[:, :, :3], pose[:, :, 3], tgt[:, :, :3], tgt[:, :, 3]
        As, bs, ks = [], [], []
        if self.sigma_pos is not None:
            As.append(J[:, :3]); bs.append(ts - t); ks.append(self.k_pos)
        if self.sigma_rot is not None and self.axis is None:
            E = Rs @ R.transpose(1, 2)
            w = 0.5 * torch.stack([E[:, 2, 1] - E[:, 1, 2], E[:, 0, 2] - E[:, 2, 0], E[:, 1, 0] - E[:, 0, 1]], -1)
            c = 0.5 * (E[:, 0, 0] + E[:, 1, 1] + E[:, 2, 2] - 1.0)
            nw = w.norm(dim=-1)
            small = nw < 1e-6
            sc = torch.where(small, torch.ones_like(nw), torch.atan2(nw, c) / torch.where(small, torch.ones_like(nw), nw))
            As.append(J[:, 3:]); bs.append(sc[:, None] * w); ks.append(self.k_rot)
        elif self.sigma_rot is not None:
            a = torch.tensor(self.axis, device=trajs.device, dtype=pose.dtype)
            u, us = R @ a, Rs @ a
            As.append(-torch.linalg.cross(u[:, :, None].expand(-1, 3, D), J[:, 3:], dim=1)); bs.append(us - u); ks.append(self.k_rot)
        m = 3 * len(As)
        rows = torch.cat(As, 1).reshape(B, n, m, D).to(**kw)
        A = torch.zeros(B, n * m, self.dim * H if d == self.dim else d * H, **kw)
        for i in range(n):
            A[:, i * m:(i + 1) * m, (h0 + i) * d:(h0 + i) * d + D] = rows[:, i]
        b = torch.cat(bs, 1).reshape(B, n * m, 1).to(**kw)
        kd = torch.cat([torch.full((3,), k, **kw) for k in ks]).repeat(n)
        K = torch.diag(kd).repeat(B, 1, 1)
        return A, b, K


def _merge_term_specs(members):
    """Group (spec, weight) pairs into as few mpb_cost_terms_eval launches as possible: a member joins a
    group when none of its terms is already in it and the shared scalar dt agrees."""
    groups = []
    for spec, w in members:
        scaled = dict(spec)
        for k in ('k_gp', 'k_start', 'k_goal', 'k_smooth', 'k_jlim'):
            if k in scaled:
                scaled[k] = scaled[k] * w
        for g in groups:
            if g['terms'] & scaled['terms']:
                continue
            if 'dt' in g and 'dt' in scaled and g['dt'] != scaled['dt']:
                continue
            g.update({k: v for k, v in scaled.items() if k != 'terms'})
            g['terms'] = g['terms'] | scaled['terms']
            break
        else:
            scaled['terms'] = set(scaled['terms'])
            groups.append(scaled)
    return groups


class CostComposite(Cost):
    """Weighted sum of member costs (cost_functions.py:56-144)."""

    def __init__(self, robot, n_support_points, cost_list, weights_cost_l=None, **kwargs):
        super().__init__(robot, n_support_points, **kwargs)
        self.cost_l = cost_list
        self.weight_cost_l = weights_cost_l if weights_cost_l is not None else [1.0] * len(cost_list)

    def eval(self, trajs, trajs_interpolated=None, return_invidual_costs_and_weights=False, **kwargs):
        """cost_functions.py:70-105.  Collision members see `trajs_interpolated` when it is given (:77-84);
        all trajectory-only members are evaluated by ONE mpb_cost_terms_eval launch."""
        trajs = self._as_3d(trajs)
        trajs_coll = trajs if trajs_interpolated is None else self._as_3d(trajs_interpolated)
        if return_invidual_costs_and_weights:
            return [c(trajs_coll if isinstance(c, CostCollision) else trajs, **kwargs) for c in self.cost_l], \
                self.weight_cost_l
        total = None
        term_members = []
        for cost, w in zip(self.cost_l, self.weight_cost_l):
            if isinstance(cost, CostEEPose):              # (its range and per-waypoint targets are those of the support points)
                if torch.is_tensor(total) and total.ndim == 1 and total.is_contiguous() and total.dtype == torch.float32:
                    cost.own_eval(trajs, weight=w, out=total, accumulate=True)
                    continue
                c = cost.own_eval(trajs, weight=w)
            elif isinstance(cost, CostCollision):
                if cost.field is None:
                    continue
                if cost.own_kernels:
                    if torch.is_tensor(total) and total.ndim == 1 and total.is_contiguous() and total.dtype == torch.float32:
                        cost.own_eval(trajs_coll, weight=w, out=total, accumulate=True)
                        continue
                    c = cost.own_eval(trajs_coll, weight=w)
                else:
                    c = ops.cost_collision_eval(trajs_coll, cost.device_geometry(trajs.device), cost.k_sigma, weight=w)
            elif isinstance(cost, _TrajectoryTermCost):
                term_members.append((cost.term_spec(trajs.device), float(w)))
                continue
            else:
                c = w * cost(trajs, **kwargs)
            total = c if total is None else total + c
        for spec in _merge_term_specs(term_members):
            if total is None or not (torch.is_tensor(total) and total.ndim == 1 and total.is_contiguous()):
                extra, _ = ops.cost_terms_eval(trajs, self.n_dof, **spec)
                total = extra if total is None else total + extra
            else:
                ops.cost_terms_eval(trajs, self.n_dof, out=total, accumulate=True, **spec)
        return 0 if total is None else total

    def device_plan(self, device):
        """How a planner kernel pipeline can serve this composite without leaving the device:
        (collision members [(CostCollision, weight)], merged term specs, other members [(cost, weight)]).  Members with kernels
        of their own (self-collision, SDF grid, end-effector pose) are in none of the three: own_terms() lists them."""
        coll, terms, other = [], [], []
        for cost, w in zip(self.cost_l, self.weight_cost_l):
            if isinstance(cost, CostEEPose):
                continue
            if isinstance(cost, CostCollision):
                if cost.field is not None and not cost.own_kernels:
                    coll.append((cost, float(w)))
            elif isinstance(cost, _TrajectoryTermCost):
                terms.append((cost.term_spec(device), float(w)))
            else:
                other.append((cost, float(w)))
        return coll, _merge_term_specs(terms), other

    def get_linear_system(self, trajs, n_interpolated_points=None, **kwargs):
        """cost_functions.py:107-144: row-concatenated A, b and block-diagonal K of the members that have a linear
        system; `n_interpolated_points` reaches the collision members (their Jacobian is then the interpolated
        trajectory's, :112-119).  Like the reference, a member whose get_linear_system returns None (the
        reference's bare `pass`: CostGPTrajectory, CostSmoothnessCHOMP, CostJointLimits) raises TypeError at the
        unpack (:122-126); (None, None, None) members are skipped (:129-130).  Composite weights do not enter
        (the reference ignores weight_cost_l here)."""
        trajs = self._as_3d(trajs)
        As, bs, Ks = [], [], []
        for cost in self.cost_l:
            A, b, K = cost.get_linear_system(trajs, n_interpolated_points=n_interpolated_points, **kwargs)
            if A is None or b is None or K is None:
                continue
            As.append(A); bs.append(b); Ks.append(K)
        A, b = torch.cat(As, 1), torch.cat(bs, 1)
        K = torch.zeros(A.shape[0], A.shape[1], A.shape[1], device=A.device, dtype=A.dtype)
        o = 0
        for Kp in Ks:
            m = Kp.shape[1]
            K[:, o:o + m, o:o + m] = Kp
            o += m
        return A, b, K

    def collision_terms(self):
        """[(CostCollision, weight)] of the members that carry an OBSTACLE field."""
        return [(c, float(w)) for c, w in zip(self.cost_l, self.weight_cost_l)
                if isinstance(c, CostCollision) and c.field is not None and not c.own_kernels]

    def own_terms(self):
        """[(member, weight)] of the members with kernels of their own (a CostCollision over a SelfCollisionField or a GridSDFField, a
        CostEEPose), in composite order."""
        return [(c, float(w)) for c, w in zip(self.cost_l, self.weight_cost_l) if isinstance(c, (CostCollision, CostEEPose)) and c.own_kernels]

    def self_terms(self):
        """[(CostCollision, weight)] of the members whose field is a SelfCollisionField."""
        return [(c, float(w)) for c, w in zip(self.cost_l, self.weight_cost_l) if isinstance(c, CostCollision) and c.is_self]

    def single_collision_term(self):
        """(collision evaluator, weight) if this composite consists of collision fields only (1..4 of them) -- the
        case the planner kernels fuse; None otherwise."""
        terms = self.collision_terms()
        if not terms or len(terms) != len(self.cost_l):
            return None
        return merge_collision_terms(terms)


class MergedCollision:
    """Several CostCollision members (same robot) as ONE chained geometry buffer: the kernels evaluate
    weight * k_sigma * sum_f s_f cost_f with k_sigma, weight of the first member and
    s_f = (w_f k_f) / (w_0 k_0).  Quacks like CostCollision where the planners need it."""

    def __init__(self, terms):
        (c0, w0) = terms[0]
        assert all(c.robot is c0.robot for c, _ in terms), 'collision members must share the robot'
        assert not any(c.own_kernels for c, _ in terms), 'a self-collision or SDF-grid member has no obstacle field to chain'
        self.robot = c0.robot
        self.fields = [c.field for c, _ in terms]
        self.k_sigma = c0.k_sigma
        self.weight = w0
        self.scales = [(w * c.k_sigma) / (w0 * c0.k_sigma) for c, w in terms]
        self._geom = None

    def device_geometry(self, device):
        if self._geom is None or self._geom.buf.device != torch.device(device):
            self._geom = ops.DeviceGeometry(self.robot, self.fields, device, scales=self.scales)
        return self._geom


def merge_collision_terms(terms):
    """[(CostCollision, weight)] -> (evaluator with device_geometry / k_sigma, weight) or None (too many fields)."""
    if len(terms) == 1:
        return terms[0]
    if len(terms) > 4 or terms[0][1] == 0:
        return None
    m = MergedCollision(terms)
    return m, m.weight


def fusable_collision(cost):
    """Return (collision evaluator, weight) when `cost` is a collision cost the kernels can fuse, else None."""
    if isinstance(cost, CostCollision) and cost.field is not None:
        return None if cost.own_kernels else (cost, 1.0)   # (a self / SDF-grid member has its own kernels: never fused)
    if isinstance(cost, CostComposite):
        key = tuple((id(c), float(w)) for c, w in zip(cost.cost_l, cost.weight_cost_l))
        cached = cost.__dict__.get('_fused_cache')
        if cached is None or cached[0] != key:
            cost.__dict__['_fused_cache'] = (key, cost.single_collision_term())
        return cost.__dict__['_fused_cache'][1]
    return None


class DevicePlan(tuple):
    """(collision evaluator or None, its weight, merged trajectory-term specs) -- unpacks as those three -- plus `.own`, the
    members with kernels of their own [(member, weight)] (self-collision and SDF-grid fields, end-effector pose costs) that a planner serves with
    member.own_eval / member.own_grad accumulating onto the obstacle member's outputs; `.selfs` is the self-collision part of it."""

    def __new__(cls, cc, weight, groups, own=()):
        self = super().__new__(cls, (cc, weight, groups))
        self.own = list(own)
        self.selfs = [(c, w) for c, w in self.own if c.is_self]
        return self


def device_plan(cost, device):
    """DevicePlan (collision evaluator or None, its weight, merged trajectory-term specs; .selfs) when every member of `cost`
    is served by the HIP library (collision fields -- up to four, chained --, self-collision and SDF-grid fields, end-effector pose costs
    and trajectory-only terms): the case a planner can run as sample kernel -> own / term kernels -> update kernel with no host round trip; None otherwise."""
    if isinstance(cost, CostComposite):
        key = ('plan', str(device)) + tuple((id(c), float(w)) for c, w in zip(cost.cost_l, cost.weight_cost_l))
        cached = cost.__dict__.get('_plan_cache')
        if cached is not None and cached[0] == key:
            return cached[1]
        coll, groups, other = cost.device_plan(device)
        own = cost.own_terms()
        plan = None
        if not other and (coll or groups or own):
            merged = merge_collision_terms(coll) if coll else (None, 0.0)
            if merged is not None:
                plan = DevicePlan(merged[0], merged[1], groups, own)
        cost.__dict__['_plan_cache'] = (key, plan)
        return plan
    if isinstance(cost, CostCollision):
        if cost.field is None:
            return None
        return DevicePlan(None, 0.0, [], [(cost, 1.0)]) if cost.own_kernels else DevicePlan(cost, 1.0, [])
    if isinstance(cost, CostEEPose):
        return DevicePlan(None, 0.0, [], [(cost, 1.0)])
    if isinstance(cost, _TrajectoryTermCost):
        return DevicePlan(None, 0.0, _merge_term_specs([(cost.term_spec(device), 1.0)]))
    return None
