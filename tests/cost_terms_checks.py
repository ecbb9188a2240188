"""The trajectory cost terms of csrc/mpb_costs.hip, element by element, decided by the fp64 oracle alone (helper module; imported like
chomp_step_checks.py and collision_kinks.py).  Nothing here looks at the code under test.

The contract (file header of mpb_costs.hip): the fp32 inputs are widened, every sum is carried in fp64, an output is ONE fp32 rounding
of an fp64 value.  The reference is torch.autograd through oracle.planners_ref in fp64 on the same fp32 inputs; dt and jl_eps are passed
as the fp64 value of their fp32 rounding (DT, EPS), which is what the kernels widen.  The oracle builds CHOMP's R in torch's default
dtype, so cost_smoothness_chomp_eval runs under a fp64 default dtype here: 1 / dt^4 is then the fp64 value, not a product of fp32 ones.

The closed form (closed_form() restates it in fp64; x = position, v = velocity channel, i = joint, c = state column):

    GP        ep_h = x_{h+1} - (x_h + dt v_h),  ev_h = v_{h+1} - v_h                          (factor h, 0 <= h < H-1)
              a_h = 2 (q11 ep_h + q12 ev_h),  b_h = 2 (q12 ep_h + q22 ev_h),  q11 = 12/dt^3, q12 = -6/dt^2, q22 = 4/dt
              g[h, x_i] = k_gp (a_{h-1} - a_h),   g[h, v_i] = k_gp (b_{h-1} - (dt a_h + b_h))  (a term is absent where its factor is)
      VEL_FD  v_h = (x_{h+1} - x_{h-1}) / 2dt on interior rows, 0 on rows 0 and H-1;  V[h] = the g[h, v_i] above (0 on rows 0, H-1);
              g[h, x_i] += (V[h-1] - V[h+1]) / 2dt
    start     g[0, c]   = -2 k_start (s_c - x_{0,c})
    goal      g[H-1, c] = -2 k_goal (goal[b // trajs_per_goal]_c - x_{H-1,c})
    smooth    df_0 = x_0, df_h = x_h - x_{h-1};  g[h, c] = (k_smooth / dt^4) (2 df_h - 2 df_{h+1} [h < H-1] + 2 x_h [h = H-1])
    jlim      lo = q_min + eps - x, hi = x - (q_max - eps);  g[h, x_i] = jl_scale k_jlim (-2 lo [lo > 0] + 2 hi [hi > 0])

The unit of a gradient element is the sum of the absolute values of every product that enters it in this form: every difference above
replaced by the sum of its operands' absolute values (|v_h| under VEL_FD by (|x_{h+1}| + |x_{h-1}|) / 2dt), every sum of terms by the
sum of their units, the joint-limit sides counted where they are active.  The bar of an element:

    |g - g64|  <=  2^-24 |g64|  +  2^-44 unit  [ + 2^-24 (|V64[h-1]| + |V64[h+1]|) / 2dt under VEL_FD ]  [ + ulp32(grad_in) / 2 ]

2^-24 |g64| is the one fp32 rounding; 2^-44 unit covers the fp64 roundings of both sides (fewer than 2^9 operations each on operands
bounded by the unit; 2^-20 of an fp32 ulp of the unit, so it cannot hide an fp32-level error); the VEL_FD term is the kernel's fp32
LDS tile of V (V64: autograd with the virtual velocities as a leaf, rows 0 and H-1 zeroed).  An element whose unit is 0 has g64 = 0
and must come back as an exact zero (or with the bits of grad_in).  No element is left out: the joint-limit hinge is C1.

Costs: the same form per trajectory, unit[b] = the sum of |products| of the enabled terms without the joint limits, bar
2^-24 |c64| + 2^-44 unit; jl_total (fp64, atomics): |jl - jl64| <= 2^-44 k_jlim sum |violation|^2.
"""
import contextlib
import functools
import types

import numpy as np
import torch

F64 = dict(device='cpu', dtype=torch.float64)
DT = float(np.float32(0.04))                      # neither is representable in fp32: the kernels widen the rounded value
EPS = float(np.float32(np.deg2rad(3.0)))
TPG = 3                                           # trajectories per goal
SIGMA_START, SIGMA_GP = 0.1, 0.5                  # cost_gp_eval's parametrisation of k_start = 100, k_gp = 4
KW = dict(k_gp=4.0, k_start=100.0, k_goal=25.0, k_smooth=2.0 ** -17, k_jlim=3.0)          # exact in fp32
ALL = ('gp', 'start', 'goal', 'smooth', 'jlim')
SHARD = 3

# terms, VEL_FD, d / D
CONFIGS = {
    'gp': (('gp',), False, 2), 'start': (('start',), False, 2), 'goal': (('goal',), False, 2), 'smooth': (('smooth',), False, 2),
    'jlim': (('jlim',), False, 2), 'all': (ALL, False, 2),
    'gp-fd': (('gp',), True, 1), 'gp+smooth+jlim-fd': (('gp', 'smooth', 'jlim'), True, 1),
    'smooth-pos': (('smooth',), False, 1), 'jlim-pos': (('jlim',), False, 1),        # CHOMP._eval passes position-only trajectories
}
# (B, H, D): B = 21 leaves the last block of four waves ragged; B = 5 with G = 2 crosses a goal inside one block
CASES = ([(21, H, 7) for H in (2, 3, 64, 65, 129, 256)] + [(21, H, D) for D in (1, 12) for H in (3, 65)]
         + [(5, 3, 7), (5, 65, 7), (1, 2, 7), (1, 65, 7)])


def case_id(c):
    return 'B%d-H%d-D%d' % c


@contextlib.contextmanager
def _default_fp64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def ulp32(t):
    """Spacing of fp32 at |t| (fp64 tensor)."""
    t32 = t.float().abs()
    return (torch.nextafter(t32, torch.full_like(t32, float('inf'))) - t32).double()


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
class Problem:
    """x (B, H, 2D) fp32, start (2D,), goals (G, 2D), q_min / q_max (D,), all fp32 and read-only; hashed by identity."""

    def __init__(self, x, D, q_min, q_max, gen):
        self.B, self.H, self.D = x.shape[0], x.shape[1], D
        self.x, self.q_min, self.q_max = x.contiguous(), q_min.contiguous(), q_max.contiguous()
        self.G = (self.B + TPG - 1) // TPG
        self.start = (x[0, 0] + 0.01 * torch.randn(2 * D, generator=gen)).contiguous()
        self.goals = torch.stack([x[min(TPG * g, self.B - 1), -1] + 0.01 * torch.randn(2 * D, generator=gen)
                                  for g in range(self.G)]).contiguous()

    def trajs(self, dmul):
        return self.x if dmul == 2 else self.x[..., :self.D].contiguous()

    def spec(self, terms, fd, dev='cpu'):
        """The keyword arguments of ops.cost_terms_eval / cost_terms_grad for these terms."""
        return dict(terms=set(terms), vel_fd=fd, dt=DT, jl_eps=EPS, trajs_per_goal=TPG, start_state=self.start.to(dev),
                    goal_states=self.goals.to(dev), q_min=self.q_min.to(dev), q_max=self.q_max.to(dev), **KW)


def pushed_rows(H):
    """The waypoints on which joints leave both limits: row 0, row H-1, the middle, and the first row of a lane's second trip."""
    return sorted({0, H - 1, H // 2} | ({64} if H > 64 else set()))


@functools.lru_cache(maxsize=None)
def problem(B, H, D):
    """Straight lines plus noise, with stored velocities; finite limits; joints pushed beyond both limits on pushed_rows(H)."""
    gen = torch.Generator().manual_seed(100000 * B + 100 * H + D)
    q0, q1 = 3.0 * torch.rand(B, 1, D, generator=gen) - 1.5, 3.0 * torch.rand(B, 1, D, generator=gen) - 1.5
    s = torch.linspace(0.0, 1.0, H).reshape(1, H, 1)
    pos = q0 + s * (q1 - q0) + 0.05 * torch.randn(B, H, D, generator=gen)
    vel = ((q1 - q0) / ((H - 1) * DT)).expand(B, H, D) + 0.05 * torch.randn(B, H, D, generator=gen)
    j = torch.arange(D, dtype=torch.float32)
    q_min, q_max = -2.0 - 0.01 * j, 2.0 + 0.013 * j
    for r in pushed_rows(H):
        for b in range(B):
            up, low = (r + b) % D, (r + b + 1) % D
            if D > 1 or (r + b) % 2 == 0:
                pos[b, r, up] = q_max[up] + 0.05 + 0.01 * b
            if D > 1 or (r + b) % 2 == 1:
                pos[b, r, low] = q_min[low] - 0.02 - 0.01 * b
    return Problem(torch.cat((pos, vel), -1).float(), D, q_min, q_max, gen)


@functools.lru_cache(maxsize=None)
def step_problem(H):
    """The composite route's trajectories (chomp_step_checks.trajs of its scene) with limits that leave 5 % of every joint's
    values outside on either side."""
    import chomp_step_checks as C
    import collision_kinks as K
    x = C.trajs(C.COMPOSITE_SCENE, H, 2 * C.base(C.COMPOSITE_SCENE, H).robot.q_dim)
    D = x.shape[-1] // 2
    flat = x[..., :D].reshape(-1, D).double()
    q_min, q_max = torch.quantile(flat, 0.05, dim=0).float(), torch.quantile(flat, 0.95, dim=0).float()
    assert x.shape[0] == K.B
    return Problem(x, D, q_min, q_max, torch.Generator().manual_seed(H))


# ------------------------------------------------------------------------------------------------
# the reference: autograd through the oracle, fp64
# ------------------------------------------------------------------------------------------------
def oracle_costs(p, terms, fd, x, goal_index=None):
    """(per-trajectory cost of the enabled terms without the joint limits (B,), joint-limit scalar or None); x fp64 (B, H, d)."""
    from oracle import planners_ref as O
    D, terms = p.D, set(terms)
    c = torch.zeros(p.B, dtype=torch.float64)
    if 'gp' in terms and fd:
        c = c + KW['k_gp'] * O.cost_gp_trajectory_pos_only_eval(x, D, DT, 1.0, F64)
    elif 'gp' in terms and 'start' in terms:
        c = c + O.cost_gp_eval(x, p.start.double(), D, DT, SIGMA_START, SIGMA_GP, F64)
    elif 'gp' in terms:
        c = c + KW['k_gp'] * O.cost_gp_trajectory_eval(x, D, DT, 1.0, F64)
    elif 'start' in terms:
        c = c + KW['k_start'] * ((p.start.double() - x[:, 0]) ** 2).sum(-1)
    if 'goal' in terms:
        c = c + KW['k_goal'] * O.cost_goal_prior_multi_eval(x, p.goals.double(), TPG, 1.0)
    if 'smooth' in terms:
        with _default_fp64():
            c = c + KW['k_smooth'] * O.cost_smoothness_chomp_eval(x, DT, F64)[0]
    jl = None
    if 'jlim' in terms:
        jl = KW['k_jlim'] * O.cost_joint_limits_eval(x, D, p.q_min.double(), p.q_max.double(), EPS)
    return c, jl


def _virtual_velocity_grad(p, pos):
    """V64: d cost_gp / d v with the central-difference velocities as a leaf; rows 0 and H-1 (at rest, not pulled back) zeroed."""
    from oracle import planners_ref as O
    v = O.finite_difference_central(pos, DT).clone().requires_grad_(True)
    cost = KW['k_gp'] * O.cost_gp_trajectory_eval(torch.cat((pos, v), -1), p.D, DT, 1.0, F64)
    V, = torch.autograd.grad(cost.sum(), v)
    V[:, 0] = 0.0
    V[:, -1] = 0.0
    return V


def closed_form(p, terms, fd, dmul, jl_scale, fault=None):
    """The module docstring's closed form in fp64 -> (g (B, H, d), unit (B, H, d)).  fault: None, or one planted error of the
    sensitivity check: 'pull_self' (the pull-back from V[h] instead of V[h -+ 1]), 'no_last_smooth' (the h = H-1 smoothness term
    dropped), 'goal_mod' (goal index b % trajs_per_goal)."""
    D, H, B, terms = p.D, p.H, p.B, set(terms)
    x = p.trajs(dmul).double()
    ax = x.abs()
    g, unit = torch.zeros_like(x), torch.zeros_like(x)
    pos, apos = x[..., :D], ax[..., :D]
    inv_2dt = 1.0 / (2.0 * DT)
    if 'gp' in terms:
        q11, q12, q22 = 12.0 / DT ** 3, -6.0 / DT ** 2, 4.0 / DT
        if fd:
            v, av = torch.zeros_like(pos), torch.zeros_like(pos)
            v[:, 1:-1] = (pos[:, 2:] - pos[:, :-2]) * inv_2dt
            av[:, 1:-1] = (apos[:, 2:] + apos[:, :-2]) * inv_2dt
        else:
            v, av = x[..., D:], ax[..., D:]
        ep, ev = pos[:, 1:] - (pos[:, :-1] + DT * v[:, :-1]), v[:, 1:] - v[:, :-1]
        EP, EV = apos[:, 1:] + apos[:, :-1] + DT * av[:, :-1], av[:, 1:] + av[:, :-1]
        a, b = 2.0 * (q11 * ep + q12 * ev), 2.0 * (q12 * ep + q22 * ev)
        A, Bb = 2.0 * (q11 * EP + abs(q12) * EV), 2.0 * (abs(q12) * EP + q22 * EV)
        gp, up, gv, uv = torch.zeros_like(pos), torch.zeros_like(pos), torch.zeros_like(pos), torch.zeros_like(pos)
        gp[:, :-1] -= a
        gp[:, 1:] += a
        up[:, :-1] += A
        up[:, 1:] += A
        gv[:, :-1] -= DT * a + b
        gv[:, 1:] += b
        uv[:, :-1] += DT * A + Bb
        uv[:, 1:] += Bb
        k = KW['k_gp']
        g[..., :D] += k * gp
        unit[..., :D] += k * up
        if fd:
            V, UV = k * gv, k * uv
            if H > 2:
                if fault == 'pull_self':          # V[h] where V[h-1] (h >= 2) and V[h+1] (h <= H-3) belong
                    g[:, 2:, :D] += V[:, 2:] * inv_2dt
                    g[:, :-2, :D] -= V[:, :-2] * inv_2dt
                else:
                    g[:, 2:, :D] += V[:, 1:-1] * inv_2dt
                    g[:, :-2, :D] -= V[:, 1:-1] * inv_2dt
                unit[:, 2:, :D] += UV[:, 1:-1] * inv_2dt
                unit[:, :-2, :D] += UV[:, 1:-1] * inv_2dt
        else:
            g[..., D:] += k * gv
            unit[..., D:] += k * uv
    if 'start' in terms:
        s = p.start.double()
        g[:, 0] -= 2.0 * KW['k_start'] * (s - x[:, 0])
        unit[:, 0] += 2.0 * KW['k_start'] * (s.abs() + ax[:, 0])
    if 'goal' in terms:
        idx = (torch.arange(B) % TPG).clamp(max=p.G - 1) if fault == 'goal_mod' else torch.arange(B) // TPG
        gl = p.goals.double()[idx]
        g[:, -1] -= 2.0 * KW['k_goal'] * (gl - x[:, -1])
        unit[:, -1] += 2.0 * KW['k_goal'] * (gl.abs() + ax[:, -1])
    if 'smooth' in terms:
        k = KW['k_smooth'] / DT ** 4
        df, adf = x.clone(), ax.clone()
        df[:, 1:] -= x[:, :-1]
        adf[:, 1:] += ax[:, :-1]
        gs, us = 2.0 * df, 2.0 * adf
        gs[:, :-1] -= 2.0 * df[:, 1:]
        us[:, :-1] += 2.0 * adf[:, 1:]
        if fault != 'no_last_smooth':
            gs[:, -1] += 2.0 * x[:, -1]
        us[:, -1] += 2.0 * ax[:, -1]
        g += k * gs
        unit += k * us
    if 'jlim' in terms:
        k = jl_scale * KW['k_jlim']
        qmin, qmax = p.q_min.double(), p.q_max.double()
        lo, hi = qmin + EPS - pos, pos - (qmax - EPS)
        g[..., :D] += k * (-2.0 * lo * (lo > 0) + 2.0 * hi * (hi > 0))
        unit[..., :D] += k * 2.0 * ((qmin.abs() + EPS + apos) * (lo > 0) + (apos + qmax.abs() + EPS) * (hi > 0))
    return g, unit


def cost_unit(p, terms, fd, dmul):
    """Per-trajectory sum of the absolute values of every product of the enabled terms' costs (without the joint limits), (B,)."""
    D, terms = p.D, set(terms)
    ax = p.trajs(dmul).double().abs()
    apos = ax[..., :D]
    u = torch.zeros(p.B, dtype=torch.float64)
    if 'gp' in terms:
        q11, q12, q22 = 12.0 / DT ** 3, 6.0 / DT ** 2, 4.0 / DT
        if fd:
            av = torch.zeros_like(apos)
            av[:, 1:-1] = (apos[:, 2:] + apos[:, :-2]) / (2.0 * DT)
        else:
            av = ax[..., D:]
        EP, EV = apos[:, 1:] + apos[:, :-1] + DT * av[:, :-1], av[:, 1:] + av[:, :-1]
        u += KW['k_gp'] * (q11 * EP * EP + 2.0 * q12 * EP * EV + q22 * EV * EV).sum((1, 2))
    if 'start' in terms:
        u += KW['k_start'] * ((p.start.double().abs() + ax[:, 0]) ** 2).sum(-1)
    if 'goal' in terms:
        u += KW['k_goal'] * ((p.goals.double()[torch.arange(p.B) // TPG].abs() + ax[:, -1]) ** 2).sum(-1)
    if 'smooth' in terms:
        adf = ax.clone()
        adf[:, 1:] += ax[:, :-1]
        u += KW['k_smooth'] / DT ** 4 * ((adf ** 2).sum((1, 2)) + (ax[:, -1] ** 2).sum(-1))
    return u


@functools.lru_cache(maxsize=None)
def reference(p, config, jl_mul=1):
    """Computed once per (problem, configuration, joint-limit scale = jl_mul * B) and shared; treat as read-only."""
    terms, fd, dmul = CONFIGS[config] if isinstance(config, str) else config
    jl_scale = float(jl_mul * p.B)
    x = p.trajs(dmul).double().clone().requires_grad_(True)
    c, jl = oracle_costs(p, terms, fd, x)
    total = c.sum() + (jl_scale * jl if jl is not None else 0.0)
    g64, = torch.autograd.grad(total, x)
    gc, unit = closed_form(p, terms, fd, dmul, jl_scale)
    ns = types.SimpleNamespace(p=p, terms=terms, fd=fd, dmul=dmul, d=dmul * p.D, jl_scale=jl_scale, x=p.trajs(dmul), g64=g64.detach(),
                               g_closed=gc, unit=unit, zero=unit == 0, c64=c.detach(), cost_unit=cost_unit(p, terms, fd, dmul),
                               jl64=None if jl is None else float(jl.detach()), vterm=torch.zeros_like(unit), V64=None)
    if jl is not None:
        ns.jl_bar = 2.0 ** -44 * ns.jl64                      # jl64 = k_jlim * sum |violation|^2: every product is positive
    if fd:
        ns.V64 = _virtual_velocity_grad(p, x.detach())
        nb = torch.zeros_like(ns.V64)
        nb[:, 1:] += ns.V64[:, :-1].abs()
        nb[:, :-1] += ns.V64[:, 1:].abs()
        ns.vterm = 2.0 ** -24 * nb / (2.0 * DT)
    return ns


def grad_bar(ref, grad_in=None):
    """(want, bar) per element, fp64; grad_in fp32 or None."""
    want = ref.g64 if grad_in is None else ref.g64 + grad_in.double()
    bar = 2.0 ** -24 * want.abs() + 2.0 ** -44 * ref.unit + ref.vterm
    if grad_in is not None:
        bar = bar + 0.5 * ulp32(grad_in.double())
    return want, bar


def ratio(got, want, bar):
    """|got - want| / bar where the bar is positive; where it is 0 the caller compares bits."""
    pos = bar > 0
    return ((got.double() - want).abs() / torch.where(pos, bar, torch.ones_like(bar))) * pos


def grad_in_for(ref, seed=0):
    """A random incoming gradient at the scale of the median non-zero |g64|."""
    nz = ref.g64.abs()[ref.g64 != 0]
    scale = float(nz.median()) if nz.numel() else 1.0
    gen = torch.Generator().manual_seed(7 + seed)
    return (scale * torch.randn(ref.g64.shape, generator=gen)).float().contiguous()


def cost_bar(ref):
    return 2.0 ** -24 * ref.c64.abs() + 2.0 ** -44 * ref.cost_unit
