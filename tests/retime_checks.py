"""The definition of mpb_traj_retime / mpb_traj_retime_sample (include/mpb.h) restated in numpy, once, with a dtype
argument: restate(inp, np.float64) is the oracle, restate(inp, np.float32) the yardstick whose own distance from the oracle sets the
bar a kernel is held to (collision_kinks.bar).  Helper module, no device: imported like path_shortcut_checks.py.  Every operation is
rounded to `dtype` (numpy never contracts), in the order the header gives."""
import functools
import types

import numpy as np

OK, STALLED, TOO_LONG = 0, 1, 2
N_TRAJ = 37                                                        # not a multiple of anything
SDOT_MAX, T_MAX = 1e3, 1e4                                         # the defaults of ops.traj_retime
PANDA_V = np.array([2.175] * 4 + [2.61] * 3)                       # Franka's data sheet: rad/s, rad/s^2
PANDA_A = np.array([15.0, 7.5, 10.0, 12.5, 15.0, 20.0, 20.0])
DUPLICATES = np.array([0, 0, 0, 1, 1, 1, 2, 2], np.float64)       # the stop-and-go path of the definition: STALLED


# ---- the definition -----------------------------------------------------------------------------------------------------------------
def path_derivatives(q):
    """q (N, H, D) -> p, c (N, H, D): central differences inside, one-sided p and c = 0 at the two ends."""
    half = q.dtype.type(0.5)
    p, c = np.empty_like(q), np.zeros_like(q)
    p[:, 1:-1] = (q[:, 2:] - q[:, :-2]) * half
    c[:, 1:-1] = (q[:, 2:] - q[:, 1:-1]) - (q[:, 1:-1] - q[:, :-2])
    p[:, 0] = q[:, 1] - q[:, 0]
    p[:, -1] = q[:, -1] - q[:, -2]
    return p, c


def interval_lines(p, c, a_max, beta_next, i):
    """The 2D + 1 line pairs of interval i, each (a, b, c+, c-): the lines a u + b x <= c+ and -a u - b x <= c-.  Pairs 0 .. D-1: the
    acceleration limit at waypoint i; D .. 2D-1: at waypoint i + 1 in terms of x_i; 2D: 0 <= x_i + 2u <= beta_{i+1}."""
    N, _, D = p.shape
    ty = p.dtype.type
    one = np.ones((N, 1), p.dtype)
    A = np.broadcast_to(a_max, (N, D))
    a = np.concatenate([p[:, i], p[:, i + 1] + ty(2) * c[:, i + 1], ty(2) * one], 1)
    b = np.concatenate([c[:, i], c[:, i + 1], one], 1)
    cp = np.concatenate([A, A, beta_next[:, None]], 1)
    cn = np.concatenate([A, A, 0 * one], 1)
    return a, b, cp, cn


def upper_lower(a, b, cp, cn):
    """Of every line pair the line that bounds u from above (a1 > 0) and the one that bounds it from below (a2 < 0), picked by the sign
    of a; `has`: a != 0."""
    s = a > 0
    upper = (np.abs(a), np.where(s, b, -b), np.where(s, cp, cn))
    lower = (-np.abs(a), np.where(s, -b, b), np.where(s, cn, cp))
    return upper, lower, a != 0


def speed_limit(p_i, v_max, sdot_max):
    """xv_i = min(sdot_max, min_j v_j / |p_ij| over p_ij != 0)^2."""
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        r = np.where(p_i != 0, v_max / np.abs(p_i), np.inf).astype(p_i.dtype)
    m = np.minimum(p_i.dtype.type(sdot_max), r.min(1))
    return m * m


def controllable(p, c, a_max, xv_i, beta_next, i):
    """beta_i: the largest x_i from which some u keeps every line of interval i (Fourier-Motzkin over upper x lower pairs)."""
    a, b, cp, cn = interval_lines(p, c, a_max, beta_next, i)
    (a1, b1, c1), (a2, b2, c2), has = upper_lower(a, b, cp, cn)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        only_x = (a == 0) & (b != 0)
        best = np.minimum(xv_i, np.where(only_x, cp / np.where(only_x, np.abs(b), 1), np.inf).min(1))
        k = a1[:, :, None] * b2[:, None, :] - a2[:, None, :] * b1[:, :, None]
        num = a1[:, :, None] * c2[:, None, :] - a2[:, None, :] * c1[:, :, None]
        ok = has[:, :, None] & has[:, None, :] & (k > 0)
        cand = np.where(ok, num / np.where(ok, k, 1), np.inf)
    return np.minimum(best, cand.reshape(len(a), -1).min(1)).astype(p.dtype)


def restate(inp, dtype):
    """The whole definition in `dtype`: beta, x, t (N, H), u (N, H-1), qd (N, H, D), status (N,), duration (N,)."""
    ty = np.dtype(dtype).type
    q = np.ascontiguousarray(inp.trajs[:, :, :inp.D]).astype(dtype)
    v_max, a_max = inp.v_max.astype(dtype), inp.a_max.astype(dtype)
    N, H, D = q.shape
    p, c = path_derivatives(q)
    beta = np.zeros((N, H), dtype)
    xv = np.stack([speed_limit(p[:, i], v_max, ty(inp.sdot_max)) for i in range(H)], 1)
    for i in range(H - 2, 0, -1):
        beta[:, i] = controllable(p, c, a_max, xv[:, i], beta[:, i + 1], i)
    x, u = np.zeros((N, H), dtype), np.zeros((N, H - 1), dtype)
    for i in range(H - 1):
        a, b, cp, cn = interval_lines(p, c, a_max, beta[:, i + 1], i)
        (a1, b1, c1), _, has = upper_lower(a, b, cp, cn)
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            u[:, i] = np.where(has, (c1 - b1 * x[:, i, None]) / np.where(has, a1, 1), np.inf).min(1)
        x[:, i + 1] = np.maximum(ty(0), np.minimum(beta[:, i + 1], x[:, i] + ty(2) * u[:, i]))
    r = np.sqrt(x)
    t = np.zeros((N, H), dtype)
    with np.errstate(divide='ignore'):
        for i in range(H - 1):
            t[:, i + 1] = t[:, i] + ty(2) / (r[:, i] + r[:, i + 1])
    T = t[:, -1]
    bad_limit = not (np.all(v_max > 0) and np.all(a_max > 0) and np.all(np.isfinite(v_max)) and np.all(np.isfinite(a_max)))
    status = np.where(np.isfinite(T) & (T <= ty(inp.t_max)) & (not bad_limit), OK, STALLED).astype(np.int32)
    return types.SimpleNamespace(beta=beta, x=x, u=u, t=t, qd=p * r[:, :, None], status=status, duration=T, p=p, c=c, xv=xv)


def sample(inp, x, u, t, status, dt, T_rows, dtype):
    """The sampler in `dtype`, fed x, u, t as given (the kernel's own fp32 bits in the tests): out (N, T_rows, 2D), n_rows, status."""
    ty = np.dtype(dtype).type
    q = np.ascontiguousarray(inp.trajs[:, :, :inp.D]).astype(dtype)
    N, H, D = q.shape
    p, _ = path_derivatives(q)
    x, u, t = x.astype(dtype), u.astype(dtype), t.astype(dtype)
    out = np.zeros((N, T_rows, 2 * D), dtype)
    n_rows, st = np.zeros(N, np.int64), np.zeros(N, np.int32)
    dt = ty(np.float32(dt))
    tau = np.arange(T_rows).astype(dtype) * dt
    for n in range(N):
        T = t[n, -1]
        if status[n] != OK or not np.isfinite(T):
            st[n] = STALLED
            out[n, :, :D] = q[n, 0]
            continue
        n_rows[n] = int(np.ceil(float(np.float32(T)) / float(dt))) + 1
        st[n] = TOO_LONG if n_rows[n] > T_rows else OK
        i = np.clip(np.searchsorted(t[n], tau, side='right') - 1, 0, H - 2)
        d = tau - t[n, i]
        r = np.sqrt(x[n, i])
        sig = np.clip(r * d + ((u[n, i] * d) * d) * ty(0.5), ty(0), ty(1))[:, None]
        sdot = np.maximum(ty(0), r + u[n, i] * d)[:, None]
        q0, q1, p0, p1 = q[n, i], q[n, i + 1], p[n, i], p[n, i + 1]
        dq = q1 - q0
        e2 = (ty(3) * dq - ty(2) * p0) - p1
        e3 = (p0 + p1) - ty(2) * dq
        pos = q0 + sig * (p0 + sig * (e2 + sig * e3))
        vel = (p0 + sig * (ty(2) * e2 + (ty(3) * sig) * e3)) * sdot
        past = (tau >= T)[:, None]
        out[n, :, :D] = np.where(past, q[n, -1], pos)
        out[n, :, D:] = np.where(past, ty(0), vel)
    return out, n_rows, st


# ---- what the limits say of a timing, independently of the passes above ----------------------------------------------------------
def overstep(inp, x, u):
    """From any x (N, H), u (N, H-1), in fp64: (velocity, acceleration) overstep of the limits at the waypoints -- the acceleration
    at BOTH ends of every interval -- each in units of 2^-23 (|p u| + |c x| + limit), the rounding scale of one evaluated line."""
    q = inp.trajs[:, :, :inp.D].astype(np.float64)
    p, c = path_derivatives(q)
    x, u = x.astype(np.float64), u.astype(np.float64)
    v, a = inp.v_max.astype(np.float64), inp.a_max.astype(np.float64)
    ulp = 2.0 ** -23
    vel = np.abs(p) * np.sqrt(x)[:, :, None]
    over_v = ((vel - v) / (ulp * (vel + v))).max()
    worst = -np.inf
    for pe, ce, xe in ((p[:, :-1], c[:, :-1], x[:, :-1]), (p[:, 1:], c[:, 1:], x[:, 1:])):
        pu, cx = pe * u[:, :, None], ce * xe[:, :, None]
        worst = max(worst, ((np.abs(pu + cx) - a) / (ulp * (np.abs(pu) + np.abs(cx) + a))).max())
    return float(over_v), float(worst)


def time_bar(x64, bar_x, t64, H):
    """First-order propagation of |dx| <= bar_x through t_{i+1} = t_i + 2 / (sqrt(x_i) + sqrt(x_{i+1})), summed, plus 4 H 2^-23 t for the
    fp32 sqrt, add, divide and running sum: d(2 / s) = 2 ds / s^2, ds <= bar_x / (2 sqrt x_i) + bar_x / (2 sqrt x_{i+1}); where an x is
    within bar_x of 0 its root moves by at most sqrt(bar_x)."""
    r = np.sqrt(x64)
    with np.errstate(divide='ignore'):
        dr = np.minimum(bar_x / (2 * r), np.sqrt(bar_x))
    s = r[:, :-1] + r[:, 1:]
    ds = np.minimum(dr[:, :-1] + dr[:, 1:], 0.5 * s)               # (first order: the sum of roots is taken to move by at most half)
    dstep = 2 * ds / (s * (s - ds))
    return np.concatenate([np.zeros((len(x64), 1)), np.cumsum(dstep, 1)], 1) + 4 * H * 2.0 ** -23 * t64


# ---- the input sets ---------------------------------------------------------------------------------------------------------------
def _inputs(trajs, D, v_max, a_max, sdot_max=SDOT_MAX, t_max=T_MAX):
    return types.SimpleNamespace(trajs=np.ascontiguousarray(trajs, np.float32), D=D, N=trajs.shape[0], H=trajs.shape[1], W=trajs.shape[2],
                                 v_max=np.asarray(v_max, np.float32), a_max=np.asarray(a_max, np.float32), sdot_max=sdot_max, t_max=t_max)


def smooth(rng, N, H, D):
    """A straight line between two random configurations plus four sine harmonics of amplitude 0.3 / k."""
    s = np.linspace(0.0, 1.0, H)[None, :, None]
    q0, q1 = rng.uniform(-1.5, 1.5, (N, 1, D)), rng.uniform(-1.5, 1.5, (N, 1, D))
    q = q0 + (q1 - q0) * s
    for k in range(1, 5):
        q = q + (0.3 / k) * rng.uniform(-1.0, 1.0, (N, 1, D)) * np.sin(k * np.pi * s)
    return q


def polylines(rng, N, H, D, knots=4):
    """Piecewise-linear paths through `knots` random configurations, resampled to H waypoints evenly in the knot parameter: corners."""
    K = rng.uniform(-1.5, 1.5, (N, knots, D))
    s = np.linspace(0.0, knots - 1.0, H)
    j = np.minimum(s.astype(int), knots - 2)
    w = (s - j)[None, :, None]
    return K[:, j] * (1.0 - w) + K[:, j + 1] * w


def _padded(q, W, rng):
    """(N, H, D) -> (N, H, W): the columns past D hold what a planner's velocity half might, never read."""
    return np.concatenate([q, rng.normal(0.0, 5.0, q.shape[:2] + (W - q.shape[2],))], 2)


SETS = ('panda_h64_w2d', 'panda_h65', 'panda_h16', 'panda_h3', 'panda_h256', 'dof12_h33', 'dof2_h4', 'panda_polyline_h64')


@functools.lru_cache(maxsize=None)
def inputs(name):
    rng = np.random.RandomState(SETS.index(name) + 1234)
    if name == 'panda_h64_w2d':
        return _inputs(_padded(smooth(rng, N_TRAJ, 64, 7), 14, rng), 7, PANDA_V, PANDA_A)
    if name.startswith('panda_h'):
        return _inputs(smooth(rng, N_TRAJ, int(name[7:]), 7), 7, PANDA_V, PANDA_A)
    if name == 'dof12_h33':                                        # 25 line pairs: 625 ordered pairs, ten trips of 64
        return _inputs(smooth(rng, N_TRAJ, 33, 12), 12, rng.uniform(1.0, 3.0, 12), rng.uniform(5.0, 20.0, 12))
    if name == 'dof2_h4':
        return _inputs(smooth(rng, N_TRAJ, 4, 2), 2, [1.0, 1.5], [2.0, 3.0])
    if name == 'panda_polyline_h64':
        return _inputs(polylines(rng, N_TRAJ, 64, 7), 7, PANDA_V, PANDA_A)
    raise KeyError(name)


def duplicates():
    """The duplicate-waypoint path of the definition in one joint: the finite differences of a stop-and-go path force a stop."""
    return _inputs(DUPLICATES[None, :, None], 1, [1.0], [1.0])


@functools.lru_cache(maxsize=None)
def reference(name):
    """(inputs, restate fp64, restate fp32) of a set, computed once and shared by the tests; nobody writes into it."""
    inp = inputs(name)
    return inp, restate(inp, np.float64), restate(inp, np.float32)
