"""The definition of mpb_path_blend / mpb_path_blend_sample (include/mpb.h) restated in numpy, once, with a dtype argument:
restate(inp, np.float64) is the oracle, restate(inp, np.float32) the yardstick the kernel is held to bit for bit (every operation is
rounded to `dtype` on its own, numpy never contracts, in the order the header gives).  Helper module, no device: imported like
retime_checks.py.  It also holds the input sets of tests/test_path_blend_cpu.py and tests/test_gpu_path_blend.py.

    python tests/path_blend_checks.py     # measures E32 (restate fp32 against fp64, per set, relative to the largest value) and the
                                          # overstep of the limits restate(fp32) shows, in units of 2^-23: what DESIGN.md 10 records
"""
import functools
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from motion_planning_baselines_amd import blend_layout as BL          # noqa: E402
from motion_planning_baselines_amd import certify_layout as CL        # noqa: E402

OK, NOT_CONVERGED, DEGENERATE_SEGMENT, BAD_INPUT, TOO_LONG = range(len(BL.STATUS))
MAX_SWEEPS = BL.BLEND_DEFAULT_MAX_SWEEPS
N_PATHS = 37                                                       # not a multiple of anything
MAX_H = 256                                                        # MPB_MAX_H
PANDA_V = np.array([2.175] * 4 + [2.61] * 3)                       # Franka's data sheet: rad/s, rad/s^2
PANDA_A = np.array([15.0, 7.5, 10.0, 12.5, 15.0, 20.0, 20.0])
DELTAS = (np.inf, 0.05, 0.01)
# measured 2026-10-21 by `python tests/path_blend_checks.py` over SETS x DELTAS (DESIGN.md 10 records them): the largest distance of
# restate(fp32) from restate(fp64) per output, relative to the output's largest value, and the largest overstep of a limit that
# restate(fp32) shows in fp64 arithmetic, in units of 2^-23 relative to the limit (velocity 0.66, acceleration 2.22, deviation 0.74)
E32_MEASURED = {'T': 1.36e-07, 'tb': 2.87e-07, 'tw': 3.66e-07, 'dev': 3.95e-07, 'duration': 2.25e-07}        # (rounded up)
OVERSTEP_MEASURED = 2.22
B_LIMIT = 4.0 * OVERSTEP_MEASURED * 2.0 ** -23                     # the b of the kernel's guarantee checks: four times that overstep


# ---- the definition -----------------------------------------------------------------------------------------------------------------
def _one(q, v_max, a_max, delta, max_sweeps, dtype):
    """One path q (L, D) of finite rows, L >= 2, in `dtype`: (status, first_bad, sweeps, T (L-1), tb (L), tw (L), dev (L), duration)."""
    ty = np.dtype(dtype).type
    L, D = q.shape
    dq = q[1:] - q[:-1]
    adq = np.abs(dq)
    zero = np.zeros(L, dtype)
    if np.any(adq.max(1) == 0):
        return DEGENERATE_SEGMENT, int(np.argmax(adq.max(1) == 0)), 0, zero[1:], zero, zero, zero, ty(0)
    T = (adq / v_max).max(1)
    row0 = np.zeros((1, D), dtype)
    inf = ty(np.inf)
    eight_delta = ty(8) * ty(delta)
    sweeps = 0
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        while True:
            v = dq / T[:, None]
            dv = np.concatenate([v, row0]) - np.concatenate([row0, v])
            adv = np.abs(dv)
            tb = (adv / a_max).max(1)
            mdv = adv.max(1)
            cap = np.where((mdv != 0) & np.isfinite(ty(delta)), eight_delta / np.where(mdv != 0, mdv, ty(1)), inf).astype(dtype)
            m = np.minimum(np.minimum(np.concatenate([[inf], T]), np.concatenate([T, [inf]])), cap).astype(dtype)
            viol = tb > m
            if not viol.any():
                break
            if sweeps == max_sweeps:
                return NOT_CONVERGED, -1, sweeps, zero[1:], zero, zero, zero, ty(0)
            f = np.where(viol, np.sqrt(np.where(viol, m / np.where(viol, tb, ty(1)), ty(1))), ty(1)).astype(dtype)
            T = T / np.minimum(f[:-1], f[1:])
            sweeps += 1
    tw = np.zeros(L, dtype)
    tw[0] = tb[0] * ty(0.5)
    for i in range(L - 1):
        tw[i + 1] = tw[i] + T[i]
    return OK, -1, sweeps, T, tb, tw, (mdv * tb) * ty(0.125), tw[L - 1] + tb[L - 1] * ty(0.5)


def restate(inp, dtype, delta=np.inf, max_sweeps=MAX_SWEEPS):
    """The whole definition in `dtype` on an input set: T (N, H-1), tb, tw, dev (N, H), duration, sweeps, status, first_bad (N,);
    entries at and past a path's length, and every entry of a path that is not OK, are 0."""
    q = np.ascontiguousarray(inp.paths[:, :, :inp.D]).astype(dtype)
    v_max, a_max = inp.v_max.astype(dtype), inp.a_max.astype(dtype)
    N, H, D = q.shape
    r = types.SimpleNamespace(T=np.zeros((N, H - 1), dtype), tb=np.zeros((N, H), dtype), tw=np.zeros((N, H), dtype), dev=np.zeros((N, H), dtype),
                              duration=np.zeros(N, dtype), sweeps=np.zeros(N, np.int32), status=np.zeros(N, np.int32),
                              first_bad=np.full(N, -1, np.int32), delta=delta)
    good_limits = bool(np.all(np.isfinite(inp.v_max)) and np.all(inp.v_max > 0) and np.all(np.isfinite(inp.a_max)) and np.all(inp.a_max > 0))
    for n in range(N):
        L = int(inp.lengths[n])
        if not good_limits or not 2 <= L <= H or not np.all(np.isfinite(q[n, :L])):
            r.status[n] = BAD_INPUT
            continue
        st, fb, sw, T, tb, tw, dev, dur = _one(q[n, :L], v_max, a_max, delta, max_sweeps, dtype)
        r.status[n], r.first_bad[n], r.sweeps[n], r.duration[n] = st, fb, sw, dur
        r.T[n, :L - 1], r.tb[n, :L], r.tw[n, :L], r.dev[n, :L] = T, tb, tw, dev
    return r


def kinematics(inp, T, tb, dtype):
    """v (N, H-1, D), dv, a (N, H, D) in `dtype` from T and tb as given: v_i = dq_i / T_i, dv_i = v_i - v_{i-1} with v_{-1} = v_{L-1} = 0,
    a_i = dv_i / tb_i and 0 where tb_i == 0; zero at and past a path's length and where T is 0."""
    q = np.ascontiguousarray(inp.paths[:, :, :inp.D]).astype(dtype)
    T, tb = T.astype(dtype), tb.astype(dtype)
    N, H, D = q.shape
    seg = (np.arange(H - 1)[None, :] < (inp.lengths - 1)[:, None]) & (T > 0)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        v = np.where(seg[:, :, None], (q[:, 1:] - q[:, :-1]) / np.where(seg, T, 1)[:, :, None], 0).astype(dtype)
        z = np.zeros((N, 1, D), dtype)
        dv = np.concatenate([v, z], 1) - np.concatenate([z, v], 1)
        a = np.where((tb > 0)[:, :, None], dv / np.where(tb > 0, tb, 1)[:, :, None], 0).astype(dtype)
    return v, dv, a


def sample(inp, T, tb, tw, duration, status, dt, T_rows, dtype, tau=None):
    """The sampler in `dtype`, fed T, tb, tw, duration as given (the kernel's own fp32 bits in the GPU tests): out (N, T_rows, 3D) --
    positions, velocities, accelerations at tau = fl32(k dt) --, n_rows, status.  `tau` (T_rows,) replaces the grid (CPU checks)."""
    ty = np.dtype(dtype).type
    q = np.ascontiguousarray(inp.paths[:, :, :inp.D]).astype(dtype)
    N, H, D = q.shape
    v, dv, a = kinematics(inp, T, tb, dtype)
    tb, tw, duration = tb.astype(dtype), tw.astype(dtype), duration.astype(dtype)
    out = np.zeros((N, T_rows, 3 * D), dtype)
    n_rows, st = np.zeros(N, np.int64), np.zeros(N, np.int32)
    dt = ty(np.float32(dt))
    tau = np.arange(T_rows).astype(dtype) * dt if tau is None else tau.astype(dtype)
    zrow = np.zeros((1, D), dtype)
    for n in range(N):
        if status[n] != OK:
            st[n] = status[n]
            out[n, :, :D] = q[n, 0]
            continue
        L = int(inp.lengths[n])
        n_rows[n] = int(np.ceil(float(np.float32(duration[n])) / float(dt))) + 1
        st[n] = TOO_LONG if n_rows[n] > T_rows else OK
        j = np.searchsorted(tw[n, :L], tau, side='right') - 1                    # -1 .. L-1: the last waypoint time <= tau
        jc = np.clip(j, 0, L - 1)
        jn = np.minimum(jc + 1, L - 1)
        in_own = (j < 0) | (j == L - 1) | ((tau - tw[n, jc]) <= tb[n, jc] * ty(0.5))
        in_next = ~in_own & ((tw[n, jn] - tau) <= tb[n, jn] * ty(0.5))
        i = np.where(in_next, jn, jc)                                            # the waypoint of the window, or the segment
        d = (tau - tw[n, i])[:, None]
        vp = np.concatenate([zrow, v[n]])[i]                                     # v_{i-1}
        vn = np.concatenate([v[n], zrow])[i]                                     # v_i (0 from the last waypoint on)
        s = d + (tb[n, i] * ty(0.5))[:, None]
        window = (in_own | in_next)[:, None]
        pos = np.where(window, (q[n, i] + vp * d) + ((a[n, i] * s) * s) * ty(0.5), q[n, i] + vn * d)
        vel = np.where(window, vp + a[n, i] * s, vn)
        acc = np.where(window, a[n, i], ty(0))
        past = (tau >= duration[n])[:, None]
        out[n, :, :D] = np.where(past, q[n, L - 1], pos)
        out[n, :, D:2 * D] = np.where(past, ty(0), vel)
        out[n, :, 2 * D:] = np.where(past, ty(0), acc)
    return out, n_rows, st


# ---- what the limits say of a timing, independently of the loop above ---------------------------------------------------------------
def overstep(inp, T, tb, delta, status):
    """From any T, tb, in fp64, over the OK paths: by how much |dq_ik| / T_i oversteps v_k, |dv_ik| / tb_i a_k and |dv_ik| tb_i / 8 delta,
    each relative to the limit and in units of 2^-23 (negative: below the limit everywhere)."""
    v, dv, _ = kinematics(inp, T, tb, np.float64)
    ok = status == OK
    vm, am = inp.v_max.astype(np.float64), inp.a_max.astype(np.float64)
    tb = tb.astype(np.float64)
    ulp = 2.0 ** -23
    with np.errstate(divide='ignore', invalid='ignore'):
        acc = np.where((tb > 0)[:, :, None], np.abs(dv) / np.where(tb > 0, tb, 1)[:, :, None], 0.0)
    ov = ((np.abs(v[ok]) - vm) / vm).max() / ulp
    oa = ((acc[ok] - am) / am).max() / ulp
    od = ((np.abs(dv[ok]) * tb[ok][:, :, None] / 8.0 - delta) / delta).max() / ulp if np.isfinite(delta) else -np.inf
    return float(ov), float(oa), float(od)


def polyline_at(inp, n, tw, tau):
    """(K, D) fp64: the point of path n's polyline guarantee 2 names for each time tau (K,): the polyline run through (tw_i, q_i) at
    constant velocity between the waypoint times, q_0 before tw_0 and q_{L-1} after tw_{L-1} -- inside a blend window this is the
    segment point at the same tau on the side of the window tau is on."""
    L = int(inp.lengths[n])
    q = inp.paths[n, :L, :inp.D].astype(np.float64)
    return np.stack([np.interp(tau, tw[n, :L].astype(np.float64), q[:, k]) for k in range(inp.D)], 1)


# ---- the input sets ---------------------------------------------------------------------------------------------------------------
def _inputs(paths, D, v_max, a_max, lengths=None):
    paths = np.ascontiguousarray(paths, np.float32)
    N, H, W = paths.shape
    return types.SimpleNamespace(paths=paths, D=D, N=N, H=H, W=W, v_max=np.asarray(v_max, np.float32), a_max=np.asarray(a_max, np.float32),
                                 lengths=np.full(N, H, np.int32) if lengths is None else np.asarray(lengths, np.int32), has_lengths=lengths is not None)


def random_walks(rng, N, H, D, scales=(0.02, 0.2, 1.0)):
    """Cumulative sums of normal steps, the step scale drawn per step from `scales`: long and short segments mixed within a path."""
    sc = np.asarray(scales)[rng.randint(0, len(scales), (N, H, 1))]
    return np.cumsum(rng.normal(0.0, 1.0, (N, H, D)) * sc, 1)


SETS = ('panda_h16', 'panda_h2', 'panda_h3', 'panda_h64', 'panda_h65', 'panda_h256', 'dof12_h33', 'dof2_h4', 'lengths_h16', 'collinear_h5')
STATUS_SETS = ('duplicate', 'bad_input')


@functools.lru_cache(maxsize=None)
def inputs(name):
    rng = np.random.RandomState((SETS + STATUS_SETS + ('needs_sweeps',)).index(name) + 4321)
    if name == 'panda_h16':
        return _inputs(random_walks(rng, N_PATHS, 16, 7), 7, PANDA_V, PANDA_A)
    if name in ('panda_h2', 'panda_h3'):                            # a single segment, a single corner
        return _inputs(random_walks(rng, N_PATHS, int(name[7:]), 7), 7, PANDA_V, PANDA_A)
    if name in ('panda_h64', 'panda_h65', 'panda_h256'):            # the trip boundary and the largest shape
        return _inputs(random_walks(rng, 5, int(name[7:]), 7), 7, PANDA_V, PANDA_A)
    if name == 'dof12_h33':
        return _inputs(random_walks(rng, 5, 33, 12), 12, rng.uniform(1.0, 3.0, 12), rng.uniform(5.0, 20.0, 12))
    if name == 'dof2_h4':
        return _inputs(random_walks(rng, N_PATHS, 4, 2), 2, [1.0, 1.5], [2.0, 3.0])
    if name == 'lengths_h16':                                        # rows at and past a length are NaN and must not matter
        q = random_walks(rng, N_PATHS, 16, 7)
        L = rng.randint(2, 17, N_PATHS)
        L[:3] = (2, 16, 3)
        q[np.arange(16)[None, :] >= L[:, None]] = np.nan
        return _inputs(q, 7, PANDA_V, PANDA_A, lengths=L)
    if name == 'collinear_h5':                                       # waypoint 2 lies on the line 1 -> 3 and both segments run at one speed
        q = random_walks(rng, 3, 5, 7, scales=(4.0,))                # (long segments: without a cap no waypoint is in violation, T_1 == T_2;
        q = np.round(q * 1024.0) / 1024.0                            # multiples of 2^-10: q_3 - q_2 == q_2 - q_1 bit for bit)
        q[:, 3] = q[:, 2] + (q[:, 2] - q[:, 1])
        return _inputs(q, 7, PANDA_V, PANDA_A)
    if name == 'duplicate':                                          # path 1: rows 4 and 5 equal -> DEGENERATE_SEGMENT, first_bad 4
        q = random_walks(rng, 3, 8, 7)
        q[1, 5] = q[1, 4]
        return _inputs(q, 7, PANDA_V, PANDA_A)
    if name == 'bad_input':                                          # path 0: a NaN, path 2: an inf, path 3: length 1, path 4: length H + 1
        q = random_walks(rng, 6, 8, 7)
        q[0, 3, 2] = np.nan
        q[2, 7, 6] = np.inf
        return _inputs(q, 7, PANDA_V, PANDA_A, lengths=[8, 8, 8, 1, 9, 5])
    if name == 'needs_sweeps':                                       # sharp corners between short segments: more than one sweep each
        return _inputs(random_walks(rng, 4, 8, 7, scales=(0.02,)), 7, PANDA_V, PANDA_A)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def handoff():
    """(scene, inputs) of the certificate hand-off: the Panda among 16 spheres (certify_checks.scene('panda')) and zigzag polylines of 5
    rows from 12 of its clearest of 400 uniform configurations, steps of at most 0.05 rad per joint on the even draws and 0.25 rad on the
    odd ones; the 10 of them the CPU prototype of the certifier (certify_checks.certify_ref, fp64) finds FREE are kept.  On the
    prototype (restate(fp64), blend_layout): the five small-step paths have margin_cert 0.115 m and are certified at every delta
    (deviation_workspace 0.02 .. 0.03 m); of the large-step ones path 8 (margin_cert 0.061 m) is certified at delta = 0.01 (0.034 m) and
    not at delta = inf (0.153 m), path 4 (0.089 m) at every delta, paths 1 and 6 (below 0.007 m) never.
    tests/test_path_blend_cpu.py holds these claims."""
    import certify_checks as C
    sc = C.scene('panda')
    rng = np.random.RandomState(7)
    N, H = 12, 5
    q0 = sc.uniform(400, 11).astype(np.float64)
    base = np.argsort(-sc.eta(q0), kind='stable')[:N]
    paths = np.zeros((N, H, 7))
    for i, b in enumerate(base):
        paths[i] = q0[b] + np.cumsum(rng.uniform(-1, 1, (H, 7)) * (0.05 if i % 2 == 0 else 0.25), 0)
    paths = paths.astype(np.float32)
    keep = [n for n in range(N) if C.certify_ref(sc, paths[n], CL.CERT_DEFAULT_SLACK)['status'] == C.FREE]
    return sc, _inputs(paths[keep], 7, PANDA_V, PANDA_A)


@functools.lru_cache(maxsize=None)
def reference(name, delta=np.inf, max_sweeps=MAX_SWEEPS):
    """(inputs, restate fp64, restate fp32) of a set at one delta, computed once and shared by the tests; nobody writes into it."""
    inp = inputs(name)
    return inp, restate(inp, np.float64, delta, max_sweeps), restate(inp, np.float32, delta, max_sweeps)


def measure():
    """E32 per set (relative to the largest value of the output) and the overstep restate(fp32) shows: what DESIGN.md 10 records."""
    worst = {'T': 0.0, 'tb': 0.0, 'tw': 0.0, 'dev': 0.0, 'duration': 0.0}
    over = [-np.inf] * 3
    for name in SETS:
        for delta in DELTAS:
            inp, r64, r32 = reference(name, delta)
            e = {k: float(np.abs(getattr(r32, k).astype(np.float64) - getattr(r64, k)).max() / np.abs(getattr(r64, k)).max()) for k in worst}
            ov = overstep(inp, r32.T, r32.tb, delta, r32.status)
            over = [max(a, b) for a, b in zip(over, ov)]
            worst = {k: max(worst[k], e[k]) for k in worst}
            print(f'{name:14s} delta {delta:5.2f}  sweeps fp64 {r64.sweeps.max():2d} fp32 {r32.sweeps.max():2d}  E32 ' +
                  ' '.join(f'{k} {v:.2e}' for k, v in e.items()) + f'  overstep v {ov[0]:.2f} a {ov[1]:.2f} dev {ov[2]:.2f} (2^-23)')
    print('largest E32:', {k: f'{v:.2e}' for k, v in worst.items()})
    print('largest overstep of restate(fp32) in units of 2^-23 (v, a, dev):', [f'{v:.2f}' for v in over])
    return worst, over


if __name__ == '__main__':
    measure()
