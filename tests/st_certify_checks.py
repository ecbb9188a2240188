"""Clearance and certification of timed trajectories among moving obstacles (ops.moving_clearance, ops.traj_certify_moving,
csrc/mpb_certify_moving.hip; definition: include/mpb.h) restated on the CPU in numpy with a dtype argument (helper module,
not collected): eta per pair, the motion bound, the bisection level by level with the device's queue order and trip counting, the row
predicate of check_trajs_moving, and the dense resamplings the soundness tests hold a certificate to.  The static scenes, the chain walk
and the oracle geometry are certify_checks.py's (C.scene and, through it, oracle/geometry_ref.py's fk_map_collision and signed_distance); the moving signed distances are
written out here because every sample has its own interpolated centres.

fp64: the definition.  fp32: the device's arithmetic operation by operation where this file can follow it -- fmaf(d, s, a) for the
interpolated configuration and centres, the fma chain of Lambda_l and V_o with their inflation, fmaf(-w, bound, sd) -- a fused
multiply-add formed as fp32(fp64 product + addend).  The chain walk and the static distances are the oracle's in fp32, whose sines and
contractions are not the device's: that difference is what the near-tie rule of tests/test_gpu_st_certify.py is for.

    python tests/st_certify_checks.py     # measures E_st = max |eta fp32 restatement - eta fp64 restatement| over 10^5 uniform
                                          # (configuration, segment, s) draws per scene: what st_certify_layout.STC_E_MEASURED records
"""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import certify_checks as C                                             # noqa: E402
from motion_planning_baselines_amd import certify_layout as CL          # noqa: E402
from motion_planning_baselines_amd import geometry as G                # noqa: E402
from motion_planning_baselines_amd import st_certify_layout as SL      # noqa: E402

FREE, COLLISION, UNDECIDED_DEPTH, UNDECIDED_QUEUE, BAD_INPUT, BUFFER_CHANGED, NOT_VALID = range(len(SL.STATUS))
F32, F64 = np.float32, np.float64
_TORCH = {F32: torch.float32, F64: torch.float64}
KEY_INSIDE = 0.37              # a keyframe time strictly inside a row interval of every scene's clock over [0, 1] (R = 6, 8, 5)


class STScene:
    """A static scene of certify_checks.py, a row count, and two fields of the same obstacles on the clock [0, 1]: `field` with a
    keyframe at KEY_INSIDE (chord_deviation > 0) and `field_rows` with keyframes at the first and last row only (chord_deviation 0)."""

    def __init__(self, name, R, field, field_rows):
        self.name, self.sc, self.R, self.field, self.field_rows = name, C.scene(name), int(R), field, field_rows
        self.D, self.L = self.sc.D, self.sc.L

    def tables(self, field=None, R=None):
        """What the packed buffer carries of a field, as fp32: centres (R, O, 3), radii (Os,), half (Ob, 3), margin."""
        field = self.field if field is None else field
        sc, bc = field.rows(self.R if R is None else R)
        return dict(centres=np.concatenate([sc, bc], 1).astype(F32), radii=field.sphere_radii.astype(F32), half=field.box_half.astype(F32),
                    margin=F32(field.margin), n_sph=field.n_spheres, n_box=field.n_boxes)


def _fields(dim, seed, n_sph, n_box, lo, hi, r_lo, r_hi, margin, bend=0.15):
    rng = np.random.RandomState(seed)
    O = n_sph + n_box
    keys = rng.uniform(lo, hi, (3, O, dim))
    keys[1] = 0.5 * (keys[0] + keys[2]) + bend * rng.uniform(-1, 1, (O, dim)) * (np.asarray(hi) - np.asarray(lo))    # a bend at the inner keyframe
    radii = rng.uniform(r_lo, r_hi, n_sph) if n_sph else None
    half = rng.uniform(r_lo, r_hi, (n_box, dim)) if n_box else None
    mk = lambda t, k: G.MovingObstacleField(t, k[:, :n_sph] if n_sph else None, radii, k[:, n_sph:] if n_box else None, half, margin=margin,
                                            t_start=0.0, t_end=1.0)
    return mk([0.0, KEY_INSIDE, 1.0], keys), mk([0.0, 1.0], keys[[0, 2]])


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == 'pm2d':            # point robot, R = 6, 2 moving circles + 1 moving box among the dense 2-D field
        return STScene(name, 6, *_fields(2, 41, 2, 1, [-0.8, -0.8], [0.8, 0.8], 0.10, 0.18, 0.02))
    if name == 'panda':           # Panda, R = 8, 2 spheres + 1 box among the 16 static spheres
        return STScene(name, 8, *_fields(3, 42, 2, 1, [0.3, -0.6, 0.2], [0.7, 0.6, 0.9], 0.06, 0.10, 0.03))
    if name == 'chain12':         # 12-joint chain, R = 5, 1 box, two chained static fields
        return STScene(name, 5, *_fields(3, 43, 0, 1, [0.4, -0.6, 0.2], [0.8, 0.6, 0.9], 0.06, 0.10, 0.04))
    raise KeyError(name)


SCENES = C.SCENES


# ---- the definition, sample by sample ---------------------------------------------------------------------------------------------
def _fma(a, b, c, T):
    """a * b + c rounded once in T (fp32: through the exact fp64 product)."""
    if T is F32:
        return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)
    return np.asarray(a, F64) * b + c


def _sumsq(v, T):
    """x^2 + y^2 + z^2 of v (..., 3) as the contracted device expression forms it: fma(z, z, fma(y, y, x * x))."""
    return _fma(v[..., 2], v[..., 2], _fma(v[..., 1], v[..., 1], v[..., 0] * v[..., 0], T), T)


def _lambda(st, q0, q1, T):
    """Lambda (N, L) of the steps q0 -> q1 in T: fp64 the real sum (certify_layout.motion_bound), fp32 the device's fma chain, inflated."""
    sc = st.sc
    if T is F64:
        return np.broadcast_to(CL.motion_bound(sc.rs, sc.rho, q0, q1), (len(q0), st.L)).astype(F64)
    ad = np.abs(q1.astype(F32) - q0.astype(F32))
    if int(sc.rs['kind']) == 0:
        ad3 = np.concatenate([ad, np.zeros((len(ad), 3 - ad.shape[1]), F32)], 1)
        s = np.zeros(len(ad), F32)
        for i in range(3):
            s = _fma(ad3[:, i], ad3[:, i], s, F32)
        return (np.sqrt(s) * F32(CL.CERT_LAMBDA_INFLATE))[:, None]
    lam = np.zeros((len(ad), st.L), F32)
    for i in range(st.D):
        lam = _fma(ad[:, i:i + 1], sc.rho[i][None, :], lam, F32)
    return lam * F32(CL.CERT_LAMBDA_INFLATE)


def evaluate(st, tab, q0, q1, h0, h1, s, w, T=F64, c_true=None):
    """N samples of the continuum in dtype T.  q0, q1 (N, D): the rows of each sample's segment; h0, h1 (N,): the rows whose centres
    bound its chord; s (N,): its parameter; w: the half-width (0: no motion bound).  c_true (N, O, 3): centres to use INSTEAD of the
    chord's (the field's own motion).  Returns a dict of fp64 arrays: eta (N,), link, obst (o >= 0 moving, -1 - f static field f),
    eta_l (N, L), pairs (N, L, F + O) the eta of every (sphere, static field | moving obstacle), bound (N,) = min over pairs of eta_pair - w bound_pair, hit (N,) the restated row predicate of check_trajs_moving."""
    sc = st.sc
    N = len(q0)
    q0, q1, s = np.asarray(q0, T), np.asarray(q1, T), np.asarray(s, T)
    m = _fma(q1 - q0, s[:, None], q0, T)
    rr, rfs = sc.ref(_TORCH[T])
    with torch.no_grad():
        xt = rr.fk_map_collision(torch.as_tensor(m, dtype=_TORCH[T]).reshape(N, st.D))
        sd_f = torch.stack([rf.signed_distance(xt) for rf in rfs], -1).numpy()                      # (N, L, F)
    x = xt.numpy().reshape(N, st.L, 3)
    r_l = np.asarray(sc.rs['link_radius'], F32).astype(T)[None, :]
    mg_f = np.array([F32(rf.margin) for rf in rfs], F32).astype(T)
    e_f = sd_f - mg_f                                                                               # (N, L, F)
    eta_s = e_f.min(-1) - r_l
    # the moving obstacles on their chords
    cen = tab['centres'].astype(T)
    c0, c1 = cen[h0], cen[h1]                                                                      # (N, O, 3)
    d = c1 - c0
    c = _fma(d, s[:, None, None], c0, T) if c_true is None else np.asarray(c_true, T)
    if T is F32:
        V = np.sqrt(_fma(d[..., 2], d[..., 2], _fma(d[..., 1], d[..., 1], d[..., 0] * d[..., 0], T), T)) * F32(CL.CERT_LAMBDA_INFLATE)
    else:
        V = np.sqrt((d * d).sum(-1))                                                                # (N, O)
    p = x[:, :, None, :] - c[:, None, :, :]                                                        # (N, L, O, 3)
    ns = tab['n_sph']
    sd = np.empty(p.shape[:3], T)
    ps = p[:, :, :ns]
    sd[:, :, :ns] = np.sqrt(_sumsq(ps, T)) - tab['radii'].astype(T)
    a = np.abs(p[:, :, ns:]) - tab['half'].astype(T)[None, None]
    qo = np.maximum(a, 0)
    sd[:, :, ns:] = np.sqrt(_sumsq(qo, T)) + np.minimum(a.max(-1), 0)
    thr = tab['margin'].astype(T) + r_l                                                            # (1, L)
    eta_m = sd.min(-1) - thr
    eta_l = np.minimum(eta_s, eta_m)
    link = eta_l.argmin(1)
    idx = np.arange(N)
    moving = (eta_m < eta_s)[idx, link]
    obst = np.where(moving, sd.argmin(-1)[idx, link], -1 - e_f.argmin(-1)[idx, link])
    out = dict(eta=eta_l.min(1).astype(F64), link=link, obst=obst, eta_l=eta_l.astype(F64))
    out['pairs'] = np.concatenate([e_f - r_l[..., None], sd - thr[..., None]], -1).astype(F64)      # (N, L, F + O): static fields, then moving
    out['hit'] = ((mg_f + r_l[..., None]) - sd_f > 0).any((1, 2)) | (thr - sd.min(-1) > 0).any(1)
    if w > 0:
        lam = _lambda(st, q0, q1, T)                                                                # (N, L)
        b_s = _fma(-T(w), lam, eta_s, T)
        b_m = _fma(-T(w), lam[:, :, None] + V[:, None, :], sd, T).min(-1) - thr
        out['bound'] = np.minimum(b_s, b_m).min(1).astype(F64)
    else:
        out['bound'] = out['eta']
    return out


# ---- the bisection ----------------------------------------------------------------------------------------------------------------
def certify_ref(st, tab, traj, S, c_req=0.0, max_depth=CL.CERT_DEFAULT_MAX_DEPTH, max_intervals=CL.CERT_DEFAULT_MAX_INTERVALS, T=F64):
    """The recursion of include/mpb.h on one trajectory (R, D) in dtype T: dict(status, witness = (row, s, link, obstacle, eta) or None,
    n_evals, depth_max, margin_cert, decision_margin).  n_evals counts whole trips of 64 up to the trip that holds the witness, as the
    device does.  decision_margin: the least distance of a quantity that decided something from its threshold, over everything
    evaluated -- |eta - c_req + S| for the collision tests, |bound - c_req - S| for the free tests."""
    traj = np.asarray(traj, F32)
    R = len(traj)
    out = dict(status=FREE, witness=None, n_evals=0, depth_max=-1, margin_cert=-np.inf, decision_margin=np.inf)
    if not np.isfinite(traj).all():
        out['status'] = BAD_INPUT
        return out
    S, c_req = (F64(F32(S)), F64(F32(c_req))) if T is F32 else (float(S), float(c_req))
    sub = (lambda v: (v.astype(F32) - F32(c_req)).astype(F64)) if T is F32 else (lambda v: v - c_req)
    rows = np.arange(R)
    e = evaluate(st, tab, traj, traj, rows, rows, np.zeros(R), 0.0, T)
    val = sub(e['eta'])
    hit = np.nonzero(val < -S)[0]
    if len(hit):
        k = int(hit[0])
        out['n_evals'] = min(R, 64 * (k // 64 + 1))
        out['decision_margin'] = float(np.abs(val[:k + 1] + S).min())
        out.update(status=COLLISION, witness=(k, 0.0, int(e['link'][k]), int(e['obst'][k]), float(e['eta'][k])))
        return out
    out['n_evals'] = R
    out['decision_margin'] = float(np.abs(val + S).min())
    cert = float(val[0]) if R == 1 else np.inf
    if R - 1 > max_intervals:
        out['status'] = UNDECIDED_QUEUE
        return out
    seg, j = np.arange(R - 1), np.zeros(R - 1, np.int64)
    undecided = False
    for d in range(max_depth + 1):
        if not len(seg):
            break
        out['depth_max'] = d
        w = 2.0 ** -(d + 1)
        s = (2 * j + 1) * w
        e = evaluate(st, tab, traj[seg], traj[seg + 1], seg, seg + 1, s, w, T)
        val, bnd = sub(e['eta']), sub(e['bound'])
        coll = val < -S
        if coll.any():
            k = int(np.nonzero(coll)[0][0])
            out['n_evals'] += min(len(seg), 64 * (k // 64 + 1))
            out['decision_margin'] = min(out['decision_margin'], float(np.abs(val[:k + 1] + S).min()))
            out.update(status=COLLISION, witness=(int(seg[k]), float(s[k]), int(e['link'][k]), int(e['obst'][k]), float(e['eta'][k])))
            return out
        out['n_evals'] += len(seg)
        out['decision_margin'] = min(out['decision_margin'], float(np.abs(val + S).min()), float(np.abs(bnd - S).min()))
        free = bnd > S
        if free.any():
            cert = min(cert, float(bnd[free].min()))
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


# ---- dense resamplings --------------------------------------------------------------------------------------------------------------
def dense_eta(st, tab, traj, n=4097, field=None):
    """min eta in fp64 over n evenly spaced parameters (both ends included) of every interval of the trajectory.  field None: the
    obstacles on the CHORDS of `tab`'s centres; a MovingObstacleField: on the field's own motion, field._centres(t), at the clock's time
    t_start + (h + s) dt_row."""
    traj = np.asarray(traj, F64)
    R = len(traj)
    rows = np.arange(R)
    if R == 1:
        return float(evaluate(st, tab, traj, traj, rows, rows, np.zeros(1), 0.0)['eta'].min())
    s = np.linspace(0.0, 1.0, n)
    worst = np.inf
    for h in range(R - 1):
        hh = np.full(n, h)
        c_true = None
        if field is not None:
            t = field.t_start + (h + s) * (field.t_end - field.t_start) / (R - 1)
            c_true = np.concatenate(field._centres(t), 1)
        e = evaluate(st, tab, np.repeat(traj[h:h + 1], n, 0), np.repeat(traj[h + 1:h + 2], n, 0), hh, hh + 1, s, 0.0, F64, c_true=c_true)
        worst = min(worst, float(e['eta'].min()))
    return worst


def trajs(st, n, short, seed, bump=0.03):
    """n trajectories (n, R, D) fp32: short straight segments with a sine perturbation (certify_checks.short_paths)."""
    return C.short_paths(st.sc, n, st.R, short, seed, bump=bump)


# (short, seed, bump) of the 32 trajectories per scene the certifier tests run: chosen on the CPU so that FREE, COLLISION and
# UNDECIDED_DEPTH (max_depth = 3) all occur and the fp32 restatement decides as the fp64 one (test_st_certify_cpu.py holds both)
CERT_CASES = dict(pm2d=(1.0, 13, 0.1), panda=(0.1, 22, 0.02), chain12=(0.3, 12, 0.03))


def decision(r):
    """What the device and a restatement must agree on exactly: status, the witness but for its eta, n_evals, depth_max."""
    return r['status'], (r['witness'][:4] if r['witness'] else None), r['n_evals'], r['depth_max']


def uniform_samples(st, n, seed):
    """n uniform (configuration fp32 (n, D), segment (n,), s fp32 (n,)) draws."""
    rng = np.random.RandomState(seed)
    return st.sc.uniform(n, seed), rng.randint(0, st.R - 1, n), rng.uniform(0.0, 1.0, n).astype(F32)


# ---- the tunnelling case ----------------------------------------------------------------------------------------------------------
TUNNEL_R, TUNNEL_ROW, TUNNEL_S, TUNNEL_HALF_WIDTH = 6, 3, 0.3, (0.02 + 0.005 + 0.005) / 2.0


def tunnel():
    """A 2-D point robot of radius 0.005 that STANDS STILL at (-0.4, 0) for R = 6 rows on the clock [0, 5]; one circle of radius 0.02
    (margin 0.005) that crosses from x = -1 to x = +1 between rows 3 and 4, its keyframes on those rows (held before and after): contact
    is centred at s = 0.3 of interval 3 and lasts (0.02 + 0.005 + 0.005) / 2 in s to either side.  The static scene is one far circle.
    Returns (STScene-like, field, trajectory (6, 2) fp32)."""
    static = G.CollisionField(spheres=np.array([[0.8, 0.8, 0.05]], F32), margin=0.005)
    sc = C.Scene('st_tunnel', G.RobotPointMass(2, radius=0.005), [static], -1.0, 1.0)
    field = G.MovingObstacleField([3.0, 4.0], sphere_centers=np.array([[[-1.0, 0.0]], [[1.0, 0.0]]]), sphere_radii=[0.02], margin=0.005,
                                  t_start=0.0, t_end=5.0)
    st = STScene.__new__(STScene)
    st.name, st.sc, st.R, st.field, st.field_rows, st.D, st.L = 'st_tunnel', sc, TUNNEL_R, field, field, sc.D, sc.L
    return st, field, np.tile(np.array([[-1.0 + 2.0 * TUNNEL_S, 0.0]], F32), (TUNNEL_R, 1))


def measure_E(n=100000, chunk=20000):
    worst = 0.0
    for name in SCENES:
        st = scene(name)
        tab = st.tables()
        q, h, s = uniform_samples(st, n, seed=20261021)
        e = 0.0
        for k in range(0, n, chunk):
            sl = slice(k, k + chunk)
            a = evaluate(st, tab, q[sl], q[sl], h[sl], h[sl] + 1, s[sl], 0.0, F32)['eta']
            b = evaluate(st, tab, q[sl], q[sl], h[sl], h[sl] + 1, s[sl], 0.0, F64)['eta']
            e = max(e, float(np.abs(a - b).max()))
        print(f'{name}: E_st = {e:.3e} over {n} uniform (configuration, segment, s) draws')
        worst = max(worst, e)
    print(f'E_st = {worst:.3e}; S = 32 E_st = {32 * worst:.3e}')
    return worst


if __name__ == '__main__':
    measure_E()
