"""The STOMP sample and update kernels, element by element, decided by the fp64 oracle alone (helper module; imported like
chomp_step_checks.py and collision_kinks.py).  Nothing here runs the code under test.

The reference is oracle/planners_ref.py -- stomp_sample, stomp_weights, stomp_update -- on the fp32 inputs widened exactly; the same
functions on the fp32 tensors are the fp32 restatement whose worst error, in the units below, is E32.  Units come from the inputs alone.

  sample   u_s[p,s,h,c] = |m[p,h,c]| + sum_k |L[h,k] eps[s,c,p,k]|  on rows 1 .. H-2; 0 on rows 0 and H-1, where an element must carry
           the bits of `means`.
  weight   x = -c / T, m = max x, a_s = (1 + extra) |x_s| + |x_s - m| + 1, u_w[p,s] = w64_s (a_s + sum_j w64_j a_j): the first-order
           movement of a softmax weight when every logit moves by one relative fp32 rounding (d w_s = w_s (d x_s - sum_j w_j d x_j)).
           An element with w64 below fp32's smallest normal is not judged by ratio: it must come out below 2^-125.  `extra`: the
           roundings of a logit a kernel adds to the restatement's (PERSISTENT_EXTRA for the persistent kernels, counted below).
  mean     the fp64 update is evaluated from the kernel's OWN returned weights, widened -- the weighted reduce and the Sigma product
           apart from the softmax's conditioning.  With r[p,k,c] = sum_s w_s |x_s[k,c] - m[k,c]|:
               u_m[p,h,c] = |m[h,c]| + lr sum_k |Sigma[h,k]| r[p,k,c]      (with Sigma)
               u_m[p,h,c] = |m[h,c]| + lr r[p,h,c]                         (Sigma = None)

Criterion, every element, none left out:  e = |got - ref64| / unit <= collision_kinks.bar(E32) = 4 max(E32, 2^-23).  The factor is
adequate because the two-kernel path uses expf, an IEEE division and fp32 fma chains like the restatement, and the noise product is
exact up to three dropped 2^-24 pairs (csrc/mpb_stomp_noise.h).

PERSISTENT_EXTRA = 5, from the source of csrc/mpb_stomp_fused.hip (csrc/mpb_stomp_fused_hx.hip has the same expressions at its lines
186, 402, 406, 496 and 507), not from its output.  Costs are >= 0, so x <= m <= 0 and every difference of logits below is at most |x|:
  1   `inv_temperature = 1.0f / temperature` (line 232) is rounded before `-cst * inv_temperature` (line 406); the product's own
      rounding stands for the restatement's division;
  2   `fast_expf(xs - mb)` (line 408) is v_exp_f32((xs - mb) * fp32(log2 e)) (csrc/mpb_common.h:178): the constant's rounding and the
      product's, each 2^-24 |x - mb|;
  2   the chunk's factor `fast_expf(mb - m_all)` (lines 552, 625-630): the same two on |mb - m_all| <= |x - m_all|.
The relative roundings of the result (two v_exp_f32, the two products of `ex * f_own * rz`, v_rcp_f32; lines 635-641) stay under
a_s's "+ 1" and the bar's factor.

Inputs.  L: 'dense' (random lower-triangular, the rows' scales span four decades, permuted, so that a small row is judged in its own
unit), 'stomp' (STOMP's own scale_tril from stomp_precision_matrix), 'identity' (with bf16-representable eps: a sample must be
fp32(mean + eps) bit for bit).  Sigma: 'spd' (D S0 D, S0 random SPD, D the same four decades), 'stomp' (inverse of STOMP's R), None.
Samples of the update cases move on EVERY row, the edge rows included (a Sigma product that stops short of k = H-1 must show).
Cost families (COSTS): flat 5 rand at T = 0.7; spread, -c/T = -200 u^3 (1 + 0.01 rand) with u a permuted linspace(0, 1, S) (0 to -200,
crowded near the maximum so that several weights are of order one while the last ones underflow); c3, 1e6 + 1e7 rand at T = 1 with the
second and third lowest costs of a particle moved to min + 2 and min + 5 -- a plain draw at that scale leaves one nonzero weight, and
the C3 regime (sigma_coll = 1e-3) is interesting where near-ties at 1e6-1e7 decide the weights; equal; onehot, one cost lower by 1e4 T;
tied, two equal minima."""
import functools
import types

import torch

import collision_kinks as K

TINY = 2.0 ** -126                # fp32's smallest normal
FLUSHED = 2.0 ** -125
LR = 0.3
PERSISTENT_EXTRA = 5
L_FAMILIES = ('dense', 'stomp', 'identity')
COSTS = ('flat', 'spread', 'c3', 'equal', 'onehot', 'tied')
TEMPERATURE = dict(flat=0.7, spread=0.7, c3=1.0, equal=0.7, onehot=0.7, tied=0.7)
DT, SIGMA_SPECTRAL = 0.04, 0.02

# ------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_stomp_kernels_elements.py (tests/test_stomp_kernels_cpu.py checks their conditions on the CPU)
# ------------------------------------------------------------------------------------------------
H64_D = (2, 3, 4, 6, 7, 14)
# (P, S, H, d).  H = 64 kernel: P S = 5 and 9 against four rollouts per workgroup (5 is prime: the one place P leaves {2, 3})
SAMPLE_H64 = [(P, S, 64, d) for d in H64_D for P, S in ((5, 1), (3, 3))]
_PS = ((2, 1), (3, 3), (2, 3), (3, 1))
_HX = [(64, 1), (64, 5), (64, 8), (64, 16), (3, 1), (3, 4), (63, 7), (65, 3), (65, 4), (100, 14), (128, 2), (129, 5), (192, 16), (255, 1),
       (256, 3)]
SAMPLE_HX = [(*_PS[i % 4], H, d) for i, (H, d) in enumerate(_HX)]
SAMPLE_DRAWN = [(3, 3, 64, 7), (2, 3, 100, 14)]              # one per kernel
# (S, H, d)
UPDATE_V4 = [(1, 4, 1), (3, 4, 2), (5, 8, 14), (32, 64, 14), (33, 64, 14), (64, 64, 16), (64, 60, 7), (9, 4, 24)]
UPDATE_GENERIC = [(2, 5, 1), (3, 3, 1), (4, 5, 3), (7, 5, 3), (70, 9, 2), (8, 6, 2), (65, 64, 14), (8, 68, 4), (6, 100, 12), (1030, 3, 1),
                  (4, 128, 1), (4, 256, 24)]
UPDATE_ALL_FAMILIES = [(33, 64, 14), (70, 9, 2)]
UPDATE_REFUSED = (8000, 256, 24)


def sample_kernel_of(H, d):
    """launch_sample's choice (csrc/mpb_kernels.hip) without a geometry: 'h64' or the chunked 'hx'."""
    return 'h64' if H == 64 and d in H64_D else 'hx'


def update_kernel_of(S, H, d, with_sigma=True):
    """mpb_stomp_launch_update's choice: 'v4', 'generic/lds', 'generic/global', 'generic/none', or None (refused)."""
    n = H * d
    if n % 4 == 0 and n <= 1024 and H <= 64 and H % 4 == 0 and S <= 64:
        return 'v4'
    base = (S + 5 * n) * 4
    in_lds = base + H * H * 4 <= 64 * 1024
    if (base + H * H * 4 if in_lds else base) > 150 * 1024:
        return None
    return 'generic/none' if not with_sigma else ('generic/lds' if in_lds else 'generic/global')


def update_P(shape):
    """P of an update case: 2 or 3."""
    return 2 if sum(shape) % 2 else 3


def update_families(shape):
    return COSTS if shape in UPDATE_ALL_FAMILIES else ('flat', 'spread')


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def _gen(*key):
    seed = 17
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def row_scales(H, gen):
    """(H,) fp64: 10^0 .. 10^-4, permuted."""
    return 10.0 ** (-4.0 * torch.linspace(0, 1, H, dtype=torch.float64)[torch.randperm(H, generator=gen)])


@functools.lru_cache(maxsize=None)
def stomp_constants(H):
    """STOMP's own (L, Sigma), fp32, from the product's stomp_precision_matrix; the inverse and the factor are taken in fp64."""
    from motion_planning_baselines_amd.planners.stomp import precision_to_scale_tril, stomp_precision_matrix
    R = stomp_precision_matrix(H, DT, SIGMA_SPECTRAL, K.F32).double()
    return precision_to_scale_tril(R).float().contiguous(), torch.inverse(R).float().contiguous()


@functools.lru_cache(maxsize=None)
def scale_tril(H, family):
    assert family in L_FAMILIES
    if family == 'stomp':
        return stomp_constants(H)[0]
    if family == 'identity':
        return torch.eye(H)
    gen = _gen(1, H)
    return (torch.tril(torch.randn(H, H, generator=gen, dtype=torch.float64)) * row_scales(H, gen)[:, None]).float().contiguous()


@functools.lru_cache(maxsize=None)
def covariance(H, kind):
    if kind is None:
        return None
    if kind == 'stomp':
        return stomp_constants(H)[1]
    assert kind == 'spd'
    gen = _gen(2, H)
    A = torch.randn(H, H, generator=gen, dtype=torch.float64) / H ** 0.5
    s = row_scales(H, gen)
    S0 = A @ A.T + 0.1 * torch.eye(H, dtype=torch.float64)
    return (0.5 * (S0 + S0.T) * s[:, None] * s[None, :]).float().contiguous()


@functools.lru_cache(maxsize=None)
def sample_problem(P, S, H, d, family):
    """means (P, H, d), L (H, H), eps (S, d, P, H) in the reference's draw order; read-only."""
    gen = _gen(3, P, S, H, d, L_FAMILIES.index(family))
    means = torch.randn(P, H, d, generator=gen)
    eps = torch.randn(S, d, P, H, generator=gen)
    if family == 'identity':
        eps = eps.bfloat16().float()
    return types.SimpleNamespace(P=P, S=S, H=H, d=d, family=family, means=means, L=scale_tril(H, family), eps=eps.contiguous())


def costs_of(family, P, S, gen):
    """(costs (P, S) fp32, temperature)"""
    T = TEMPERATURE[family]
    r = torch.rand(P, S, generator=gen)
    if family == 'flat':
        c = 5.0 * r
    elif family == 'spread':
        u = torch.stack([torch.linspace(0, 1, S)[torch.randperm(S, generator=gen)] for _ in range(P)])
        c = T * 200.0 * u ** 3 * (1.0 + 0.01 * r)
    elif family == 'c3':
        c = 1.0e6 + 1.0e7 * r
        order = c.argsort(dim=1)
        for p in range(P):
            for rank, off in ((1, 2.0), (2, 5.0)):
                if S > rank:
                    c[p, order[p, rank]] = c[p, order[p, 0]] + off
    elif family == 'equal':
        c = torch.full((P, S), 3.25)
    elif family == 'onehot':
        c = 5.0 * r + 1.0e4 * T
        for p in range(P):
            i = int(torch.randint(S, (1,), generator=gen))
            c[p, i] = 5.0 * r[p, i]
    elif family == 'tied':
        c = 3.0 + 5.0 * r
        for p in range(P):
            ij = torch.randperm(S, generator=gen)[:2]
            c[p, ij] = 0.5
    else:
        raise KeyError(family)
    return c.float().contiguous(), T


@functools.lru_cache(maxsize=None)
def update_problem(P, S, H, d, family, sigma_kind):
    """means (P, H, d), samples (P, S, H, d) moving on every row, costs (P, S), temperature, Sigma (H, H) or None, lr; read-only."""
    gen = _gen(4, P, S, H, d, COSTS.index(family))
    means = torch.randn(P, H, d, generator=gen)
    samples = (means.unsqueeze(1) + 0.3 * torch.randn(P, S, H, d, generator=gen)).contiguous()
    costs, T = costs_of(family, P, S, gen)
    return types.SimpleNamespace(P=P, S=S, H=H, d=d, family=family, means=means, samples=samples, costs=costs, temperature=T,
                                 Sigma=covariance(H, sigma_kind), sigma_kind=sigma_kind, lr=LR)


# ------------------------------------------------------------------------------------------------
# the references and their units
# ------------------------------------------------------------------------------------------------
def errors(got, ref64, unit):
    """e per element; 0 where the unit is 0 (those elements are compared by bits)."""
    zero = unit == 0
    return (got.double() - ref64).abs() / torch.where(zero, torch.ones_like(unit), unit) * (~zero)


def sample_reference(means, L, eps):
    from oracle import planners_ref as O
    H = means.shape[1]
    x64 = O.stomp_sample(means.double(), L.double(), eps.double())
    x32 = O.stomp_sample(means, L, eps)
    n = torch.matmul(L.double().abs(), eps.double().abs().unsqueeze(-1)).squeeze(-1)         # (S, d, P, H)
    unit = means.double().abs().unsqueeze(1) + n.permute(2, 0, 3, 1)
    unit[:, :, 0] = 0
    unit[:, :, H - 1] = 0
    ns = types.SimpleNamespace(x64=x64, x32=x32, unit=unit, zero=unit == 0,
                               carried=means.unsqueeze(1).expand_as(x32))                   # what a unit-0 element must hold
    ns.e32 = errors(x32, x64, unit)
    ns.E32 = float(ns.e32.max())
    return ns


def weights_reference(costs, temperature, extra=0):
    from oracle import planners_ref as O
    w64 = O.stomp_weights(costs.double(), temperature)
    w32 = O.stomp_weights(costs, temperature)
    x = -costs.double() / temperature
    a = (1 + extra) * x.abs() + (x - x.max(dim=1, keepdim=True)[0]).abs() + 1.0
    unit = w64 * (a + (w64 * a).sum(1, keepdim=True))
    tiny = w64 < TINY
    ns = types.SimpleNamespace(w64=w64, w32=w32, unit=unit, tiny=tiny, judged=~tiny)
    ns.e32 = errors(w32, w64, unit) * ns.judged
    ns.E32 = float(ns.e32.max())
    return ns


def _update(means, samples, weights, Sigma, lr):
    from oracle import planners_ref as O
    if Sigma is not None:
        return O.stomp_update(means, samples, weights, Sigma, lr)
    P, S = weights.shape                                       # stoch_gpmp.py:272-275: no covariance product
    return means + lr * (weights.reshape(P, S, 1, 1) * (samples - means.unsqueeze(1))).sum(1)


def mean_reference(means, samples, weights, Sigma, lr):
    """weights: the fp32 weights the update is evaluated from (a kernel's own; the fp32 restatement's on the CPU)."""
    w64 = weights.double()
    Sg64 = None if Sigma is None else Sigma.double()
    m64 = _update(means.double(), samples.double(), w64, Sg64, lr)
    m32 = _update(means, samples, weights, Sigma, lr)
    r = (w64[:, :, None, None] * (samples.double() - means.double().unsqueeze(1)).abs()).sum(1)
    unit = means.double().abs() + lr * (r if Sigma is None else Sg64.abs() @ r)
    ns = types.SimpleNamespace(m64=m64, m32=m32, unit=unit, r=r)
    ns.e32 = errors(m32, m64, unit)
    ns.E32 = float(ns.e32.max())
    return ns


# ------------------------------------------------------------------------------------------------
# the criterion
# ------------------------------------------------------------------------------------------------
def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def judge(label, got, ref64, unit, E32, judged=None):
    """Prints E32, the worst e and the bar; returns (worst e, bar, indices of the elements over the bar -- NaN is over it)."""
    e = errors(got, ref64, unit)
    if judged is not None:
        e = torch.where(judged, e, torch.zeros_like(e))
    bar = K.bar(E32)
    worst = float(e.max()) if bool(torch.isfinite(e).all()) else float('nan')
    print(f'STOMP-ELEM {label}: E32 {E32:.3e} worst e {worst:.3e} bar {bar:.3e}')
    return worst, bar, torch.nonzero(~(e <= bar))


def check_samples(label, got, ref):
    """Every element of the samples: the bar where the unit is positive, the bits of `means` where it is 0.  Returns (worst, bar)."""
    worst, bar, bad = judge(label + ' samples', got, ref.x64, ref.unit, ref.E32)
    assert len(bad) == 0, (label, 'first of', len(bad), 'elements (p, s, h, c) over the bar', bad[0].tolist())
    assert same_bits(got[ref.zero], ref.carried[ref.zero]), (label, 'an edge row does not carry the bits of the means')
    return worst, bar


def check_weights(label, got, ref):
    worst, bar, bad = judge(label + ' weights', got, ref.w64, ref.unit, ref.E32, ref.judged)
    assert len(bad) == 0, (label, 'first of', len(bad), 'weights (p, s) over the bar', bad[0].tolist())
    assert bool((got[ref.tiny].abs() < FLUSHED).all()), (label, 'a weight below the smallest normal came out above 2^-125')
    return worst, bar


def check_means(label, got, ref, means0):
    worst, bar, bad = judge(label + ' means', got, ref.m64, ref.unit, ref.E32)
    assert len(bad) == 0, (label, 'first of', len(bad), 'elements (p, h, c) over the bar', bad[0].tolist())
    zero = ref.unit == 0
    assert same_bits(got[zero], means0[zero])
    return worst, bar
