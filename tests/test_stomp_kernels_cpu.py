"""No GPU: the conditions tests/test_gpu_stomp_kernels_elements.py relies on (helper: tests/stomp_kernels_checks.py), and what its
per-element bar is worth on faults planted in a numpy fp32 restatement of the kernels' loop structure.

Conditions, for every shape of the GPU file and every input family: every interior unit is positive; every E32 is positive (except a
softmax whose judged weights are exactly representable -- S = 1 and the one-hot family give the weights 1 and 0 in any precision);
the spread family has at least 3 weights above 1e-3 and at least one below fp32's smallest normal per particle whenever S >= 8; the
C3-like family has at least two weights above 1e-3 in at least half the particles; the dispatch path of every case is the one its
list claims.

Planted faults, each at the smallest shape of the GPU file that exercises it, each against the unfaulted restatement passing the
same bar on the same inputs.  "old": the earlier global norm max|a-b| / max|b| of the faulted output on these inputs, against its
bars (2e-6 on means; 2e-5 / 1e-4 on samples) -- measured by this file, which prints each figure:

  fault                                                      shape                      per-element             old norm
  last sample of a sample group dropped                      (S, H, d) = (4, 5, 3)      27 of 30 means over     2.3e-2, fails
  Sigma product stops at k = H-2                             (3, 3, 1)                  2 of 6 means            4.0e-6, fails (bar 2e-6)
  delta read from the wrong channel, d not dividing 4        (4, 5, 3)                  28 of 30 means          4.2e-2, fails
  an edge row of the noise not zeroed                        (H, d) = (3, 1)            bits of row H-1         5.9e-5 / 6.8e-3, fails
  last 64-column block of L dropped                          (H, d) = (66, 3)           9 of 9 in row 64        3.8e-5 / 1.3e-2: the dense L
                                                                                                                passes the 1e-4 bar
  maximum not subtracted before exp, C3-like costs           (70, 9, 2)                 NaN                     NaN, fails
  softmax trips beyond the first 1024 samples dropped        (1030, 3, 1)               all 2060 weights        1.1e-4 on the means, fails
  lr applied per term and again at the end                   (3, 3, 1)                  5 of 6 means            1.4e-2, fails

So on THESE inputs the global norms would have stopped all but one of them too: what the earlier tests lacked is the inputs.  None of
them ran S > 1024, an interior row behind column 63 next to a one-column last block, or costs of 1e6-1e7 through stomp_update alone;
with flat costs (5 rand, T = 0.7) the unsubtracted maximum changes nothing beyond rounding (asserted below), and the Sigma product
stopping one column short sits within a factor two of the 2e-6 bar even with a delta on the edge rows, which STOMP's samples never
have (the earlier update tests do).

At H = 65, the shape named for the dropped block, that block is the single column 64, which only row 64 = H-1 reads -- the row the
reference zeroes: the fault changes no bit of the output there (asserted below), so it is planted at H = 66, where row 64 is
interior.  The GPU file's chunked cases with H in {100, 128, 129, 192, 255, 256} have interior rows behind column 63."""
import numpy as np
import pytest
import torch

import collision_kinks as K
import stomp_kernels_checks as C

F32 = np.float32


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


# ------------------------------------------------------------------------------------------------
# the kernels' loop structure in numpy fp32 (csrc/mpb_kernels.hip), with the faults
# ------------------------------------------------------------------------------------------------
def restate_sample(means, L, eps, fault=None):
    """stomp_sample_cost_hx_kernel: noise[hc] = sum_{kc <= hc} L[hc][kc] eps[kc] over 64 x 64 blocks; edge rows zeroed; + mean."""
    m, Lm, e = means.numpy(), L.numpy(), eps.permute(2, 0, 3, 1).contiguous().numpy()         # e (P, S, k, c)
    P, H, d = m.shape
    Mc = (H + 63) // 64
    noise = np.zeros((P, e.shape[1], H, d), F32)
    for hc in range(Mc):
        for kc in range(hc + 1):
            if fault == 'last_block' and kc == Mc - 1:
                continue
            rows, cols = slice(64 * hc, min(H, 64 * hc + 64)), slice(64 * kc, min(H, 64 * kc + 64))
            noise[:, :, rows] += np.einsum('hk,pskc->pshc', Lm[rows, cols], e[:, :, cols]).astype(F32)
    noise[:, :, 0] = 0
    if fault != 'edge':
        noise[:, :, H - 1] = 0
    return torch.from_numpy(m[:, None] + noise)


def restate_update(means, samples, costs, Sigma, lr, temperature, fault=None):
    """stomp_update_kernel: softmax in trips of 1024 threads; SG sample groups [sg S / SG, (sg + 1) S / SG) reduced in order and
    combined in order; mean += (lr Sigma) @ delta as an fma chain over k.  Returns (means, weights)."""
    m, x, c = means.numpy(), samples.numpy(), costs.numpy()
    P, S, H, d = x.shape
    lr = F32(lr)
    logit = (-c / F32(temperature)).astype(F32)
    seen = logit[:, :1024] if fault == 'trips' else logit
    mx = seen.max(1, keepdims=True)
    e = np.exp(seen - (0 if fault == 'nomax' else mx), dtype=F32)
    with np.errstate(invalid='ignore', divide='ignore'):
        w = np.zeros((P, S), F32)
        w[:, :seen.shape[1]] = e / e.sum(1, keepdims=True, dtype=F32)
    SG = 4 if S >= 4 else 1
    delta = np.zeros((P, H, d), F32)
    for sg in range(SG):
        s0, s1 = (sg * S) // SG, ((sg + 1) * S) // SG
        if fault == 'group_last':
            s1 = max(s0, s1 - 1)
        acc = np.zeros((P, H, d), F32)
        for s in range(s0, s1):
            acc = acc + w[:, s, None, None] * (x[:, s] - m)
        delta = acc if sg == 0 else delta + acc
    if Sigma is None:
        step = lr * delta
    else:
        sig = lr * Sigma.numpy()
        src = np.roll(delta, 1, axis=2) if (fault == 'channel' and d % 4) else delta
        step = np.zeros((P, H, d), F32)
        for k in range(H - 1 if fault == 'k_stop' else H):
            step = _fma(sig[None, :, k, None], src[:, None, k, :], step)
        if fault == 'lr_twice':
            step = lr * step
    return torch.from_numpy(m + step), torch.from_numpy(w)


def _old_norm(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max())


def _over(got, ref64, unit, E32, judged=None):
    """Number of elements over the bar (NaN counts)."""
    e = C.errors(got, ref64, unit)
    if judged is not None:
        e = torch.where(judged, e, torch.zeros_like(e))
    return int((~(e <= K.bar(E32))).sum())


# ------------------------------------------------------------------------------------------------
# conditions on the inputs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P,S,H,d', C.SAMPLE_H64 + C.SAMPLE_HX + C.SAMPLE_DRAWN)
def test_sample_inputs_meet_their_conditions(P, S, H, d):
    assert C.sample_kernel_of(H, d) == ('h64' if (P, S, H, d) in C.SAMPLE_H64 + C.SAMPLE_DRAWN[:1] else 'hx')
    for family in C.L_FAMILIES:
        pr = C.sample_problem(P, S, H, d, family)
        ref = C.sample_reference(pr.means, pr.L, pr.eps)
        assert bool((ref.unit[:, :, 1:H - 1] > 0).all()) and bool(ref.zero[:, :, 0].all()) and bool(ref.zero[:, :, H - 1].all())
        if family == 'identity':      # one rounding, the restatement's own: E32 is half an ulp of the sum at most
            assert C.same_bits(ref.x32, pr.means.unsqueeze(1) + pr.eps.permute(2, 0, 3, 1) * ~ref.zero) and ref.E32 <= 2.0 ** -24
        assert ref.E32 > 0 or family == 'identity', (family, ref.E32)      # (identity: most sums are exact, and bits decide)
        if family == 'dense' and H >= 8:      # interior rows of L span the decades: a global maximum hides the small ones
            L_rows = pr.L.abs().amax(1)[1:H - 1]
            assert float(L_rows.max() / L_rows.min()) > 1.0e3


@pytest.mark.parametrize('S,H,d', C.UPDATE_V4 + C.UPDATE_GENERIC)
def test_update_inputs_meet_their_conditions(S, H, d):
    want_v4 = (S, H, d) in C.UPDATE_V4
    assert (C.update_kernel_of(S, H, d) == 'v4') == want_v4
    assert C.update_kernel_of(*C.UPDATE_REFUSED) is None
    P = C.update_P((S, H, d))
    for family in C.COSTS:
        for kind in ('spd', 'stomp', None):
            pr = C.update_problem(P, S, H, d, family, kind)
            wr = C.weights_reference(pr.costs, pr.temperature)
            exact = bool((wr.w64.float().double() == wr.w64)[wr.judged].all())
            assert bool((wr.unit[wr.judged] > 0).all()) and (wr.E32 > 0 or exact), (family, wr.E32)
            mr = C.mean_reference(pr.means, pr.samples, wr.w32, pr.Sigma, pr.lr)
            assert bool((mr.unit > 0).all()) and mr.E32 > 0, (family, kind, mr.E32)
            if kind is not None:
                continue
            big = (wr.w64 > 1e-3).sum(1)
            if family == 'spread' and S >= 8:
                assert bool((big >= 3).all()) and bool((wr.tiny.sum(1) >= 1).all()), (big, wr.tiny.sum(1))
            if family == 'c3' and S >= 2:
                assert int((big >= 2).sum()) * 2 >= P, big
            if family == 'equal':
                assert bool((wr.w32 == wr.w32[0, 0]).all())
            if family == 'onehot':
                assert bool((big == 1).all()) and bool((wr.tiny.sum(1) == S - 1).all())
            if family == 'tied' and S >= 2:
                top = wr.w64.topk(2, dim=1)[0]
                assert bool((top[:, 0] == top[:, 1]).all())


def test_generic_cases_name_the_paths_they_claim():
    assert C.update_kernel_of(2, 5, 1) == 'generic/lds' and C.update_kernel_of(4, 128, 1) == 'generic/global'
    assert C.update_kernel_of(4, 256, 24) == 'generic/global' and C.update_kernel_of(6, 100, 12) == 'generic/lds'
    assert C.update_kernel_of(8, 6, 2) == 'generic/lds'            # n = 12, H <= 64, S <= 64: everything of v4 but H & 3
    assert C.update_kernel_of(8, 6, 2, with_sigma=False) == 'generic/none'
    assert 64 * 16 == 1024 and 60 * 7 == 420 and 420 % 64 != 0 and 100 * 12 > 1024 and 1030 > 1024


# ------------------------------------------------------------------------------------------------
# planted faults
# ------------------------------------------------------------------------------------------------
UPDATE_FAULTS = [          # fault, (S, H, d), cost family, Sigma, what the fault must move
    ('group_last', (4, 5, 3), 'flat', 'spd', 'means'),
    ('k_stop', (3, 3, 1), 'flat', 'spd', 'means'),
    ('channel', (4, 5, 3), 'flat', 'spd', 'means'),
    ('nomax', (70, 9, 2), 'c3', 'spd', 'weights'),
    ('trips', (1030, 3, 1), 'flat', 'spd', 'weights'),
    ('lr_twice', (3, 3, 1), 'flat', 'spd', 'means'),
]


@pytest.mark.parametrize('fault,shape,family,kind,moved', UPDATE_FAULTS)
def test_planted_update_fault_leaves_the_bar(fault, shape, family, kind, moved):
    pr = C.update_problem(2, *shape, family, kind)
    wr = C.weights_reference(pr.costs, pr.temperature)
    full64 = C._update(pr.means.double(), pr.samples.double(), wr.w64, pr.Sigma.double(), pr.lr)
    res = {}
    for f in (None, fault):
        m, w = restate_update(pr.means, pr.samples, pr.costs, pr.Sigma, pr.lr, pr.temperature, f)
        mr = C.mean_reference(pr.means, pr.samples, w, pr.Sigma, pr.lr)
        res[f] = (_over(w, wr.w64, wr.unit, wr.E32, wr.judged), _over(m, mr.m64, mr.unit, mr.E32), _old_norm(m, full64))
    print(f'fault {fault} at {shape}: elements over the bar (weights, means) {res[fault][:2]}, unfaulted {res[None][:2]}; '
          f'old global norm of the means {res[fault][2]:.3g} (bar 2e-6: {"passes" if res[fault][2] < 2e-6 else "fails"})')
    assert res[None][:2] == (0, 0)
    assert res[fault][0 if moved == 'weights' else 1] > 0


SAMPLE_FAULTS = [('edge', (2, 1, 3, 1)), ('last_block', (3, 1, 66, 3))]


@pytest.mark.parametrize('fault,shape', SAMPLE_FAULTS)
def test_planted_sample_fault_leaves_the_bar(fault, shape):
    for family in ('dense', 'stomp'):
        pr = C.sample_problem(*shape, family)
        ref = C.sample_reference(pr.means, pr.L, pr.eps)
        ok = restate_sample(pr.means, pr.L, pr.eps)
        bad = restate_sample(pr.means, pr.L, pr.eps, fault)
        assert _over(ok, ref.x64, ref.unit, ref.E32) == 0 and C.same_bits(ok[ref.zero], ref.carried[ref.zero])
        over, bits = _over(bad, ref.x64, ref.unit, ref.E32), C.same_bits(bad[ref.zero], ref.carried[ref.zero])
        old = _old_norm(bad, ref.x64)
        print(f'fault {fault} at {shape}, L {family}: {over} elements over the bar, edge rows carry the means: {bits}; '
              f'old global norm {old:.3g} (bar 2e-5: {"passes" if old < 2e-5 else "fails"})')
        assert over > 0 or not bits


def test_dropped_last_block_is_invisible_at_h65():
    """Column 64 of a 65-row L is read by row 64 = H-1 alone, which the reference zeroes: no test can see this fault at H = 65."""
    pr = C.sample_problem(3, 1, 65, 3, 'dense')
    assert C.same_bits(restate_sample(pr.means, pr.L, pr.eps), restate_sample(pr.means, pr.L, pr.eps, 'last_block'))


def test_unsubtracted_maximum_is_invisible_on_flat_costs():
    """exp(x) / sum exp(x) without the maximum is the same softmax to rounding while x stays small: only the C3-like family sees it."""
    pr = C.update_problem(2, 70, 9, 2, 'flat', 'spd')
    wr = C.weights_reference(pr.costs, pr.temperature)
    _, w = restate_update(pr.means, pr.samples, pr.costs, pr.Sigma, pr.lr, pr.temperature, 'nomax')
    assert _over(w, wr.w64, wr.unit, wr.E32, wr.judged) == 0
