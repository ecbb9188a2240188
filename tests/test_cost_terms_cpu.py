"""CPU: the conditions tests/test_gpu_cost_terms_elements.py relies on, from the oracle alone (tests/cost_terms_checks.py).

Per case and configuration: the helper's fp64 closed form, rounded once to fp32, meets the bar against fp64 autograd through the
oracle (the oracle stays inside its own condition, and the closed form the unit is read from is the oracle's gradient); every enabled
term is active with a non-zero contribution where the GPU test needs it (both joint-limit sides, every goal, row 0, row H-1, a row
>= 64 where H allows); the unit is positive wherever the fp64 gradient is non-zero.  Then the argument that the per-element bar can
fail where a global norm could not: three planted faults in the restated arithmetic each break it."""
import pytest
import torch

import chomp_step_checks as C
import cost_terms_checks as T


@pytest.mark.parametrize('case', T.CASES, ids=T.case_id)
def test_oracle_meets_its_own_bar(case):
    p = T.problem(*case)
    for name, (terms, fd, dmul) in T.CONFIGS.items():
        for jl_mul in ((1, T.SHARD) if 'jlim' in terms else (1,)):
            ref = T.reference(p, name, jl_mul)
            want, bar = T.grad_bar(ref)
            r = T.ratio(ref.g_closed.float(), want, bar)
            print(f'{T.case_id(case)} {name} jl_scale={ref.jl_scale:g}: judged {ref.g64.numel()} elements ({int(ref.zero.sum())} exact '
                  f'zeros), closed form rounded to fp32: worst error / bar {float(r.max()):.3f}')
            assert torch.isfinite(ref.g64).all() and torch.isfinite(ref.unit).all()
            assert float(r.max()) <= 1.0
            # the unit is positive wherever the gradient is non-zero; a zero unit is an exact zero on both sides
            assert bool((ref.unit[ref.g64 != 0] > 0).all())
            assert bool((ref.g64[ref.zero] == 0).all()) and bool((ref.g_closed[ref.zero] == 0).all())
            assert float(ref.g64.abs().max()) > 0
            # costs: positive unit, finite, non-zero
            assert bool((ref.cost_unit * (1 + 2.0 ** -40) >= ref.c64.abs()).all())
            if set(terms) - {'jlim'}:
                assert bool((ref.c64 > 0).all())
            if 'jlim' in terms:
                assert ref.jl64 > 0


@pytest.mark.parametrize('case', T.CASES, ids=T.case_id)
def test_every_term_is_active(case):
    B, H, D = case
    p = T.problem(*case)
    rows = [0, H - 1] + ([64] if H > 64 else [])
    assert set(rows) <= set(T.pushed_rows(H))
    # joint limits: both sides, on row 0, row H-1 and a row of the second lane trip
    pos = p.x[..., :D].double()
    lo, hi = p.q_min.double() + T.EPS - pos, pos - (p.q_max.double() - T.EPS)
    assert torch.isfinite(p.q_min).all() and torch.isfinite(p.q_max).all()
    for r in rows:
        assert bool((hi[:, r] > 0).any()) and (bool((lo[:, r] > 0).any()) or B == 1 and D == 1), r
    assert bool((lo > 0).any()) and bool((hi > 0).any())
    for name in ('gp', 'start', 'goal', 'smooth', 'jlim', 'gp-fd', 'smooth-pos', 'jlim-pos'):
        g = T.reference(p, name).g64
        if name == 'start':
            assert bool((g[:, 0] != 0).all()) and bool((g[:, 1:] == 0).all())
        elif name == 'goal':
            assert bool((g[:, -1] != 0).all()) and bool((g[:, :-1] == 0).all())
            assert p.G == (B + T.TPG - 1) // T.TPG                       # every goal owns a trajectory
            assert len({tuple(p.goals[i].tolist()) for i in range(p.G)}) == p.G
        elif name.startswith('jlim'):
            assert bool((g[..., D:] == 0).all())
            for r in rows:
                assert float(g[:, r].max()) > 0 and (float(g[:, r].min()) < 0 or B == 1 and D == 1)
        else:                                                            # gp, smooth: every row, every channel
            for r in rows:
                assert bool((g[:, r] != 0).any(0).all()), (name, r)
    if H > 2:
        assert float(T.reference(p, 'gp-fd').V64.abs().max()) > 0


FAULTS = {'pull_self': ('gp+smooth+jlim-fd', 'gp+smooth+jlim-fd'), 'no_last_smooth': ('smooth', 'all'), 'goal_mod': ('goal', 'all')}


@pytest.mark.parametrize('fault', list(FAULTS))
def test_planted_faults_break_the_bar(fault):
    """The kernel's arithmetic restated in fp64 with one fault planted: at H = 3 and H = 65 with the fault's own term, and with every
    term on that the fault's route admits (all five; under VEL_FD: gp, smooth, jlim), at least one element leaves the bar."""
    own, everything = FAULTS[fault]
    for case, name in (((21, 3, 7), own), ((21, 65, 7), own), ((21, 65, 7), everything), ((5, 3, 7), everything)):
        p = T.problem(*case)
        ref = T.reference(p, name)
        terms, fd, dmul = T.CONFIGS[name]
        want, bar = T.grad_bar(ref)
        g, _ = T.closed_form(p, terms, fd, dmul, ref.jl_scale, fault=fault)
        r = T.ratio(g.float(), want, bar)
        n_bad = int((r > 1.0).sum())
        ok, _ = T.closed_form(p, terms, fd, dmul, ref.jl_scale)
        assert float(T.ratio(ok.float(), want, bar).max()) <= 1.0
        # what the global norm of test_gpu_chomp_composite.py sees of the same fault
        glob = float((g - want).abs().max() / want.abs().max())
        print(f'{fault} {T.case_id(case)} {name}: caught on {n_bad} elements, worst error / bar {float(r.max()):.3e}; '
              f'max|a-b| / max|b| = {glob:.3e}')
        assert n_bad >= 1


@pytest.mark.parametrize('H,dmul,clipped', C.COMPOSITE_TERM_CASES)
def test_step_with_terms_conditions(H, dmul, clipped):
    """The step with the terms on (chomp_step_checks.composite_reference extended): the terms dominate the incoming gradient, the
    clamp splits the interior, at most 1 % of it is undecided, rows 0 and H-1 keep their bits; without terms the reference is
    the one tests/test_gpu_chomp_step_elements.py uses, untouched."""
    ref = C.composite_reference(H, dmul, clipped, C.COMPOSITE_TERMS[dmul])
    tref = ref.tref
    print(f'step + {C.COMPOSITE_TERMS[dmul]} H={H} d={ref.d} clip={ref.grad_clip}: E32 {ref.E32:.3e}, undecided {ref.undecided_share * 100:.3f} %, '
          f'median |g_terms64| / median |grad_in| = {float(tref.g64.abs().median() / ref.grad_in.abs().median()):.3g}')
    assert ref.E32 == ref.E32 and 0 < ref.E32 < 1.0 and torch.isfinite(ref.x64).all()
    assert torch.equal(ref.x64[:, 0], ref.x0[:, 0].double()) and torch.equal(ref.x64[:, -1], ref.x0[:, -1].double())
    assert float(tref.g64[:, 1:-1].abs().min(0).values.max()) > 0 and tref.jl64 > 0
    pos = ref.x0[..., :ref.D]
    assert bool((pos < tref.p.q_min).any()) and bool((pos > tref.p.q_max).any())
    if dmul == 1:
        assert tref.fd and float(tref.vterm.max()) > 0
    if clipped:
        assert ref.undecided_share <= C.UNDECIDED_CAP and 0.2 <= ref.clamped_share <= 0.8
        assert C.same_bits(ref.x32[ref.clamped], ref.want_clamped[ref.clamped])
    if H in (37, 150):
        plain = C.composite_reference(H, dmul, clipped)
        assert plain.terms is None and torch.equal(plain.grad_in, ref.grad_in) and not torch.equal(plain.x64, ref.x64)
