"""CPU: the conditions tests/test_gpu_chomp_step_elements.py relies on, from the oracle alone (tests/chomp_step_checks.py).

Per case: the kink classifier excludes at most K.CAP of the waypoints in contact and leaves at least 100 conditioned ones; a clipped
case leaves at most 1 % of its interior elements undecided and clamps a real share of the rest; the fp64 step moves a position
channel -- and a velocity channel where the prior acts on one -- while rows 0 and H-1 keep their bits; the fp32 oracle's own error
E32 in the per-element unit is finite and near rounding (the unit is the right size).  E32 is printed per case."""
import pytest
import torch

import chomp_step_checks as C
import collision_kinks as K

ORACLE_CASES = sorted({(c[1], c[3], c[4]) for c in C.STEP_CASES})


def _common(ref, tag):
    bs = ref.base
    print(f'{tag}: {bs.n_contact} waypoints in contact, {bs.share * 100:.2f} % of them excluded, judged {int(ref.judged.sum())} of '
          f'{int(ref.interior.sum())} interior elements, E32 {ref.E32:.3e}, cost E32 {ref.cost_E32:.3e} on {int(ref.cost_ok.sum())} particles')
    assert bs.share <= K.CAP and bs.n_conditioned_contact >= 100, (bs.share, bs.n_conditioned_contact)
    assert torch.isfinite(ref.x64).all() and torch.isfinite(ref.x32).all()
    assert ref.E32 == ref.E32 and ref.E32 < 1e-4                       # finite, and the unit is the right size
    assert int(ref.judged.sum()) > 0
    step = ref.x64 - ref.x0.double()
    assert float(step[:, 1:-1, :ref.D].abs().max()) > 0
    if ref.d > ref.D:
        if ref.w_prior != 0.0:
            assert float(step[:, 1:-1, ref.D:].abs().max()) > 0
        else:
            assert float(step[..., ref.D:].abs().max()) == 0.0
    for x in (ref.x64, ref.x32):
        assert torch.equal(x[:, 0], ref.x0[:, 0].to(x.dtype)) and torch.equal(x[:, -1], ref.x0[:, -1].to(x.dtype))
    assert bool(ref.zero[:, 0].all()) and bool(ref.zero[:, -1].all())
    assert bool(((ref.x64 == ref.x0.double()) | ~ref.zero).all())         # a zero unit never hides a move of the oracle's


@pytest.mark.parametrize('family', C.FAMILIES)
@pytest.mark.parametrize('name,H,dmul', ORACLE_CASES)
def test_unclipped_conditions(name, H, dmul, family):
    ref = C.reference(name, H, dmul, family)
    _common(ref, f'{name} H={H} d={dmul}D {family}')
    if family == 'prior':
        assert bool((ref.judged == (ref.interior & (ref.unit > 0))).all()) and int(ref.judged.sum()) == int(ref.interior.sum())
    else:
        assert float(ref.c64.max()) > 0 and ref.cost_E32 < 1e-4


@pytest.mark.parametrize('case', C.CLIPPED)
def test_clipped_conditions(case):
    _, name, _, H, dmul, _, _ = C.CASE[case]
    clip = C.pick_clip(name, H, dmul)
    ref = C.reference(name, H, dmul, 'both', clip)
    _common(ref, f'{name} H={H} d={dmul}D clip={clip}')
    print(f'    clip {clip}: {ref.clamped_share * 100:.1f} % of the interior elements clamped, {ref.undecided_share * 100:.3f} % undecided')
    assert ref.undecided_share <= C.UNDECIDED_CAP
    assert 0.2 <= ref.clamped_share <= 0.8
    assert int(ref.clamped.sum()) > 100 and int(ref.judged.sum()) > 100
    # the oracle's own clamped elements are the exact step
    assert C.same_bits(ref.x32[ref.clamped], ref.want_clamped[ref.clamped])
    moved = (ref.x64 - ref.x0.double())[ref.clamped]
    assert bool((moved.abs() == C.LR * clip).all())


@pytest.mark.parametrize('case', C.SHARDED)
def test_shard_conditions(case):
    _, name, _, H, dmul, _, _ = C.CASE[case]
    ref = C.reference(name, H, dmul, 'both', None, C.SHARD)
    _common(ref, f'{name} H={H} d={dmul}D B_global={ref.B_global}')
    whole = C.reference(name, H, dmul, 'both')
    assert float((ref.x64 - whole.x64).abs().max()) > 0                  # the shard's scaling is visible


@pytest.mark.parametrize('H,dmul,clipped', C.COMPOSITE_CASES)
def test_composite_conditions(H, dmul, clipped):
    ref = C.composite_reference(H, dmul, clipped)
    print(f'composite H={H} d={dmul}D clip={ref.grad_clip}: E32 {ref.E32:.3e}, undecided {ref.undecided_share * 100:.3f} %')
    assert ref.E32 == ref.E32 and ref.E32 < 1e-4
    assert torch.equal(ref.x64[:, 0], ref.x0[:, 0].double()) and torch.equal(ref.x64[:, -1], ref.x0[:, -1].double())
    if clipped:
        assert ref.undecided_share <= C.UNDECIDED_CAP and 0.2 <= ref.clamped_share <= 0.8
        assert C.same_bits(ref.x32[ref.clamped], ref.want_clamped[ref.clamped])


def test_new_scenes_fill_the_quad_slots_partially():
    for name, (n_sph, n_box, dim) in dict(point3d_13s5b=(13, 5, 3), point2d_8b=(0, 8, 2), point2d_30s=(30, 0, 2)).items():
        robot, (field,), _ = C.scene(name)
        assert (len(field.spheres), len(field.boxes), robot.q_dim) == (n_sph, n_box, dim)
        assert n_sph <= 32 and n_box <= 8 and (n_sph < 32 or n_box < 8)
