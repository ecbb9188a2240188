"""CPU: the kink classifier of tests/collision_kinks.py on the scenes tests/test_gpu_collision_grad_elements.py judges kernels on.

Per scene and horizon used there: the share of waypoints in contact that the classifier excludes stays under the cap (3 %),
enough conditioned waypoints in contact are left to judge, and on those the fp32 ORACLE's autograd gradient is within a bound
an fp32 evaluation owes the fp64 one off the kinks -- i.e. the classifier removes what fp32 cannot decide, and nothing else
is allowed to hide behind it.

The bound on the fp32 oracle (e in the bar's units: max_j |g32 - g64| per active sphere): a conditioned active sphere is at
least RHO from what its direction is measured against (a sphere's centre, a box's edge) or has an axis direction, so a position
error p turns the unit direction by at most p / RHO; p <= DELTA / 4 is what the GPU test asserts of fp32 forward kinematics;
the Jacobian's own rounding (<= 16 joints' worth of ulps on a reach of 1.2 m) adds 16 * 2^-23 * 1.2 on lever arms of at most
1.2 m.  Together E_DECIDE = 1.2 * DELTA / (4 * RHO) + 16 * 2^-23 * 1.2 * 1.2 ~ 3.0e-4 -- a hundred times below what ONE
sphere on the wrong side of a kink costs a Panda waypoint (a unit force on a lever arm of ~0.3 m over at most 31 spheres ~ 1e-2).
The measured values are printed; they sit near 5e-7."""
import pytest
import torch

import collision_kinks as K

E_DECIDE = 1.2 * K.DELTA / (4 * K.RHO) + 16 * 2.0 ** -23 * 1.2 * 1.2

# (scene, H) pairs the GPU file uses
CASES = [(name, 64) for name in K.SCENES] + [
    ('point3d', 150), ('point2d_56', 37), ('panda_s3d', 37), ('panda_s3d', 150), ('panda_many', 37), ('arm5', 37),
    ('panda_boxes_only', 150)]


@pytest.mark.parametrize('name,H', CASES)
def test_cap_and_fp32_oracle_on_conditioned_waypoints(name, H):
    ref = K.reference(name, H)
    n, nc, share = K.excluded_share(ref.cl)
    cond = ref.cl.conditioned
    e32 = float(ref.e32[cond].max())
    print(f'{name} H={H}: {n} of {cond.numel()} waypoints in contact, {share * 100:.2f} % of them excluded, '
          f'fp32 oracle max e on conditioned waypoints {e32:.2e}')
    assert share <= K.CAP, (name, H, share)
    assert nc >= 100, (name, H, nc)
    assert e32 <= E_DECIDE, (name, H, e32)
    assert e32 <= K.bar(ref.E32)
    assert torch.isfinite(ref.g32).all() and torch.isfinite(ref.g64).all()


def _field(spheres=None, boxes=None, margin=0.25, radius=0.25):
    from oracle.geometry_ref import RefCollisionField
    import numpy as np
    spec = dict(spheres=np.zeros((0, 4)) if spheres is None else np.asarray(spheres, np.float64),
                boxes=np.zeros((0, 6)) if boxes is None else np.asarray(boxes, np.float64), margin=margin)
    return RefCollisionField(spec, np.array([radius]), tensor_args=K.F64)


def _one(field, p):
    return K.classify_points(field, torch.tensor([[p]], dtype=torch.float64))


def test_hand_made_kinks_are_flagged():
    """Exactly representable points on each kind of kink, and one plain point beside each that is not."""
    two = _field(spheres=[[-0.5, 0, 0, 0.25], [0.5, 0, 0, 0.25]])
    box = _field(boxes=[[0, 0, 0, 0.5, 0.5, 0.5]])
    # hinge boundary: sd = 0.5 = margin + r
    sph = _field(spheres=[[0, 0, 0, 0.5]])
    c = _one(sph, [1.0, 0, 0])
    assert float(c.a) == 0.0 and bool(c.kink) and not bool(c.conditioned)
    c = _one(sph, [0.75, 0, 0])
    assert bool(c.active) and not bool(c.kink) and int(c.kind) == K.KIND_SPHERE and int(c.n_active) == 1
    assert torch.equal(c.direction, torch.tensor([[[1.0, 0, 0]]], dtype=torch.float64))
    assert not bool(_one(sph, [2.0, 0, 0]).kink)                       # far outside: inactive and decided
    # bisector of two spheres
    c = _one(two, [0.0, 0.125, 0])
    assert bool(c.active) and float(c.sd_second) == float(c.sd_min) and bool(c.kink) and int(c.index) == 0
    c = _one(two, [0.125, 0.125, 0])
    assert not bool(c.kink) and int(c.index) == 1
    # a box's inner diagonal (ax == ay > az), and off it
    c = _one(box, [0.25, 0.25, 0.0])
    assert bool(c.active) and int(c.kind) == K.KIND_BOX and bool(c.kink)
    c = _one(box, [0.25, 0.125, 0.0])
    assert not bool(c.kink) and torch.equal(c.direction, torch.tensor([[[1.0, 0, 0]]], dtype=torch.float64))
    # outside a box beside an edge (direction q / |q| with a tiny |q|), and in front of a face
    assert bool(_one(box, [0.501, 0.501, 0.0]).kink)
    assert not bool(_one(box, [0.625, 0.25, 0.0]).kink)
    # a sphere's centre
    c = _one(sph, [0.0, 0, 0])
    assert bool(c.active) and bool(c.kink) and float(c.direction.abs().max()) == 0.0
    # two chained fields: conditioned only when conditioned in both
    from oracle.geometry_ref import RefRobot
    import numpy as np
    robot = RefRobot(dict(kind=0, n_dof=3, joint_tf=np.zeros((0, 3, 4)), link_frame=np.zeros(1, np.int32),
                          link_offset=np.zeros((1, 3)), link_radius=np.array([0.25])), tensor_args=K.F64)
    q = torch.tensor([[0.75, 0, 0], [1.0, 0, 0]], dtype=torch.float64)
    both = K.classify(robot, [sph, _field(spheres=[[0, 0, 0, 0.25]])], q)          # the second field's boundary is at 0.75
    assert both.conditioned.tolist() == [False, False] and both.n_active.tolist() == [[1, 0], [0, 0]]
    assert K.classify(robot, sph, q).conditioned.tolist() == [True, False]
