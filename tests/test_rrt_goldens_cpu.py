"""RRT-Connect without a GPU: the goldens of the unmodified reference (tests/golden/make_rrt_goldens.py) pass the
structural checker and their own screen, the checker bites, and the host side of the new C-ABI entries answers."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden, ref_geometry_from_golden
from rrt_checks import check_rrt_result, golden_problem

SCENES = ('rrt_pm2d_grid', 'rrt_pm2d_dense', 'rrt_panda_spheres')


def _scene(name):
    g = load_golden(name)
    robot, field = ref_geometry_from_golden(g, torch.float64)
    return g, robot, field


@pytest.mark.parametrize('name', SCENES)
def test_every_golden_passes_the_checker(name):
    g, robot, field = _scene(name)
    assert int(g['n_problems']) >= 8
    for k in range(int(g['n_problems'])):
        start, goal, trees, path = golden_problem(g, k)
        check_rrt_result(robot, field, start, goal, trees, path, float(g['step_size']), float(g['n_radius']),
                         slack=float(g['factor']) * float(g['E_gap']))


@pytest.mark.parametrize('name', SCENES)
def test_every_stored_margin_clears_the_screen(name):
    g = load_golden(name)
    assert float(g['factor']) == 32.0
    m = g['margins']                                             # hinge, argmin, count, radius
    assert m.shape == (int(g['n_problems']), 4)
    assert (m[:, 0] >= 32.0 * float(g['E_gap'])).all()
    assert (m[:, 1:] >= 32.0 * float(g['E_dist'])).all()
    assert 0.0 < float(g['E_gap']) < 1e-5 and 0.0 < float(g['E_dist']) < 1e-5      # fp32 rounding of O(1) quantities
    assert int(g['n_eligible']) <= int(g['n_candidates']) and int(g['n_screened']) <= int(g['n_eligible'])


@pytest.mark.parametrize('name', SCENES)
def test_the_checker_bites(name):
    g, robot, field = _scene(name)
    start, goal, trees, path = golden_problem(g, 0)
    args = (float(g['step_size']), float(g['n_radius']), float(g['factor']) * float(g['E_gap']))
    # a node pushed into an obstacle: the centre of the first obstacle sphere (point robot), or the configuration
    # whose hinge argument is largest among many draws (arm)
    t = 0 if len(trees[0][0]) > 1 else 1
    nodes = trees[t][0].copy()
    if int(g['robot_kind']) == 0:
        nodes[-1] = g['spheres'][0, :nodes.shape[1]]
    else:
        from rrt_checks import hinge_argument
        q = np.random.RandomState(0).uniform(-2.5, 2.5, size=(4000, nodes.shape[1]))
        h = hinge_argument(robot, field, q)
        assert h.max() > 1e-3
        nodes[-1] = q[h.argmax()]
    bad = list(trees)
    bad[t] = (nodes, trees[t][1])
    with pytest.raises(AssertionError, match='in collision|n_radius'):
        check_rrt_result(robot, field, start, goal, tuple(bad), None, *args)
    # a parent pointing forward
    parents = trees[t][1].copy()
    parents[1] = len(parents) - 1 if len(parents) > 2 else 1
    bad[t] = (trees[t][0], parents)
    with pytest.raises(AssertionError, match='precede'):
        check_rrt_result(robot, field, start, goal, tuple(bad), None, *args)
    # a path that does not reach the goal
    with pytest.raises(AssertionError, match='join'):
        check_rrt_result(robot, field, start, goal, trees, path[:-1], *args)


def test_library_exports_the_rrt_symbols():
    from motion_planning_baselines_amd import _lib
    h = _lib.lib()
    for name in ('mpb_rrt_connect_workspace_bytes', 'mpb_rrt_connect_init', 'mpb_rrt_connect_run', 'mpb_collision_check'):
        assert hasattr(h, name) and name in _lib.SIGNATURES
    assert (h.mpb_version() & 0xFFFF) == _lib.ABI_VERSION == 7


def test_workspace_bytes_is_monotone():
    from motion_planning_baselines_amd import _lib
    f = _lib.lib().mpb_rrt_connect_workspace_bytes
    base = dict(B=4, max_nodes=100, n_pre=1000, D=7)
    b0 = f(*base.values())
    assert b0 > 0 and b0 % 4 == 0
    for key, bigger in (('B', 5), ('max_nodes', 101), ('n_pre', 1002), ('D', 9)):
        assert f(*{**base, key: bigger}.values()) > b0, key
    assert f(4, 100, 1000, 8) >= b0                           # (D is padded to a multiple of 4: 7 and 8 tie)
    # trees (configurations padded to float4 + a parent each) and the uint16 pool list are what it has to hold
    assert b0 >= 4 * (4 * 2 * 100 * (8 + 1)) + 2 * 4 * 1000


def test_shapes_beyond_the_kernel_are_refused_with_a_message():
    from motion_planning_baselines_amd import _lib
    h = _lib.lib()
    null = ctypes.c_void_p(0)
    UNSUPPORTED = 2                                            # include/mpb.h MPB_E_UNSUPPORTED
    for n_pre, D, word in ((16385, 7, 'n_pre'), (1000, 13, 'MPB_MAX_DOF')):
        assert h.mpb_rrt_connect_workspace_bytes(4, 100, n_pre, D) == 0
        assert word in h.mpb_last_error().decode()
        rc = h.mpb_rrt_connect_init(null, 0, null, null, null, 0, 4, 100, n_pre, D, null)
        assert rc == UNSUPPORTED and word in h.mpb_last_error().decode()
        rc = h.mpb_rrt_connect_run(null, 0, null, 0, null, 0, null, null, null, null, 4, 100, n_pre, D, 64, 0, 1, 1, 0.1, 0.3, 0, 0, null)
        assert rc == UNSUPPORTED and word in h.mpb_last_error().decode()
    assert h.mpb_collision_check(null, null, 0, null, null, 10, 13, null) == UNSUPPORTED
    assert 'MPB_MAX_DOF' in h.mpb_last_error().decode()
    # valid shapes, null pointers / a workspace that is too small: MPB_E_INVALID
    assert h.mpb_rrt_connect_init(null, 0, null, null, null, 0, 4, 100, 1000, 7, null) == 1
    assert h.mpb_collision_check(null, null, 0, null, null, 10, 7, null) == 1
