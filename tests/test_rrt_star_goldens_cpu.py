"""RRT* / informed RRT* without a GPU: the goldens of the unmodified reference (tests/golden/make_rrt_star_goldens.py)
pass the structural checker and their own screen and cover what they must, the checker bites, and the host side of the
new C-ABI entries answers."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden, ref_geometry_from_golden
from rrt_star_checks import check_rrt_star_result, golden_star_problem

SCENES_2D = ('rrt_star_pm2d_grid', 'rrt_star_pm2d_grid_inf', 'rrt_star_pm2d_dense', 'rrt_star_pm2d_dense_inf')
SCENES = SCENES_2D + ('rrt_star_panda_spheres',)


def _scene(name):
    g = load_golden(name)
    robot, field = ref_geometry_from_golden(g, torch.float64)
    return g, robot, field


def _tolerances(g):
    f = float(g['factor'])
    return dict(slack=f * float(g['E_gap']), e_dist=f * float(g['E_dist']), e_cost=f * float(g['E_cost']))


@pytest.mark.parametrize('name', SCENES)
def test_every_golden_passes_the_checker(name):
    from motion_planning_baselines_amd import ops
    g, robot, field = _scene(name)
    assert int(g['n_problems']) >= 8
    assert int(g['n_iters']) == 400 and int(g['n_iters_after_success']) == 150
    for k in range(int(g['n_problems'])):
        check_rrt_star_result(robot, field, *golden_star_problem(g, k), float(g['step_size']), float(g['n_radius']), **_tolerances(g))
        assert int(g['stop_reason'][k]) in (ops.RRT_STOP_ITERS, ops.RRT_STOP_AFTER_SUCCESS) and int(g['n_iterations'][k]) <= 401


@pytest.mark.parametrize('name', SCENES)
def test_every_stored_margin_clears_the_screen(name):
    g = load_golden(name)
    f = float(g['factor'])
    assert f == 32.0
    m = g['margins']                          # hinge, argmin, count, radius, rewire, nbr, informed, best, eps
    assert m.shape == (int(g['n_problems']), 9)
    assert (m[:, 0] >= f * float(g['E_gap'])).all()
    assert (m[:, [1, 2, 3, 5]] >= f * float(g['E_dist'])).all()
    assert (m[:, [4, 6, 7]] >= f * float(g['E_cost'])).all()
    assert (m[:, 8] >= f * float(g['E_eps'])).all()
    for e in ('E_gap', 'E_dist', 'E_cost'):
        assert 0.0 < float(g[e]) < 1e-5, e                       # fp32 rounding of O(1) quantities
    assert 2.0 ** -23 <= float(g['E_eps']) < 1e-5 and float(g['E_eps']) >= float(g['E_eps_measured'])
    assert int(g['n_eligible']) <= int(g['n_candidates']) and int(g['n_screened']) <= int(g['n_eligible'])
    assert bool(g['informed']) == name.endswith('_inf')
    assert np.isfinite(m[:, 6]).any() == bool(g['informed'])    # the informed test was taken iff the scene is informed


@pytest.mark.parametrize('name', SCENES)
def test_goldens_cover_what_they_must(name):
    g = load_golden(name)
    assert g['cov_rewire_with_children'].sum() > 0              # a rewire of a node that has children
    assert (g['rewires'] > 0).any()
    if name in SCENES_2D:
        assert g['cov_goal_cost_drops'].sum() > 0               # a rewire that lowers the goal's cost after the first success
        assert g['cov_rejected_edges'].sum() > 0                # an edge rejected by collision during rewiring
        assert g['cov_duplicates'].sum() > 0                    # a duplicate-node extension
        assert (g['informed_rejections'].sum() > 0) == bool(g['informed'])
    # the structural ties the one-distance-routine rule is there for occur in the stored problems
    if name in SCENES_2D:
        assert g['structural_ties'].sum() > 0


@pytest.mark.parametrize('name', ('rrt_star_pm2d_grid', 'rrt_star_panda_spheres'))
def test_the_checker_bites(name):
    g, robot, field = _scene(name)
    args = (float(g['step_size']), float(g['n_radius']))
    tol = _tolerances(g)
    k = int(np.argmax([len(g[f'p{i}_path']) for i in range(int(g['n_problems']))]))
    start, goal, nodes, parents, d, cost, goal_idx, path = golden_star_problem(g, k)
    assert len(path) > 2
    check_rrt_star_result(robot, field, start, goal, nodes, parents, d, cost, goal_idx, path, *args, **tol)
    # a forged cost
    bad = cost.copy()
    bad[goal_idx] *= 0.9
    with pytest.raises(AssertionError, match=r'differs from cost\[parent\] \+ d'):
        check_rrt_star_result(robot, field, start, goal, nodes, parents, d, bad, goal_idx, path, *args, **tol)
    # a cycle: the goal's parent hangs below the goal
    par = parents.copy()
    par[parents[goal_idx]] = goal_idx
    with pytest.raises(AssertionError, match='cycle'):
        check_rrt_star_result(robot, field, start, goal, nodes, par, d, cost, goal_idx, path, *args, **tol)
    # an edge through an obstacle: a node moved across an obstacle from its parent keeps its distance but not its free edge
    if int(g['robot_kind']) == 0:
        from rrt_checks import hinge_argument
        centre, radius = g['spheres'][0, :2].astype(np.float64), float(g['spheres'][0, 3])
        reach = radius + float(g['margin']) + 0.02
        assert 2 * reach <= float(g['n_radius'])
        qn, par = nodes.copy(), parents.copy()
        qn = np.concatenate((qn, [centre - [reach, 0.0], centre + [reach, 0.0]])).astype(np.float32)
        assert hinge_argument(robot, field, qn[-2:]).max() < 0
        far = int(np.argmin(np.linalg.norm(nodes - qn[-2], axis=1)))
        par = np.concatenate((par, [far, len(nodes)]))
        dd = np.concatenate((d, [np.linalg.norm(qn[-2] - nodes[far]), np.linalg.norm(qn[-1] - qn[-2])])).astype(np.float32)
        cc = np.concatenate((cost, [cost[far] + dd[-2], cost[far] + dd[-2] + dd[-1]])).astype(np.float32)
        with pytest.raises(AssertionError, match='edge|n_radius'):
            check_rrt_star_result(robot, field, start, goal, qn, par, dd, cc, goal_idx, path, *args, **tol)
    # a truncated path
    with pytest.raises(AssertionError, match='retrace'):
        check_rrt_star_result(robot, field, start, goal, nodes, parents, d, cost, goal_idx, path[:-1], *args, **tol)


def test_library_exports_the_rrt_star_symbols():
    from motion_planning_baselines_amd import _lib
    h = _lib.lib()
    for name in ('mpb_rrt_star_workspace_bytes', 'mpb_rrt_star_init', 'mpb_rrt_star_run'):
        assert hasattr(h, name) and name in _lib.SIGNATURES
    assert (h.mpb_version() & 0xFFFF) == _lib.ABI_VERSION == 7


def test_workspace_bytes_is_monotone():
    from motion_planning_baselines_amd import _lib
    f = _lib.lib().mpb_rrt_star_workspace_bytes
    base = dict(B=4, max_nodes=100, n_pre=1000, D=7)
    b0 = f(*base.values())
    assert b0 > 0 and b0 % 16 == 0
    for key, bigger in (('B', 5), ('max_nodes', 101), ('n_pre', 1002), ('D', 9)):
        assert f(*{**base, key: bigger}.values()) > b0, key
    assert f(4, 100, 1000, 8) >= b0                           # (D is padded to a multiple of 4: 7 and 8 tie)
    # per node: the padded configuration, parent, d, cost and three words of neighbour scratch; plus the uint16 pool list
    assert b0 >= 4 * (4 * 100 * (8 + 1 + 1 + 1 + 3)) + 2 * 4 * 1000


def _run_args(h, null, n_pre=1000, D=7, ws=None, nbytes=0, ptr=None, idx=None, draw=None, Lmax=64, step=0.1):
    p = null if ptr is None else ptr
    return h.mpb_rrt_star_run(null if ws is None else ws, nbytes, p, 0, p, 0, null if idx is None else idx,
                              null if draw is None else draw, p, p, p, p, 4, 100, n_pre, D, Lmax, 0, 1, 401, 1000, 150, 0,
                              step, 0.3, 0.1, 1e-2, 1e-6, 0, 0, null)


def test_refusals_return_the_right_code_and_message():
    from motion_planning_baselines_amd import _lib
    h = _lib.lib()
    null = ctypes.c_void_p(0)
    INVALID, UNSUPPORTED = 1, 2                                # include/mpb.h MPB_E_*
    for n_pre, D, word in ((16385, 7, 'n_pre'), (1000, 13, 'MPB_MAX_DOF')):
        assert h.mpb_rrt_star_workspace_bytes(4, 100, n_pre, D) == 0
        assert word in h.mpb_last_error().decode()
        assert h.mpb_rrt_star_init(null, 0, null, null, null, 0, 4, 100, n_pre, D, null) == UNSUPPORTED
        assert word in h.mpb_last_error().decode()
        assert _run_args(h, null, n_pre=n_pre, D=D) == UNSUPPORTED and word in h.mpb_last_error().decode()
    assert h.mpb_rrt_star_workspace_bytes(1 << 20, 1 << 20, 1000, 7) == 0 and 'too large' in h.mpb_last_error().decode()
    # valid shapes: null pointers, a short workspace, one of the two draw arrays without the other, a bad step
    assert h.mpb_rrt_star_init(null, 0, null, null, null, 0, 4, 100, 1000, 7, null) == INVALID
    assert 'null pointer' in h.mpb_last_error().decode()
    assert _run_args(h, null) == INVALID and 'null pointer' in h.mpb_last_error().decode()
    buf = (ctypes.c_float * 64)()                              # a host buffer: every call below is refused before any launch
    ptr = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    assert h.mpb_rrt_star_init(ptr, 64, ptr, ptr, ptr, 0, 4, 100, 1000, 7, null) == INVALID
    assert 'needed' in h.mpb_last_error().decode()
    assert _run_args(h, null, ws=ptr, nbytes=64, ptr=ptr, idx=ptr) == INVALID and 'together' in h.mpb_last_error().decode()
    assert _run_args(h, null, ws=ptr, nbytes=64, ptr=ptr) == INVALID and 'needed' in h.mpb_last_error().decode()
    assert _run_args(h, null, ws=ptr, nbytes=1 << 30, ptr=ptr, Lmax=1) == INVALID and 'Lmax' in h.mpb_last_error().decode()
    assert _run_args(h, null, ws=ptr, nbytes=1 << 30, ptr=ptr, step=0.0) == INVALID and 'step_size' in h.mpb_last_error().decode()


def test_planner_refusals_need_no_gpu():
    """n_knn > 0, n_iters < 2 and a non-GPU device are refused in Python before anything is launched."""
    from motion_planning_baselines_amd._lib import MPBError
    from motion_planning_baselines_amd.planners import InfRRTStar, RRTStar
    z = torch.zeros(2)
    with pytest.raises(MPBError, match='no CPU fallback'):
        RRTStar(task=None, n_iters=10, start_state_pos=z, goal_state_pos=z, tensor_args=dict(device='cpu'))
    for cls in (RRTStar, InfRRTStar):
        with pytest.raises(ValueError, match='n_knn'):
            cls(task=None, n_iters=10, start_state_pos=z, goal_state_pos=z, n_knn=3, tensor_args=dict(device='cpu'))
        with pytest.raises(ValueError, match='n_iters'):
            cls(task=None, n_iters=1, start_state_pos=z, goal_state_pos=z, tensor_args=dict(device='cpu'))
    assert issubclass(InfRRTStar, RRTStar)
    from motion_planning_baselines_amd.planners.multi_sample_based_planner import MultiSampleBasedPlanner
    with pytest.raises(TypeError, match='RRTConnect, RRTStar or InfRRTStar'):
        MultiSampleBasedPlanner(object())
