"""Batched path shortcutting on the GPU (csrc/mpb_path_shortcut.hip) against the definition restated on the CPU
(tests/path_shortcut_checks.py): the kernel's log held to the fp64 oracle wherever fp64 can decide, its paths bit for bit; the device
Philox draws, batch independence, the edges, and the planners' surface."""
import types

import numpy as np
import pytest
import torch

import path_shortcut_checks as K
from conftest import load_golden, product_geometry_from_golden

pytestmark = pytest.mark.gpu
CODE = (1 << K.SHIFT) - 1


def _geom(p, dev, use_model=True):
    from motion_planning_baselines_amd import ops
    if len(p.fields) == 1:
        return ops.DeviceGeometry(p.robot, p.fields[0], dev, use_model=use_model)
    return ops.DeviceGeometry(p.robot, p.fields, dev, scales=p.scales, use_model=use_model)


def _run(p, geom, dev, draws='recorded', in_place=False, **kw):
    """One launch over the input set p: host copies of what the kernel leaves behind."""
    from motion_planning_baselines_amd import ops
    paths = torch.from_numpy(p.paths).to(dev).contiguous()
    lengths = torch.from_numpy(p.lengths).to(dev)
    d = torch.from_numpy(p.draws).to(dev).contiguous() if isinstance(draws, str) else draws
    out = (paths, lengths) if in_place else None
    po, lo, stats, log = ops.path_shortcut(paths, lengths, geom, p.n_iters, float(p.step), draws=d, with_log=True, out=out, **kw)
    torch.cuda.synchronize()
    if in_place:
        assert po is paths and lo is lengths
    else:
        assert np.array_equal(paths.cpu().numpy().view(np.uint32), p.paths.view(np.uint32))       # the inputs are not touched
    return types.SimpleNamespace(paths=po.cpu().numpy(), lengths=lo.cpu().numpy(), stats=stats.cpu().numpy(), log=log.cpu().numpy())


def _same_bits(a, b, rows_a=None, rows_b=None):
    ra = np.arange(len(a.lengths)) if rows_a is None else np.asarray(rows_a)
    rb = np.arange(len(b.lengths)) if rows_b is None else np.asarray(rows_b)
    for k in ('paths', 'stats', 'log', 'lengths'):
        x, y = getattr(a, k)[ra], getattr(b, k)[rb]
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), k


@pytest.mark.parametrize('name', K.SETS + ('panda:generic', 'panda_chain:generic'))
def test_replay_with_recorded_draws(gpu_device, name):
    """1. The kernel's log against replay64: every decision fp64 can decide equals the log (code and first-collision index), the
    undecidable ones are at most 2 % of the tested candidates, and the replayed paths, lengths and stats are the kernel's bit for bit."""
    name, _, form = name.partition(':')
    p = K.problem(name)
    got = _run(p, _geom(p, gpu_device, use_model=form != 'generic'), gpu_device)
    r64 = K.replay64(p, got.log)                                 # (raises on the first decidable decision that differs)
    share = K.undecidable_share(r64.cands)
    r32 = K.reference(name).r32
    counts = np.bincount((got.log & CODE).ravel(), minlength=5)
    print(f'{name} {form}: IDLE / SKIP / REJECT / OVERFLOW / ACCEPT {counts.tolist()}; {len(r64.cands)} candidates tested, undecidable '
          f'{sum(not c.decidable for c in r64.cands)} (share {share:.4f}); log entries that differ from the fp32 restatement '
          f'{int((got.log != r32.log).sum())}; smallest margin / bar over the decidable {min(c.margin / c.bar for c in r64.cands if c.decidable):.2f}')
    assert share <= 0.02
    assert counts[K.REJECT] > 0 and counts[K.ACCEPT] > 0
    assert np.array_equal(got.lengths, r64.lengths)
    assert np.array_equal(got.paths.view(np.uint32), r64.paths.view(np.uint32))
    assert np.array_equal(got.stats.view(np.uint32), r64.stats.view(np.uint32)), np.abs(got.stats - r64.stats).max()


@pytest.mark.parametrize('name', ('pm2d_dense', 'panda_chain'))
def test_device_philox_equals_the_same_uniforms_recorded(gpu_device, name):
    """2. draws=None: one Philox4x32-10 call per (path, iteration), counter (problem_offset + b, iteration, tag, 0), key seed; the top
    24 bits of .x and .y times 2^-24."""
    from motion_planning_baselines_amd import ops
    p = K.problem(name)
    geom = _geom(p, gpu_device)
    seed, offset = 0x1234567811223344, 5
    b, it = np.meshgrid(np.arange(p.N), np.arange(p.n_iters), indexing='ij')
    ctr = np.stack([b.ravel() + offset, it.ravel(), np.full(b.size, ops.SHORTCUT_PHILOX_TAG), np.zeros(b.size, np.int64)], 1)
    key = np.tile(np.array([[seed & 0xFFFFFFFF, seed >> 32]], np.int64), (b.size, 1))
    words = ops.debug_philox(ctr, key, 10)
    u = ((words[:, :2] >> 8).astype(np.float32) * np.float32(2.0 ** -24)).reshape(p.N, p.n_iters, 2)
    assert u.min() >= 0.0 and u.max() < 1.0
    device = _run(p, geom, gpu_device, draws=None, seed=seed, problem_offset=offset)
    recorded = _run(K.with_inputs(p, p.paths, p.lengths, u), geom, gpu_device)
    _same_bits(device, recorded)
    assert (device.log & CODE == K.ACCEPT).any()
    other = _run(p, geom, gpu_device, draws=None, seed=seed + 1, problem_offset=offset)
    assert not np.array_equal(device.log, other.log)
    # a path's stream is its global index: the second half alone, offset by the first half's size, repeats it
    h = p.N // 2
    half = _run(K.with_inputs(p, p.paths[h:], p.lengths[h:], p.draws[h:]), geom, gpu_device, draws=None, seed=seed, problem_offset=offset + h)
    _same_bits(device, half, rows_a=np.arange(h, p.N))


@pytest.mark.parametrize('name', ('pm2d_grid', 'arm12_chain'))
def test_a_path_depends_on_its_own_inputs_only(gpu_device, name):
    """3. The same problems in another batch order and batch size; two runs of the same batch."""
    p = K.problem(name)
    geom = _geom(p, gpu_device)
    a = _run(p, geom, gpu_device)
    _same_bits(a, _run(p, geom, gpu_device))
    rows = np.arange(p.N)[::-1][::2]                              # every other path, back to front
    assert 1 < len(rows) < p.N
    _same_bits(a, _run(K.with_inputs(p, p.paths[rows], p.lengths[rows], p.draws[rows]), geom, gpu_device), rows_a=rows)
    one = [int(np.argmax(p.lengths))]
    _same_bits(a, _run(K.with_inputs(p, p.paths[one], p.lengths[one], p.draws[one]), geom, gpu_device), rows_a=one)


def _against_restatement(q, geom, dev, **kw):
    got, want = _run(q, geom, dev, **kw), K.restate32(q)
    _same_bits(got, want)
    return got


def test_edges(gpu_device):
    """4. On the 2-D grid of circles, every case also held to the fp32 restatement bit for bit (the decisions are far from any surface)."""
    from motion_planning_baselines_amd import ops
    p = K.problem('pm2d_grid')
    geom = _geom(p, gpu_device)
    zig, below = K.ZIGZAG, K.ONE_BELOW
    # lengths 0, 1 and 2 pass through (0 stays 0), a length outside 0 .. Lmax is flagged
    paths = np.tile(zig[None], (6, 1, 1))
    lengths = np.array([0, 1, 2, -1, 6, 5], np.int32)
    draws = np.tile(np.array([[[0.0, below], [0.3, 0.9]]], np.float32), (6, 1, 1))
    got = _against_restatement(K.with_inputs(p, paths, lengths, draws), geom, gpu_device)
    assert got.lengths.tolist() == [0, 1, 2, 0, 0, 2]
    assert np.isnan(got.stats[3:5]).all() and not got.paths[3:5].any() and not np.isnan(got.stats[[0, 1, 2, 5]]).any()
    assert not got.paths[0].any() and np.array_equal(got.paths[1, :1], zig[:1]) and not got.paths[1, 1:].any()
    assert np.array_equal(got.paths[2, :2], zig[:2]) and not got.paths[2, 2:].any()
    assert (got.log[:5] & CODE == K.IDLE).all() and got.log[5].tolist() == [K.ACCEPT, K.IDLE]
    assert got.stats[:3, :2].tolist() == [[0, 0]] * 3 and got.stats[2, 2] == got.stats[2, 3] > 0
    # u = 0: t == 0, node 0 serves and no duplicate row is inserted; both draws on one segment, u = 0 twice, an existing edge: SKIP
    got = _against_restatement(K.with_inputs(p, zig[None], [5], np.array([[[0.3, 0.4], [0.0, 0.0], [0.0, 0.25], [0.6, 0.0]]], np.float32)),
                               geom, gpu_device)
    assert (got.log & CODE).tolist() == [[K.SKIP, K.SKIP, K.SKIP, K.ACCEPT]] and got.lengths.tolist() == [4]
    assert np.array_equal(got.paths[0, [0, 2, 3]].view(np.uint32), zig[[0, 3, 4]].view(np.uint32))
    assert len({r.tobytes() for r in got.paths[0, :4]}) == 4
    # a full path with a corner-cutting draw: OVERFLOW and unchanged; with one spare row the same draw is accepted
    cut = np.array([[[0.1, 0.4]]], np.float32)
    got = _against_restatement(K.with_inputs(p, zig[None], [5], cut), geom, gpu_device)
    assert got.log.tolist() == [[K.OVERFLOW]] and got.lengths.tolist() == [5] and got.stats[0, :2].tolist() == [1, 0]
    assert np.array_equal(got.paths[0].view(np.uint32), zig.view(np.uint32))
    got = _against_restatement(K.with_inputs(p, np.concatenate([zig, zig[:1]])[None], [5], cut), geom, gpu_device)
    assert got.log.tolist() == [[K.ACCEPT]] and got.lengths.tolist() == [6]
    # a long candidate at a small check_step: more than 64 points, the first collision in the second trip of the scan
    wall = np.array([[-0.66, -0.56], [-0.5, -0.68], [-0.34, -0.56]], np.float32)        # the line y = -0.56 grazes the circle at (-0.5, -0.5)
    q = K.with_inputs(p, wall[None], [3], np.array([[[0.0, below]]], np.float32), step=0.001)
    got = _against_restatement(q, geom, gpu_device)
    code, first = int(got.log[0, 0]) & CODE, int(got.log[0, 0]) >> K.SHIFT
    r64 = K.replay64(q, got.log)
    assert code == K.REJECT and 64 <= first < 128 and r64.cands[0].decidable and r64.cands[0].n_pts > 300, (code, first, vars(r64.cands[0]))
    assert got.lengths.tolist() == [3] and np.array_equal(got.paths[0].view(np.uint32), wall.view(np.uint32))
    # in place equals out of place; n_iters == 0 copies
    a = _run(p, geom, gpu_device)
    _same_bits(a, _run(p, geom, gpu_device, in_place=True))
    none = _run(K.with_inputs(p, p.paths, p.lengths, p.draws[:, :0]), geom, gpu_device)
    assert none.log.shape == (p.N, 0) and np.array_equal(none.lengths, p.lengths)
    assert np.array_equal(none.paths.view(np.uint32), p.paths.view(np.uint32))
    assert not none.stats[:, :2].any() and np.array_equal(none.stats[:, 2].view(np.uint32), none.stats[:, 3].view(np.uint32))
    assert np.array_equal(none.stats[:, 2].view(np.uint32), a.stats[:, 2].view(np.uint32))
    # the wrapper's own refusals
    dev_paths, dev_len = torch.from_numpy(p.paths).to(gpu_device), torch.from_numpy(p.lengths).to(gpu_device)
    with pytest.raises(ValueError):
        ops.path_shortcut(dev_paths[:, :, :1].contiguous(), dev_len, geom, 4, 0.1)
    with pytest.raises(ValueError):
        ops.path_shortcut(dev_paths, dev_len.long(), geom, 4, 0.1)
    with pytest.raises(ops._lib.MPBError, match='check_step'):
        ops.path_shortcut(dev_paths, dev_len, geom, 4, 0.0)


def test_the_longest_path_lds_holds(gpu_device):
    """The launch that takes all 160 KB of LDS (Lmax = 9 152 at D = 2: beyond the default dynamic-LDS limit, which the launcher raises):
    a full path, a shortcut whose tail of 7 000 rows moves towards the front in many trips, then a corner cut that moves it one row back."""
    p = K.problem('pm2d_grid')
    geom = _geom(p, gpu_device)
    Lmax = 9152
    j = np.arange(Lmax)
    path = np.stack([-0.64 + 0.03 * j / (Lmax - 1), np.where(j % 2 == 0, -0.64, -0.61)], 1).astype(np.float32)   # in free space throughout
    one = K.restate32(K.with_inputs(p, path[None], [Lmax], np.array([[[0.1, 0.2]]], np.float32)))
    L1 = int(one.lengths[0])
    assert one.log.tolist() == [[K.ACCEPT]] and L1 < Lmax - 900
    draws = np.array([[[0.1, 0.2], [0.2 / (L1 - 1), 1.6 / (L1 - 1)], [0.0, K.ONE_BELOW]]], np.float32)
    paths = np.stack([path, path[::-1], path])
    q = K.with_inputs(p, paths, [Lmax, Lmax, 3], np.tile(draws, (3, 1, 1)))
    got = _against_restatement(q, geom, gpu_device)
    assert (got.log[0] & CODE).tolist() == [K.ACCEPT] * 3 and got.lengths.tolist() == [3, 3, 2]     # (u just below 1 is no node at this L)
    mid = _against_restatement(K.with_inputs(p, paths, [Lmax, Lmax, 3], np.tile(draws[:, :2], (3, 1, 1))), geom, gpu_device)
    assert mid.lengths[0] == L1 + 1 and np.array_equal(mid.paths[0, L1].view(np.uint32), path[-1].view(np.uint32))


def test_it_shortcuts(gpu_device):
    """5. A zig-zag in free space and the draw (0, just below 1) become the two endpoints; a zig-zag around an obstacle that blocks the
    straight line keeps the detour."""
    p = K.problem('pm2d_grid')
    geom = _geom(p, gpu_device)
    draw = np.array([[[0.0, K.ONE_BELOW]]], np.float32)
    got = _against_restatement(K.with_inputs(p, K.ZIGZAG[None], [5], draw), geom, gpu_device)
    assert got.lengths.tolist() == [2] and got.log.tolist() == [[K.ACCEPT]] and got.stats[0, :2].tolist() == [1, 1]
    assert np.array_equal(got.paths[0, :2].view(np.uint32), K.ZIGZAG[[0, -1]].view(np.uint32)) and not got.paths[0, 2:].any()
    assert got.stats[0, 3] < 0.2 * got.stats[0, 2]
    around = np.array([[-0.5, -0.6], [-0.59, -0.58], [-0.6, -0.5], [-0.58, -0.41], [-0.5, -0.4]], np.float32)   # round the circle at (-0.5, -0.5)
    got = _against_restatement(K.with_inputs(p, around[None], [5], draw), geom, gpu_device)
    assert got.lengths.tolist() == [5] and int(got.log[0, 0]) & CODE == K.REJECT and got.stats[0, :2].tolist() == [1, 0]
    assert np.array_equal(got.paths[0].view(np.uint32), around.view(np.uint32)) and got.stats[0, 2] == got.stats[0, 3]


def _polyline_length(x):
    return torch.linalg.norm((x[:, 1:] - x[:, :-1]).double(), dim=-1).sum(-1)


def test_planners(gpu_device):
    """6. RRTConnect.shortcut, HybridPlanner(shortcut_iters=...), and the refusal of tasks whose fields the kernel does not know."""
    from motion_planning_baselines_amd import geometry as G, ops
    from motion_planning_baselines_amd.planners.hybrid_planner import HybridPlanner
    from motion_planning_baselines_amd.planners.multi_sample_based_planner import MultiSampleBasedPlanner
    from motion_planning_baselines_amd.planners.rrt_connect import RRTConnect
    from motion_planning_baselines_amd.robot_field import PlanningTask
    g = load_golden('rrt_pm2d_grid')
    robot, field = product_geometry_from_golden(g)
    ta = dict(device=gpu_device, dtype=torch.float32)
    task = PlanningTask(robot, field, tensor_args=ta)
    D = robot.q_dim

    def rrt(starts, goals):
        return RRTConnect(task=task, n_iters=int(g['n_iters']), start_state_pos=torch.from_numpy(starts), goal_state_pos=torch.from_numpy(goals),
                          step_size=float(g['step_size']), n_radius=float(g['n_radius']), tensor_args=ta, n_pre_samples=g['pool'].shape[0],
                          pre_samples=torch.from_numpy(g['pool']), max_path_nodes=70, seed=2)
    planner = rrt(g['starts'], g['goals'])
    paths, lengths, status = planner.optimize_batched()
    before = (paths.clone(), lengths.clone(), status.clone())
    assert (status == ops.RRT_FOUND).sum() >= 2 and int(lengths.max()) > 3
    sp, sl, stats = planner.shortcut(paths, lengths, 32)
    assert all(torch.equal(x, y) for x, y in zip(before, (paths, lengths, status)))            # the planner's outputs and statuses stay
    assert (sl <= paths.shape[1]).all() and ((sl == 0) == (lengths == 0)).all() and (sl[lengths > 0] >= 2).all()   # (a corner cut adds a node)
    for b in range(paths.shape[0]):
        n0, n1 = int(lengths[b]), int(sl[b])
        assert _polyline_length(sp[b:b + 1, :n1]) <= _polyline_length(paths[b:b + 1, :n0]) + 1e-5
        if n0:
            assert torch.equal(sp[b, 0], paths[b, 0]) and torch.equal(sp[b, n1 - 1], paths[b, n0 - 1])
    assert float(stats[:, 3].sum()) < 0.9 * float(stats[:, 2].sum()) and (stats[:, 3] <= stats[:, 2] * (1 + 1e-6)).all()
    again = planner.shortcut(paths, lengths, 32, check_step=planner.step_size)               # the default step is step_size; same bits
    assert torch.equal(again[0], sp) and torch.equal(again[1], sl)

    class Opt:                                                   # the slice of an optimisation-based planner HybridPlanner calls
        n_support_points, dt, opt_iters = 64, 0.1, 0

        def reset(self, initial_particle_means=None):
            self.means = initial_particle_means

        def get_traj(self):
            return self.means

    k = int(np.argmax([len(g[f'p{i}_path']) for i in range(int(g['n_problems']))]))
    multi = lambda: MultiSampleBasedPlanner(rrt(g['starts'][k], g['goals'][k]), n_trajectories=5)
    plain = HybridPlanner(multi(), Opt(), tensor_args=ta).optimize()
    zero = HybridPlanner(multi(), Opt(), shortcut_iters=0, tensor_args=ta).optimize()
    assert plain.shape == (1, 5, 64, 2 * D) and torch.equal(plain, zero)
    hyb = HybridPlanner(multi(), Opt(), shortcut_iters=48, tensor_args=ta)
    cut = hyb.optimize()
    len0, len1 = _polyline_length(plain[0, :, :, :D]), _polyline_length(cut[0, :, :, :D])
    print('polyline length of the initial means without / with shortcutting:', len0.tolist(), len1.tolist(), hyb.shortcut_stats.tolist())
    assert (len1 <= len0).all() and (len1 < len0).any()
    assert torch.allclose(cut[0, :, 0, :D], plain[0, :, 0, :D], atol=1e-6) and torch.allclose(cut[0, :, -1, :D], plain[0, :, -1, :D], atol=1e-6)

    class ListPlanner:                                           # a foreign planner: a list of paths, no shortcut() of its own
        start_state_pos, goal_state_pos = torch.from_numpy(g['starts'][k]), torch.from_numpy(g['goals'][k])

        def optimize(self, refill_samples_buffer=False, debug=False, **kw):
            return [q.cpu() if q is not None else None for q in multi().optimize()]

    with pytest.raises(NotImplementedError, match='task'):
        HybridPlanner(ListPlanner(), Opt(), shortcut_iters=8, shortcut_step=0.01, tensor_args=ta).optimize()
    with_task = Opt()
    with_task.task = task
    by_list = HybridPlanner(ListPlanner(), with_task, shortcut_iters=48, shortcut_step=planner.step_size, tensor_args=ta)
    listed = by_list.optimize()                                  # (padded to the longest path + 1 and drawn from seed 0: other bits than `cut`)
    assert listed.shape == plain.shape and float(by_list.shortcut_stats[:, 1].sum()) > 0 and not torch.equal(listed, plain)
    assert torch.allclose(listed[0, :, 0, :D], plain[0, :, 0, :D], atol=1e-6) and torch.allclose(listed[0, :, -1, :D], plain[0, :, -1, :D], atol=1e-6)

    for kw, word in ((dict(self_field=G.SelfCollisionField(G.RobotPanda())), 'self_field'),
                     (dict(sdf_field=G.GridSDFField.from_field(G.env_spheres_3d(), (-1.2, -1.2, -0.6), (1.2, 1.2, 1.6), 0.05)), 'sdf_field')):
        t = PlanningTask(G.RobotPanda(), G.env_spheres_3d(), tensor_args=ta, **kw)
        q = torch.zeros(2, 4, 7, device=gpu_device)
        with pytest.raises(NotImplementedError, match=word):
            t.shortcut_paths(q, torch.full((2,), 4, device=gpu_device, dtype=torch.int32), n_iters=4, check_step=0.1)
