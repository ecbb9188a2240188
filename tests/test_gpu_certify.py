"""Clearance and path certification on the GPU (csrc/mpb_certify.hip, ops.clearance, ops.path_certify, PlanningTask.compute_clearance /
certify_paths / certify_trajs) against the fp64 oracle and the restatement of certify_checks.py: accuracy of eta within a quarter of the
slack, soundness of every FREE and every COLLISION without exceptions, completeness at the derived depth, the tunnelling scene the sampled
validator passes, depth / queue limits, shapes and edges, refusals, and the cap on undecided paths.

Scenes: a 2-D point among circles and boxes, the Panda among 16 spheres, a 12-joint chain among boxes in two chained fields of different
margins (D = 2, 7, 12).  Batches: N = 0, 1, 3, 65; lengths 1, 2, 65, 66 (more than 64 segments: two trips of a level)."""
import functools

import numpy as np
import pytest
import torch

import certify_checks as C
from motion_planning_baselines_amd import certify_layout as CL

pytestmark = pytest.mark.gpu
S = CL.CERT_DEFAULT_SLACK


@functools.lru_cache(maxsize=None)
def _task(name, dev):
    from motion_planning_baselines_amd.robot_field import PlanningTask
    sc = C.tunnel_scene()[0] if name == 'tunnel' else C.scene(name)
    return sc, PlanningTask(sc.robot, sc.field, tensor_args=dict(device=dev, dtype=torch.float32))


def _host(cert):
    torch.cuda.synchronize()
    return {k: getattr(cert, k).cpu().numpy() for k in ('status', 'witness_segment', 'witness_t', 'witness_link', 'witness_eta', 'n_evals',
                                                         'depth_max', 'margin_cert')}


def _same(x, y):
    return all(np.array_equal(x[k].view(np.int32), y[k].view(np.int32)) for k in x)


def _pad(paths):
    """[(Lp, D)] -> (N, Lmax, D) fp32 zero padded, lengths (N,) int32."""
    Lmax = max(len(p) for p in paths)
    out = np.zeros((len(paths), Lmax, paths[0].shape[1]), np.float32)
    for n, p in enumerate(paths):
        out[n, :len(p)] = p
    return out, np.array([len(p) for p in paths], np.int32)


@functools.lru_cache(maxsize=None)
def _mixed_batch(name):
    """20 paths of 4 rows and 4 of 66 rows (65 segments: a level of more than one trip), zero padded, with lengths.  Read-only."""
    sc = C.scene(name)
    paths = list(C.short_paths(sc, 20, 4, 0.1, seed=7)) + list(C.short_paths(sc, 4, 66, 0.15, seed=8, bump=0.01))
    p, ln = _pad(paths)
    p.setflags(write=False)
    return p, ln


@pytest.mark.parametrize('name', C.SCENES)
def test_clearance_against_the_fp64_oracle(gpu_device, name):
    """max |eta_gpu - eta_64| <= S / 4 over 512 uniform configurations; the arg-min sphere agrees wherever the two smallest eta_l differ
    by more than S / 2."""
    sc, task = _task(name, gpu_device)
    q = sc.uniform(512, seed=5)
    eta, link = task.compute_clearance(torch.from_numpy(q).to(gpu_device), return_link=True)
    torch.cuda.synchronize()
    eta, link = eta.cpu().numpy().astype(np.float64), link.cpu().numpy()
    e64 = sc.eta_links(q)
    err = float(np.abs(eta - e64.min(1)).max())
    print(f'{name}: max |eta_gpu - eta_64| = {err:.3e} = {err / S:.3f} S (bound S / 4 = {S / 4:.3e}); eta in [{e64.min():.3f}, {e64.min(1).max():.3f}]')
    assert err <= S / 4
    two = np.sort(e64, 1)[:, :2] if sc.L > 1 else None
    clear = np.ones(len(q), bool) if two is None else (two[:, 1] - two[:, 0] > S / 2)
    assert clear.mean() > 0.9 and np.array_equal(link[clear], e64.argmin(1)[clear])
    # the predicate of compute_collision is eta < 0 wherever eta is farther than S from 0
    decided = np.abs(e64.min(1)) > S
    hit = task.compute_collision(torch.from_numpy(q).to(gpu_device)).cpu().numpy()
    assert np.array_equal(hit[decided], (e64.min(1) < 0)[decided])


@pytest.mark.parametrize('c_req', (0.0, 0.01))
@pytest.mark.parametrize('name', C.SCENES)
def test_soundness_without_exceptions(gpu_device, name, c_req):
    """Every FREE path: its dense fp64 resampling (2^(depth_max + 3) points per segment) keeps eta - c_req >= margin_cert - S.  Every
    COLLISION witness has fp64 eta - c_req <= S / 4."""
    sc, task = _task(name, gpu_device)
    p, ln = _mixed_batch(name)
    r = _host(task.certify_paths(torch.from_numpy(p.copy()).to(gpu_device), torch.from_numpy(ln).to(gpu_device), c_req=c_req, max_depth=8))
    n_free = n_coll = 0
    for n in range(len(p)):
        path = p[n, :ln[n]]
        if r['status'][n] == C.FREE:
            n_free += 1
            dense = C.dense_clearance(sc, path, 2 ** (int(r['depth_max'][n]) + 3))
            assert dense - c_req >= float(r['margin_cert'][n]) - S, (n, dense, r['margin_cert'][n])
            assert r['witness_segment'][n] == -1 and r['witness_link'][n] == -1
        elif r['status'][n] == C.COLLISION:
            n_coll += 1
            q = C.witness_q(path, int(r['witness_segment'][n]), float(r['witness_t'][n]))
            e = sc.eta_links(q[None])[0]
            assert e.min() - c_req <= S / 4, (n, e.min())
            assert abs(float(r['witness_eta'][n]) - e.min()) <= S / 4 and np.isneginf(r['margin_cert'][n])
        else:
            assert r['status'][n] == C.UNDECIDED_DEPTH and np.isneginf(r['margin_cert'][n])
    print(f'{name} c_req {c_req}: FREE {n_free}, COLLISION {n_coll}, undecided {len(p) - n_free - n_coll}; depth_max up to {r["depth_max"].max()}, '
          f'n_evals up to {r["n_evals"].max()}')
    assert n_free >= 1 and n_coll >= 1 and (r['status'][20:] != C.UNDECIDED_QUEUE).all()


@pytest.mark.parametrize('name', ('pm2d', 'panda'))
def test_completeness_at_the_derived_depth(gpu_device, name):
    """Paths that keep fp64 clearance >= c (verified here by dense sampling, 1024 points per segment, with 5 % to spare) end FREE with
    depth_max <= ceil(log2(Lambda_max / (c - 2 S))): at that depth w Lambda_l <= c - 2 S, so eta_gpu - w Lambda_l > S."""
    sc, task = _task(name, gpu_device)
    c = 0.02
    cand = C.short_paths(sc, 64, 3, 0.1, seed=21)
    keep = [p for p in cand if C.dense_clearance(sc, p, 1024) >= 1.05 * c]
    assert len(keep) >= 6, len(keep)
    p = np.stack(keep)
    r = _host(task.certify_paths(torch.from_numpy(p).to(gpu_device), max_depth=20))
    lam = np.array([sc.motion_bound(q[:-1], q[1:]).max() for q in p])
    limit = np.ceil(np.log2(lam / (c - 2 * S))).astype(int)
    print(f'{name}: {len(keep)} paths with clearance >= {c}; depth_max {r["depth_max"].tolist()} against the derived limit {limit.tolist()}')
    assert (limit >= 0).all()
    assert (r['status'] == C.FREE).all() and (r['depth_max'] <= limit).all()
    assert (r['margin_cert'] > S).all()


def test_tunnelling_between_the_samples(gpu_device):
    """get_trajs_collision_and_free(num_interpolation=5) reports the path free; certify_trajs reports COLLISION, the witness inside
    the obstacle."""
    sc, task = _task('tunnel', gpu_device)
    path = C.tunnel_scene()[1]
    trajs = torch.from_numpy(path[None].copy()).to(gpu_device)
    coll, free = task.get_trajs_collision_and_free(trajs, num_interpolation=5)
    assert coll is None and free is not None and free.shape[0] == 1
    cert = task.certify_trajs(trajs)
    r = _host(cert)
    assert r['status'][0] == C.COLLISION and r['witness_segment'][0] == 0 and r['witness_link'][0] == 0
    q = cert.witness_q(trajs).cpu().numpy().astype(np.float64)[0]
    assert np.array_equal(q, C.witness_q(path, 0, float(r['witness_t'][0])).astype(np.float32).astype(np.float64))
    assert sc.eta(q[None])[0] < 0 and np.linalg.norm(q - [-0.25, 0.0]) < 0.02
    assert bool(cert.collision[0]) and not bool(cert.free[0]) and not bool(cert.undecided[0])


def test_depth_and_queue_limits(gpu_device):
    """A segment that passes an obstacle at clearance 1e-4 is UNDECIDED_DEPTH at max_depth = 4 and FREE at 20; a tiny max_intervals gives
    UNDECIDED_QUEUE; max_depth = 0 works."""
    sc, task = _task('tunnel', gpu_device)
    graze = np.array([[[-0.5, 0.0201], [0.5, 0.0201]]], np.float32)
    assert abs(C.dense_clearance(sc, graze[0], 4095) - 1e-4) < 1e-6
    g = torch.from_numpy(graze).to(gpu_device)
    assert _host(task.certify_trajs(g, max_depth=4))['status'][0] == C.UNDECIDED_DEPTH
    r = _host(task.certify_trajs(g, max_depth=20))
    print(f'graze: depth_max {r["depth_max"][0]}, n_evals {r["n_evals"][0]}, margin_cert {r["margin_cert"][0]:.3e}')
    assert r['status'][0] == C.FREE and S < r['margin_cert'][0] <= 1e-4 + S
    assert _host(task.certify_trajs(g, max_depth=20, max_intervals=1))['status'][0] == C.UNDECIDED_QUEUE
    assert _host(task.certify_trajs(g, max_depth=20, max_intervals=2))['status'][0] == C.UNDECIDED_QUEUE
    far = torch.tensor([[[-0.5, 0.9], [-0.45, 0.9]]], device=gpu_device)
    r = _host(task.certify_trajs(far, max_depth=0))
    assert r['status'][0] == C.FREE and r['depth_max'][0] == 0 and r['n_evals'][0] == 3
    # three segments against a queue of two: level 0 does not fit
    three = torch.tensor([[[-0.5, 0.9], [-0.45, 0.9], [-0.4, 0.9], [-0.35, 0.9]]], device=gpu_device)
    assert _host(task.certify_trajs(three, max_intervals=2))['status'][0] == C.UNDECIDED_QUEUE
    assert _host(task.certify_trajs(three, max_intervals=3))['status'][0] == C.FREE


@pytest.mark.parametrize('name', C.SCENES)
def test_shapes_and_edges(gpu_device, name):
    """N = 0, 1, 3, 65; lengths 1, 2, 65, 66; a zero-length segment and duplicate nodes; a NaN row; a strided (N, H, W) trajectory read
    in place; the same bits on two runs; a batch equals its paths run one at a time; agreement with the fp64 restatement wherever that
    keeps its answer when the slack is halved and doubled."""
    from motion_planning_baselines_amd import ops
    sc, task = _task(name, gpu_device)
    N, H = 65, 66
    base = C.short_paths(sc, N, H, 0.12, seed=31, bump=0.01)
    ln = np.array([(1, 2, 65, 66)[n % 4] for n in range(N)], np.int32)
    base[2, 10] = base[2, 9]                                   # a zero-length segment
    base[3, 20:23] = base[3, 19]                               # duplicate nodes
    base[7, 30, sc.D - 1] = np.nan                             # a NaN inside the length ...
    base[4, 40, 0] = np.nan                                    # ... and one past it (lengths[4] = 1): never read
    p, lens = torch.from_numpy(base).to(gpu_device), torch.from_numpy(ln).to(gpu_device)
    r = _host(task.certify_paths(p, lens))
    assert _same(r, _host(task.certify_paths(p, lens)))                                          # the same bits on two runs
    assert r['status'][7] == C.BAD_INPUT and r['status'][4] != C.BAD_INPUT
    assert set(np.unique(r['status'])) <= {C.FREE, C.COLLISION, C.UNDECIDED_DEPTH, C.BAD_INPUT}
    one = (ln == 1) & (r['status'] != C.COLLISION)
    assert (r['depth_max'][one] == -1).all() and (r['n_evals'][one] == 1).all()
    for n in (0, 1, 2, 3, 7, 62, 63, 64):                                                        # one at a time
        solo = _host(task.certify_paths(p[n:n + 1].contiguous(), lens[n:n + 1].contiguous()))
        assert all(np.array_equal(solo[k].view(np.int32), r[k][n:n + 1].view(np.int32)) for k in r), n
    for cnt in (0, 1, 3):
        part = _host(task.certify_paths(p[:cnt].contiguous(), lens[:cnt].contiguous()))
        assert all(part[k].shape == (cnt,) and np.array_equal(part[k].view(np.int32), r[k][:cnt].view(np.int32)) for k in r)
    # strided: the rows carry W = 2 D columns, the velocity half is NaN and never read; without lengths every row counts
    full = [n for n in range(N) if ln[n] == H and n != 7]
    wide = np.full((len(full), H, 2 * sc.D), np.nan, np.float32)
    wide[:, :, :sc.D] = base[full]
    rs = _host(task.certify_trajs(torch.from_numpy(wide).to(gpu_device)))
    assert all(np.array_equal(rs[k].view(np.int32), r[k][full].view(np.int32)) for k in r)
    # the restatement, where its answer does not hang on the slack
    agree = 0
    for n in list(range(0, 12)) + [62, 63, 64]:
        path = base[n, :ln[n]]
        refs = [C.certify_ref(sc, path, s) for s in (S / 2, S, 2 * S)]
        if len({(x['status'], x['witness'][:2] if x['witness'] else None, x['depth_max']) for x in refs}) == 1:
            agree += 1
            assert r['status'][n] == refs[1]['status'] and r['depth_max'][n] == refs[1]['depth_max'], n
            if refs[1]['status'] == C.COLLISION:
                assert (r['witness_segment'][n], float(r['witness_t'][n])) == refs[1]['witness'][:2], n
            if refs[1]['status'] == C.FREE:
                assert abs(float(r['margin_cert'][n]) - refs[1]['margin_cert']) <= S / 2, n
    print(f'{name}: statuses {np.bincount(r["status"], minlength=6).tolist()}, {agree} of 15 paths compared with the restatement')
    assert agree >= 8


def test_refusals_by_name(gpu_device):
    from motion_planning_baselines_amd import _lib, geometry as G, ops
    from motion_planning_baselines_amd.robot_field import PlanningTask
    ta = dict(device=gpu_device, dtype=torch.float32)
    q = torch.zeros(2, 4, 7, device=gpu_device)
    for kw, word in ((dict(self_field=G.SelfCollisionField(G.RobotPanda())), 'self_field'),
                     (dict(sdf_field=G.GridSDFField.from_field(G.env_spheres_3d(), (-1.2, -1.2, -0.6), (1.2, 1.2, 1.6), 0.05)), 'sdf_field')):
        t = PlanningTask(G.RobotPanda(), G.env_spheres_3d(), tensor_args=ta, **kw)
        for call in (lambda: t.certify_trajs(q), lambda: t.certify_paths(q), lambda: t.compute_clearance(q[0])):
            with pytest.raises(NotImplementedError, match=word):
                call()
    moving = G.MovingObstacleField([0.0, 1.0], sphere_centers=np.zeros((2, 1, 3)), sphere_radii=[0.1])
    with pytest.raises(TypeError, match='MovingObstacleField'):
        PlanningTask(G.RobotPanda(), moving, tensor_args=ta)
    sc, task = _task('panda', gpu_device)
    geom, reach = task._certify_buffers('test')
    with pytest.raises(ValueError, match='CERT_MAX_ROWS'):
        task.certify_trajs(torch.zeros(1, CL.CERT_MAX_ROWS + 1, 7, device=gpu_device))
    with pytest.raises(ValueError, match='CERT_MAX_DEPTH'):
        task.certify_trajs(q, max_depth=CL.CERT_MAX_DEPTH + 1)
    with pytest.raises(ValueError, match='CERT_MAX_INTERVALS'):
        task.certify_trajs(q, max_intervals=CL.CERT_MAX_INTERVALS + 1)
    with pytest.raises(ValueError, match='slack'):
        task.certify_trajs(q, slack=-1.0)
    with pytest.raises(ValueError, match='keep_all_links'):
        ops.path_certify(q, _pruned(task), reach)
    with pytest.raises(ValueError, match='reach buffer'):
        ops.path_certify(q, geom, ops.DeviceReach(C.scene('chain12').robot, gpu_device))
    # the C entry point refuses the same shapes by name
    oi, of = torch.zeros(2, 5, dtype=torch.int32, device=gpu_device), torch.zeros(2, 3, device=gpu_device)
    lib = _lib.lib()
    for kw, word in ((dict(H=CL.CERT_MAX_ROWS + 1), 'MPB_CERT_MAX_ROWS'), (dict(depth=21), 'MPB_CERT_MAX_DEPTH'),
                     (dict(queue=0), 'MPB_CERT_MAX_INTERVALS'), (dict(links=0), 'MPB_CERT_MAX_LINKS')):
        rc = lib.mpb_path_certify(ops._ptr(q), 7, None, ops._ptr(geom.buf), ops._ptr(reach.buf), kw.get('links', reach.n_links), S, 0.0,
                                  kw.get('depth', 4), kw.get('queue', 64), ops._ptr(oi), ops._ptr(of), 2, kw.get('H', 4), 7, None)
        assert rc != 0 and word in lib.mpb_last_error().decode()
    # a reach header that no longer says what the launch was told: BUFFER_CHANGED, nothing else of it is read
    other = ops.DeviceReach(sc.robot, gpu_device)
    other.buf.view(torch.int32)[2] = other.n_links + 1
    r = _host(ops.path_certify(q, geom, other))
    assert (r['status'] == C.BUFFER_CHANGED).all() and np.isneginf(r['margin_cert']).all()


def _pruned(task):
    """A geometry of the task's scene that does not promise the whole link table."""
    from motion_planning_baselines_amd import ops
    g = ops.DeviceGeometry(task.robot, task.field, task.device)
    g.all_links = False
    return g


def test_undecided_share_on_the_rrt_paths(gpu_device):
    """The RRT-Connect paths of rrt_panda_spheres at the default arguments: the share of UNDECIDED paths is printed and stays below
    10 % (the fp64 restatement alone: test_certify_cpu.py); every answer is sound."""
    sc, task = _task('panda', gpu_device)
    paths = C.rrt_paths()
    p, ln = _pad(paths)
    cert = task.certify_paths(torch.from_numpy(p).to(gpu_device), torch.from_numpy(ln).to(gpu_device))
    r = _host(cert)
    share = float(cert.undecided.float().mean())
    print(f'rrt_panda_spheres: {len(paths)} paths, statuses {[CL.STATUS[s] for s in r["status"]]}, depth_max {r["depth_max"].tolist()}, '
          f'n_evals {r["n_evals"].tolist()}, undecided share {share:.3f}')
    assert share < 0.10
    ref = [C.certify_ref(sc, q, S) for q in paths]
    assert (r['status'] == C.FREE).sum() >= sum(x['status'] == C.FREE for x in ref) - 1
    for n in np.nonzero(r['status'] == C.FREE)[0][:2]:
        assert C.dense_clearance(sc, paths[n], 2 ** (int(r['depth_max'][n]) + 3)) >= float(r['margin_cert'][n]) - S
