"""Space-time certification on the CPU (no GPU): the generated layout header, the ABI and the kernels' resources, the chord deviation
against a brute-force maximum, the restated eta against the restated row predicate of check_trajs_moving at the nodes, the soundness of
the fp64 restatement of the bisection (st_certify_checks.certify_ref) against a dense resampling on the chord motion, the share of
trajectories on which its fp32 form decides differently, and the tunnelling case every row of which is free."""
import json
import os

import numpy as np
import pytest

import st_certify_checks as K
from motion_planning_baselines_amd import certify_layout as CL
from motion_planning_baselines_amd import st_certify_layout as SL

S = SL.STC_DEFAULT_SLACK


def test_layout_header_is_generated_and_the_public_numbers_are_pinned():
    from motion_planning_baselines_amd import build, model_gen
    assert open(model_gen.ST_CERTIFY_LAYOUT_HEADER).read() == model_gen.st_certify_layout_header_text()
    assert not model_gen.stale_headers()
    assert SL.STATUS == CL.STATUS + ('NOT_VALID',) and SL.STC_OUT_INTS == 6 and SL.STC_OUT_FLOATS == 3
    assert SL.STC_NO_OBSTACLE < -1 - 4                          # below every static field's code -1 - f
    assert SL.STC_DEFAULT_SLACK == 32.0 * SL.STC_E_MEASURED and 0.0 < SL.STC_E_MEASURED < 1e-5
    assert 'mpb_st_certify_layout.h' in open(build.__file__).read()     # listed among the headers a build depends on


def test_abi_and_kernel_resources():
    """The entry points are declared, bound and exported (additive: the ABI version stays); both kernels have 0 B of scratch, no vector
    spills and no static LDS."""
    from motion_planning_baselines_amd import _lib, build, ops
    mpb_h = open(os.path.join(K.ROOT, 'include', 'mpb.h')).read()
    assert 'int mpb_moving_clearance(' in mpb_h and 'int mpb_traj_certify_moving(' in mpb_h and '#include "mpb_st_certify_layout.h"' in mpb_h
    assert 'mpb_certify_moving.hip' in build.SOURCES and (_lib.lib().mpb_version() & 0xFFFF) == _lib.ABI_VERSION == 7
    assert ops.STC_STATUS_NAMES is SL.STATUS and ops.STC_NOT_VALID == K.NOT_VALID and ops.STC_DEFAULT_SLACK == S
    build.build(verbose=False)
    res = json.load(open(build.RESOURCES))
    for name in ('_Z23moving_clearance_kernel7STCArgsPfPiS1_i', '_Z26traj_certify_moving_kernel7STCArgs'):
        r = res[name]
        print(name, r)
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['lds'] == 0, (name, r)


@pytest.mark.parametrize('name', K.SCENES)
def test_chord_deviation_against_brute_force(name):
    """chord_deviation equals the fp64 maximum of |c_o(t) - chord| over 10^4 times per interval (the keyframe's own time among them) to
    1e-12, and the maximum over the plain 10^4-point grid alone to what such a grid can miss (half a step times the largest slope); a
    field whose keyframes lie on rows has 0."""
    st = K.scene(name)
    f, R = st.field, st.R
    rows = np.concatenate(f.rows(R), 1)
    t_rows = f.times(R)
    worst = plain = 0.0
    # what the plain grid can miss: the difference is piecewise linear in s with slope at most (the field's speed per unit s + the
    # chord's length), and its peak lies within half a grid step of a grid point
    speed = np.concatenate([np.abs(np.diff(k, axis=0)).sum(-1) / np.diff(f.t_key)[:, None] for k in (f.sphere_centers, f.box_centers)], 1).max()
    slope = speed * (t_rows[1] - t_rows[0]) + np.linalg.norm(np.diff(rows, axis=0), axis=-1).max()
    for h in range(R - 1):
        s = np.linspace(0.0, 1.0, 10000)
        t = t_rows[h] + s * (t_rows[h + 1] - t_rows[h])
        grid = rows[h][None] + s[:, None, None] * (rows[h + 1] - rows[h])[None]
        plain = max(plain, float(np.linalg.norm(np.concatenate(f._centres(t), 1) - grid, axis=-1).max()))
        inside = f.t_key[(f.t_key > t_rows[h]) & (f.t_key < t_rows[h + 1])]
        t = np.concatenate([t, inside])
        s = np.concatenate([s, (inside - t_rows[h]) / (t_rows[h + 1] - t_rows[h])])
        true = np.concatenate(f._centres(t), 1)
        chord = rows[h][None] + s[:, None, None] * (rows[h + 1] - rows[h])[None]
        worst = max(worst, float(np.linalg.norm(true - chord, axis=-1).max()))
    dev = SL.chord_deviation(f, R)
    print(f'{name}: chord_deviation = {dev:.6e}, brute force {worst:.6e}')
    assert dev > 1e-3 and abs(dev - worst) <= 1e-12
    # independently of where chord_deviation looks: the maximum over the plain grid, no keyframe time added
    assert plain <= dev + 1e-12 and dev - plain <= slope * 0.5 / 9999, (dev, plain, slope)
    assert SL.chord_deviation(st.field_rows, R) == 0.0
    assert SL.chord_deviation(f, 1) == 0.0


@pytest.mark.parametrize('name', K.SCENES)
def test_eta_sign_is_the_row_predicate_at_the_nodes(name):
    """On 2 000 random rows (uniform configuration, uniform row) the restated eta < 0 equals the restated predicate of
    check_trajs_moving -- static hinge OR moving hinge -- in fp64 and in fp32; a row where they differ is a tie and has |eta| <= E_st."""
    st = K.scene(name)
    tab = st.tables()
    rng = np.random.RandomState(5)
    q, h = st.sc.uniform(2000, seed=6), rng.randint(0, st.R, 2000)
    for T in (K.F64, K.F32):
        e = K.evaluate(st, tab, q, q, h, h, np.zeros(2000), 0.0, T)
        tie = (e['eta'] < 0) != e['hit']
        print(f'{name} {T.__name__}: {int(e["hit"].sum())} rows in collision, {int(tie.sum())} ties')
        assert (np.abs(e['eta'][tie]) <= SL.STC_E_MEASURED).all()
        assert 0.1 < e['hit'].mean() < 0.9


@pytest.mark.parametrize('name', K.SCENES)
def test_restatement_is_sound_and_its_fp32_form_decides_alike(name):
    """Every FREE certificate of the fp64 restatement is held to 4 097 fp64 points per interval on the chord motion: their minimum eta
    is at least margin_cert + c_req.  FREE, COLLISION and UNDECIDED_DEPTH (max_depth = 3) all occur on the trajectories the GPU test
    uses, and the fp32 restatement decides as the fp64 one on at least 98 % of them."""
    st = K.scene(name)
    tab = st.tables()
    trajs = K.trajs(st, 32, *K.CERT_CASES[name])
    seen, differ = {}, 0
    for c_req in (0.0, 0.01):
        for t in trajs[:16] if c_req else trajs:
            r = K.certify_ref(st, tab, t, S, c_req=c_req, max_depth=3)
            if not c_req:
                seen[r['status']] = seen.get(r['status'], 0) + 1
                r32 = K.certify_ref(st, tab, t, S, max_depth=3, T=K.F32)
                differ += K.decision(r) != K.decision(r32)
            if r['status'] == K.FREE:
                dense = K.dense_eta(st, tab, t)
                assert dense >= r['margin_cert'] + c_req and r['margin_cert'] > S, (dense, r)
            elif r['status'] == K.COLLISION:
                assert r['witness'][4] - c_req < -S
    print(f'{name}: {seen}, fp32 decides differently on {differ} of {len(trajs)}')
    assert all(seen.get(k, 0) >= 1 for k in (K.FREE, K.COLLISION, K.UNDECIDED_DEPTH))
    assert differ <= 0.02 * len(trajs)
    queue = [K.certify_ref(st, tab, t, S, max_intervals=4)['status'] for t in trajs[:8]]
    assert K.UNDECIDED_QUEUE in queue


def test_tunnelling_case_is_a_collision_between_rows_that_are_all_free():
    """The robot stands still, the circle crosses it between rows 3 and 4: every row is free by a wide margin, the restated certifier
    returns COLLISION in interval 3 within the contact's half-width of s = 0.3, against moving obstacle 0."""
    st, field, traj = K.tunnel()
    tab = st.tables(field)
    rows = np.arange(st.R)
    e = K.evaluate(st, tab, traj, traj, rows, rows, np.zeros(st.R), 0.0)
    assert (e['eta'] > 0.1).all() and not e['hit'].any()
    assert SL.chord_deviation(field, st.R) == 0.0
    for T in (K.F64, K.F32):
        r = K.certify_ref(st, tab, traj, S, T=T)
        assert r['status'] == K.COLLISION
        row, s, link, obst, eta = r['witness']
        assert row == K.TUNNEL_ROW and abs(s - K.TUNNEL_S) < K.TUNNEL_HALF_WIDTH and link == 0 and obst == 0 and eta < -S
