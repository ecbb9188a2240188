"""Host side of space-time shortcutting (ops.st_shortcut, csrc/mpb_st_shortcut.hip): the generated layout header, what the compiler made
of the kernel and of the kernels it shares code with, the restatement's guarantee on every input set of the GPU tests, the statuses and
log codes those sets reach, SKIP_FAST / SKIP_STRAIGHT on hand-made cases, the draws, and the condition the GPU tests' inputs are held to --
by the fp64 oracle alone.  No GPU."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT
import st_shortcut_checks as C

f32 = np.float32
# (vgprs, sgprs, scratch, vgpr_spill, static lds) of the kernels on the moving-obstacle clock as the parent commit's build recorded them
PARENT = {'_Z12strrt_kernelILi0ELi0EEv6StArgs': (248, 106, 0, 0, 17408),
          '_Z12strrt_kernelILi2ELi0EEv6StArgs': (183, 106, 0, 0, 17408),
          '_Z12strrt_kernelILi3ELi0EEv6StArgs': (188, 106, 0, 0, 17408),
          '_Z12strrt_kernelILi7ELi0EEv6StArgs': (208, 106, 0, 0, 17408),
          '_Z12strrt_kernelILi7ELi1EEv6StArgs': (221, 104, 0, 0, 17408),
          '_Z17strrt_init_kernelILi0EEvPiPKfS2_S2_S2_8StMovingiiii': (108, 106, 0, 0, 17408),
          '_Z17strrt_init_kernelILi1EEvPiPKfS2_S2_S2_8StMovingiiii': (108, 106, 0, 0, 17408),
          '_Z18moving_cost_kernelILb0EEvPKfS1_PfS2_S2_iiiffiiiii': (106, 106, 0, 0, 0),
          '_Z18moving_cost_kernelILb1EEvPKfS1_PfS2_S2_iiiffiiiii': (226, 106, 0, 0, 0),
          '_Z19moving_check_kernelPKfS0_PhPfiiiiiii': (105, 106, 0, 0, 0),
          '_Z21path_time_plan_kernel6PtArgs': (96, 106, 0, 0, 256)}


def test_layout_header_is_generated_and_the_numbers_are_pinned():
    from motion_planning_baselines_amd import _lib, build, model_gen, ops, st_shortcut_layout as L
    text = open(model_gen.ST_SHORTCUT_LAYOUT_HEADER).read()
    assert text == model_gen.st_shortcut_layout_header_text()
    assert not model_gen.stale_headers()
    assert L.STATUS == ('OK', 'NOT_VALID', 'BUFFER_CHANGED', 'INPUT_IN_COLLISION', 'INPUT_TOO_FAST')
    assert L.LOG_CODES == ('IDLE', 'SKIP_SHORT', 'SKIP_FAST', 'SKIP_STRAIGHT', 'REJECT', 'ACCEPT')
    assert (L.STS_LOG_INDEX_SHIFT, L.STS_PHILOX_TAG, L.STS_MIN_ROWS, L.STS_MAX_ROWS, L.STS_MAX_ITERS) == (8, 0x53545343, 3, 1024, 1 << 20)
    for line in ('#define MPB_STS_OK 0', '#define MPB_STS_INPUT_TOO_FAST 4', '#define MPB_STS_LOG_ACCEPT 5', '#define MPB_STS_PHILOX_TAG 0x53545343',
                 '#define MPB_STS_MAX_ROWS 1024', '#define MPB_STS_GATE_LIMIT 0x1.0001p+0f', '#define MPB_STS_LDS_BYTES(R, D)'):
        assert line in text, line
    # the gate's limit: the same fp32 number in C and in Python, exact, and what the derivation asks of it
    assert float.fromhex(L.STS_GATE_LIMIT_C.rstrip('f')) == L.STS_GATE_LIMIT == float(f32(L.STS_GATE_LIMIT)) == 1 + 2.0 ** -16
    assert 1e-5 + 2e-7 < 2.0 ** -16
    # the macro and lds_bytes say the same: evaluated as Python (integer division spelled //)
    expr = L.C_LDS_BYTES.replace('/', '//').replace('MPB_STS_STATIC_LDS_BYTES', str(L.STS_STATIC_LDS_BYTES))
    for R, D in ((3, 1), (33, 2), (130, 7), (1024, 12)):
        assert eval(expr, dict(R=R, D=D)) == L.lds_bytes(R, D)
    assert L.traj_lds_bytes(1024, 12) == 48 * 1024 and L.lds_bytes(1024, 12) <= L.STS_MAX_LDS_BYTES
    assert 'mpb_st_shortcut_layout.h' in open(build.__file__).read() and 'mpb_st_shortcut.hip' in build.SOURCES
    assert 'mpb_st_shortcut' in _lib.SIGNATURES and hasattr(_lib.lib(), 'mpb_st_shortcut')
    mpb_h = open(os.path.join(ROOT, 'include', 'mpb.h')).read()
    assert 'int mpb_st_shortcut(' in mpb_h and '#include "mpb_st_shortcut_layout.h"' in mpb_h
    assert (_lib.lib().mpb_version() & 0xFFFF) == _lib.ABI_VERSION == 7                       # additive: the ABI version stays
    assert ops.STS_STATUS_NAMES is L.STATUS and ops.STS_LOG_ACCEPT == C.ACCEPT and ops.STShortcut._fields == ('trajs', 'ok', 'status', 'first_bad', 'stats', 'log')


def test_kernel_resources():
    """csrc/kernel_resources.json: the five instantiations of the new kernel have 0 B of scratch and no vector spills; the STRRT, moving
    obstacle and path-timing kernels -- two of them now read strrt_collides / strrt_tau from a shared header -- came out as at the parent
    commit."""
    from motion_planning_baselines_amd import build
    build.build(verbose=False)
    res = json.load(open(build.RESOURCES))
    new = {k: v for k, v in res.items() if k.startswith('_Z18st_shortcut_kernel')}
    assert len(new) == 5, list(new)
    for name, r in new.items():
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['lds'] == 17408, (name, r)
    for name, want in PARENT.items():
        r = res[name]
        assert (r['vgprs'], r['sgprs'], r['scratch'], r['vgpr_spill'], r['lds']) == want, (name, r)


@pytest.mark.parametrize('name', C.SETS)
def test_restatement_guarantee_and_fp64_cap(name):
    """On every input set of the GPU tests the restated pass keeps the guarantee (free on every row, end rows kept, written steps within
    w (1 + VEL_SLACK), the fp64 length within the derived slack of not increasing), refuses exactly the trajectories made to be refused,
    equals itself followed from its own log -- and the cap, a condition on the inputs and not a measurement: by fp64 alone at most 2 % of
    its decisions are undecidable, so the GPU test cannot hide behind the cap."""
    r = C.restated(name)
    s = r.s
    C.check_guarantee(s.p, s.trajs, r.r32)
    C.same_bits(r.r32, r.r64, name)
    for n in range(s.N):
        assert (int(r.r32.status[n]), int(r.r32.first_bad[n])) == s.expect.get(n, (C.OK, -1)), (name, n, r.r32.status[n], r.r32.first_bad[n])
    share = C.undecidable_share(r.seen)
    ok = r.r32.status == C.OK
    ratio = r.r32.stats[ok, 3] / r.r32.stats[ok, 2]
    print(f'{name}: N {s.N}, R {s.p.R}, {len(r.seen)} scans audited, {share:.4f} undecidable, accepted {int(r.r32.stats[ok, 1].sum())} of '
          f'{int(r.r32.stats[ok, 0].sum())} checked, length after / before {ratio.min():.2f} .. {ratio.max():.2f}')
    assert len(r.seen) > 0 and share <= C.CAP
    assert (r.r32.stats[ok, 1] > 0).any() or name == 'tiny3'
    if name == 'tiny3':                              # its one candidate puts row 1 into the sphere in the gap
        assert set(r.r32.log[0].tolist()) == {C.SKIP_SHORT, C.REJECT | (1 << C.SHIFT)}


def test_every_status_and_log_code_occurs():
    """Across the sets: every status but BUFFER_CHANGED (which only a device buffer can have: tests/test_gpu_st_shortcut.py) and every
    log code; SKIP_FAST among them at least on the hand-made case below."""
    statuses, codes = set(), set()
    for name in C.SETS:
        r = C.restated(name).r32
        statuses |= set(r.status.tolist())
        codes |= set((r.log & ((1 << C.SHIFT) - 1)).ravel().tolist())
    assert statuses == {C.OK, C.NOT_VALID, C.INPUT_IN_COLLISION, C.INPUT_TOO_FAST}
    assert codes >= {C.IDLE, C.SKIP_SHORT, C.SKIP_STRAIGHT, C.REJECT, C.ACCEPT}, codes
    assert codes | _hand_made_codes() == set(range(len(C.L.LOG_CODES)))


def _hand_made_codes():
    """SKIP_FAST: a straight line whose every step is w (1 + 6e-6) -- within the gate's 2^-16, but b - a rows of it are more than
    (b - a) w; SKIP_STRAIGHT: an exactly representable straight line; a second pass over a shortcut line logs only skips."""
    p = C.scene('ptgate')
    R, w = p.R, p.w
    seen = set()
    x = -0.7 + float(w[0]) * (1 + 6e-6) * np.arange(R)
    fast = np.stack([x, np.zeros(R)], -1).astype(f32)[None]
    draws = np.array([[[0, R - 1], [3, 40], [7, 8], [20, 5]]], np.int32)
    free = lambda n, tr: -1
    r = C.run(p, fast, 4, free, lambda *a: pytest.fail('nothing may be evaluated'), draws=draws)
    assert r.status[0] == C.OK and r.log[0].tolist() == [C.SKIP_FAST, C.SKIP_FAST, C.SKIP_SHORT, C.SKIP_FAST], r.log
    assert np.array_equal(r.trajs, fast) and r.stats[0, 0] == 0
    seen |= set(r.log[0].tolist())
    line = np.stack([-0.5 + 2.0 ** -6 * np.arange(R), np.full(R, 0.0625)], -1).astype(f32)[None]
    r = C.run(p, line, 4, free, lambda *a: pytest.fail('nothing may be evaluated'), draws=draws)
    assert r.log[0].tolist() == [C.SKIP_STRAIGHT, C.SKIP_STRAIGHT, C.SKIP_SHORT, C.SKIP_STRAIGHT], r.log
    seen |= set(r.log[0].tolist())
    # a zig-zag, shortcut whole by its first draw (nothing collides); the second pass finds a straight line
    zig = line.copy()
    zig[0, 1:-1:2, 1] += f32(0.01)
    judge = lambda n, it, cand, rows: -1
    first = C.run(p, zig, 4, free, judge, draws=draws)
    assert first.log[0, 0] == C.ACCEPT and first.stats[0, 1] == 1 and first.rows_written[0] == R - 2
    second = C.run(p, first.trajs, 4, free, lambda *a: pytest.fail('nothing may be evaluated'), draws=draws)
    assert set(second.log[0].tolist()) <= {C.SKIP_SHORT, C.SKIP_STRAIGHT, C.SKIP_FAST} and np.array_equal(second.trajs, first.trajs)
    return seen


def test_skip_fast_and_skip_straight_on_hand_made_cases():
    assert _hand_made_codes() >= {C.SKIP_FAST, C.SKIP_STRAIGHT, C.SKIP_SHORT}


def test_draws_and_max_span():
    """device_draws against a Philox counter written out by hand; the clamp of recorded draws and of max_span as defined."""
    from motion_planning_baselines_amd import st_shortcut_layout as L
    seed, R = (5 << 32) | 77, 33
    d = C.device_draws(seed, 3, 4, R, offset=9)
    x, y, _, _ = C.philox4x32_10((9 + 2, 3, 0x53545343, 0), (77, 5))
    assert L.STS_PHILOX_TAG == 0x53545343 and d[2, 3].tolist() == [(x * R) >> 32, (y * R) >> 32]
    assert d.min() >= 0 and d.max() <= R - 1 and len(np.unique(d)) > 4
    assert not np.array_equal(d, C.device_draws(seed, 3, 4, R, offset=10)) and np.array_equal(d[1:], C.device_draws(seed, 2, 4, R, offset=10))
    assert C.span_of((30, 4), R) == (4, 30) and C.span_of((-7, 99), R) == (0, 32) and C.span_of((4, 30), R, max_span=5) == (4, 9)
    assert C.span_of((4, 6), R, max_span=5) == (4, 6) and C.span_of((9, 9), R, max_span=1) == (9, 9)
    # max_span = 1 leaves nothing to shortcut: every iteration is SKIP_SHORT
    s = C.inputs('tiny3')
    r = C.restate32(s.p, s.trajs, 8, seed=1, max_span=1)
    assert (r.log == C.SKIP_SHORT).all() and np.array_equal(r.trajs, s.trajs)
