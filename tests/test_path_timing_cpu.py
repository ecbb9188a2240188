"""Host side of path timing among moving obstacles (ops.path_time_plan, csrc/mpb_path_timing.hip): the restated recurrence against the
outright enumeration of every monotone timing, the fixed-point segment costs on hand-made paths, the conditions the GPU tests' scenes
are held to -- by the fp64 oracle alone --, the generated layout header and what the compiler made of the kernel.  No GPU."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT
import path_timing_checks as T

f32 = np.float32


def test_recurrence_equals_exhaustive_enumeration_on_random_tables():
    """S, R <= 6, random free tables and random segment costs (some zero, some exactly 1): FOUND iff a monotone timing exists, the arrival
    row is the earliest of any, idx is the one the tie-break names; otherwise the status is the first of START_BLOCKED, GOAL_NOT_HOLDABLE,
    NO_TIMING that applies."""
    rng = np.random.RandomState(3)
    seen = {k: 0 for k in range(len(T.PL.STATUS))}
    ties = 0
    for trial in range(600):
        S, R = rng.randint(2, 7), rng.randint(2, 7)
        w = np.array([1.0], f32)
        steps = rng.choice([0.0, 0.25, 0.5, 1.0], S - 1, p=[0.15, 0.35, 0.35, 0.15])     # exact in fp32: c(i) = the step
        P = np.concatenate([[0.0], np.cumsum(steps)]).astype(f32)[:, None]
        F = rng.uniform(size=(R, S)) < rng.choice([0.6, 0.8, 0.95])
        if trial % 3:
            F[0, 0] = F[R - 1, S - 1] = True
        got, want = T.restate(P, w, F), T.enumerated_answer(P, w, F)
        seen[got.status] += 1
        if want is None:
            expect = T.START_BLOCKED if not F[0, 0] else T.GOAL_NOT_HOLDABLE if not F[R - 1, S - 1] else T.NO_TIMING
            assert got.status == expect and got.arrival == -1 and (got.idx == -1).all() and not got.traj.any(), (trial, got.status, expect)
            continue
        assert got.status == T.FOUND and got.arrival == want[0], (trial, got.arrival, want[0])
        assert np.array_equal(got.idx, want[1]), (trial, got.idx, want[1])
        assert np.array_equal(got.traj, P[got.idx])
        ties += len([1 for a, _ in T.enumerate_timings(P, w, F) if a == want[0]]) > 1
    assert seen[T.FOUND] > 100 and seen[T.START_BLOCKED] > 10 and seen[T.GOAL_NOT_HOLDABLE] > 10 and seen[T.NO_TIMING] > 10, seen
    assert ties > 50, ties                                          # the tie-break was exercised


def test_segment_too_long_wins_over_the_table():
    P, w = np.array([[0.0], [0.5], [1.75]], f32), np.array([1.0], f32)
    for F in (np.ones((4, 3), bool), np.zeros((4, 3), bool)):
        assert T.restate(P, w, F).status == T.SEGMENT_TOO_LONG and T.enumerated_answer(P, w, F) is None


def test_fixed_point_costs_and_interval_starts_on_hand_made_paths():
    w = np.array([0.5, 0.25], f32)
    # segments: joint 1 decides (0.125 / 0.25 = 0.5); exactly 1 on joint 0; zero length; 2^-17 of a row rounds UP to one unit
    P = np.array([[0.0, 0.0], [0.125, 0.125], [0.625, 0.125], [0.625, 0.125], [0.625 + 2.0 ** -18, 0.125]], np.float64).astype(f32)
    assert P[4, 0] > P[3, 0]
    cfix, C, lo, too_long = T.cfix_lo(P, w)
    assert not too_long
    assert cfix.tolist() == [32768, 65536, 0, 1]
    assert C.tolist() == [0, 32768, 98304, 98304, 98305]
    assert lo.tolist() == [0, 0, 1, 1, 2]                            # sample 4 is one unit too far from sample 1
    # just above 1: the next float32 after 0.5 over w = 0.5
    Q = np.array([[0.0, 0.0], [np.nextafter(f32(0.5), f32(1.0)), 0.0]], f32)
    assert T.cfix_lo(Q, w)[3] and not T.cfix_lo(np.array([[0.0, 0.0], [0.5, 0.0]], f32), w)[3]
    for bad in (np.inf, np.nan):
        assert T.cfix_lo(np.array([[0.0, 0.0], [bad, 0.0]], f32), w)[3]
    # the sum of per-segment maxima bounds every joint's travel: any admitted row step stays within w
    rng = np.random.RandomState(0)
    P = np.cumsum(rng.uniform(-0.2, 0.2, (40, 2)), 0).astype(f32)
    _, C, lo, too_long = T.cfix_lo(P, w)
    assert not too_long
    for i in range(40):
        assert (np.abs(P[i].astype(np.float64) - P[lo[i]:i + 1].astype(np.float64)) <= w.astype(np.float64) * (1 + T.VEL_SLACK)).all()


@pytest.mark.parametrize('name', T.ALL)
def test_scenes_are_decidable_and_say_what_they_are_for(name):
    """From the fp64 restatement alone: at most CAP of a scene's cells lie within UNDECIDED of the hinge boundary; the status scenes have
    the status they are named for, the gate scene waits and arrives later than with the sphere away."""
    r = T.reference(name)
    print(f'{name}: N {r.s.N} S {r.s.S} R {r.s.R}, undecidable share {r.share:.5f}, statuses {[t.status for t in r.timing]}, '
          f'arrivals {[t.arrival for t in r.timing]}, free share {np.mean([f.mean() for f in r.F]):.3f}')
    assert r.share <= T.CAP
    if name in T.STATUS_SCENES:
        assert r.timing[0].status == T.STATUS_SCENES[name]
    if name == 'gate':
        t, away = r.timing[0], T.reference('gate_away').timing[0]
        assert away.arrival == r.s.S - 1 and t.arrival == T.GATE['b'] + 1 + (r.s.S - 1 - 13) > away.arrival
        assert (t.idx[12:21] == 12).all() and (np.diff(t.idx) >= 0).all()
    if name in T.SHAPES:
        assert any(t.status == T.FOUND for t in r.timing), 'a shape scene must time at least one path'
        mixed = [0 < f.mean() < 1 for f in r.F]
        assert any(mixed) or name == 'pm2_2_2', 'the table of a shape scene must hold both answers'


def test_layout_header_is_generated_and_the_numbers_are_pinned():
    from motion_planning_baselines_amd import _lib, build, model_gen, path_timing_layout as L
    assert open(model_gen.PATH_TIMING_LAYOUT_HEADER).read() == model_gen.path_timing_layout_header_text()
    assert not model_gen.stale_headers()
    assert L.STATUS == ('FOUND', 'START_BLOCKED', 'GOAL_NOT_HOLDABLE', 'SEGMENT_TOO_LONG', 'NO_TIMING', 'BUFFER_CHANGED')
    assert (L.PT_MIN_SAMPLES, L.PT_MAX_SAMPLES, L.PT_MIN_ROWS, L.PT_MAX_ROWS, L.PT_THREADS, L.PT_COST_ONE) == (2, 256, 2, 1024, 256, 65536)
    text = open(model_gen.PATH_TIMING_LAYOUT_HEADER).read()
    for line in ('#define MPB_PT_FOUND 0', '#define MPB_PT_NO_TIMING 4', '#define MPB_PT_MAX_SAMPLES 256', '#define MPB_PT_MAX_ROWS 1024',
                 '#define MPB_PT_MAX_LDS_BYTES 163840', '#define MPB_PT_LDS_WORDS(L, S, R)'):
        assert line in text, line
    # the macro and lds_words say the same: evaluated as Python (integer division spelled //)
    expr = L.C_LDS_WORDS.replace('/', '//').replace('MPB_PT_SCRATCH_WORDS', str(L.PT_SCRATCH_WORDS))
    for Lk, S, R in ((1, 2, 2), (31, 256, 1024), (25, 33, 65), (64, 256, 1024)):
        assert eval(expr, dict(L=Lk, S=S, R=R)) == L.lds_words(Lk, S, R)
    assert L.lds_bytes(31, 256, 1024) <= L.PT_MAX_LDS_BYTES < L.lds_bytes(64, 256, 1024)       # the Panda fits at the limits, 64 spheres do not
    assert 'mpb_path_timing_layout.h' in open(build.__file__).read() and 'mpb_path_timing.hip' in build.SOURCES
    assert 'mpb_path_time_plan' in _lib.SIGNATURES and hasattr(_lib.lib(), 'mpb_path_time_plan')
    assert 'int mpb_path_time_plan(' in open(os.path.join(ROOT, 'include', 'mpb.h')).read()
    assert (_lib.lib().mpb_version() & 0xFFFF) == _lib.ABI_VERSION == 7                       # additive: the ABI version stays


def test_the_kernel_keeps_out_of_scratch():
    """build() records what the compiler made of every kernel (csrc/kernel_resources.json): the one new kernel keeps its chain state, its
    sphere group and its eight interval masks in registers -- 0 B of scratch, no vector spills."""
    from motion_planning_baselines_amd import build
    build.build(verbose=False)
    res = json.load(open(build.RESOURCES))
    hits = {k: v for k, v in res.items() if 'path_time_plan_kernel' in k}
    assert len(hits) == 1, list(hits)
    for name, r in hits.items():
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0, (name, r)
