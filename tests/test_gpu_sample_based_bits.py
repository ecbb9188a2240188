"""GPU: the sample-based kernels leave behind the bits tests/golden/sample_based_bits.npz recorded from the library of the commit named
in it (tests/golden/make_sample_based_bits.py; the cases: tests/sample_based_bits.py) -- trees, parents, counts, pools, header words,
paths, lengths, costs of RRT-Connect and RRT* in every instantiation, and one D = 3 launch of the roadmap's knn and edge kernels and of
the shortcut kernel.  Equality of every word; a difference is named by (case, array, problem, index)."""
import numpy as np
import pytest

from conftest import load_golden
import sample_based_bits as S

pytestmark = pytest.mark.gpu
_FIXTURE = {}


def _fixture():
    if not _FIXTURE:
        _FIXTURE.update(load_golden('sample_based_bits'))
    return _FIXTURE


def _compare(case, want, got):
    assert sorted(want) == sorted(got), (case, sorted(set(want) ^ set(got)))
    for name in sorted(want):
        a, b = want[name], got[name]
        assert a.shape == b.shape and a.dtype == b.dtype, (case, name, a.shape, b.shape, a.dtype, b.dtype)
        if not np.array_equal(a, b):
            at = tuple(int(i) for i in np.argwhere(a != b)[0])
            pytest.fail(f'{case}: array {name!r} differs first at problem {at[0] if at else 0}, index {at}: recorded {a[at]:#x}, '
                        f'this library {b[at]:#x} ({int((a != b).sum())} words differ)')


@pytest.mark.parametrize('kind,name', S.CASES)
def test_the_rrt_kernels_leave_the_recorded_bits(gpu_device, kind, name):
    f = _fixture()
    starts, goals, radius, seed = S.unpack_inputs(f[f'{kind}.{name}.inputs'])
    geom, _, _, pool, _ = S.scene(name, gpu_device)
    got = S.run(kind, geom, gpu_device, starts, goals, pool, radius, seed, (kind, name) == S.INFORMED)
    want = S.unpack(f[f'{kind}.{name}'], got)
    cond, n_nodes = S.conditions(kind, want, radius)
    assert all(cond.values()), (kind, name, cond)                       # the recorded run reaches every loop's second trip
    _compare(f'{kind} {name}', want, got)


def test_the_d3_roadmap_and_shortcut_kernels_leave_the_recorded_bits(gpu_device):
    got = S.run_extra(gpu_device)
    _compare('D = 3 knn / edge check / shortcut', S.unpack(_fixture()[S.EXTRA], got), got)


def test_the_fixture_names_its_parent_commit_and_stays_small():
    import os
    from conftest import GOLDEN
    f = _fixture()
    commit = bytes(f['parent_commit']).decode()
    assert len(commit) == 40 and set(commit) <= set('0123456789abcdef'), commit
    assert all(v.dtype in (np.uint32, np.uint8) for v in f.values())
    assert os.path.getsize(os.path.join(GOLDEN, 'sample_based_bits.npz')) <= 91654      # the largest RRT golden
