"""Trajectory validation without a GPU: the host side of mpb_traj_collision_stats answers (export, the argument checks in
their order, the empty batch), and the ops wrapper refuses CPU tensors."""
import ctypes
import types

import pytest
import torch

INVALID, UNSUPPORTED = 1, 2                                      # include/mpb.h MPB_E_INVALID, MPB_E_UNSUPPORTED
NAME = 'mpb_traj_collision_stats'


def _call(h, trajs=0, row_stride=7, geom=0, n_interp=5, count=0, first=0, gap=0, flags=0, N=10, H=8, D=7):
    p = ctypes.c_void_p
    rc = h.mpb_traj_collision_stats(p(trajs), row_stride, p(geom), 0, n_interp, p(count), p(first), p(gap), p(flags), N, H, D, p(0))
    return rc, h.mpb_last_error().decode()


def test_library_exports_the_symbol():
    from motion_planning_baselines_amd import _lib
    h = _lib.lib()
    assert NAME in _lib.SIGNATURES and hasattr(h, NAME)
    assert len(_lib.SIGNATURES[NAME]) == 13
    assert (h.mpb_version() & 0xFFFF) == _lib.ABI_VERSION == 7   # additive: the ABI version does not move


def test_argument_checks_answer_in_order_and_name_the_function():
    from motion_planning_baselines_amd import _lib
    h = _lib.lib()
    # nothing is launched by any of these calls: every pointer is null or a host address that is never dereferenced
    rc, msg = _call(h, D=13)
    assert rc == UNSUPPORTED and msg.startswith(NAME) and 'MPB_MAX_DOF' in msg
    rc, msg = _call(h, D=13, H=1)                                # wrong in two ways: the earlier check answers
    assert rc == UNSUPPORTED and 'MPB_MAX_DOF' in msg
    for bad in (dict(N=-1), dict(H=1), dict(D=0), dict(n_interp=-1), dict(row_stride=6), dict(H=2 ** 30, n_interp=3),
                dict(H=2, n_interp=2 ** 31 - 1)):
        rc, msg = _call(h, **bad)
        assert rc == INVALID and msg.startswith(NAME) and 'bad shape' in msg, (bad, rc, msg)
    rc, msg = _call(h, H=2, n_interp=2 ** 31 - 3)                # P = 2^31 - 1 still fits: the next check answers
    assert rc == INVALID and 'null pointer' in msg
    rc, msg = _call(h, N=0, H=1)                                 # a bad shape is refused before the empty batch returns
    assert rc == INVALID and 'bad shape' in msg
    assert _call(h, N=0)[0] == 0                                 # N = 0: MPB_OK with every pointer null
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    a += (-a) % 16
    ok = dict(trajs=a, geom=a, count=a, first=a, gap=a)
    for missing in ok:
        rc, msg = _call(h, **{**ok, missing: 0})
        assert rc == INVALID and msg.startswith(NAME) and 'null pointer' in msg, (missing, rc, msg)
    rc, msg = _call(h, **{**ok, 'geom': a + 4})
    assert rc == INVALID and msg.startswith(NAME) and '16-byte aligned' in msg
    rc, msg = _call(h, **{**ok, 'geom': a + 4, 'trajs': 0})      # null before alignment
    assert rc == INVALID and 'null pointer' in msg


def test_ops_wrapper_refuses_cpu_tensors():
    from motion_planning_baselines_amd import ops
    from motion_planning_baselines_amd._lib import MPBError
    geom = types.SimpleNamespace(n_dof=2, buf=torch.zeros(16), flags=0)
    with pytest.raises(MPBError, match='no CPU fallback'):
        ops.traj_collision_stats(torch.zeros(4, 8, 2), geom)
    with pytest.raises(MPBError, match='no CPU fallback'):
        ops.traj_collision_stats(torch.zeros(4, 8, 4), geom, n_interp=0, with_flags=True)
