"""CPU: the host restatement of torch's CPU Mersenne Twister (motion_planning_baselines_amd/mt19937.py) against live torch --
uniforms and state bit for bit, the jump ahead against sequential advance, the state bytes, normal_()'s tail rule -- and the
device draw's segment layout, restated on the host, against torch's draws."""
import numpy as np
import pytest
import torch

from motion_planning_baselines_amd import mt19937 as MT


def _state():
    return MT.MTState.from_bytes(torch.get_rng_state())


def _mid_array(seed, k):
    torch.manual_seed(seed)
    if k:
        torch.empty(k).uniform_()
    return _state()


@pytest.mark.parametrize('seed,k', [(0, 0), (7, 0), (2 ** 32 + 5, 0), (7, 100), (123, 623), (123, 624), (9, 1000)])
def test_uniform_and_state_bit_for_bit(seed, k):
    st = _mid_array(seed, k)
    for n in (1, 17, 624, 5000):
        u, st = st.uniform(n)
        ref = torch.empty(n).uniform_().numpy()
        assert np.array_equal(u.view(np.uint32), ref.view(np.uint32)), n
        assert st.to_bytes() == bytes(torch.get_rng_state().numpy().tobytes()), n


def test_seeding_and_state_layout():
    torch.manual_seed(7)
    st = _state()
    assert st.to_bytes() == MT.MTState.seeded_with(7).to_bytes()[:24 + 8 * 624] + st.tail
    assert (st.next, st.left, st.pos) == (0, 1, 624)
    torch.empty(100).normal_()
    st = _state()
    assert (st.left, st.next) == (509, 116)                   # 100 normals consume 116 words


def _advance(st, n):
    """The array and index n words later, by whole twists (no output kept)."""
    p = st.pos
    arr, k = st.arr, p
    left = n
    while left:
        if k == MT.N:
            arr, k = MT.twist(arr), 0
        take = min(left, MT.N - k)
        k += take
        left -= take
    return arr, k


@pytest.mark.parametrize('k', [0, 100])
def test_jump_equals_sequential_advance(k):
    st = _mid_array(11, k)
    assert st.pos == (624 if k == 0 else k)
    prefix, _ = st.raw(MT.PREFIX_WORDS)
    for n in (1, 623, 624, 625, 19937, 10 ** 6 + 7, 3670016 * 20):
        win = MT.jump_raw(prefix, n)
        arr, j = _advance(st, n)
        # the 624 words from word n of the draw on: the rest of the array after n words, then its twist
        seq = np.concatenate([arr, MT.twist(arr)])[j:j + MT.N]
        assert np.array_equal(win, seq), n


def test_char_poly_is_regenerated():
    phi = MT.char_poly()
    assert phi.bit_length() - 1 == MT.DEG and phi & 1
    assert bin(phi).count('1') == 135                          # mt19937's characteristic polynomial has 135 terms
    # t^DEG mod phi is phi without its leading term; a jump by the period of a 624-word shift is consistent with twisting
    assert MT.jump_poly(MT.DEG) == phi ^ (1 << MT.DEG)


def test_state_round_trips_through_set_rng_state():
    st = _mid_array(3, 333)
    b = st.to_bytes()
    torch.manual_seed(99)
    torch.set_rng_state(torch.frombuffer(bytearray(b), dtype=torch.uint8).clone())
    assert bytes(torch.get_rng_state().numpy().tobytes()) == b
    u, _ = st.uniform(2000)
    assert np.array_equal(torch.empty(2000).uniform_().numpy().view(np.uint32), u.view(np.uint32))


def _ulp_ok(a, b):
    ulp = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    return (ulp <= 4) | (np.abs(a.astype(np.float64) - b) <= 2.0 ** -22)


@pytest.mark.parametrize('n', [16, 17, 100, 3670016])
def test_normal_within_ulp_and_words_consumed(n):
    st = _mid_array(5, 77)
    out, after = st.normal(n)
    ref = torch.empty(n).normal_().numpy()
    assert _ulp_ok(out, ref).all()
    assert after.to_bytes() == bytes(torch.get_rng_state().numpy().tobytes())
    _, expect = st.raw(n + (16 if n % 16 else 0))
    assert after.to_bytes() == expect.to_bytes()


def _device_layout_restated(st, n, n_calls, uniform):
    """The device draw (csrc/mpb_mt19937.h) restated: prefix, jump by the packed lists, segments, final array."""
    polys, rows, total, _ = MT.jump_tables(n, n_calls, MT.segments_per_call(n, n_calls), uniform)
    idx, cnt = MT.jump_lists(polys)
    pos = st.pos
    prefix, _ = st.raw(MT.PREFIX_WORDS)
    xs = np.concatenate([prefix, np.zeros(MT.N, np.uint32)])
    wins = []
    for r in range(len(rows) + 1):
        acc = np.zeros(MT.N, np.uint32)
        for i in idx[r, :cnt[r]]:
            acc ^= xs[i:i + MT.N]
        wins.append(acc)
    out = np.full((n_calls, n), np.nan, np.float32)
    rem, Q = n & 15, n >> 4
    for s, (_, c, q0, nq, last) in enumerate(rows):
        tail = last and rem
        tw, tlen, tout = (16 * (Q - q0), rem, 16 * Q) if uniform else (n - 16 * q0, 16, n - 16)
        clip = n - 16 if (not uniform and rem) else n
        words = tw + tlen if tail else 16 * nq
        seq, a = [wins[s]], wins[s]
        while sum(len(x) for x in seq) < words + 16:
            a = MT.twist(a)
            seq.append(a)
        u = MT.uniform_from_words(MT.temper(np.concatenate(seq)))

        def put(w0, e0, lim):
            ch = u[w0:w0 + 16] if uniform else MT.box_muller(u[w0:w0 + 16])
            for jj in range(16):
                if e0 + jj < lim:
                    out[c, e0 + jj] = ch[jj]
        for qq in range(nq):
            put(16 * qq, 16 * (q0 + qq), clip)
        if tail:
            put(tw, tout, tout + tlen)
    fi = MT.final_index(pos, total)
    arr = st.arr if fi < 0 else np.concatenate([wins[-1], MT.twist(wins[-1])])[fi:fi + MT.N]
    return out, MT.state_after(st, total, arr)


@pytest.mark.parametrize('n,n_calls', [(16, 2), (17, 3), (100, 5), (33, 40), (5000, 2)])
@pytest.mark.parametrize('uniform', [True, False])
@pytest.mark.parametrize('k', [0, 100, 623])
def test_device_layout_restated_against_torch(n, n_calls, uniform, k):
    st = _mid_array(n + n_calls, k)
    out, after = _device_layout_restated(st, n, n_calls, uniform)
    ref = np.stack([(torch.empty(n).uniform_() if uniform else torch.empty(n).normal_()).numpy() for _ in range(n_calls)])
    assert after.to_bytes() == bytes(torch.get_rng_state().numpy().tobytes())
    if uniform:
        assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))
    else:
        assert _ulp_ok(out, ref).all()


def test_jump_tables_build_time_at_c3():
    n = 128 * 32 * 14 * 64
    MT.jump_tables.cache_clear()
    polys, rows, total, secs = MT.jump_tables(n, 16, MT.segments_per_call(n, 16))
    assert total == 16 * n and polys.shape == (len(rows) + 1, MT.POLY_WORDS)
    assert secs < 30.0, secs
