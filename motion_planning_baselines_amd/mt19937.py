"""Host side of noise='mt19937': torch's CPU Mersenne Twister restated in numpy, its state bytes, and the jump-ahead tables
the device generator (csrc/mpb_mt19937.hip) reads.

The stream.  torch's generator keeps mt19937's 624-word array A, an index `next` and a countdown `left`.  Let x[b .. b+623] = A
and continue the raw (untempered) word sequence by the recurrence x[k+624] = x[k+397] ^ twist(x[k], x[k+1]); torch's in-place
twist of the array computes exactly these words.  The next word the generator tempers and returns is x[b+p] with
p = 624 if left == 1 (the array is about to be twisted; this includes the freshly seeded state) else p = next, p in [1, 624].

Jump ahead (Haramoto et al. 2008).  The recurrence is linear over GF(2) with characteristic polynomial phi of degree 19 937;
phi is found once by Berlekamp-Massey on one output bit.  Every word x[m] with m > b is a linear function of the 19 937-bit
state, so the word sequence from x[b+1] on satisfies the recurrence phi: with t^n mod phi = sum_i g_i t^i,
x[o + n + j] = XOR_{g_i = 1} x[o + i + j] for every o > b.  The device takes the PREFIX x[b+p .. b+p+20 559] (19 937 + 623
words, from the start state by ~33 twists) and forms any 624-word window n words later as the XOR of the prefix windows at
the set coefficients.  The offsets are measured from the first word drawn, so the tables depend on the draw's shape only.

normal_() on a contiguous fp32 tensor of n >= 16 elements (ATen normal_fill): n uniforms (w & 0xFFFFFF) * 2^-24, Box-Muller on
every full 16-chunk (u1 = 1 - u[j], u2 = u[j+8], j < 8), and if n % 16 != 0 the last 16 outputs are recomputed from 16 fresh
words: a call consumes n + 16 [n % 16 != 0] words.
"""
import functools
import time

import numpy as np

N, M = 624, 397
MATRIX_A = 0x9908B0DF
UPPER, LOWER = 0x80000000, 0x7FFFFFFF
DEG = 19937                      # degree of the characteristic polynomial: the state's bits
PREFIX_WORDS = DEG + N - 1       # 20 560: the windows x[i .. i + 623] for i < DEG
POLY_WORDS = N                   # a jump polynomial packed in 624 uint32 words (19 968 bits, coefficient i in word i >> 5)
STATE_BYTES = 5056               # torch.get_rng_state() of the CPU generator
_OFF_SEED, _OFF_LEFT, _OFF_SEEDED, _OFF_NEXT, _OFF_STATE = 0, 8, 12, 16, 24
TWO_PI = np.float32(2.0 * np.pi)  # the vectorised normal_fill_16: theta = fl32(2 pi) * u2 in fp32


# ---- the generator, sequentially --------------------------------------------------------------------------------------------
def _tw(a, b):
    y = (a & UPPER) | (b & LOWER)
    return (y >> 1) ^ np.where(b & 1, np.uint32(MATRIX_A), np.uint32(0)).astype(np.uint32)


def twist(arr):
    """torch's next_state(): the array's next 624 raw words, x[b+624 .. b+1247] from x[b .. b+623]."""
    a = np.asarray(arr, dtype=np.uint32)
    new = np.empty(N, np.uint32)
    new[:227] = a[M:] ^ _tw(a[:227], a[1:228])
    new[227:454] = new[:227] ^ _tw(a[227:454], a[228:455])
    new[454:623] = new[227:396] ^ _tw(a[454:623], a[455:624])
    new[623] = new[396] ^ _tw(a[623:624], new[0:1])[0]
    return new


def temper(w):
    y = np.asarray(w, dtype=np.uint32).copy()
    y ^= y >> np.uint32(11)
    y ^= (y << np.uint32(7)) & np.uint32(0x9D2C5680)
    y ^= (y << np.uint32(15)) & np.uint32(0xEFC60000)
    y ^= y >> np.uint32(18)
    return y


class MTState:
    """torch's mt19937 state: the array, `next`, `left` (and the seed fields, carried unchanged)."""

    def __init__(self, arr, next_, left, seed=0, seeded=1, tail=None):
        self.arr = np.array(arr, dtype=np.uint32)
        self.next, self.left, self.seed, self.seeded = int(next_), int(left), int(seed), int(seeded)
        self.tail = tail                 # the rest of torch's state bytes (the scalar normal caches), carried through

    @classmethod
    def seeded_with(cls, seed):
        """init_genrand(seed & 0xffffffff), as torch.manual_seed(seed)."""
        mt = np.empty(N, np.uint32)
        mt[0] = seed & 0xFFFFFFFF
        for j in range(1, N):
            prev = int(mt[j - 1])
            mt[j] = (1812433253 * (prev ^ (prev >> 30)) + j) & 0xFFFFFFFF
        return cls(mt, 0, 1, seed=seed & 0xFFFFFFFF)

    @classmethod
    def from_bytes(cls, state):
        """From torch.get_rng_state() / Generator.get_state() (a uint8 tensor or bytes of STATE_BYTES)."""
        b = bytes(state.numpy().tobytes() if hasattr(state, 'numpy') else state)
        if len(b) != STATE_BYTES:
            raise ValueError('a CPU generator state is %d bytes, got %d' % (STATE_BYTES, len(b)))
        hdr = np.frombuffer(b, dtype=np.uint8)
        seed = int(hdr[_OFF_SEED:_OFF_SEED + 8].view(np.uint64)[0])
        left = int(hdr[_OFF_LEFT:_OFF_LEFT + 4].view(np.int32)[0])
        seeded = int(hdr[_OFF_SEEDED:_OFF_SEEDED + 4].view(np.int32)[0])
        nxt = int(hdr[_OFF_NEXT:_OFF_NEXT + 8].view(np.uint64)[0])
        arr = hdr[_OFF_STATE:_OFF_STATE + 8 * N].view(np.uint64).astype(np.uint32)
        return cls(arr, nxt, left, seed, seeded, tail=b[_OFF_STATE + 8 * N:])

    def to_bytes(self):
        out = bytearray(STATE_BYTES)
        out[_OFF_SEED:_OFF_SEED + 8] = np.uint64(self.seed).tobytes()
        out[_OFF_LEFT:_OFF_LEFT + 4] = np.int32(self.left).tobytes()
        out[_OFF_SEEDED:_OFF_SEEDED + 4] = np.int32(self.seeded).tobytes()
        out[_OFF_NEXT:_OFF_NEXT + 8] = np.uint64(self.next).tobytes()
        out[_OFF_STATE:_OFF_STATE + 8 * N] = self.arr.astype(np.uint64).tobytes()
        if self.tail is not None:
            out[_OFF_STATE + 8 * N:] = self.tail
        return bytes(out)

    def to_tensor(self):
        import torch
        return torch.frombuffer(bytearray(self.to_bytes()), dtype=torch.uint8).clone()

    @property
    def pos(self):
        """p: the next word drawn is x[b + p] (module docstring)."""
        p = N if self.left == 1 else self.next
        if not 1 <= p <= N or (self.left != 1 and self.left != N + 1 - self.next):
            raise ValueError('not a state torch leaves behind: next = %d, left = %d' % (self.next, self.left))
        return p

    def copy(self):
        return MTState(self.arr.copy(), self.next, self.left, self.seed, self.seeded, self.tail)

    def raw(self, n):
        """(the next n raw words, the state after them), sequentially."""
        p = self.pos
        out = np.empty(n, np.uint32)
        arr, k, done = self.arr, p, 0
        while done < n:
            if k == N:
                arr, k = twist(arr), 0
            take = min(n - done, N - k)
            out[done:done + take] = arr[k:k + take]
            done += take
            k += take
        st = self.copy()
        st.arr = arr
        if n > 0:
            st.next, st.left = k, N + 1 - k
        return out, st

    def words(self, n):
        w, st = self.raw(n)
        return temper(w), st

    def uniform(self, n):
        """torch.empty(n).uniform_() in fp32: (w & 0xFFFFFF) * 2^-24."""
        w, st = self.words(n)
        return uniform_from_words(w), st

    def normal(self, n):
        """torch.empty(n).normal_() for a contiguous fp32 tensor, n >= 16 (module docstring)."""
        if n < 16:
            raise ValueError('the vectorised normal_() path needs n >= 16')
        u, st = self.uniform(n + (16 if n % 16 else 0))
        out = box_muller(u[:n])
        if n % 16:
            out[n - 16:] = box_muller(u[n:])
        return out, st


def uniform_from_words(w):
    return ((np.asarray(w, dtype=np.uint32) & np.uint32(0xFFFFFF)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def box_muller(u):
    """normal_fill_16 on every full 16-chunk of u (fp32, len(u) >= 16); the remainder is left as uniforms."""
    u = np.asarray(u, dtype=np.float32)
    q = len(u) // 16
    out = u.copy()
    c = u[:16 * q].reshape(q, 16)
    u1 = np.float32(1.0) - c[:, :8]
    r = np.sqrt(np.float32(-2.0) * np.log(u1))
    th = TWO_PI * c[:, 8:]
    out[:16 * q].reshape(q, 16)[:, :8] = r * np.cos(th)
    out[:16 * q].reshape(q, 16)[:, 8:] = r * np.sin(th)
    return out


def words_per_call(n):
    return n + (16 if n % 16 else 0)


# ---- GF(2) polynomials (bit i of a Python int = coefficient of t^i) -------------------------------------------------------------
def berlekamp_massey(bits):
    """The shortest LFSR of a GF(2) sequence: (connection polynomial C as an int, its length L)."""
    C, B, L, m, R = 1, 1, 0, 1, 0
    for n, s in enumerate(bits):
        R = (R << 1) | int(s)                       # bit i of R = s[n - i]
        if (C & R).bit_count() & 1:
            T = C
            C ^= B << m
            if 2 * L <= n:
                L, B, m = n + 1 - L, T, 1
                continue
        m += 1
    return C, L


@functools.lru_cache(maxsize=1)
def char_poly():
    """phi, the characteristic polynomial of mt19937's state transition (degree 19 937), by Berlekamp-Massey on the lowest bit
    of 2 x 19 937 raw words of a seeded stream (the words after the array's first, which is not part of the state)."""
    st = MTState.seeded_with(5489)
    w, _ = st.raw(2 * DEG + 64)
    C, L = berlekamp_massey((w[1:] & 1).tolist())
    if L != DEG:
        raise RuntimeError('Berlekamp-Massey found an LFSR of length %d, not %d' % (L, DEG))
    phi = 0
    for i in range(L + 1):                          # phi(t) = t^L C(1 / t)
        if (C >> i) & 1:
            phi |= 1 << (L - i)
    return phi


def _spread_table():
    t = np.zeros(256, np.uint16)
    for v in range(256):
        s = 0
        for b in range(8):
            s |= ((v >> b) & 1) << (2 * b)
        t[v] = s
    return t


_SPREAD = _spread_table()


def _sqr(a):
    """a^2 over GF(2): the bits spread to the even positions."""
    if a == 0:
        return 0
    b = np.frombuffer(a.to_bytes((a.bit_length() + 7) // 8, 'little'), dtype=np.uint8)
    return int.from_bytes(_SPREAD[b].astype('<u2').tobytes(), 'little')


def _clmul(a, b):
    """a * b over GF(2), through an exact float64 FFT convolution of the coefficient vectors."""
    if a == 0 or b == 0:
        return 0
    na, nb = a.bit_length(), b.bit_length()
    va = np.unpackbits(np.frombuffer(a.to_bytes((na + 7) // 8, 'little'), dtype=np.uint8), bitorder='little')[:na]
    vb = np.unpackbits(np.frombuffer(b.to_bytes((nb + 7) // 8, 'little'), dtype=np.uint8), bitorder='little')[:nb]
    L = 1 << (na + nb).bit_length()
    c = np.fft.irfft(np.fft.rfft(va.astype(np.float64), L) * np.fft.rfft(vb.astype(np.float64), L), L)[:na + nb - 1]
    bits = (np.rint(c).astype(np.int64) & 1).astype(np.uint8)
    return int.from_bytes(np.packbits(bits, bitorder='little').tobytes(), 'little')


class _Mod:
    """Reduction modulo phi by Barrett's method over GF(2) (two carry-less products per reduction)."""

    def __init__(self, phi):
        self.phi, self.d = phi, phi.bit_length() - 1
        # mu = floor(t^(2d) / phi), by long division (once)
        num, q = 1 << (2 * self.d), 0
        while num.bit_length() - 1 >= self.d:
            s = num.bit_length() - 1 - self.d
            q |= 1 << s
            num ^= phi << s
        self.mu = q

    def __call__(self, a):
        d = self.d
        if a.bit_length() <= d:
            return a
        q = _clmul(a >> d, self.mu) >> d
        r = a ^ _clmul(q, self.phi)
        assert r.bit_length() <= d
        return r

    def mul(self, a, b):
        return self(_clmul(a, b))

    def pow_t(self, n):
        """t^n mod phi."""
        r = 1
        for bit in bin(n)[2:]:
            r = self(_sqr(r))
            if bit == '1':
                r <<= 1
                if r >> self.d:
                    r ^= self.phi
        return r


@functools.lru_cache(maxsize=1)
def _mod():
    return _Mod(char_poly())


def jump_poly(n):
    """t^n mod phi as an int (bit i = coefficient of t^i)."""
    return _mod().pow_t(int(n))


def jump_raw(prefix, n, length=N):
    """Host restatement of the device jump: the `length` raw words n words after the prefix's first, from the prefix
    x[s .. s + PREFIX_WORDS - 1] (s > b).  Checked against the sequential stream by the tests."""
    prefix = np.asarray(prefix, dtype=np.uint32)
    g = jump_poly(n)
    acc = np.zeros(length, np.uint32)
    i = 0
    while g:
        if g & 1:
            acc ^= prefix[i:i + length]
        g >>= 1
        i += 1
    return acc


def pack_poly(g):
    """An int polynomial of degree < DEG as POLY_WORDS little-endian uint32 words."""
    return np.frombuffer(g.to_bytes(4 * POLY_WORDS, 'little'), dtype='<u4').astype(np.uint32)


# ---- the draw's layout --------------------------------------------------------------------------------------------------------
# segments of one draw (a jump and a generating workgroup each, at least one per call).  Measured at C3 (16 calls of 3.67 M): 256
# segments + the final window -- jump 0.21 ms, generation 0.31 ms a draw; 240 + 1 (one jump workgroup per CU, 83 KB of LDS
# each): jump 0.21 ms, generation 0.34 ms
TARGET_SEGMENTS = 256


def segments_per_call(n, n_calls):
    Q = n // 16
    return max(1, min(Q, -(-TARGET_SEGMENTS // n_calls)))


def segment_layout(n, n_calls, segs_per_call, uniform=False):
    """The device draw's segments: every call of n elements is cut into `segs_per_call` runs of whole 16-chunks; a call's last
    run also takes its tail (normal_(): the 16 fresh words of the tail rule; uniform_(): the n % 16 words after the last
    chunk).  Returns int64 rows (word offset of the run's first word from the draw's first word, call, first 16-chunk,
    16-chunks, last run of its call) and the draw's total word count."""
    Q = n // 16
    W = n if uniform else words_per_call(n)
    k = max(1, min(int(segs_per_call), Q))
    rows = []
    for c in range(n_calls):
        for s in range(k):
            q0, q1 = (s * Q) // k, ((s + 1) * Q) // k
            rows.append((c * W + 16 * q0, c, q0, q1 - q0, int(s == k - 1)))
    return np.array(rows, dtype=np.int64), n_calls * W


def final_window_offset(total_words):
    """Offset from the draw's first word of the 1 248-word window that holds torch's array after the draw."""
    return max(0, total_words - N)


def final_index(pos, total_words):
    """Where torch's array after a draw of `total_words` words from position `pos` starts within the final window
    (-1: the draw does not reach the end of the array, which stays as it was)."""
    q = pos + total_words
    if q <= N:
        return -1
    return total_words - ((q - 1) % N + 1) - final_window_offset(total_words)


def pos_after(pos, total_words):
    """The position (MTState.pos) after a draw of `total_words` words; torch's `next` = it, `left` = 625 - it."""
    q = pos + total_words
    return q if q <= N else (q - 1) % N + 1


def state_after(st, total_words, arr):
    """torch's state after `total_words` words drawn from `st`, given the array after the draw."""
    out = st.copy()
    out.arr = np.asarray(arr, dtype=np.uint32).copy()
    out.next = pos_after(st.pos, total_words)
    out.left = N + 1 - out.next
    return out


def jump_lists(polys):
    """The set coefficients of each packed polynomial as uint16 lists padded to a multiple of 8 with PREFIX_WORDS (the zero
    window of the device's LDS): (uint16 (rows, stride), int32 counts)."""
    lists = [np.nonzero(np.unpackbits(p.astype('<u4').view(np.uint8), bitorder='little'))[0] for p in polys]
    cnt = np.array([-(-len(l) // 8) * 8 for l in lists], dtype=np.int32)
    stride = max(8, int(cnt.max()))
    idx = np.full((len(lists), stride), PREFIX_WORDS, dtype=np.uint16)
    for r, l in enumerate(lists):
        idx[r, :len(l)] = l
    return idx, cnt


@functools.lru_cache(maxsize=16)
def jump_tables(n, n_calls, segs_per_call, uniform=False):
    """(packed jump polynomials, one row per segment and one for the final window, uint32 (rows, POLY_WORDS); segment rows;
    total words; host seconds spent).  Depends on the shape only: cached per planner shape."""
    t0 = time.perf_counter()
    rows, total = segment_layout(n, n_calls, segs_per_call, uniform)
    offs = [int(o) for o in rows[:, 0]] + [final_window_offset(total)]
    mod = _mod()
    polys, cache = [], {}
    prev_off, prev = None, None
    for o in offs:
        # successive offsets differ by a few distinct steps: t^o = t^prev * t^(o - prev)
        if prev is not None and o >= prev_off:
            step = o - prev_off
            if step not in cache:
                cache[step] = mod.pow_t(step)
            g = mod.mul(prev, cache[step])
        else:
            g = mod.pow_t(o)
        polys.append(pack_poly(g))
        prev_off, prev = o, g
    return np.stack(polys), rows, total, time.perf_counter() - t0
