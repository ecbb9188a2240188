// mpb_path_blend.hip -- joint-space polylines turned into executable trajectories: linear segments at constant velocity, a
// constant-acceleration (parabolic) blend around every waypoint, a cap on how far a blend may leave its corner (Kunz & Stilman 2012;
// the idea behind MoveIt's TOTG; the reference has none -- the semantics are build-defined, DESIGN.md 10, include/mpb.h).  The limits
// hold for EVERY t and every point of the trajectory is within a known per-joint distance of the polyline: what lets a path
// certificate (mpb_path_certify) carry over to the trajectory.  Not time-optimal.
//
// mpb_path_blend: ONE launch, one single-wave workgroup per path.  The rows are staged once into LDS as (H, Dp) floats (Dp = D | 1:
// an odd row stride, lane i reads row i without a bank conflict; read in place with the caller's stride, the columns past D and the
// rows past the path's length never).  One lane per waypoint / segment, in trips of 64 for H > 64; a lane walks its joints in a
// loop and keeps two running maxima -- no lane holds an array.  The segment durations T live in LDS: a waypoint reads T_{i-1} and T_i,
// a segment the factors f_i and f_{i+1} of its two waypoints.  "Any waypoint in violation" is a wave ballot ORed over the trips.  The
// waypoint times are a running sum in the order of the definition: every lane holds its segment's T, the wave walks the 64 lanes of
// a trip with v_readlane.  No atomics: the same bits on every run.  All arithmetic that defines the result is rounded after every
// operation (fp contract(off), plain operators; see mpb_retime.hip).
//
// mpb_path_blend_sample: one thread per output row, a binary search in the path's waypoint times, then the blend window or the
// segment the row falls into.
#include <climits>
#include <string.h>

#include "mpb_common.h"
#include "mpb_host.h"

#pragma clang fp contract(off)

struct PbArgs {
    const float* paths;
    size_t row_stride;
    const int* lengths;
    const float* v_max;
    const float* a_max;
    float* T;
    float* tb;
    float* tw;
    float* dev;
    float* duration;
    int* sweeps;
    int* status;
    int* first_bad;
    int H, D, max_sweeps, has_cap;
    float eight_delta;
};

// the words of a float in memory, a finite float > 0, a finite float.  The build assumes finite math: a test on a float VALUE, even on
// its bits, is the compiler's to fold away (it did: an exponent-mask test on __float_as_uint of a loaded float never fired) -- what may be
// an inf or a NaN is loaded as an integer and only then handed on as a float
__device__ __forceinline__ unsigned pb_word(const float* p) {
    unsigned u;
    __builtin_memcpy(&u, p, 4);
    return u;
}
__device__ __forceinline__ bool pb_positive_finite(unsigned u) { return (u - 1u) < 0x7F7FFFFFu; }
__device__ __forceinline__ bool pb_finite(unsigned u) { return (u & 0x7F800000u) != 0x7F800000u; }

// a path that is not OK: zeros in every output
__device__ __forceinline__ void pb_refuse(const PbArgs& g, int n, int lane, int status, int sweeps, int first_bad) {
    const int H = g.H;
    for (int i = lane; i < H; i += 64) {
        g.tb[(size_t)n * H + i] = 0.f;
        g.tw[(size_t)n * H + i] = 0.f;
        g.dev[(size_t)n * H + i] = 0.f;
        if (i < H - 1) g.T[(size_t)n * (H - 1) + i] = 0.f;
    }
    if (lane == 0) {
        g.duration[n] = 0.f;
        g.sweeps[n] = sweeps;
        g.status[n] = status;
        g.first_bad[n] = first_bad;
    }
}

// waypoint i < L of the staged path: tb_i = max_k |dv_ik| / a_k and max_k |dv_ik|, dv_i = v_i - v_{i-1}, v_i = dq_i / T_i, v_{-1} = v_{L-1} = 0
__device__ __forceinline__ void pb_waypoint(const float* P, const float* Ts, const float* lim_a, int Dp, int D, int L, int i, float& tb, float& mdv) {
    const bool has_prev = i > 0, has_next = i < L - 1;
    const float Tp = Ts[max(i - 1, 0)], Tn = Ts[min(i, L - 2)];
    const float* r0 = P + i * Dp;
    const float* rm = P + max(i - 1, 0) * Dp;
    const float* rp = P + min(i + 1, L - 1) * Dp;
    tb = 0.f;
    mdv = 0.f;
    for (int k = 0; k < D; ++k) {
        const float q0 = r0[k];
        const float vp = has_prev ? (q0 - rm[k]) / Tp : 0.f;
        const float vn = has_next ? (rp[k] - q0) / Tn : 0.f;
        const float adv = fabsf(vn - vp);
        mdv = fmaxf(mdv, adv);
        tb = fmaxf(tb, adv / lim_a[k]);
    }
}

__global__ __launch_bounds__(64) void path_blend_kernel(const PbArgs g) {
    extern __shared__ float pb_lds[];
    const int H = g.H, D = g.D, Dp = D | 1;
    const int n = blockIdx.x, lane = threadIdx.x;
    float* P = pb_lds;                                           // (H, Dp) positions
    float* Ts = P + H * Dp;                                      // (H) segment durations
    float* fs = Ts + H;                                          // (H) the slow-down factor of every waypoint
    float* tbs = fs + H;                                         // (H) blend durations
    float* mdvs = tbs + H;                                       // (H) max_k |dv_ik|
    float* lim_v = mdvs + H;                                     // (MPB_MAX_DOF)
    float* lim_a = lim_v + MPB_MAX_DOF;                          // (MPB_MAX_DOF)

    const int L = g.lengths ? g.lengths[n] : H;
    const int jl = min(lane, D - 1);
    const unsigned V = pb_word(g.v_max + jl), A = pb_word(g.a_max + jl);
    if (lane < D) {
        lim_v[lane] = __uint_as_float(V);
        lim_a[lane] = __uint_as_float(A);
    }
    bool bad = !pb_positive_finite(V) || !pb_positive_finite(A);
    const bool bad_length = L < 2 || L > H;                      // (wave-uniform)
    const float* Q = g.paths + (size_t)n * H * g.row_stride;
    if (!bad_length) {
        for (int i = lane; i < L * Dp; i += 64) {
            const int r = i / Dp, k = i - r * Dp;
            const unsigned q = (k < D) ? pb_word(Q + (size_t)r * g.row_stride + k) : 0u;
            bad = bad || !pb_finite(q);
            P[i] = __uint_as_float(q);
        }
    }
    if (bad_length || __ballot(bad) != 0ull) {
        pb_refuse(g, n, lane, MPB_BLEND_BAD_INPUT, 0, -1);
        return;
    }
    __syncthreads();

    // ---- T_i = max_k |dq_ik| / v_k; a segment that does not move: DEGENERATE_SEGMENT, first_bad the lowest such segment ----------------
    int first_bad = -1;                                          // (wave-uniform)
    for (int base = 0; base < L - 1; base += 64) {
        const int i = base + lane;
        const bool live = i < L - 1;
        const int ic = min(i, L - 2);
        float t = 0.f, mx = 0.f;
        for (int k = 0; k < D; ++k) {
            const float d = fabsf(P[(ic + 1) * Dp + k] - P[ic * Dp + k]);
            mx = fmaxf(mx, d);
            t = fmaxf(t, d / lim_v[k]);
        }
        if (live) Ts[i] = t;
        const unsigned long long still = __ballot(live && mx == 0.f);
        if (still != 0ull && first_bad < 0) first_bad = base + (int)__builtin_ctzll(still);
    }
    if (first_bad >= 0) {
        pb_refuse(g, n, lane, MPB_BLEND_DEGENERATE_SEGMENT, 0, first_bad);
        return;
    }
    __syncthreads();

    // ---- the sweeps: waypoint i is in violation iff tb_i > m_i = min(T_{i-1}, T_i, cap_i); its two segments slow down by sqrt(m_i / tb_i) ----
    int sweeps = 0;                                              // (wave-uniform)
    for (;;) {
        unsigned long long any = 0ull;
        for (int base = 0; base < L; base += 64) {
            const int i = base + lane;
            const bool live = i < L;
            const int ic = min(i, L - 1);
            float tb, mdv;
            pb_waypoint(P, Ts, lim_a, Dp, D, L, ic, tb, mdv);
            float m = (ic > 0) ? Ts[ic - 1] : Ts[0];
            if (ic < L - 1) m = fminf(m, Ts[ic]);
            if (g.has_cap && mdv != 0.f) m = fminf(m, g.eight_delta / mdv);
            const bool viol = live && tb > m;
            any |= __ballot(viol);
            if (live) {
                fs[i] = viol ? sqrtf(m / tb) : 1.f;
                tbs[i] = tb;
                mdvs[i] = mdv;
            }
        }
        if (any == 0ull) break;
        if (sweeps == g.max_sweeps) {
            pb_refuse(g, n, lane, MPB_BLEND_NOT_CONVERGED, sweeps, -1);
            return;
        }
        __syncthreads();
        for (int base = 0; base < L - 1; base += 64) {
            const int i = base + lane;
            if (i < L - 1) Ts[i] = Ts[i] / fminf(fs[i], fs[i + 1]);
        }
        ++sweeps;
        __syncthreads();
    }
    __syncthreads();

    // ---- the timeline: tw_0 = tb_0 / 2, tw_{i+1} = tw_i + T_i summed in that order; the outputs, zeros at and past the length -------------
    float run = tbs[0] * 0.5f;                                   // (wave-uniform)
    for (int base = 0; base < H; base += 64) {
        const int i = base + lane;
        const float t = (i < L - 1) ? Ts[i] : 0.f;
        float mine = 0.f;
        if (base < L) {
#pragma unroll 8                                                 // (unrolled in full the 64 lane reads are all in flight: scalar registers spill)
            for (int l = 0; l < 64; ++l) {
                mine = (lane == l) ? run : mine;
                run = run + readlane_f32(t, l);
            }
        }
        if (i < H) {
            const bool way = i < L;
            const float tb = way ? tbs[i] : 0.f;
            g.tb[(size_t)n * H + i] = tb;
            g.tw[(size_t)n * H + i] = way ? mine : 0.f;
            g.dev[(size_t)n * H + i] = way ? (mdvs[i] * tb) * 0.125f : 0.f;
            if (i < H - 1) g.T[(size_t)n * (H - 1) + i] = t;
        }
    }
    if (lane == 0) {
        g.duration[n] = run + tbs[L - 1] * 0.5f;                 // (run is tw_{L-1}: the segments past L - 2 added 0)
        g.sweeps[n] = sweeps;
        g.status[n] = MPB_BLEND_OK;
        g.first_bad[n] = -1;
    }
}

// ---- the sampler -------------------------------------------------------------------------------------------------------------
struct PbSampleArgs {
    const float* paths;
    size_t row_stride;
    const int* lengths;
    const float* T;
    const float* tb;
    const float* tw;
    const float* duration;
    const int* blend_status;
    float* out;
    int* n_rows;
    int* status;
    int H, D, T_rows, blocks_per_path;
    float dt;
};

__global__ __launch_bounds__(256) void path_blend_sample_kernel(const PbSampleArgs g) {
    const int H = g.H, D = g.D;
    const int n = blockIdx.x / g.blocks_per_path;
    const int row = (blockIdx.x - n * g.blocks_per_path) * 256 + threadIdx.x;
    const float* Q = g.paths + (size_t)n * H * g.row_stride;
    const float* Tseg = g.T + (size_t)n * (H - 1);
    const float* tbn = g.tb + (size_t)n * H;
    const float* twn = g.tw + (size_t)n * H;
    const int L = g.lengths ? g.lengths[n] : H;
    const unsigned dur_word = pb_word(g.duration + n);
    const float dur = __uint_as_float(dur_word);
    const int bst = g.blend_status[n];
    const bool bad_shape = L < 2 || L > H || !pb_finite(dur_word) || (dur_word >> 31) != 0u;    // (a duration that is not finite, or negative)
    const bool held = bst != MPB_BLEND_OK || bad_shape;
    if (row == 0) {
        // ceil(duration / dt) + 1 in fp64 from the fp32 values: the quotient of two floats is exact to a double's rounding
        const double rows = held ? 0.0 : ceil((double)dur / (double)g.dt) + 1.0;
        g.n_rows[n] = rows > (double)INT_MAX ? INT_MAX : (int)rows;
        g.status[n] = bst != MPB_BLEND_OK ? bst : bad_shape ? MPB_BLEND_BAD_INPUT : rows > (double)g.T_rows ? MPB_BLEND_TOO_LONG : MPB_BLEND_OK;
    }
    if (row >= g.T_rows) return;
    float* o = g.out + ((size_t)n * g.T_rows + row) * 3 * D;
    const float tau = (float)row * g.dt;
    if (held || tau >= dur) {                                    // a path that is not OK holds its first waypoint, a finished one its last
        const float* r = Q + (size_t)(held ? 0 : L - 1) * g.row_stride;
        for (int k = 0; k < D; ++k) {
            o[k] = r[k];
            o[D + k] = 0.f;
            o[2 * D + k] = 0.f;
        }
        return;
    }
    int lo = -1, hi = L;                                         // tw[lo] <= tau < tw[hi], tw[-1] = -inf, tw[L] = +inf
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (twn[mid] <= tau) lo = mid; else hi = mid;
    }
    const int jc = max(lo, 0), jn = min(jc + 1, L - 1);
    const bool own = lo < 0 || lo == L - 1 || (tau - twn[jc]) <= tbn[jc] * 0.5f;
    const bool next = !own && (twn[jn] - tau) <= tbn[jn] * 0.5f;
    const bool window = own || next;
    const int i = next ? jn : jc;                                // the waypoint of the window, or the segment
    const bool has_prev = i > 0, has_next = i < L - 1;
    const float tbi = tbn[i], d = tau - twn[i], s = d + tbi * 0.5f;
    const float Tp = Tseg[max(i - 1, 0)], Tn = Tseg[min(i, L - 2)];
    const float* r0 = Q + (size_t)i * g.row_stride;
    const float* rm = Q + (size_t)max(i - 1, 0) * g.row_stride;
    const float* rp = Q + (size_t)min(i + 1, L - 1) * g.row_stride;
    for (int k = 0; k < D; ++k) {
        const float q0 = r0[k];
        const float vp = has_prev ? (q0 - rm[k]) / Tp : 0.f;
        const float vn = has_next ? (rp[k] - q0) / Tn : 0.f;
        const float a = tbi > 0.f ? (vn - vp) / tbi : 0.f;
        o[k] = window ? (q0 + vp * d) + ((a * s) * s) * 0.5f : q0 + vn * d;
        o[D + k] = window ? vp + a * s : vn;
        o[2 * D + k] = window ? a : 0.f;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
static bool pb_host_positive_finite(float v) {
    uint32_t bits;
    memcpy(&bits, &v, 4);                                        // (on the bits: the build assumes finite math)
    return (bits - 1u) < 0x7F7FFFFFu;
}

// > 0 and not NaN; +inf passes (no cap)
static bool pb_host_positive(float v) {
    uint32_t bits;
    memcpy(&bits, &v, 4);
    return (bits - 1u) < 0x7F800000u;
}

static int pb_check_shape(const char* who, int N, int H, int D, size_t row_stride) {
    if (D > MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "%s: D = %d exceeds MPB_MAX_DOF = %d", who, D, MPB_MAX_DOF);
    if (H > MPB_MAX_H) return mpb_failf(MPB_E_UNSUPPORTED, "%s: H = %d exceeds MPB_MAX_H = %d", who, H, MPB_MAX_H);
    if (H < 2 || N < 0 || D < 1 || row_stride < (size_t)D) return mpb_failf(MPB_E_INVALID, "%s: bad shape (N %d, H %d, D %d, row stride %zu)", who, N, H, D, row_stride);
    return MPB_OK;
}

extern "C" int mpb_path_blend(const float* paths, size_t row_stride, const int* lengths, const float* v_max, const float* a_max,
                              float max_deviation, int max_sweeps, float* T, float* tb, float* tw, float* dev, float* duration, int* sweeps,
                              int* status, int* first_bad, int N, int H, int D, void* stream) {
    const int rc = pb_check_shape("mpb_path_blend", N, H, D, row_stride);
    if (rc) return rc;
    if (!pb_host_positive(max_deviation)) return mpb_fail(MPB_E_INVALID, "mpb_path_blend: max_deviation must be > 0 (+inf: no cap)");
    if (max_sweeps < 1) return mpb_failf(MPB_E_INVALID, "mpb_path_blend: max_sweeps = %d, at least one sweep", max_sweeps);
    if (!paths || !v_max || !a_max || !T || !tb || !tw || !dev || !duration || !sweeps || !status || !first_bad)
        return mpb_fail(MPB_E_INVALID, "mpb_path_blend: null pointer");
    if (N == 0) return MPB_OK;
    const int has_cap = pb_host_positive_finite(max_deviation) ? 1 : 0;
    const PbArgs a = {paths, row_stride, lengths, v_max, a_max, T, tb, tw, dev, duration, sweeps, status, first_bad, H, D, max_sweeps, has_cap,
                      has_cap ? 8.f * max_deviation : 0.f};
    const size_t lds = ((size_t)H * ((D | 1) + 4) + 2 * MPB_MAX_DOF) * sizeof(float);     // at most 17.5 KB
    hipLaunchKernelGGL(path_blend_kernel, dim3(N), dim3(64), lds, (hipStream_t)stream, a);
    return mpb_check_launch("mpb_path_blend");
}

extern "C" int mpb_path_blend_sample(const float* paths, size_t row_stride, const int* lengths, const float* T, const float* tb,
                                     const float* tw, const float* duration, const int* blend_status, float* out, int* n_rows, int* status,
                                     int N, int H, int D, float dt, int T_rows, void* stream) {
    const int rc = pb_check_shape("mpb_path_blend_sample", N, H, D, row_stride);
    if (rc) return rc;
    if (!pb_host_positive_finite(dt)) return mpb_fail(MPB_E_INVALID, "mpb_path_blend_sample: dt must be finite and positive");
    if (T_rows < 1) return mpb_failf(MPB_E_INVALID, "mpb_path_blend_sample: T_rows = %d, at least one output row", T_rows);
    const long long bpp = ((long long)T_rows + 255) / 256;
    if (bpp * (long long)N > INT_MAX) return mpb_fail(MPB_E_INVALID, "mpb_path_blend_sample: N x T_rows / 256 blocks do not fit an int");
    if (!paths || !T || !tb || !tw || !duration || !blend_status || !out || !n_rows || !status)
        return mpb_fail(MPB_E_INVALID, "mpb_path_blend_sample: null pointer");
    if (N == 0) return MPB_OK;
    const PbSampleArgs a = {paths, row_stride, lengths, T, tb, tw, duration, blend_status, out, n_rows, status, H, D, T_rows, (int)bpp, dt};
    hipLaunchKernelGGL(path_blend_sample_kernel, dim3((unsigned)(bpp * N)), dim3(256), 0, (hipStream_t)stream, a);
    return mpb_check_launch("mpb_path_blend_sample");
}
