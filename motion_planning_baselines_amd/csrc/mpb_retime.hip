// mpb_retime.hip -- time parameterisation of a trajectory batch under per-joint velocity and acceleration limits: the pass between
// the optimiser and a controller (MoveIt's TOTG, cuRobo's retiming; the reference has none -- the semantics are build-defined,
// DESIGN.md 10, include/mpb.h).  Reachability-based path parameterisation (TOPP-RA, Pham & Pham 2018) for limits symmetric about
// zero, rest to rest: every 2-variable LP of the two passes has a closed form (a minimum over pairs of lines), so there is no
// solver and no infeasible case.
//
// mpb_traj_retime: ONE launch, one single-wave workgroup per trajectory.  The positions are staged once into LDS as (H, Dp) floats
// (Dp = D rounded up to 4; the rows are read in place with the caller's stride, the columns past D never).  Both passes are serial
// in H by nature; a step's parallelism is over its lines:
//   - lane m < 2D + 1 builds line pair m of the interval (a, b, c+, c-: the lines a u + b x <= c+ and -a u - b x <= c-) from the LDS
//     rows -- no lane holds an array, nothing is indexed at run time in registers;
//   - backward: the pairs go to LDS, the (2D+1)^2 ordered (upper, lower) pairs are spread over the lanes in trips (pair = trip * 64 +
//     lane; which line of a pair bounds u from above is picked by the sign of a, nothing is compacted), a wave min closes the step;
//     beta goes to LDS for the forward pass and stays in a register for the next step;
//   - forward: every lane turns its own pair into a bound on u at the current x, a wave min closes the step; the time advances in
//     the same step (its sqrt and divide are off the chain x_i -> x_{i+1}).
// A minimum does not depend on its order: the result is that of the sequential definition.  No atomics: the same bits on every
// run.  All arithmetic that defines the result is rounded after every operation (the file is compiled under fp contract(off), plain
// operators; see mpb_path_shortcut.hip on the __f*_rn intrinsics).
//
// mpb_traj_retime_sample: one thread per output row, a binary search in the trajectory's t, a cubic Hermite of the two waypoints.
#include <climits>
#include <string.h>

#include "mpb_common.h"
#include "mpb_host.h"

#pragma clang fp contract(off)

#define RT_BIG 3.4028235e38f                                  // the neutral element of the minima (never survives: see below)
#define RT_LINES 32                                           // LDS slots of the 2 * MPB_MAX_DOF + 1 = 25 line pairs

struct RtArgs {
    const float* trajs;
    size_t row_stride;
    const float* v_max;
    const float* a_max;
    float* x;
    float* u;
    float* t;
    float* qd;
    int* status;
    int H, D;
    float sdot_max, t_max;
};

// bits of a finite float > 0 (tested on the bits: the build assumes finite math)
__device__ __forceinline__ bool rt_positive_finite(float v) { return (__float_as_uint(v) - 1u) < 0x7F7FFFFFu; }
__device__ __forceinline__ bool rt_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

__device__ __forceinline__ float rt_wave_min(float v) {
    MPB_ASSERT_FULL_WAVE();
    v = fminf(v, dpp_f32<0xB1>(v));
    v = fminf(v, dpp_f32<0x4E>(v));
    v = fminf(v, dpp_f32<0x141>(v));
    v = fminf(v, dpp_f32<0x140>(v));
    return fminf(fminf(readlane_f32(v, 0), readlane_f32(v, 16)), fminf(readlane_f32(v, 32), readlane_f32(v, 48)));
}

// the path derivatives at a waypoint from its row and the two next to it (at an end the row itself stands in for the missing one):
// inside p = (q+ - q-) / 2, c = (q+ - q) - (q - q-); at the ends p the one-sided difference and c = 0
__device__ __forceinline__ void rt_derivs(float qm, float q0, float qp, bool at_end, float& p, float& c) {
    const float d = qp - qm;
    p = at_end ? d : d * 0.5f;
    c = at_end ? 0.f : (qp - q0) - (q0 - qm);
}

__device__ __forceinline__ void rt_derivs_lds(const float* P, int Dp, int H, int w, int j, float& p, float& c) {
    const int wm = max(w - 1, 0), wp = min(w + 1, H - 1);
    rt_derivs(P[wm * Dp + j], P[w * Dp + j], P[wp * Dp + j], w == 0 || w == H - 1, p, c);
}

// line pair m of interval i (include/mpb.h): m < D the acceleration limit of joint m at waypoint i; D <= m < 2D that of joint m - D at
// waypoint i + 1 written in x_i (x_{i+1} = x_i + 2u); m == 2D: 0 <= x_i + 2u <= beta_{i+1}.  Lanes past 2D get a = b = 0 (no line).
__device__ __forceinline__ void rt_line(const float* P, int Dp, int H, int D, int i, int m, float A, float beta_next, float& a, float& b,
                                        float& cp, float& cn) {
    const bool second = m >= D;
    const int j = min(second ? m - D : m, D - 1);
    float p, c;
    rt_derivs_lds(P, Dp, H, second ? i + 1 : i, j, p, c);
    a = second ? p + 2.f * c : p;
    b = c;
    cp = cn = A;
    if (m == 2 * D) {
        a = 2.f;
        b = 1.f;
        cp = beta_next;
        cn = 0.f;
    }
    if (m > 2 * D) a = b = 0.f;
}

__global__ __launch_bounds__(64) void retime_kernel(const RtArgs g) {
    extern __shared__ float rt_lds[];
    const int H = g.H, D = g.D, Dp = (D + 3) & ~3, n = 2 * D + 1;
    const int b_ = blockIdx.x, lane = threadIdx.x;
    float* P = rt_lds;                                           // (H, Dp) positions
    float* beta = P + H * Dp;                                    // (H)
    float* xs = beta + H;                                        // (H)
    float* us = xs + H;                                          // (H)
    float* ts = us + H;                                          // (H)
    float* La = ts + H;                                          // the line pairs of the current interval
    float* Lb = La + RT_LINES;
    float* Lcp = Lb + RT_LINES;
    float* Lcn = Lcp + RT_LINES;
    float* x_out = g.x + (size_t)b_ * H;
    float* u_out = g.u + (size_t)b_ * (H - 1);
    float* t_out = g.t + (size_t)b_ * H;
    float* qd_out = g.qd + (size_t)b_ * H * D;

    // the limits of this lane's joint; a limit that is not finite and positive: STALLED, zeros, nothing else is read
    const int jl = (lane < D) ? lane : (lane < 2 * D ? lane - D : 0);
    const float V = g.v_max[jl], A = g.a_max[jl];
    if (__ballot(!rt_positive_finite(V) || !rt_positive_finite(A)) != 0ull) {
        for (int i = lane; i < H; i += 64) {
            x_out[i] = 0.f;
            t_out[i] = 0.f;
            if (i < H - 1) u_out[i] = 0.f;
        }
        for (int i = lane; i < H * D; i += 64) qd_out[i] = 0.f;
        if (lane == 0) g.status[b_] = MPB_RETIME_STALLED;
        return;
    }

    const float* T = g.trajs + (size_t)b_ * H * g.row_stride;
    for (int i = lane; i < H * Dp; i += 64) {
        const int r = i / Dp, k = i - r * Dp;
        P[i] = (k < D) ? T[(size_t)r * g.row_stride + k] : 0.f;
    }
    __syncthreads();

    // ---- backward: beta_i, the largest x_i from which beta_{i+1} can be reached within the limits ---------------------------------
    const int nn = n * n, q64 = 64 / n, r64 = 64 - q64 * n;
    const int m1_0 = lane / n, m2_0 = lane - m1_0 * n;
    float beta_next = 0.f;                                       // (wave-uniform)
    if (lane == 0) beta[H - 1] = 0.f;
    for (int i = H - 2; i >= 1; --i) {
        float a, b, cp, cn;
        rt_line(P, Dp, H, D, i, lane, A, beta_next, a, b, cp, cn);
        if (lane < RT_LINES) {
            La[lane] = a;
            Lb[lane] = b;
            Lcp[lane] = cp;
            Lcn[lane] = cn;
        }
        // the speed limit of the lane's joint at waypoint i (lanes < D hold p_ij in a), squared after the min with sdot_max: both
        // are monotone, so the min over the joints of the squares is the square of the min; and the lane's own x-only line
        float best = RT_BIG;
        if (lane < D) {
            const float r = fminf(a != 0.f ? V / fabsf(a) : RT_BIG, g.sdot_max);
            best = r * r;
        }
        if (a == 0.f && b != 0.f) best = fminf(best, cp / fabsf(b));
        __syncthreads();
        int m1 = m1_0, m2 = m2_0;
        for (int base = 0; base < nn; base += 64) {
            const bool live = base + lane < nn;
            const int i1 = live ? m1 : 0, i2 = live ? m2 : 0;
            const float a1r = La[i1], b1r = Lb[i1], a2r = La[i2], b2r = Lb[i2];
            const bool s1 = a1r > 0.f, s2 = a2r > 0.f;
            const float c1 = s1 ? Lcp[i1] : Lcn[i1], c2 = s2 ? Lcn[i2] : Lcp[i2];
            const float a1 = fabsf(a1r), b1 = s1 ? b1r : -b1r;    // the line of pair m1 with a > 0: u <= (c1 - b1 x) / a1
            const float a2 = -fabsf(a2r), b2 = s2 ? -b2r : b2r;   // the line of pair m2 with a < 0: u >= (c2 - b2 x) / a2
            const float k = a1 * b2 - a2 * b1;
            const float num = a1 * c2 - a2 * c1;
            if (live && a1r != 0.f && a2r != 0.f && k > 0.f) best = fminf(best, num / k);
            m1 += q64;
            m2 += r64;
            if (m2 >= n) {
                m2 -= n;
                ++m1;
            }
        }
        beta_next = rt_wave_min(best);                           // (at most sdot_max^2: lane 0's speed limit always takes part)
        if (lane == 0) beta[i] = beta_next;
        __syncthreads();
    }

    // ---- forward: the largest u at x_i, x_{i+1} = x_i + 2u clamped into [0, beta_{i+1}]; the time in the same step ------------------
    float x = 0.f, t = 0.f, r = 0.f;                             // (wave-uniform)
    bool stalled = false;
    if (lane == 0) {
        xs[0] = 0.f;
        ts[0] = 0.f;
    }
    for (int i = 0; i < H - 1; ++i) {
        const float bn = beta[i + 1];
        float a, b, cp, cn;
        rt_line(P, Dp, H, D, i, lane, A, bn, a, b, cp, cn);
        const bool s = a > 0.f;
        const float a1 = fabsf(a), b1 = s ? b : -b, c1 = s ? cp : cn;
        const float u = rt_wave_min(a != 0.f ? (c1 - b1 * x) / a1 : RT_BIG);   // (pair 2D always bounds u)
        const float xn = fmaxf(0.f, fminf(bn, x + 2.f * u));
        const float rn = sqrtf(xn), sum = r + rn;
        stalled = stalled || !(sum > 0.f);
        t = t + 2.f / sum;
        if (lane == 0) {
            us[i] = u;
            xs[i + 1] = xn;
            ts[i + 1] = t;
        }
        x = xn;
        r = rn;
    }
    __syncthreads();

    for (int i = lane; i < H; i += 64) {
        x_out[i] = xs[i];
        t_out[i] = ts[i];
        if (i < H - 1) u_out[i] = us[i];
    }
    for (int i = lane; i < H * D; i += 64) {
        const int w = i / D, j = i - w * D;
        float p, c;
        rt_derivs_lds(P, Dp, H, w, j, p, c);
        qd_out[i] = p * sqrtf(xs[w]);
    }
    if (lane == 0) g.status[b_] = (!stalled && rt_finite(t) && t <= g.t_max) ? MPB_RETIME_OK : MPB_RETIME_STALLED;
}

// ---- the sampler -------------------------------------------------------------------------------------------------------------
struct RtSampleArgs {
    const float* trajs;
    size_t row_stride;
    const float* x;
    const float* u;
    const float* t;
    const int* retime_status;
    float* out;
    int* n_rows;
    int* status;
    int H, D, T_rows, blocks_per_traj;
    float dt;
};

__global__ __launch_bounds__(256) void retime_sample_kernel(const RtSampleArgs g) {
    const int H = g.H, D = g.D;
    const int n = blockIdx.x / g.blocks_per_traj;
    const int k = (blockIdx.x - n * g.blocks_per_traj) * 256 + threadIdx.x;
    const float* Q = g.trajs + (size_t)n * H * g.row_stride;
    const float* tn = g.t + (size_t)n * H;
    const float T = tn[H - 1];
    const bool stalled = g.retime_status[n] != MPB_RETIME_OK || !rt_finite(T) || T < 0.f;
    if (k == 0) {
        // ceil(T / dt) + 1 in fp64 from the fp32 values: the quotient of two floats is exact to a double's rounding
        const double rows = stalled ? 0.0 : ceil((double)T / (double)g.dt) + 1.0;
        g.n_rows[n] = rows > (double)INT_MAX ? INT_MAX : (int)rows;
        g.status[n] = stalled ? MPB_RETIME_STALLED : rows > (double)g.T_rows ? MPB_RETIME_TOO_LONG : MPB_RETIME_OK;
    }
    if (k >= g.T_rows) return;
    float* o = g.out + ((size_t)n * g.T_rows + k) * 2 * D;
    const float tau = (float)k * g.dt;
    if (stalled || tau >= T) {                                   // a stalled trajectory holds its first waypoint, a finished one its last
        const float* row = Q + (size_t)(stalled ? 0 : H - 1) * g.row_stride;
        for (int j = 0; j < D; ++j) {
            o[j] = row[j];
            o[D + j] = 0.f;
        }
        return;
    }
    int lo = 0, hi = H - 1;                                      // t[lo] <= tau < t[hi]: t[0] = 0 <= tau < T = t[H - 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tn[mid] <= tau) lo = mid; else hi = mid;
    }
    const int i = lo;
    const float d = tau - tn[i];
    const float ui = g.u[(size_t)n * (H - 1) + i];
    const float r = sqrtf(g.x[(size_t)n * H + i]);
    const float sig = fminf(fmaxf(r * d + ((ui * d) * d) * 0.5f, 0.f), 1.f);
    const float sdot = fmaxf(0.f, r + ui * d);
    const float* r0 = Q + (size_t)i * g.row_stride;
    const float* rm = Q + (size_t)max(i - 1, 0) * g.row_stride;
    const float* r1 = r0 + g.row_stride;
    const float* r2 = Q + (size_t)min(i + 2, H - 1) * g.row_stride;
    for (int j = 0; j < D; ++j) {
        const float q0 = r0[j], q1 = r1[j];
        float p0, p1, c;
        rt_derivs(rm[j], q0, q1, i == 0, p0, c);
        rt_derivs(q0, q1, r2[j], i + 1 == H - 1, p1, c);
        const float dq = q1 - q0;
        const float e2 = (3.f * dq - 2.f * p0) - p1;
        const float e3 = (p0 + p1) - 2.f * dq;
        o[j] = q0 + sig * (p0 + sig * (e2 + sig * e3));
        o[D + j] = (p0 + sig * (2.f * e2 + (3.f * sig) * e3)) * sdot;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
static bool rt_host_positive_finite(float v) {
    uint32_t bits;
    memcpy(&bits, &v, 4);                                        // (on the bits: the build assumes finite math)
    return (bits - 1u) < 0x7F7FFFFFu;
}

static int rt_check_shape(const char* who, int N, int H, int D, size_t row_stride) {
    if (D > MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "%s: D = %d exceeds MPB_MAX_DOF = %d", who, D, MPB_MAX_DOF);
    if (H > MPB_MAX_H) return mpb_failf(MPB_E_UNSUPPORTED, "%s: H = %d exceeds MPB_MAX_H = %d", who, H, MPB_MAX_H);
    if (H < 3 || N < 0 || D < 1 || row_stride < (size_t)D) return mpb_failf(MPB_E_INVALID, "%s: bad shape (N %d, H %d, D %d, row stride %zu)", who, N, H, D, row_stride);
    return MPB_OK;
}

extern "C" int mpb_traj_retime(const float* trajs, size_t row_stride, const float* v_max, const float* a_max, float* x, float* u, float* t,
                               float* qd, int* status, int N, int H, int D, float sdot_max, float t_max, void* stream) {
    const int rc = rt_check_shape("mpb_traj_retime", N, H, D, row_stride);
    if (rc) return rc;
    if (!rt_host_positive_finite(sdot_max)) return mpb_fail(MPB_E_INVALID, "mpb_traj_retime: sdot_max must be finite and positive");
    if (!rt_host_positive_finite(t_max)) return mpb_fail(MPB_E_INVALID, "mpb_traj_retime: t_max must be finite and positive");
    if (!trajs || !v_max || !a_max || !x || !u || !t || !qd || !status) return mpb_fail(MPB_E_INVALID, "mpb_traj_retime: null pointer");
    if (N == 0) return MPB_OK;
    const RtArgs a = {trajs, row_stride, v_max, a_max, x, u, t, qd, status, H, D, sdot_max, t_max};
    const int Dp = (D + 3) & ~3;
    const size_t lds = ((size_t)H * (Dp + 4) + 4 * RT_LINES) * sizeof(float);          // at most 17 KB
    hipLaunchKernelGGL(retime_kernel, dim3(N), dim3(64), lds, (hipStream_t)stream, a);
    return mpb_check_launch("mpb_traj_retime");
}

extern "C" int mpb_traj_retime_sample(const float* trajs, size_t row_stride, const float* x, const float* u, const float* t,
                                      const int* retime_status, float* out, int* n_rows, int* status, int N, int H, int D, float dt,
                                      int T_rows, void* stream) {
    const int rc = rt_check_shape("mpb_traj_retime_sample", N, H, D, row_stride);
    if (rc) return rc;
    if (!rt_host_positive_finite(dt)) return mpb_fail(MPB_E_INVALID, "mpb_traj_retime_sample: dt must be finite and positive");
    if (T_rows < 1) return mpb_failf(MPB_E_INVALID, "mpb_traj_retime_sample: T_rows = %d, at least one output row", T_rows);
    const long long bpt = ((long long)T_rows + 255) / 256;
    if (bpt * (long long)N > INT_MAX) return mpb_fail(MPB_E_INVALID, "mpb_traj_retime_sample: N x T_rows / 256 blocks do not fit an int");
    if (!trajs || !x || !u || !t || !retime_status || !out || !n_rows || !status) return mpb_fail(MPB_E_INVALID, "mpb_traj_retime_sample: null pointer");
    if (N == 0) return MPB_OK;
    const RtSampleArgs a = {trajs, row_stride, x, u, t, retime_status, out, n_rows, status, H, D, T_rows, (int)bpt, dt};
    hipLaunchKernelGGL(retime_sample_kernel, dim3((unsigned)(bpt * N)), dim3(256), 0, (hipStream_t)stream, a);
    return mpb_check_launch("mpb_traj_retime_sample");
}
