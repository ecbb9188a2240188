// mpb_ee_cost.hip -- the end-effector pose cost of a trajectory batch and its gradient (mpb_ee_cost_eval / _grad; build-defined, DESIGN.md
// 10): per waypoint h of a range, with (R, t) the pose mpb_fk_ee_pose returns for q_h and [R* | t*] the target,
//   c_h = k_pos |t* - t|^2 + k_rot (|e_w|^2  or  |R a - R* a|^2),   out[b] (+)= weight * sum_h c_h,
// e_w the rotation error of mpb_ik_solve, a a unit axis of the tool frame.  The gradient is the closed form through the geometric
// Jacobian: d c_h / d q_j = -2 (J_v,j . k_pos e_p + J_w,j . k_rot m), m = e_w or (R a) x (R* a).
//
// Two launch forms, chosen by the shape alone (a shape always gives the same bits):
//   wave form (a range of more than one waypoint): one wave per trajectory (a workgroup IS one wave), one lane per waypoint, trips of 64
//     for H > 64; a lane sums its trips in ascending order, then the fixed-order wave reduction of mpb_common.h.
//   lane form (a range of exactly one waypoint, the goal): one lane per trajectory, 64 trajectories per wave, no cross-lane arithmetic.
// No LDS, no barrier, no atomics.  Per lane: the walk (ee_walk of mpb_ee.h for the gradient; the same fk_advance arithmetic without the
// joint tables for the cost alone), the error, then dq_j joint by joint in a loop unrolled over MPB_MAX_DOF, joints at or beyond n_dof
// contributing zero through selects -- no register array is indexed by a run-time value.  The term set is a template parameter: the
// position-only and axis instantiations carry no atan2 and none of the registers of E = R* R^T.
// Every row / target index is formed from the numbers the launcher was given; the kernels compare the header with the D they were
// launched with and answer NaN on the range's waypoints (and in out) when it has changed since.
#include <limits.h>
#include <math.h>
#include <string.h>

#include "mpb_ee.h"
#include "mpb_member_cost.h"   // add_rounded

#define MPB_EE_POS 0        // position term alone
#define MPB_EE_ROT 1        // position (k_pos may be 0) + full rotation
#define MPB_EE_AXIS 2       // position (k_pos may be 0) + one tool axis

struct EeCostArgs {
    const float* trajs;
    const float* geom;
    const float* target;
    float* out;
    float* per_wp;
    float* grad;
    int B, H, d, D, h_begin, h_end, group, stride_g, stride_h;
    float k_pos, k_rot, ax, ay, az, weight;
    int accumulate;
};

// c_h of one waypoint against the target pose T (12 words); GRAD: dq[j] = d c_h / d q_j (0 for j >= D)
template <int TERMS, bool GRAD>
__device__ __forceinline__ float ee_waypoint_cost(const GeomView& G, const EeCostArgs& A, const float* __restrict__ T,
                                                  const float (&q)[MPB_MAX_DOF], float (&dq)[MPB_MAX_DOF]) {
    FKState<GRAD> F;
    if constexpr (GRAD) {
        ee_walk(G, q, F);
    } else {
        fk_identity(F);
        F.frame = 0;
        for (int j = 0; j <= G.n_dof; ++j) fk_advance<false>(G, F, q);
    }
    const float ex = T[3] - F.tx, ey = T[7] - F.ty, ez = T[11] - F.tz;
    const float cp = fmaf(ez, ez, fmaf(ey, ey, ex * ex));
    float cr = 0.f, mx = 0.f, my = 0.f, mz = 0.f;          // the rotation cost and the torque its gradient pulls through J_w
    if constexpr (TERMS == MPB_EE_ROT) {
        const float s00 = T[0], s01 = T[1], s02 = T[2], s10 = T[4], s11 = T[5], s12 = T[6], s20 = T[8], s21 = T[9], s22 = T[10];
        // E = R* R^T, w = vee(E - E^T) / 2, c = (tr E - 1) / 2: the error of ik_solve_kernel, operation for operation
        const float e00 = dot3(s00, F.r00, s01, F.r01, s02, F.r02), e01 = dot3(s00, F.r10, s01, F.r11, s02, F.r12),
                    e02 = dot3(s00, F.r20, s01, F.r21, s02, F.r22);
        const float e10 = dot3(s10, F.r00, s11, F.r01, s12, F.r02), e11 = dot3(s10, F.r10, s11, F.r11, s12, F.r12),
                    e12 = dot3(s10, F.r20, s11, F.r21, s12, F.r22);
        const float e20 = dot3(s20, F.r00, s21, F.r01, s22, F.r02), e21 = dot3(s20, F.r10, s21, F.r11, s22, F.r12),
                    e22 = dot3(s20, F.r20, s21, F.r21, s22, F.r22);
        const float wx = 0.5f * (e21 - e12), wy = 0.5f * (e02 - e20), wz = 0.5f * (e10 - e01);
        const float c = 0.5f * (((e00 + e11) + e22) - 1.0f);
        const float nw = sqrtf(fmaf(wz, wz, fmaf(wy, wy, wx * wx)));
        const float th = atan2f(nw, c);
        const float sc = (nw < 1e-6f) ? 1.0f : th / nw;
        mx = sc * wx; my = sc * wy; mz = sc * wz;
        cr = fmaf(mz, mz, fmaf(my, my, mx * mx));
    } else if constexpr (TERMS == MPB_EE_AXIS) {
        // u = R a, u* = R* a, c_a = |u - u*|^2, torque u x u*
        const float ux = dot3(F.r00, A.ax, F.r01, A.ay, F.r02, A.az), uy = dot3(F.r10, A.ax, F.r11, A.ay, F.r12, A.az),
                    uz = dot3(F.r20, A.ax, F.r21, A.ay, F.r22, A.az);
        const float vx = dot3(T[0], A.ax, T[1], A.ay, T[2], A.az), vy = dot3(T[4], A.ax, T[5], A.ay, T[6], A.az),
                    vz = dot3(T[8], A.ax, T[9], A.ay, T[10], A.az);
        const float dx = ux - vx, dy = uy - vy, dz = uz - vz;
        cr = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
        mx = fmaf(uy, vz, -(uz * vy)); my = fmaf(uz, vx, -(ux * vz)); mz = fmaf(ux, vy, -(uy * vx));
    }
    if constexpr (GRAD) {
        const float fx = A.k_pos * ex, fy = A.k_pos * ey, fz = A.k_pos * ez;
        const float tx = A.k_rot * mx, ty = A.k_rot * my, tz = A.k_rot * mz;
        static_for<0, MPB_MAX_DOF>([&](auto jc) {
            constexpr int J = decltype(jc)::value;
            // (a joint the chain has not: ee_walk left its axis at zero, so its column and its dq are zero without a select on D)
            float cx, cy, cz;
            ee_jv<J>(F, MPB_MAX_DOF, cx, cy, cz);
            float s = dot3(cx, fx, cy, fy, cz, fz);
            if constexpr (TERMS != MPB_EE_POS) s = fmaf(F.zz[J], tz, fmaf(F.zy[J], ty, fmaf(F.zx[J], tx, s)));
            dq[J] = -2.0f * s;
        });
    }
    return TERMS == MPB_EE_POS ? A.k_pos * cp : fmaf(A.k_rot, cr, A.k_pos * cp);
}

__device__ __forceinline__ const float* ee_target_of(const EeCostArgs& A, int b, int h) {
    return A.target + ((size_t)(b / A.group) * (size_t)A.stride_g + (size_t)h * (size_t)A.stride_h) * 12;
}

template <int TERMS, bool GRAD>
__global__ __launch_bounds__(64) void ee_cost_wave_kernel(const EeCostArgs A) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const bool ok = ik_header_matches(A.geom, A.D);
    const GeomView G = ik_chain_view(A.geom);
    const float nan = __uint_as_float(0x7FC00000u);
    float csum = 0.f;
    for (int h0 = 0; h0 < A.H; h0 += 64) {
        const int h = h0 + lane;
        // (D as this trip sees it: the empty asm keeps the twelve comparisons i < D from being hoisted out of the trip loop as twelve
        // SGPR pairs, which spilled; they are scalar compares where they are used)
        int Dl = A.D;
        asm volatile("" : "+s"(Dl));
        const bool in_range = h >= A.h_begin && h < A.h_end;            // (h_end <= H: the launcher checked)
        float q[MPB_MAX_DOF], dq[MPB_MAX_DOF];
#pragma unroll
        for (int i = 0; i < MPB_MAX_DOF; ++i) { q[i] = 0.f; dq[i] = 0.f; }
        float c = 0.f;
        if (ok && h0 < A.h_end && h0 + 64 > A.h_begin) {                 // (wave-uniform: the trip holds a waypoint of the range)
            // a lane outside the range walks along on the nearest waypoint of the range and its result is dropped: no divergent walk
            const int hc = min(max(h, A.h_begin), A.h_end - 1);
            const float* row = A.trajs + ((size_t)b * A.H + hc) * A.d;
#pragma unroll
            for (int i = 0; i < MPB_MAX_DOF; ++i) q[i] = (i < Dl) ? row[i] : 0.f;
            c = ee_waypoint_cost<TERMS, GRAD>(G, A, ee_target_of(A, b, hc), q, dq);
            if (!in_range) c = 0.f;
        }
        if (in_range && !ok) c = nan;
        if (h < A.H) {
            if (A.per_wp) A.per_wp[(size_t)b * A.H + h] = c;
            if constexpr (GRAD) {
                float* grow = A.grad + ((size_t)b * A.H + h) * A.d;
                if (in_range) {
#pragma unroll
                    for (int i = 0; i < MPB_MAX_DOF; ++i) {
                        if (i < Dl) {
                            const float g = ok ? A.weight * dq[i] : nan;
                            grow[i] = A.accumulate ? add_rounded(grow[i], g) : g;
                        }
                    }
                    if (!A.accumulate)
                        for (int i = Dl; i < A.d; ++i) grow[i] = 0.f;    // the velocity channels
                } else if (!A.accumulate) {
                    for (int i = 0; i < A.d; ++i) grow[i] = 0.f;          // a row outside the range
                }
            }
        }
        csum += c;
    }
    csum = wave_sum_f32(csum);
    if (lane == 0) {
        const float v = A.weight * csum;
        A.out[b] = A.accumulate ? add_rounded(A.out[b], v) : v;
    }
}

// the range is the one waypoint h_begin
template <int TERMS, bool GRAD>
__global__ __launch_bounds__(64) void ee_cost_lane_kernel(const EeCostArgs A) {
    const int lane = threadIdx.x, b0 = blockIdx.x * 64, b = b0 + lane, h = A.h_begin;
    const int nb = min(64, A.B - b0);                                     // trajectories of this wave
    const bool valid = b < A.B;
    const bool ok = ik_header_matches(A.geom, A.D);
    const GeomView G = ik_chain_view(A.geom);
    const float nan = __uint_as_float(0x7FC00000u);
    float q[MPB_MAX_DOF], dq[MPB_MAX_DOF];
#pragma unroll
    for (int i = 0; i < MPB_MAX_DOF; ++i) { q[i] = 0.f; dq[i] = 0.f; }
    float c = nan;
    if (valid && ok) {
        const float* row = A.trajs + ((size_t)b * A.H + h) * A.d;
#pragma unroll
        for (int i = 0; i < MPB_MAX_DOF; ++i) q[i] = (i < A.D) ? row[i] : 0.f;
        c = ee_waypoint_cost<TERMS, GRAD>(G, A, ee_target_of(A, b, h), q, dq);
    }
    // what lies outside the range is 0: the wave's 64 trajectories are one contiguous block of rows, cleared by all lanes together
    // (64 * H * d fits an int: the launcher checked); the elements of the range's own row are left to their lane below
    if (A.per_wp) {
        float* base = A.per_wp + (size_t)b0 * A.H;
        for (int i = lane; i < nb * A.H; i += 64)
            if (i % A.H != h) base[i] = 0.f;
    }
    if constexpr (GRAD) {
        if (!A.accumulate) {
            float* base = A.grad + (size_t)b0 * A.H * A.d;
            for (int i = lane; i < nb * A.H * A.d; i += 64) {
                const int col = i % A.d, row = (i / A.d) % A.H;
                if (!(row == h && col < A.D)) base[i] = 0.f;
            }
        }
    }
    if (!valid) return;
    if (A.per_wp) A.per_wp[(size_t)b * A.H + h] = c;
    if constexpr (GRAD) {
        float* grow = A.grad + ((size_t)b * A.H + h) * A.d;
#pragma unroll
        for (int i = 0; i < MPB_MAX_DOF; ++i) {
            if (i < A.D) {
                const float g = ok ? A.weight * dq[i] : nan;
                grow[i] = A.accumulate ? add_rounded(grow[i], g) : g;
            }
        }
    }
    const float v = A.weight * c;
    A.out[b] = A.accumulate ? add_rounded(A.out[b], v) : v;
}

// ---- host side ------------------------------------------------------------------------------------------------------
template <int TERMS, bool GRAD>
static void ee_cost_dispatch(const EeCostArgs& A, hipStream_t stream) {
    if (A.h_end - A.h_begin == 1)
        hipLaunchKernelGGL((ee_cost_lane_kernel<TERMS, GRAD>), dim3((A.B + 63) / 64), dim3(64), 0, stream, A);
    else
        hipLaunchKernelGGL((ee_cost_wave_kernel<TERMS, GRAD>), dim3(A.B), dim3(64), 0, stream, A);
}

// finite, read off the bits, unoptimised: the library is compiled with -ffinite-math-only, under which a comparison -- and a bit test the
// optimiser recognises as one -- may be assumed to see neither a NaN nor an infinity
__attribute__((optnone, noinline)) static bool ee_finite(float v) {
    uint32_t u;
    memcpy(&u, &v, sizeof(u));
    return (u & 0x7F800000u) != 0x7F800000u;
}

template <bool GRAD>
static int ee_cost_launch(const char* who, EeCostArgs A, int use_axis, void* stream) {
    // the refusals of include/mpb.h, in its order; nothing before the header read touches HIP
    if (A.D > MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "%s: D = %d exceeds MPB_MAX_DOF = %d", who, A.D, MPB_MAX_DOF);
    if (A.d > 2 * MPB_MAX_DOF)
        return mpb_failf(MPB_E_UNSUPPORTED, "%s: rows of d = %d exceed positions + velocities of MPB_MAX_DOF = %d joints", who, A.d, MPB_MAX_DOF);
    if (A.B < 0 || A.H < 1 || A.D < 1 || (long long)A.H * A.d * 64 > INT_MAX) return mpb_failf(MPB_E_INVALID, "%s: bad shape", who);
    if (A.d < A.D) return mpb_failf(MPB_E_INVALID, "%s: rows of d = %d are narrower than the chain's D = %d coordinates", who, A.d, A.D);
    if (A.h_begin < 0 || A.h_end > A.H || A.h_begin >= A.h_end)
        return mpb_failf(MPB_E_INVALID, "%s: bad range [%d, %d) of H = %d waypoints", who, A.h_begin, A.h_end, A.H);
    if (A.group < 1 || A.B % A.group != 0)
        return mpb_failf(MPB_E_INVALID, "%s: a group of %d trajectories per target does not divide B = %d", who, A.group, A.B);
    if (A.stride_g < 0 || A.stride_h < 0) return mpb_failf(MPB_E_INVALID, "%s: negative target stride", who);
    if (!ee_finite(A.k_pos) || !ee_finite(A.k_rot) || A.k_pos < 0.f || A.k_rot < 0.f)
        return mpb_failf(MPB_E_INVALID, "%s: k_pos and k_rot must be finite and not negative", who);
    if (A.k_pos == 0.f && A.k_rot == 0.f) return mpb_failf(MPB_E_INVALID, "%s: both terms are off (k_pos = k_rot = 0)", who);
    if (use_axis) {
        if (A.k_rot == 0.f) return mpb_failf(MPB_E_INVALID, "%s: an axis needs the rotation term (k_rot > 0)", who);
        const double n = sqrt((double)A.ax * A.ax + (double)A.ay * A.ay + (double)A.az * A.az);
        if (!ee_finite(A.ax) || !ee_finite(A.ay) || !ee_finite(A.az) || fabs(n - 1.0) > 1e-3) return mpb_failf(MPB_E_INVALID, "%s: axis of length %g is not a unit vector (within 1e-3)", who, n);
    }
    if (A.B == 0) return MPB_OK;
    if (!A.trajs || !A.geom || !A.target || !A.out || (GRAD && !A.grad)) return mpb_failf(MPB_E_INVALID, "%s: null pointer", who);
    if (mpb_misaligned16(A.geom)) return mpb_failf(MPB_E_INVALID, "%s: geom must be 16-byte aligned", who);
    const int rc = ik_chain_check(A.geom, A.D, who);
    if (rc) return rc;
    const hipStream_t s = (hipStream_t)stream;
    if (A.k_rot == 0.f) ee_cost_dispatch<MPB_EE_POS, GRAD>(A, s);
    else if (use_axis) ee_cost_dispatch<MPB_EE_AXIS, GRAD>(A, s);
    else ee_cost_dispatch<MPB_EE_ROT, GRAD>(A, s);
    return mpb_check_launch(who);
}

extern "C" int mpb_ee_cost_eval(const float* trajs, const float* geom, const float* target, float* out, float* per_waypoint, int B, int H, int d,
                                int D, int h_begin, int h_end, int group, int stride_g, int stride_h, float k_pos, float k_rot, int use_axis,
                                float ax, float ay, float az, float weight, int accumulate, void* stream) {
    const EeCostArgs A = {trajs, geom, target, out, per_waypoint, nullptr, B, H, d, D, h_begin, h_end, group, stride_g, stride_h,
                          k_pos, k_rot, ax, ay, az, weight, accumulate};
    return ee_cost_launch<false>(__func__, A, use_axis, stream);
}

extern "C" int mpb_ee_cost_grad(const float* trajs, const float* geom, const float* target, float* out, float* grad, int B, int H, int d, int D,
                                int h_begin, int h_end, int group, int stride_g, int stride_h, float k_pos, float k_rot, int use_axis, float ax,
                                float ay, float az, float weight, int accumulate, void* stream) {
    const EeCostArgs A = {trajs, geom, target, out, nullptr, grad, B, H, d, D, h_begin, h_end, group, stride_g, stride_h,
                          k_pos, k_rot, ax, ay, az, weight, accumulate};
    return ee_cost_launch<true>(__func__, A, use_axis, stream);
}
