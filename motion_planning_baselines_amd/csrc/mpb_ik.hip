// mpb_ik.hip -- the end effector: its pose and geometric Jacobian (mpb_fk_ee_pose) and batched inverse kinematics by damped least
// squares with a fixed budget (mpb_ik_solve).  What the reference's Panda examples ask of the robot (robot.get_EE_position,
// panda_spheres_GPMP.py:63-64; provider: torch_robotics, absent -- the semantics are build-defined) and the front end
// that turns "put the hand there" into the goal configurations the planners take.
//
// One LANE per problem: a configuration for the pose op, a (target, seed) pair for the solver.  No LDS, no barrier, no atomics, no
// cross-lane arithmetic -- a problem's bits depend on its own inputs only, whatever wave it rides in.  The one cross-lane operation is
// the ballot that lets a wave leave the iteration loop when all of its problems have converged; it changes which waves keep working,
// never a value.
//   - The walk is fk_identity / fk_advance<true> of mpb_geom.h through a GeomView filled from the buffer's first header (kind, n_dof,
//     n_tf, joint_tf: nothing else is read, no obstacle is touched): the chain's transforms are wave-uniform scalar loads, and the pose
//     the solver sees is, bit for bit, the pose mpb_fk_ee_pose returns.
//   - J (6 x D) is never stored.  Column j is (z_j x (t - p_j), z_j) from the z / p arrays FKState<true> keeps; the 21 (position only: 6)
//     distinct entries of J J^T are accumulated joint by joint in a loop fully unrolled over MPB_MAX_DOF, joints at or beyond n_dof
//     contributing zero through selects; the system is solved by a fully unrolled unpivoted Cholesky in registers (damping >= 1e-2
//     bounds its condition number, include/mpb.h), and dq_j = J_j^T y is formed from the same arrays.
//   - No register array is indexed by a run-time value: every loop over joints or matrix entries has compile-time bounds.
//   - The square roots and reciprocals of the Cholesky are the IEEE ones (six of each per iteration, next to a chain walk and a
//     joint loop of several hundred instructions each): a step is up to several radians long and multiplies their error.
#include <limits.h>

#include "mpb_ee.h"   // ik_chain_view, ik_header_matches, ee_walk, ee_jv, spd_solve and the launchers' ik_chain_check: shared with
                      // mpb_ee_cost.hip and mpb_cartesian.hip

__global__ __launch_bounds__(64) void fk_ee_pose_kernel(const float* __restrict__ q_in, const float* __restrict__ geom, float* __restrict__ pose,
                                                        float* __restrict__ jac, int N, int D) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    float* po = pose + (size_t)n * 12;
    float* jo = jac ? jac + (size_t)n * 6 * D : nullptr;
    if (!ik_header_matches(geom, D)) {
        const float nan = __int_as_float(0x7FC00000);
        for (int i = 0; i < 12; ++i) po[i] = nan;
        if (jo) for (int i = 0; i < 6 * D; ++i) jo[i] = nan;
        return;
    }
    const GeomView G = ik_chain_view(geom);
    float q[MPB_MAX_DOF];
#pragma unroll
    for (int i = 0; i < MPB_MAX_DOF; ++i) q[i] = (i < D) ? q_in[(size_t)n * D + i] : 0.f;
    FKState<true> F;
    ee_walk(G, q, F);
    po[0] = F.r00; po[1] = F.r01; po[2] = F.r02; po[3] = F.tx;
    po[4] = F.r10; po[5] = F.r11; po[6] = F.r12; po[7] = F.ty;
    po[8] = F.r20; po[9] = F.r21; po[10] = F.r22; po[11] = F.tz;
    if (jo) {
        static_for<0, MPB_MAX_DOF>([&](auto jc) {
            constexpr int J = decltype(jc)::value;
            if (J < D) {
                float cx, cy, cz;
                ee_jv<J>(F, D, cx, cy, cz);
                jo[0 * D + J] = cx; jo[1 * D + J] = cy; jo[2 * D + J] = cz;
                jo[3 * D + J] = F.zx[J]; jo[4 * D + J] = F.zy[J]; jo[5 * D + J] = F.zz[J];
            }
        });
    }
}

// PO: position only -- the error is e_p, the system the 3 x 3 of the Jacobian's upper half
// (The iteration is written out here and once more as ee_rot_error / ee_rot_step_error / ee_dls_step of mpb_ee.h, which cart_path_kernel
// calls: operation for operation the same.  Calling them here gives the same values but another register allocation -- 169 instead of
// 179 VGPRs, other spill counts: the functions are optimised on their own before they are inlined -- and tests/test_ee_cost_cpu.py holds
// this kernel to the figures it has.  tests/test_gpu_cartesian.py holds the two forms to the same bits.)
template <bool PO>
__global__ __launch_bounds__(64) void ik_solve_kernel(const float* __restrict__ target, const float* __restrict__ q_seed,
                                                      const float* __restrict__ geom, const float* __restrict__ q_min,
                                                      const float* __restrict__ q_max, float* __restrict__ q_out, float* __restrict__ pos_err,
                                                      float* __restrict__ rot_err, unsigned char* __restrict__ converged,
                                                      int* __restrict__ iters_used, int total, int S, int D, int n_iters, float damping,
                                                      float pos_tol, float rot_tol) {
    constexpr int NR = PO ? 3 : 6;
    const int p = blockIdx.x * 64 + threadIdx.x;
    const bool valid = p < total;
    const int pc = valid ? p : total - 1;                    // (a lane past the end works on the last problem and stores nothing)
    const float nan = __int_as_float(0x7FC00000);
    if (!ik_header_matches(geom, D)) {
        if (valid) {
            for (int i = 0; i < D; ++i) q_out[(size_t)p * D + i] = nan;
            pos_err[p] = nan; rot_err[p] = nan; converged[p] = 0; iters_used[p] = 0;
        }
        return;
    }
    const GeomView G = ik_chain_view(geom);
    const float* T = target + (size_t)(pc / S) * 12;
    const float s00 = T[0], s01 = T[1], s02 = T[2], gx = T[3], s10 = T[4], s11 = T[5], s12 = T[6], gy = T[7], s20 = T[8], s21 = T[9],
                s22 = T[10], gz = T[11];
    float q[MPB_MAX_DOF];
#pragma unroll
    for (int i = 0; i < MPB_MAX_DOF; ++i) q[i] = (i < D) ? q_seed[(size_t)pc * D + i] : 0.f;
    const float lam2 = damping * damping;
    const bool limits = q_min != nullptr;
    int used = 0;
    float pe = nan, th = nan;
    bool conv = false;
    for (int it = 0;; ++it) {
        FKState<true> F;
        ee_walk(G, q, F);
        float e[NR];
        e[0] = gx - F.tx; e[1] = gy - F.ty; e[2] = gz - F.tz;
        pe = sqrtf(fmaf(e[2], e[2], fmaf(e[1], e[1], e[0] * e[0])));
        // E = R* R^T, w = vee(E - E^T) / 2, c = (tr E - 1) / 2
        const float e00 = dot3(s00, F.r00, s01, F.r01, s02, F.r02), e01 = dot3(s00, F.r10, s01, F.r11, s02, F.r12),
                    e02 = dot3(s00, F.r20, s01, F.r21, s02, F.r22);
        const float e10 = dot3(s10, F.r00, s11, F.r01, s12, F.r02), e11 = dot3(s10, F.r10, s11, F.r11, s12, F.r12),
                    e12 = dot3(s10, F.r20, s11, F.r21, s12, F.r22);
        const float e20 = dot3(s20, F.r00, s21, F.r01, s22, F.r02), e21 = dot3(s20, F.r10, s21, F.r11, s22, F.r12),
                    e22 = dot3(s20, F.r20, s21, F.r21, s22, F.r22);
        const float wx = 0.5f * (e21 - e12), wy = 0.5f * (e02 - e20), wz = 0.5f * (e10 - e01);
        const float c = 0.5f * (((e00 + e11) + e22) - 1.0f);
        const float nw = sqrtf(fmaf(wz, wz, fmaf(wy, wy, wx * wx)));
        th = atan2f(nw, c);
        conv = pe <= pos_tol && (PO || th <= rot_tol);
        if (it >= n_iters) break;
        if (__ballot(!conv) == 0ull) break;                  // wave-uniform: every problem of the wave is frozen
        if constexpr (!PO) {
            const float sc = (nw < 1e-6f) ? 1.0f : th / nw;  // (exactly half a turn away: w = 0, no rotation step)
            e[3] = sc * wx; e[4] = sc * wy; e[5] = sc * wz;
        }
        // A = J J^T + damping^2 I, lower triangle, joint by joint
        float A[NR][NR];
#pragma unroll
        for (int a = 0; a < NR; ++a)
#pragma unroll
            for (int b = 0; b < NR; ++b) A[a][b] = 0.f;
        static_for<0, MPB_MAX_DOF>([&](auto jc) {
            constexpr int J = decltype(jc)::value;
            float col[6];
            ee_jv<J>(F, D, col[0], col[1], col[2]);
            const bool on = J < D;
            col[3] = on ? F.zx[J] : 0.f; col[4] = on ? F.zy[J] : 0.f; col[5] = on ? F.zz[J] : 0.f;
#pragma unroll
            for (int a = 0; a < NR; ++a)
#pragma unroll
                for (int b = 0; b <= a; ++b) A[a][b] = fmaf(col[a], col[b], A[a][b]);
        });
#pragma unroll
        for (int a = 0; a < NR; ++a) A[a][a] += lam2;
        float y[NR];
        spd_solve<NR>(A, e, y);
        // q <- clamp(q + J^T y); a converged problem is frozen
        static_for<0, MPB_MAX_DOF>([&](auto jc) {
            constexpr int J = decltype(jc)::value;
            if (J < D) {
                float cx, cy, cz;
                ee_jv<J>(F, D, cx, cy, cz);
                float dq = fmaf(cz, y[2], fmaf(cy, y[1], cx * y[0]));
                if constexpr (!PO) dq = fmaf(F.zz[J], y[5], fmaf(F.zy[J], y[4], fmaf(F.zx[J], y[3], dq)));
                float qn = q[J] + dq;
                if (limits) qn = fminf(fmaxf(qn, q_min[J]), q_max[J]);
                q[J] = conv ? q[J] : qn;
            }
        });
        used += conv ? 0 : 1;
    }
    if (valid) {
        static_for<0, MPB_MAX_DOF>([&](auto jc) {
            constexpr int J = decltype(jc)::value;
            if (J < D) q_out[(size_t)p * D + J] = q[J];
        });
        pos_err[p] = pe;
        rot_err[p] = th;
        converged[p] = conv ? 1 : 0;
        iters_used[p] = used;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
extern "C" int mpb_fk_ee_pose(const float* q, const float* geom, float* pose, float* jac, int N, int D, void* stream) {
    if (D > MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "%s: D = %d exceeds MPB_MAX_DOF = %d", __func__, D, MPB_MAX_DOF);
    if (N < 0 || D < 1) return mpb_failf(MPB_E_INVALID, "%s: bad shape", __func__);
    if (N == 0) return MPB_OK;
    if (!q || !geom || !pose) return mpb_failf(MPB_E_INVALID, "%s: null pointer", __func__);
    if (mpb_misaligned16(geom)) return mpb_failf(MPB_E_INVALID, "%s: geom must be 16-byte aligned", __func__);
    const int rc = ik_chain_check(geom, D, __func__);
    if (rc) return rc;
    hipLaunchKernelGGL(fk_ee_pose_kernel, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, q, geom, pose, jac, N, D);
    return mpb_check_launch(__func__);
}

extern "C" int mpb_ik_solve(const float* target, const float* q_seed, const float* geom, const float* q_min, const float* q_max, float* q_out,
                            float* pos_err, float* rot_err, unsigned char* converged, int* iters_used, int N, int S, int D, int n_iters,
                            float damping, float pos_tol, float rot_tol, int position_only, void* stream) {
    if (D > MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "%s: D = %d exceeds MPB_MAX_DOF = %d", __func__, D, MPB_MAX_DOF);
    if (N < 0 || S < 0 || D < 1 || (long long)N * (long long)S > INT_MAX - 64) return mpb_failf(MPB_E_INVALID, "%s: bad shape", __func__);
    if (n_iters < 0 || n_iters > MPB_IK_MAX_ITERS)
        return mpb_failf(MPB_E_INVALID, "%s: n_iters = %d outside 0..%d", __func__, n_iters, MPB_IK_MAX_ITERS);
    // (written so that a NaN is refused)
    if (!(damping >= MPB_IK_MIN_DAMPING)) return mpb_failf(MPB_E_INVALID, "%s: damping = %g below %g", __func__, (double)damping, (double)MPB_IK_MIN_DAMPING);
    if (!(pos_tol >= 0.f) || !(rot_tol >= 0.f)) return mpb_failf(MPB_E_INVALID, "%s: negative tolerance", __func__);
    if (N == 0 || S == 0) return MPB_OK;
    if (!target || !q_seed || !geom || !q_out || !pos_err || !rot_err || !converged || !iters_used || (q_min == nullptr) != (q_max == nullptr))
        return mpb_failf(MPB_E_INVALID, "%s: null pointer (q_min and q_max: both or neither)", __func__);
    if (mpb_misaligned16(geom)) return mpb_failf(MPB_E_INVALID, "%s: geom must be 16-byte aligned", __func__);
    const int rc = ik_chain_check(geom, D, __func__);
    if (rc) return rc;
    const int total = N * S;
    if (position_only)
        hipLaunchKernelGGL(ik_solve_kernel<true>, dim3((total + 63) / 64), dim3(64), 0, (hipStream_t)stream, target, q_seed, geom, q_min, q_max, q_out,
                           pos_err, rot_err, converged, iters_used, total, S, D, n_iters, damping, pos_tol, rot_tol);
    else
        hipLaunchKernelGGL(ik_solve_kernel<false>, dim3((total + 63) / 64), dim3(64), 0, (hipStream_t)stream, target, q_seed, geom, q_min, q_max, q_out,
                           pos_err, rot_err, converged, iters_used, total, S, D, n_iters, damping, pos_tol, rot_tol);
    return mpb_check_launch(__func__);
}
