// mpb_cartesian.hip -- Cartesian end-effector moves: from many start configurations at once, follow the pose interpolated on the straight
// line (position) and the geodesic (rotation) between the start's own pose and a goal pose, K steps, every step warm-started from the
// last accepted configuration (mpb_cartesian_path; the definition is include/mpb.h).  What MoveIt calls
// computeCartesianPath, batched: the approach to a grasp, the retreat after it, a lift, an insertion.
//
// One LANE per problem (target n, start s), the per-lane state of ik_solve_kernel carried along a path: no LDS, no barrier, no atomics,
// no cross-lane arithmetic -- a problem's bits depend on its own inputs only.  The one cross-lane operation is the ballot that lets a
// wave leave the inner loop when none of its problems still iterates, and the step loop when all of them have stopped; it changes which
// waves keep working, never a value.  A short trailing loop then fills the rows the wave did not reach.
//   - An inner iteration is ik_solve_kernel's, operation for operation: ee_walk, ee_rot_error, ee_dls_step of mpb_ee.h.  The start pose is the
//     walk of q_0, the bits mpb_fk_ee_pose returns.
//   - The step target is computed in the lane from the two end poses: nothing else is read.
//   - The chain's transforms and the joint limits are wave-uniform scalar loads; no register array is indexed by a run-time value.
//   - No collision walk here: the lane already holds the chain's axes and origins and the 6 x 6 system, and nothing may go to scratch.
//     PlanningTask.cartesian_path runs the task's predicates over the finished rows in one call.
#include <limits.h>

#include "mpb_ee.h"

// PO: position only -- the rotation is ignored altogether (no geodesic, rot_err = 0)
template <bool PO>
__global__ __launch_bounds__(64) void cart_path_kernel(const float* __restrict__ target, const float* __restrict__ q_start,
                                                       const float* __restrict__ geom, const float* __restrict__ q_min,
                                                       const float* __restrict__ q_max, float* __restrict__ q_path, float* __restrict__ pos_err,
                                                       float* __restrict__ rot_err, int* __restrict__ n_ok_out, int* __restrict__ status_out,
                                                       int total, int S, int D, int K, int n_inner, float damping, float pos_tol,
                                                       float rot_tol, float jump_max) {
    constexpr int NR = PO ? 3 : 6;
    const int p = blockIdx.x * 64 + threadIdx.x;
    const bool valid = p < total;
    const int pc = valid ? p : total - 1;                    // (a lane past the end works on the last problem and stores nothing)
    const size_t rows = (size_t)K + 1;
    float* qp = q_path + (size_t)pc * rows * D;
    float* pep = pos_err + (size_t)pc * rows;
    float* rep = rot_err + (size_t)pc * rows;
    if (!ik_header_matches(geom, D)) {
        if (valid) {
            const float nan = __int_as_float(0x7FC00000);
            for (size_t i = 0; i < rows * D; ++i) qp[i] = nan;
            for (size_t i = 0; i < rows; ++i) { pep[i] = nan; rep[i] = nan; }
            n_ok_out[p] = 0; status_out[p] = MPB_CART_LOST;
        }
        return;
    }
    const GeomView G = ik_chain_view(geom);
    const float* T = target + (size_t)(pc / S) * 12;
    const float gx = T[3], gy = T[7], gz = T[11];
    float q[MPB_MAX_DOF], qa[MPB_MAX_DOF];                   // q: the iterate; qa: the last accepted configuration
#pragma unroll
    for (int i = 0; i < MPB_MAX_DOF; ++i) q[i] = qa[i] = (i < D) ? q_start[(size_t)pc * D + i] : 0.f;
    // the start pose, and once per problem the rotation from R_0 to R*: angle theta about the unit axis a
    float b00 = 0.f, b01 = 0.f, b02 = 0.f, b10 = 0.f, b11 = 0.f, b12 = 0.f, b20 = 0.f, b21 = 0.f, b22 = 0.f, t0x, t0y, t0z;
    float ax = 0.f, ay = 0.f, az = 0.f, theta = 0.f;
    int status = MPB_CART_OK;
    {
        FKState<true> F;
        ee_walk(G, q, F);
        t0x = F.tx; t0y = F.ty; t0z = F.tz;
        if constexpr (!PO) {
            b00 = F.r00; b01 = F.r01; b02 = F.r02; b10 = F.r10; b11 = F.r11; b12 = F.r12; b20 = F.r20; b21 = F.r21; b22 = F.r22;
            float wx, wy, wz, nw;
            ee_rot_error(T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10], F, wx, wy, wz, nw, theta);
            // (written so that a NaN angle is refused; the angle itself decides: exactly half a turn away, |w| = 0, is a bad target)
            if (!(theta <= MPB_CART_MAX_TURN)) status = MPB_CART_BAD_TARGET;
            const bool none = nw < 1e-6f;
            theta = none ? 0.f : theta;
            ax = none ? 0.f : wx / nw; ay = none ? 0.f : wy / nw; az = none ? 0.f : wz / nw;
        }
    }
    if (valid) {
        static_for<0, MPB_MAX_DOF>([&](auto jc) {
            constexpr int J = decltype(jc)::value;
            if (J < D) qp[J] = qa[J];                        // row 0: q_0's bits
        });
        pep[0] = 0.f; rep[0] = 0.f;
    }
    const float lam2 = damping * damping;
    const bool limits = q_min != nullptr;
    const float fK = (float)K;
    bool active = status == MPB_CART_OK;
    int n_ok = 0;
    int k = 1;
    for (; k <= K; ++k) {
        if (__ballot(active) == 0ull) break;                 // wave-uniform: every problem of the wave has stopped
        // the step target: t_k = (1 - s) t_0 + s t*,  R_k = Rod(a, s theta) R_0
        const float s = (float)k / fK, u = 1.0f - s;
        const float hx = fmaf(s, gx, u * t0x), hy = fmaf(s, gy, u * t0y), hz = fmaf(s, gz, u * t0z);
        float s00 = 0.f, s01 = 0.f, s02 = 0.f, s10 = 0.f, s11 = 0.f, s12 = 0.f, s20 = 0.f, s21 = 0.f, s22 = 0.f;
        if constexpr (!PO) {
            const float phi = s * theta;
            const float sn = sinf(phi), cs = cosf(phi), v = 1.0f - cs;
            const float vx = v * ax, vy = v * ay, vz = v * az;
            const float d00 = fmaf(vx, ax, cs), d01 = fmaf(vx, ay, -(sn * az)), d02 = fmaf(vx, az, sn * ay);
            const float d10 = fmaf(vy, ax, sn * az), d11 = fmaf(vy, ay, cs), d12 = fmaf(vy, az, -(sn * ax));
            const float d20 = fmaf(vz, ax, -(sn * ay)), d21 = fmaf(vz, ay, sn * ax), d22 = fmaf(vz, az, cs);
            s00 = dot3(d00, b00, d01, b10, d02, b20); s01 = dot3(d00, b01, d01, b11, d02, b21); s02 = dot3(d00, b02, d01, b12, d02, b22);
            s10 = dot3(d10, b00, d11, b10, d12, b20); s11 = dot3(d10, b01, d11, b11, d12, b21); s12 = dot3(d10, b02, d11, b12, d12, b22);
            s20 = dot3(d20, b00, d21, b10, d22, b20); s21 = dot3(d20, b01, d21, b11, d22, b21); s22 = dot3(d20, b02, d21, b12, d22, b22);
        }
        // at most n_inner iterations of mpb_ik_solve from the last accepted configuration; a stopped problem is frozen like a converged one
        float pe = 0.f, th = 0.f;
        bool conv = false;
        for (int it = 0;; ++it) {
            FKState<true> F;
            ee_walk(G, q, F);
            float e[NR];
            e[0] = hx - F.tx; e[1] = hy - F.ty; e[2] = hz - F.tz;
            pe = sqrtf(fmaf(e[2], e[2], fmaf(e[1], e[1], e[0] * e[0])));
            float wx = 0.f, wy = 0.f, wz = 0.f, nw = 0.f;
            if constexpr (!PO) ee_rot_error(s00, s01, s02, s10, s11, s12, s20, s21, s22, F, wx, wy, wz, nw, th);
            conv = pe <= pos_tol && (PO || th <= rot_tol);
            if (it >= n_inner) break;
            if (__ballot(active && !conv) == 0ull) break;    // wave-uniform: nothing in the wave iterates any more
            if constexpr (!PO) ee_rot_step_error(wx, wy, wz, nw, th, e);
            ee_dls_step<PO>(F, D, e, lam2, limits, q_min, q_max, conv || !active, q);
        }
        // lost, jumped or accepted
        float jump = 0.f;
        static_for<0, MPB_MAX_DOF>([&](auto jc) {
            constexpr int J = decltype(jc)::value;
            if (J < D) jump = fmaxf(jump, fabsf(q[J] - qa[J]));
        });
        const bool was = active;
        const bool lost = !conv, jumped = !(jump <= jump_max);      // (a NaN is never accepted)
        const bool accept = was && !lost && !jumped;
        status = (was && lost) ? MPB_CART_LOST : (was && jumped) ? MPB_CART_JUMP : status;
        n_ok = accept ? k : n_ok;
        active = accept;
        static_for<0, MPB_MAX_DOF>([&](auto jc) {
            constexpr int J = decltype(jc)::value;
            qa[J] = accept ? q[J] : qa[J];
            q[J] = qa[J];
        });
        if (valid) {
            // row k: the accepted configuration, or the held one; the errors of the step that was judged, 0 once stopped
            static_for<0, MPB_MAX_DOF>([&](auto jc) {
                constexpr int J = decltype(jc)::value;
                if (J < D) qp[(size_t)k * D + J] = qa[J];
            });
            pep[k] = was ? pe : 0.f;
            rep[k] = was ? th : 0.f;
        }
    }
    if (valid) {
        for (; k <= K; ++k) {                                // the rows the wave did not reach: hold still
            static_for<0, MPB_MAX_DOF>([&](auto jc) {
                constexpr int J = decltype(jc)::value;
                if (J < D) qp[(size_t)k * D + J] = qa[J];
            });
            pep[k] = 0.f; rep[k] = 0.f;
        }
        n_ok_out[p] = n_ok;
        status_out[p] = status;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
extern "C" int mpb_cartesian_path(const float* target, const float* q_start, const float* geom, const float* q_min, const float* q_max,
                                  float* q_path, float* pos_err, float* rot_err, int* n_ok, int* status, int N, int S, int D, int K,
                                  int n_inner, float damping, float pos_tol, float rot_tol, float jump_max, int position_only, void* stream) {
    if (D > MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "%s: D = %d exceeds MPB_MAX_DOF = %d", __func__, D, MPB_MAX_DOF);
    if (N < 0 || S < 0 || D < 1 || (long long)N * (long long)S > INT_MAX - 64) return mpb_failf(MPB_E_INVALID, "%s: bad shape", __func__);
    if (K < 1 || K > MPB_CART_MAX_STEPS) return mpb_failf(MPB_E_INVALID, "%s: K = %d outside 1..%d", __func__, K, MPB_CART_MAX_STEPS);
    if (n_inner < 0 || n_inner > MPB_IK_MAX_ITERS)
        return mpb_failf(MPB_E_INVALID, "%s: n_inner = %d outside 0..%d", __func__, n_inner, MPB_IK_MAX_ITERS);
    if ((long long)K * n_inner > MPB_CART_MAX_WORK)
        return mpb_failf(MPB_E_INVALID, "%s: K * n_inner = %lld beyond %d", __func__, (long long)K * n_inner, MPB_CART_MAX_WORK);
    // (written so that a NaN is refused)
    if (!(damping >= MPB_IK_MIN_DAMPING)) return mpb_failf(MPB_E_INVALID, "%s: damping = %g below %g", __func__, (double)damping, (double)MPB_IK_MIN_DAMPING);
    if (!(pos_tol >= 0.f) || !(rot_tol >= 0.f)) return mpb_failf(MPB_E_INVALID, "%s: negative tolerance", __func__);
    if (!(jump_max > 0.f)) return mpb_failf(MPB_E_INVALID, "%s: jump_max = %g, must be positive (infinity turns the check off)", __func__, (double)jump_max);
    if (N == 0 || S == 0) return MPB_OK;
    if (!target || !q_start || !geom || !q_path || !pos_err || !rot_err || !n_ok || !status || (q_min == nullptr) != (q_max == nullptr))
        return mpb_failf(MPB_E_INVALID, "%s: null pointer (q_min and q_max: both or neither)", __func__);
    if (mpb_misaligned16(geom)) return mpb_failf(MPB_E_INVALID, "%s: geom must be 16-byte aligned", __func__);
    const int rc = ik_chain_check(geom, D, __func__);
    if (rc) return rc;
    const int total = N * S;
    if (position_only)
        hipLaunchKernelGGL(cart_path_kernel<true>, dim3((total + 63) / 64), dim3(64), 0, (hipStream_t)stream, target, q_start, geom, q_min, q_max,
                           q_path, pos_err, rot_err, n_ok, status, total, S, D, K, n_inner, damping, pos_tol, rot_tol, jump_max);
    else
        hipLaunchKernelGGL(cart_path_kernel<false>, dim3((total + 63) / 64), dim3(64), 0, (hipStream_t)stream, target, q_start, geom, q_min, q_max,
                           q_path, pos_err, rot_err, n_ok, status, total, S, D, K, n_inner, damping, pos_tol, rot_tol, jump_max);
    return mpb_check_launch(__func__);
}
