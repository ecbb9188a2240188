// mpb_ee.h -- what the end-effector kernels share (mpb_ik.hip: the pose op and the IK solver; mpb_ee_cost.hip: the pose cost;
// mpb_cartesian.hip: straight-line tracking): the chain of a geometry buffer as fk_advance reads it, the header guard of the kernels,
// the walk to the last frame, a column of the Jacobian's upper half, the rotation error and one damped-least-squares step (the solver's
// iteration, operation for operation, for the tracker), and the launchers' cached read of a device buffer's header.  Every kernel that walks
// through ee_walk sees the bits mpb_fk_ee_pose returns.
#pragma once
#include "mpb_common.h"
#include "mpb_geom.h"
#include "mpb_host.h"

// the chain of a geometry buffer's first field as the GeomView fk_advance reads (tf, n_dof); no links, no obstacles
__device__ __forceinline__ GeomView ik_chain_view(const float* __restrict__ g) {
    const int* gi = reinterpret_cast<const int*>(g);
    GeomView v = {};
    v.kind = gi[MPB_GW_KIND];
    v.n_dof = gi[MPB_GW_N_DOF];
    v.n_tf = gi[MPB_GW_N_TF];
    v.tf = g + gi[MPB_GW_OFF_TF];
    return v;
}

// the launcher read kind / n_dof from the header once per buffer address; the kernels walk by the BUFFER's numbers and refuse (NaN
// outputs, nothing converged) when those are not the launcher's -- an address that got another robot since
__device__ __forceinline__ bool ik_header_matches(const float* __restrict__ g, int D) {
    const int* gi = reinterpret_cast<const int*>(g);
    return gi[MPB_GW_MAGIC] == MPB_GEOM_MAGIC && gi[MPB_GW_KIND] == MPB_KIND_CHAIN && gi[MPB_GW_N_DOF] == D && gi[MPB_GW_N_TF] == D + 1;
}

// frame_{n_dof + 1} of configuration q: the end effector's R, t in F, the joints' axes z_j and origins p_j in its arrays
__device__ __forceinline__ void ee_walk(const GeomView& G, const float (&q)[MPB_MAX_DOF], FKState<true>& F) {
    fk_identity(F);
    F.frame = 0;
#pragma unroll
    for (int i = 0; i < MPB_MAX_DOF; ++i) { F.zx[i] = F.zy[i] = F.zz[i] = F.px[i] = F.py[i] = F.pz[i] = 0.f; }
    for (int j = 0; j <= G.n_dof; ++j) fk_advance<true>(G, F, q);
}

// column j of the Jacobian's upper half, z_j x (t - p_j), in the fma form of joint_term (mpb_geom.h); zero for a joint the chain has not
template <int J>
__device__ __forceinline__ void ee_jv(const FKState<true>& F, int D, float& cx, float& cy, float& cz) {
    const float ex = F.tx - F.px[J], ey = F.ty - F.py[J], ez = F.tz - F.pz[J];
    const bool on = J < D;
    cx = on ? fmaf(F.zy[J], ez, -(F.zz[J] * ey)) : 0.f;
    cy = on ? fmaf(F.zz[J], ex, -(F.zx[J] * ez)) : 0.f;
    cz = on ? fmaf(F.zx[J], ey, -(F.zy[J] * ex)) : 0.f;
}

// ---- one damped-least-squares iteration of ik_solve_kernel (mpb_ik.hip, which keeps it written out: see there) as functions: what
// cart_path_kernel (mpb_cartesian.hip) calls; spd_solve is shared by both --------------------------------------------------------
// the rotation error of include/mpb.h against the target rotation (s00 .. s22): E = R* R^T, w = vee(E - E^T) / 2, c = (tr E - 1) / 2,
// nw = |w|, th = atan2(|w|, c)
__device__ __forceinline__ void ee_rot_error(float s00, float s01, float s02, float s10, float s11, float s12, float s20, float s21, float s22,
                                             const FKState<true>& F, float& wx, float& wy, float& wz, float& nw, float& th) {
    const float e00 = dot3(s00, F.r00, s01, F.r01, s02, F.r02), e01 = dot3(s00, F.r10, s01, F.r11, s02, F.r12),
                e02 = dot3(s00, F.r20, s01, F.r21, s02, F.r22);
    const float e10 = dot3(s10, F.r00, s11, F.r01, s12, F.r02), e11 = dot3(s10, F.r10, s11, F.r11, s12, F.r12),
                e12 = dot3(s10, F.r20, s11, F.r21, s12, F.r22);
    const float e20 = dot3(s20, F.r00, s21, F.r01, s22, F.r02), e21 = dot3(s20, F.r10, s21, F.r11, s22, F.r12),
                e22 = dot3(s20, F.r20, s21, F.r21, s22, F.r22);
    wx = 0.5f * (e21 - e12), wy = 0.5f * (e02 - e20), wz = 0.5f * (e10 - e01);
    const float c = 0.5f * (((e00 + e11) + e22) - 1.0f);
    nw = sqrtf(fmaf(wz, wz, fmaf(wy, wy, wx * wx)));
    th = atan2f(nw, c);
}

// e_w = (theta / |w|) w into e[3..5]
__device__ __forceinline__ void ee_rot_step_error(float wx, float wy, float wz, float nw, float th, float (&e)[6]) {
    const float sc = (nw < 1e-6f) ? 1.0f : th / nw;  // (exactly half a turn away: w = 0, no rotation step)
    e[3] = sc * wx; e[4] = sc * wy; e[5] = sc * wz;
}

// x = A^{-1} e for the SPD A given by its lower triangle (A[i][j], j <= i): unpivoted Cholesky A = L L^T with reciprocal pivots, the
// two substitutions.  Fully unrolled, every index a compile-time constant.
template <int NR>
__device__ __forceinline__ void spd_solve(float (&A)[NR][NR], const float (&e)[NR], float (&x)[NR]) {
    float inv[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            float s = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) s = fmaf(-A[i][k], A[j][k], s);
            if (i == j) {
                const float l = sqrtf(s);
                inv[i] = 1.0f / l;
                A[i][i] = l;
            } else {
                A[i][j] = s * inv[j];
            }
        }
    }
    float y[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        float s = e[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = fmaf(-A[i][k], y[k], s);
        y[i] = s * inv[i];
    }
#pragma unroll
    for (int i = NR - 1; i >= 0; --i) {
        float s = y[i];
#pragma unroll
        for (int k = i + 1; k < NR; ++k) s = fmaf(-A[k][i], x[k], s);
        x[i] = s * inv[i];
    }
}

// q <- clamp(q + J^T (J J^T + lam2 I)^{-1} e) at the walk F of q; a frozen problem keeps its q.  PO: position only -- e is e_p, the
// system the 3 x 3 of the Jacobian's upper half.
template <bool PO>
__device__ __forceinline__ void ee_dls_step(const FKState<true>& F, int D, const float (&e)[PO ? 3 : 6], float lam2, bool limits,
                                            const float* q_min, const float* q_max, bool frozen,
                                            float (&q)[MPB_MAX_DOF]) {
    constexpr int NR = PO ? 3 : 6;
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
    static_for<0, MPB_MAX_DOF>([&](auto jc) {
        constexpr int J = decltype(jc)::value;
        if (J < D) {
            float cx, cy, cz;
            ee_jv<J>(F, D, cx, cy, cz);
            float dq = fmaf(cz, y[2], fmaf(cy, y[1], cx * y[0]));
            if constexpr (!PO) dq = fmaf(F.zz[J], y[5], fmaf(F.zy[J], y[4], fmaf(F.zx[J], y[3], dq)));
            float qn = q[J] + dq;
            if (limits) qn = fminf(fmaxf(qn, q_min[J]), q_max[J]);
            q[J] = frozen ? q[J] : qn;
        }
    });
}

// ---- host side ------------------------------------------------------------------------------------------------------
// kind / n_dof of a device geometry buffer's first header, through the cache of mpb_host.h (its contract is stated there) -- ONE table for
// the translation units that include this header (an inline variable).  A geometry buffer has no invalidate: an entry that does not agree
// with the caller's D is read again, in place, before the call is refused (the address may hold another robot by now).
struct IkShape { const void* ptr; int dev, kind, n_dof; };
inline MpbHeaderCache<IkShape, MPB_GEOM_HEADER_WORDS> g_ik_cache;

// refusals 5 and 6 of include/mpb.h: what only the buffer's header tells
inline int ik_chain_check(const float* geom, int D, const char* who) {
    IkShape S;
    const int rc = g_ik_cache.get(
        geom, S, who, "geometry",
        [who](const int32_t* hdr, IkShape& s) {
            if (hdr[MPB_GW_MAGIC] != MPB_GEOM_MAGIC || (hdr[MPB_GW_VERSION] != MPB_GEOM_VERSION && hdr[MPB_GW_VERSION] != MPB_GEOM_VERSION_LIST))
                return mpb_failf(MPB_E_INVALID, "%s: bad magic/version of the geometry buffer", who);
            s.kind = hdr[MPB_GW_KIND], s.n_dof = hdr[MPB_GW_N_DOF];
            return MPB_OK;
        },
        [D](const IkShape& s) { return s.kind == MPB_KIND_CHAIN && s.n_dof == D; });
    if (rc) return rc;
    if (S.kind != MPB_KIND_CHAIN) return mpb_failf(MPB_E_UNSUPPORTED, "%s: a point robot has no end effector", who);
    if (D != S.n_dof) return mpb_failf(MPB_E_INVALID, "%s: D = %d, the chain has %d joints", who, D, S.n_dof);
    return MPB_OK;
}
