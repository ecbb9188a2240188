// mpb_self.h -- the per-lane device functions of a packed self-collision buffer (include/mpb_self_layout.h), shared by the stand-alone
// kernels of mpb_self_collision.hip and the world predicate of mpb_world.h: the chain view, the three phases (centres to LDS as
// [link][xyz][lane], the pair sum, J^T) and the header comparison.  mpb_self_collision.hip has the definitions in words (mapping, LDS
// sizing, order of the sums); the text below is what stood there, unchanged.
#pragma once
#include "mpb_common.h"
#include "mpb_geom.h"
#include "mpb_member_cost.h"
#include "../../include/mpb_self_layout.h"

// the chain of a self buffer as the GeomView fk_advance reads (tf, n_dof) and the walks below read (links, n_links); no obstacles
__device__ __forceinline__ GeomView self_view(const float* __restrict__ s) {
    const int* si = reinterpret_cast<const int*>(s);
    GeomView v = {};
    v.kind = MPB_KIND_CHAIN;
    v.n_dof = si[MPB_SW_N_DOF];
    v.n_tf = si[MPB_SW_N_TF];
    v.n_links = si[MPB_SW_N_LINKS];
    v.margin = s[MPB_SW_MARGIN];
    v.tf = s + si[MPB_SW_OFF_TF];
    v.links = s + si[MPB_SW_OFF_LINKS];
    return v;
}

// phase 1: centres of the L collision spheres of configuration q into this lane's column of pos ([link][xyz][lane]); GRAD: zero the
// lane's column of the force array
template <bool GRAD>
__device__ __forceinline__ void self_store_centres(const GeomView& G, int L, const float (&q)[MPB_MAX_DOF], float* __restrict__ pos,
                                                   float* __restrict__ frc, int lane) {
    FKState<false> F;
    fk_identity(F);
    F.frame = 0;
    for (int l = 0; l < L; ++l) {
        const float4 lk = *reinterpret_cast<const float4*>(G.links + 8 * l);   // frame, ox, oy, oz
        const int f = min(__float_as_int(lk.x), G.n_tf);                       // (a checked buffer never clamps: keeps the walk inside tf)
        while (F.frame < f) fk_advance<false>(G, F, q);
        float* p = pos + l * 192 + lane;
        p[0] = mad3(F.r00, lk.y, F.r01, lk.z, F.r02, lk.w, F.tx);
        p[64] = mad3(F.r10, lk.y, F.r11, lk.z, F.r12, lk.w, F.ty);
        p[128] = mad3(F.r20, lk.y, F.r21, lk.z, F.r22, lk.w, F.tz);
        if (GRAD) {
            float* g = frc + l * 192 + lane;
            g[0] = g[64] = g[128] = 0.f;
        }
    }
}

// phase 2: sum of the hinges over the pair table (table order, fp32); GRAD: d c / d x_a = -(x_a - x_b) / n, d c / d x_b = +(x_a - x_b) / n
// of every active pair into frc; a pair with n == 0 contributes no force (the oracle's safe-norm sub-gradient).  Returns c; `any` is set
// when a force was written.
template <bool GRAD>
__device__ __forceinline__ float self_pair_sum(const float* __restrict__ pairs, int n_pairs, int L, const float* __restrict__ pos,
                                               float* __restrict__ frc, int lane, bool& any) {
    float c = 0.f;
    for (int p = 0; p < n_pairs; ++p) {
        const unsigned w = __float_as_uint(pairs[MPB_SELF_PAIR_WORDS * p]);
        const float T = pairs[MPB_SELF_PAIR_WORDS * p + 1];
        const int a = min((int)(w & MPB_SELF_PAIR_A_MASK), L - 1), b = min((int)(w >> MPB_SELF_PAIR_B_SHIFT), L - 1);   // (wave-uniform; a checked buffer never clamps)
        const float* pa = pos + a * 192 + lane;
        const float* pb = pos + b * 192 + lane;
        const float dx = pa[0] - pb[0], dy = pa[64] - pb[64], dz = pa[128] - pb[128];
        const float n = fast_sqrt(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
        const float hng = T - n;
        if (hng > 0.f) {
            c += hng;
            if (GRAD && n > 0.f) {
                const float ux = dx / n, uy = dy / n, uz = dz / n;
                float* ga = frc + a * 192 + lane;
                float* gb = frc + b * 192 + lane;
                ga[0] -= ux; ga[64] -= uy; ga[128] -= uz;
                gb[0] += ux; gb[64] += uy; gb[128] += uz;
                any = true;
            }
        }
    }
    return c;
}

// phase 3: dq = J^T frc by a second walk (d x_l / d q_i = z_i x (x_l - p_i) for the joints upstream of the sphere's frame)
__device__ __forceinline__ void self_apply_jt(const GeomView& G, int L, const float (&q)[MPB_MAX_DOF], const float* __restrict__ frc,
                                              int lane, float (&dq)[MPB_MAX_DOF]) {
    FKState<true> F;
    fk_identity(F);
    F.frame = 0;
#pragma unroll
    for (int i = 0; i < MPB_MAX_DOF; ++i) { F.zx[i] = F.zy[i] = F.zz[i] = F.px[i] = F.py[i] = F.pz[i] = 0.f; }
    for (int l = 0; l < L; ++l) {
        const float4 lk = *reinterpret_cast<const float4*>(G.links + 8 * l);
        const int f = min(__float_as_int(lk.x), G.n_tf);
        while (F.frame < f) fk_advance<true>(G, F, q);
        const float* g = frc + l * 192 + lane;
        const float fx = g[0], fy = g[64], fz = g[128];
        float x, y, z;
        link_centre(F, lk, x, y, z);
#pragma unroll
        for (int i = 0; i < MPB_MAX_DOF; ++i)
            if (i < f && i < G.n_dof) dq[i] += joint_term(F.zx[i], F.zy[i], F.zz[i], F.px[i], F.py[i], F.pz[i], x, y, z, fx, fy, fz);
    }
}

// the launcher read n_dof / n_links / n_pairs from the header to size the LDS and to check the row width; the kernels use ITS numbers
// for every LDS address and every row index and refuse (NaN outputs) a buffer whose header has changed since
__device__ __forceinline__ bool self_header_matches(const float* __restrict__ s, int n_dof, int L, int n_pairs) {
    const int* si = reinterpret_cast<const int*>(s);
    return si[MPB_SW_MAGIC] == MPB_SELF_MAGIC && si[MPB_SW_N_DOF] == n_dof && si[MPB_SW_N_LINKS] == L && si[MPB_SW_N_PAIRS] == n_pairs;
}
