// mpb_ee.h -- what the end-effector kernels share (mpb_ik.hip: the pose op and the IK solver; mpb_ee_cost.hip: the pose cost): the chain
// of a geometry buffer as fk_advance reads it, the header guard of the kernels, the walk to the last frame, a column of the Jacobian's
// upper half, and the launchers' cached read of a device buffer's header.  Every kernel that walks through ee_walk sees the bits
// mpb_fk_ee_pose returns.
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
