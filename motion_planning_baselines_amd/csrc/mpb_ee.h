// mpb_ee.h -- what the end-effector kernels share (mpb_ik.hip: the pose op and the IK solver; mpb_ee_cost.hip: the pose cost): the chain
// of a geometry buffer as fk_advance reads it, the header guard of the kernels, the walk to the last frame, a column of the Jacobian's
// upper half, and the launchers' cached read of a device buffer's header.  Every kernel that walks through ee_walk sees the bits
// mpb_fk_ee_pose returns.
#pragma once
#include <mutex>

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
// kind / n_dof of a DEVICE geometry buffer's first header: read once per buffer address and device -- a 128-byte synchronous copy -- and
// kept in a small table, as mpb_sdf_grid.hip does -- ONE table for the translation units that include this header (inline variables).  An entry that does not agree with the caller's D is read again before the call is
// refused (the address may hold another robot by now); one that agrees although the buffer changed is caught by the kernels, which compare
// the header with the D they were launched with and answer NaN.
struct IkShape { const void* ptr; int dev, kind, n_dof; };
inline std::mutex g_ik_mu;
inline IkShape g_ik_table[16];
inline int g_ik_n = 0, g_ik_next = 0;

inline int ik_shape(const float* geom, int D, IkShape& out, const char* who) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return mpb_failf(MPB_E_HIP, "%s: hipGetDevice failed", who);
    std::lock_guard<std::mutex> lock(g_ik_mu);
    int slot = -1;
    for (int i = 0; i < g_ik_n; ++i)
        if (g_ik_table[i].ptr == geom && g_ik_table[i].dev == dev) slot = i;
    if (slot >= 0 && g_ik_table[slot].kind == MPB_KIND_CHAIN && g_ik_table[slot].n_dof == D) { out = g_ik_table[slot]; return MPB_OK; }
    int32_t hdr[MPB_GEOM_HEADER_WORDS];
    const hipError_t e = hipMemcpy(hdr, geom, sizeof(hdr), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return mpb_failf(MPB_E_HIP, "%s: reading the geometry header failed: %s", who, hipGetErrorString(e));
    if (hdr[MPB_GW_MAGIC] != MPB_GEOM_MAGIC || (hdr[MPB_GW_VERSION] != MPB_GEOM_VERSION && hdr[MPB_GW_VERSION] != MPB_GEOM_VERSION_LIST))
        return mpb_failf(MPB_E_INVALID, "%s: bad magic/version of the geometry buffer", who);
    out = {geom, dev, hdr[MPB_GW_KIND], hdr[MPB_GW_N_DOF]};
    if (slot < 0) {
        slot = g_ik_next;
        g_ik_next = (g_ik_next + 1) % 16;
        g_ik_n = g_ik_n < 16 ? g_ik_n + 1 : 16;
    }
    g_ik_table[slot] = out;
    return MPB_OK;
}

// refusals 5 and 6 of include/mpb.h: what only the buffer's header tells
inline int ik_chain_check(const float* geom, int D, const char* who) {
    IkShape S;
    const int rc = ik_shape(geom, D, S, who);
    if (rc) return rc;
    if (S.kind != MPB_KIND_CHAIN) return mpb_failf(MPB_E_UNSUPPORTED, "%s: a point robot has no end effector", who);
    if (D != S.n_dof) return mpb_failf(MPB_E_INVALID, "%s: D = %d, the chain has %d joints", who, D, S.n_dof);
    return MPB_OK;
}
