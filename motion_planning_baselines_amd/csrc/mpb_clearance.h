// mpb_clearance.h -- the clearance walk of one configuration (definition: include/mpb.h):
//   eta_l(q) = min_f (sd_f(x_l(q)) - margin_f) - r_l
// for every collision sphere l in link-table order, handed to the caller one sphere at a time so that it keeps the running minima
// its decision needs (mpb_certify.hip: the clearance op keeps min / arg-min, the certifier also eta_l - w Lambda_l per sphere).
//
// One LANE walks one configuration, as in mpb_geom.h: the chain through FKState / fk_advance / link_centre (a point robot: the
// configuration is the centre), every table word through wave-uniform indices (scalar loads).  The obstacle walk is EXHAUSTIVE --
// sphere_sd / box_sd of mpb_geom.h over every obstacle of every chained field: the broad-phase grids and the cull table only know
// obstacles within the hinge threshold, a distance needs them all.  The robot tables are the FIRST field's; every field of the
// chain must carry the whole link table (the host side asks for a geometry packed with keep_all_links).
// Nothing here edits or re-instantiates an evaluator of mpb_geom.h.
#pragma once
#include "mpb_common.h"
#include "mpb_geom.h"
#include "mpb_member_cost.h"

// what a launch knows of the geometry chain beside the robot: does every header of it describe a robot of D joints and L spheres of
// this kind?  (At most MPB_MAX_FIELDS headers are looked at; a longer chain is a changed buffer.)
__device__ __forceinline__ bool clr_headers_ok(const float* __restrict__ geom, int D, int L) {
    const float* gp = geom;
    bool ok = true;
    int n = 0;
    for (; gp != nullptr && n < MPB_MAX_FIELDS; ++n) {
        const int* gi = reinterpret_cast<const int*>(gp);
        ok = ok && gi[MPB_GW_MAGIC] == MPB_GEOM_MAGIC && gi[MPB_GW_N_DOF] == D && gi[MPB_GW_N_LINKS] == L &&
             (gi[MPB_GW_KIND] == MPB_KIND_POINT || gi[MPB_GW_KIND] == MPB_KIND_CHAIN) && gi[MPB_GW_KIND] == reinterpret_cast<const int*>(geom)[MPB_GW_KIND];
        if (!ok) break;
        gp = geom_next(gp);
    }
    return ok && gp == nullptr;
}

// min_f (sd_f(x) - margin_f) over the chained fields: every obstacle sphere and box of every field
__device__ __forceinline__ float clr_point_distance(const float* __restrict__ geom, float x, float y, float z) {
    float best = 3.0e38f;
    int n = 0;
    for (const float* gp = geom; gp != nullptr && n < MPB_MAX_FIELDS; gp = geom_next(gp), ++n) {
        const int* gi = reinterpret_cast<const int*>(gp);
        const int n_sph = gi[MPB_GW_N_SPH], n_box = gi[MPB_GW_N_BOX];
        const float4* sp = reinterpret_cast<const float4*>(gp + gi[MPB_GW_OFF_SPH]);
        const float4* bp = reinterpret_cast<const float4*>(gp + gi[MPB_GW_OFF_BOX]);
        float sd = 3.0e38f;
        for (int o = 0; o < n_sph; ++o) sd = fminf(sd, sphere_sd(x, y, z, sp[o]));
        for (int o = 0; o < n_box; ++o) sd = fminf(sd, box_sd(x, y, z, bp[2 * o], bp[2 * o + 1]));
        best = fminf(best, sd - gp[MPB_GW_MARGIN]);
    }
    return best;
}

// per_sphere(l, eta_l) for l = 0 .. n_links - 1 of configuration q, in link-table order
template <class Fn>
__device__ __forceinline__ void clearance_walk(const float* __restrict__ geom, const float (&q)[MPB_MAX_DOF], Fn&& per_sphere) {
    const GeomView G = geom_view(geom);
    if (G.kind == MPB_KIND_POINT) {
        per_sphere(0, clr_point_distance(geom, q[0], q[1], (G.n_dof > 2) ? q[2] : 0.f) - G.links[4]);
        return;
    }
    FKState<false> F;
    fk_identity(F);
    F.frame = 0;
    for (int l = 0; l < G.n_links; ++l) {
        const float4 lk = *reinterpret_cast<const float4*>(G.links + 8 * l);   // frame, ox, oy, oz
        const int f = min(__float_as_int(lk.x), G.n_tf);
        while (F.frame < f) fk_advance<false>(G, F, q);
        float x, y, z;
        link_centre(F, lk, x, y, z);
        per_sphere(l, clr_point_distance(geom, x, y, z) - G.links[8 * l + 4]);
    }
}
