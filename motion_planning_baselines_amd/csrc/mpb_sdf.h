// mpb_sdf.h -- the per-lane device functions of a packed SDF-grid buffer (include/mpb_sdf_layout.h), shared by the stand-alone kernels of
// mpb_sdf_grid.hip and the world predicate of mpb_world.h: the robot view, the lattice, the sampler (sdf_axis, sdf_load, sdf_value,
// sdf_gradient), the waypoint cost and the header comparison.  mpb_sdf_grid.hip has the definitions in words (sampling, mapping, order of
// the sums); the text below is what stood there, unchanged.  Compiled under the build's contraction in every kernel that includes it.
#pragma once
#include "mpb_common.h"
#include "mpb_geom.h"
#include "mpb_member_cost.h"
#include "../../include/mpb_sdf_layout.h"

#define MPB_SDF_GROUP 4

// the robot of an SDF buffer as the GeomView fk_advance reads (tf, n_dof) and the walk below reads (links, n_links); no obstacles
__device__ __forceinline__ GeomView sdf_robot_view(const float* __restrict__ s) {
    const int* si = reinterpret_cast<const int*>(s);
    GeomView v = {};
    v.kind = si[MPB_DW_KIND];
    v.n_dof = si[MPB_DW_N_DOF];
    v.n_tf = si[MPB_DW_N_TF];
    v.n_links = si[MPB_DW_N_LINKS];
    v.margin = s[MPB_DW_MARGIN];
    v.tf = s + si[MPB_DW_OFF_TF];
    v.links = s + si[MPB_DW_OFF_LINKS];
    return v;
}

// the lattice: dims as the LAUNCHER read them (every node index is formed from these), the rest from the header
struct SdfLattice {
    int nx, ny, nz;
    float lx, ly, lz, inv;
    const float* nodes;
};

__device__ __forceinline__ SdfLattice sdf_lattice(const float* __restrict__ s, int nx, int ny, int nz) {
    const int* si = reinterpret_cast<const int*>(s);
    SdfLattice S;
    S.nx = nx; S.ny = ny; S.nz = nz;
    S.lx = s[MPB_DW_LO]; S.ly = s[MPB_DW_LO + 1]; S.lz = s[MPB_DW_LO + 2];
    S.inv = s[MPB_DW_INV_CELL];
    S.nodes = s + si[MPB_DW_OFF_NODES];
    return S;
}

// one axis: cell index i0 in [0, n - 2], fraction f in [0, 1], inside = the point is not beyond the box on this axis (a NaN coordinate
// lands on node 0 and counts as outside)
__device__ __forceinline__ void sdf_axis(float x, float lo, float inv, int n, int& i0, float& f, bool& inside) {
    const float u = (x - lo) * inv;
    const float top = (float)(n - 1);
    inside = (u >= 0.f) && (u <= top);
    const float uc = fminf(fmaxf(u, 0.f), top);
    i0 = min((int)floorf(uc), n - 2);
    f = uc - (float)i0;
}

// the nodes around one point and where it sits among them: the loads are issued here, their first use is in sdf_value / sdf_gradient
struct SdfTaps {
    float v000, v100, v010, v110, v001, v101, v011, v111;
    float fx, fy, fz;
    bool inx, iny, inz;
};

// (Loading the two x-neighbours as ONE 8-byte word pair was measured and changed nothing -- 3.007 against 3.011 ms at N = 131 072, DESIGN.md
// 10: the kernels wait for the four cache lines a sphere's gather touches, not for the address cycles -- so the plain form stays.)
__device__ __forceinline__ void sdf_load(const SdfLattice& S, float x, float y, float z, SdfTaps& T) {
    int i0, j0, k0 = 0;
    sdf_axis(x, S.lx, S.inv, S.nx, i0, T.fx, T.inx);
    sdf_axis(y, S.ly, S.inv, S.ny, j0, T.fy, T.iny);
    const float* p = S.nodes + (j0 * S.nx + i0);                 // (the two x-neighbours are adjacent words)
    if (S.nz > 1) {                                             // (wave-uniform)
        sdf_axis(z, S.lz, S.inv, S.nz, k0, T.fz, T.inz);
        p += k0 * S.ny * S.nx;                                  // (< 2^27: the validator's node limit)
        const float* pz = p + S.ny * S.nx;
        T.v001 = pz[0]; T.v101 = pz[1]; T.v011 = pz[S.nx]; T.v111 = pz[S.nx + 1];
    }
    T.v000 = p[0]; T.v100 = p[1]; T.v010 = p[S.nx]; T.v110 = p[S.nx + 1];
    if (S.nz <= 1) {
        T.fz = 0.f; T.inz = false;
        T.v001 = T.v000; T.v101 = T.v100; T.v011 = T.v010; T.v111 = T.v110;
    }
}

__device__ __forceinline__ float sdf_lerp(float f, float v0, float v1) { return fmaf(f, v1 - v0, v0); }

__device__ __forceinline__ float sdf_value(const SdfTaps& T) {
    const float c00 = sdf_lerp(T.fx, T.v000, T.v100), c10 = sdf_lerp(T.fx, T.v010, T.v110);
    const float c01 = sdf_lerp(T.fx, T.v001, T.v101), c11 = sdf_lerp(T.fx, T.v011, T.v111);
    return sdf_lerp(T.fz, sdf_lerp(T.fy, c00, c10), sdf_lerp(T.fy, c01, c11));
}

// value and d s / d x of the interpolant: along x the y-z interpolation of the four x-differences, along y the z interpolation of the two
// y-differences of the x-interpolated edges, along z the difference of the two faces; times inv_cell (d u / d x), 0 on a clamped axis
__device__ __forceinline__ float sdf_gradient(const SdfTaps& T, float inv, float& gx, float& gy, float& gz) {
    const float c00 = sdf_lerp(T.fx, T.v000, T.v100), c10 = sdf_lerp(T.fx, T.v010, T.v110);
    const float c01 = sdf_lerp(T.fx, T.v001, T.v101), c11 = sdf_lerp(T.fx, T.v011, T.v111);
    const float c0 = sdf_lerp(T.fy, c00, c10), c1 = sdf_lerp(T.fy, c01, c11);
    const float dx0 = sdf_lerp(T.fy, T.v100 - T.v000, T.v110 - T.v010), dx1 = sdf_lerp(T.fy, T.v101 - T.v001, T.v111 - T.v011);
    const float dx = sdf_lerp(T.fz, dx0, dx1);
    const float dy = sdf_lerp(T.fz, c10 - c00, c11 - c01);
    const float dz = c1 - c0;
    gx = T.inx ? dx * inv : 0.f;
    gy = T.iny ? dy * inv : 0.f;
    gz = T.inz ? dz * inv : 0.f;
    return sdf_lerp(T.fz, c0, c1);
}

// c(q) of one waypoint; GRAD: dq[i] = d c / d q_i (i < n_dof).  q / dq are register arrays indexed only with compile-time indices.
template <bool GRAD>
__device__ __forceinline__ float sdf_waypoint_cost(const GeomView& G, const SdfLattice& S, int L, const float (&q)[MPB_MAX_DOF],
                                                   float (&dq)[MPB_MAX_DOF]) {
    constexpr int N = MPB_SDF_GROUP;
    if (G.kind == MPB_KIND_POINT) {
        SdfTaps T;
        sdf_load(S, q[0], q[1], (G.n_dof > 2) ? q[2] : 0.f, T);
        float gx = 0.f, gy = 0.f, gz = 0.f;
        const float s = GRAD ? sdf_gradient(T, S.inv, gx, gy, gz) : sdf_value(T);
        const float h = fmaxf(G.margin + G.links[4] - s, 0.f);
        if (GRAD) {
            const bool on = h > 0.f;
            dq[0] = on ? -gx : 0.f;
            dq[1] = on ? -gy : 0.f;
            if (G.n_dof > 2) dq[2] = on ? -gz : 0.f;
        }
        return h;
    }
    FKState<GRAD> F;
    fk_identity(F);
    F.frame = 0;
    if (GRAD) {
#pragma unroll
        for (int i = 0; i < MPB_MAX_DOF; ++i) { F.zx[i] = F.zy[i] = F.zz[i] = F.px[i] = F.py[i] = F.pz[i] = 0.f; }
    }
    float cost = 0.f;
    for (int l0 = 0; l0 < L; l0 += N) {
        float x[N], y[N], z[N], thr[N];
        int fr[N];
        SdfTaps T[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if (l0 + i < L) {                                                          // (wave-uniform)
                const float4 lk = *reinterpret_cast<const float4*>(G.links + 8 * (l0 + i));   // frame, ox, oy, oz
                const int f = min(__float_as_int(lk.x), G.n_tf);                         // (a checked buffer never clamps: keeps the walk inside tf)
                while (F.frame < f) fk_advance<GRAD>(G, F, q);
                link_centre(F, lk, x[i], y[i], z[i]);
                thr[i] = G.margin + G.links[8 * (l0 + i) + 4];
                fr[i] = f;
            } else {                                                                   // parked slot: hinge 0 whatever the grid holds
                x[i] = y[i] = z[i] = 0.f;
                thr[i] = -3.0e38f;
                fr[i] = 0;
            }
            sdf_load(S, x[i], y[i], z[i], T[i]);
        }
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if constexpr (GRAD) {
                float gx, gy, gz;
                const float s = sdf_gradient(T[i], S.inv, gx, gy, gz);
                const float h = fmaxf(thr[i] - s, 0.f);
                cost += h;
                if (__ballot(h > 0.f) != 0ull) {
                    const bool on = h > 0.f;
                    const float fx = on ? -gx : 0.f, fy = on ? -gy : 0.f, fz = on ? -gz : 0.f;
#pragma unroll
                    for (int ii = 0; ii < MPB_MAX_DOF; ++ii)
                        if (ii < fr[i] && ii < G.n_dof)
                            dq[ii] += joint_term(F.zx[ii], F.zy[ii], F.zz[ii], F.px[ii], F.py[ii], F.pz[ii], x[i], y[i], z[i], fx, fy, fz);
                }
            } else {
                cost += fmaxf(thr[i] - sdf_value(T[i]), 0.f);
            }
        }
    }
    return cost;
}

// the launcher read kind / n_dof / n_links / dims from the header; the kernels use ITS numbers for every row and node index and refuse
// (NaN outputs) a buffer whose header has changed since
__device__ __forceinline__ bool sdf_header_matches(const float* __restrict__ s, int n_dof, int L, int nx, int ny, int nz) {
    const int* si = reinterpret_cast<const int*>(s);
    return si[MPB_DW_MAGIC] == MPB_SDF_MAGIC && si[MPB_DW_N_DOF] == n_dof && si[MPB_DW_N_LINKS] == L && si[MPB_DW_DIMS] == nx &&
           si[MPB_DW_DIMS + 1] == ny && si[MPB_DW_DIMS + 2] == nz;
}
