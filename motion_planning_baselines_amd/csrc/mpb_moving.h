// mpb_moving.h -- the device-side pieces the kernels that see moving obstacles share (mpb_moving_obstacles.hip, mpb_strrt.hip): the robot
// of a packed moving-obstacle buffer as a GeomView, the obstacle tables, the walk of a group of the robot's spheres past the obstacles of
// one row, the hinge sum c_row(q) of one configuration at one row, and the header comparison by which a kernel refuses a buffer that
// changed under its launcher.  The buffer in numbers is include/mpb_moving_layout.h (generated from moving_layout.py); the definition of
// the cost is at the head of mpb_moving_obstacles.hip.  Also the host-side shape record of a buffer, read through that file's header cache.
#pragma once
#include "mpb_common.h"
#include "mpb_geom.h"
#include "mpb_member_cost.h"
#include "../../include/mpb_moving_layout.h"

// the robot of a moving-obstacle buffer as the GeomView fk_advance reads (tf, n_dof) and the walk below reads (links); no static obstacles
__device__ __forceinline__ GeomView moving_robot_view(const float* __restrict__ s) {
    const int* si = reinterpret_cast<const int*>(s);
    GeomView v = {};
    v.kind = si[MPB_VW_N_TF] == 0 ? MPB_KIND_POINT : MPB_KIND_CHAIN;
    v.n_dof = si[MPB_VW_N_DOF];
    v.n_tf = si[MPB_VW_N_TF];
    v.n_links = si[MPB_VW_N_LINKS];
    v.margin = s[MPB_VW_MARGIN];
    v.tf = s + si[MPB_VW_OFF_TF];
    v.links = s + si[MPB_VW_OFF_LINKS];
    return v;
}

// the obstacle tables: counts and the row stride as the LAUNCHER read them (every centre index is formed from these), the sections from
// the header
struct MovingTables {
    int n_sph, n_box, stride;      // stride: the padded rows, words between the components of a centre
    const float* radii;            // n_sph
    const float* half;             // n_box x 4
    const float* centres;          // [o][xyz][row]
};

__device__ __forceinline__ MovingTables moving_tables(const float* __restrict__ s, int H, int n_sph, int n_box) {
    const int* si = reinterpret_cast<const int*>(s);
    MovingTables T;
    T.n_sph = n_sph; T.n_box = n_box;
    T.stride = (H + MPB_MOVING_ROW_PAD - 1) / MPB_MOVING_ROW_PAD * MPB_MOVING_ROW_PAD;
    T.radii = s + si[MPB_VW_OFF_RADII];
    T.half = s + si[MPB_VW_OFF_HALF];
    T.centres = s + si[MPB_VW_OFF_CENTRES];
    return T;
}

// min signed distance of the first NS slots of C to every obstacle as it stands at row `row` (row < T.stride)
template <bool GRAD, int NS>
__device__ __forceinline__ void moving_chunk_vs_obstacles(const MovingTables& T, int row, LinkChunk<GRAD>& C) {
    const float* cp = T.centres + row;
#pragma unroll 2
    for (int o = 0; o < T.n_sph; ++o) {
        const float cx = cp[0], cy = cp[T.stride], cz = cp[2 * T.stride];
        const float r = T.radii[o];
        static_for<0, NS>([&](auto ic) { exact_sphere<GRAD, decltype(ic)::value>(C, cx, cy, cz, r); });
        cp += 3 * T.stride;
    }
    const float4* hp = reinterpret_cast<const float4*>(T.half);
    for (int o = 0; o < T.n_box; ++o) {
        const float4 c = make_float4(cp[0], cp[T.stride], cp[2 * T.stride], 0.f);
        const float4 h = hp[o];
        static_for<0, NS>([&](auto ic) { exact_box<GRAD, decltype(ic)::value>(C, c, h); });
        cp += 3 * T.stride;
    }
}

// c_row(q); GRAD: dq[i] += d c / d q_i (i < n_dof; the caller zeroes dq).  q / dq are register arrays indexed only with compile-time
// indices.  L: the robot's spheres as the launcher read them.
template <bool GRAD>
__device__ __forceinline__ float moving_row_cost(const GeomView& G, const MovingTables& T, int L, int row, const float (&q)[MPB_MAX_DOF],
                                                 float (&dq)[MPB_MAX_DOF]) {
    constexpr int N = LinkChunk<GRAD>::N;
    constexpr float FAR = 1.0e9f;                      // parked slot: farther than any obstacle, hinge 0
    LinkChunk<GRAD> C;
    if (G.kind == MPB_KIND_POINT) {
        C.x[0] = q[0]; C.y[0] = q[1]; C.z[0] = (G.n_dof > 2) ? q[2] : 0.f;
        C.best[0] = 3.0e38f;
        if (GRAD) { C.vx[0] = C.vy[0] = C.vz[0] = 0.f; C.vn[0] = 1.f; }
        moving_chunk_vs_obstacles<GRAD, 1>(T, row, C);
        const float h = fmaxf(G.margin + G.links[4] - C.best[0], 0.f);
        if (GRAD) {
            const float s = (h > 0.f) ? -1.0f / C.vn[0] : 0.f;
            dq[0] = C.vx[0] * s;
            dq[1] = C.vy[0] * s;
            if (G.n_dof > 2) dq[2] = C.vz[0] * s;
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
        float thr[N];
        int fr[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            C.best[i] = 3.0e38f;
            if (GRAD) { C.vx[i] = C.vy[i] = C.vz[i] = 0.f; C.vn[i] = 1.f; }
            if (l0 + i < L) {                                                          // (wave-uniform)
                const float4 lk = *reinterpret_cast<const float4*>(G.links + 8 * (l0 + i));   // frame, ox, oy, oz
                const int f = min(__float_as_int(lk.x), G.n_tf);                         // (a checked buffer never clamps: keeps the walk inside tf)
                while (F.frame < f) fk_advance<GRAD>(G, F, q);
                link_centre(F, lk, C.x[i], C.y[i], C.z[i]);
                thr[i] = G.margin + G.links[8 * (l0 + i) + 4];
                fr[i] = f;
            } else {
                C.x[i] = C.y[i] = C.z[i] = FAR;
                thr[i] = 0.f;
                fr[i] = 0;
            }
        }
        moving_chunk_vs_obstacles<GRAD, N>(T, row, C);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const float h = fmaxf(thr[i] - C.best[i], 0.f);                              // parked slots: best ~ 1e9 -> 0
            cost += h;
            if constexpr (GRAD) {
                if (__ballot(h > 0.f) != 0ull) {
                    const float s = (h > 0.f) ? -1.0f / C.vn[i] : 0.f;
                    const float fx = C.vx[i] * s, fy = C.vy[i] * s, fz = C.vz[i] * s;
#pragma unroll
                    for (int ii = 0; ii < MPB_MAX_DOF; ++ii)
                        if (ii < fr[i] && ii < G.n_dof)
                            dq[ii] += joint_term(F.zx[ii], F.zy[ii], F.zz[ii], F.px[ii], F.py[ii], F.pz[ii], C.x[i], C.y[i], C.z[i], fx, fy, fz);
                }
            }
        }
    }
    return cost;
}

// the launcher read n_dof / n_links / n_rows / n_spheres / n_boxes from the header; the kernels use ITS numbers for every row and centre
// index and refuse (NaN outputs) a buffer whose header has changed since
__device__ __forceinline__ bool moving_header_matches(const float* __restrict__ s, int n_dof, int L, int H, int n_sph, int n_box) {
    const int* si = reinterpret_cast<const int*>(s);
    return si[MPB_VW_MAGIC] == MPB_MOVING_MAGIC && si[MPB_VW_N_DOF] == n_dof && si[MPB_VW_N_LINKS] == L && si[MPB_VW_N_ROWS] == H &&
           si[MPB_VW_N_SPHERES] == n_sph && si[MPB_VW_N_BOXES] == n_box;
}

// ---- host side: what a launch needs of a device buffer's header, served by the cache of mpb_moving_obstacles.hip (announce a new buffer
// at a seen address with mpb_moving_invalidate); the file-local moving_shape() of that file under a name other files can link against
struct MovingShape { const void* ptr; int dev, n_dof, n_links, n_rows, n_sph, n_box; };
int mpb_moving_shape_cached(const float* mob, MovingShape& out, const char* who);
