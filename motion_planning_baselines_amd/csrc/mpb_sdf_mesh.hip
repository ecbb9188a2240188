// mpb_sdf_mesh.hip -- the node values of a GridSDFField from a triangle mesh: the exact distance to the nearest triangle, signed by the
// angle-weighted pseudonormal of the nearest feature (GridSDFField.from_mesh of geometry.py; include/mpb.h has the definition word for
// word, DESIGN.md 10 the derivation of the culling slack).
//
// Mapping: one thread per node; a wave's 64 nodes are a block of 4 x 4 x 4 (planar grid: 8 x 8), so that its lanes agree on which
// triangles matter; four waves per workgroup, no barrier, no LDS.  A lane beyond the grid takes the clamped node of its block (a copy of
// a live lane: it changes no ballot) and stores nothing.
// Loads: a triangle record (MPB_MESH_TRI_WORDS = 32 words) and a group box (8 words) sit at wave-uniform addresses -- the loops run over
// group and record indices, never over anything a lane holds --, so they go through the constant cache as uniform loads; the one
// per-lane load is the winner's pseudonormal after the walk.
// Arithmetic: contraction off in the whole file, every fused operation is an fmaf written out; no atomics, no cross-lane arithmetic
// on values (the one cross-lane operation is the ballot that skips a group); the closest feature is picked with selects, no register
// array is indexed by a run-time value: the same bits on every run, and with and without culling (the bound only culls).
#include <string.h>

#include "mpb_common.h"
#include "mpb_host.h"
#include "mpb_sdf_host.h"

#pragma clang fp contract(off)

struct MeshPose { float r[12]; int on; };           // [R | t] row-major 3 x 4, mesh frame to grid frame; on == 0: none

__device__ __forceinline__ float mesh_dot(float ax, float ay, float az, float bx, float by, float bz) { return fmaf(az, bz, fmaf(ay, by, ax * bx)); }

// squared distance from p to one triangle record, the offset r = p - (closest point) and the feature code of the closest point
__device__ __forceinline__ float mesh_tri_dist2(const float* __restrict__ T, float px, float py, float pz, float& rx, float& ry, float& rz, int& feat) {
    const float ax = T[MPB_TRI_A], ay = T[MPB_TRI_A + 1], az = T[MPB_TRI_A + 2];
    const float bx = T[MPB_TRI_B], by = T[MPB_TRI_B + 1], bz = T[MPB_TRI_B + 2];
    const float cx = T[MPB_TRI_C], cy = T[MPB_TRI_C + 1], cz = T[MPB_TRI_C + 2];
    const float abx = bx - ax, aby = by - ay, abz = bz - az;
    const float acx = cx - ax, acy = cy - ay, acz = cz - az;
    const float bcx = cx - bx, bcy = cy - by, bcz = cz - bz;
    const float apx = px - ax, apy = py - ay, apz = pz - az;
    const float bpx = px - bx, bpy = py - by, bpz = pz - bz;
    const float cpx = px - cx, cpy = py - cy, cpz = pz - cz;
    const float d1 = mesh_dot(abx, aby, abz, apx, apy, apz), d2 = mesh_dot(acx, acy, acz, apx, apy, apz);
    const float d3 = mesh_dot(abx, aby, abz, bpx, bpy, bpz), d4 = mesh_dot(acx, acy, acz, bpx, bpy, bpz);
    const float d5 = mesh_dot(abx, aby, abz, cpx, cpy, cpz), d6 = mesh_dot(acx, acy, acz, cpx, cpy, cpz);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float e43 = d4 - d3, e56 = d5 - d6;
    const bool in_a = d1 <= 0.f && d2 <= 0.f, in_b = d3 >= 0.f && d4 <= d3, in_c = d6 >= 0.f && d5 <= d6;
    const bool in_ab = vc <= 0.f && d1 >= 0.f && d3 <= 0.f, in_ca = vb <= 0.f && d2 >= 0.f && d6 <= 0.f;
    const bool in_bc = va <= 0.f && e43 >= 0.f && e56 >= 0.f;
    // from the last of the walk to the first: what comes earlier overrides
    int f = MPB_FEAT_FACE;
    float nu = vb, nw = vc, den = (va + vb) + vc;
    if (in_bc) { f = MPB_FEAT_BC; nu = e43; nw = 0.f; den = e43 + e56; }
    if (in_ca) { f = MPB_FEAT_CA; nu = d2; nw = 0.f; den = d2 - d6; }
    if (in_ab) { f = MPB_FEAT_AB; nu = d1; nw = 0.f; den = d1 - d3; }
    if (in_c) { f = MPB_FEAT_C; nu = 0.f; nw = 0.f; den = 1.f; }
    if (in_b) { f = MPB_FEAT_B; nu = 0.f; nw = 0.f; den = 1.f; }
    if (in_a) { f = MPB_FEAT_A; nu = 0.f; nw = 0.f; den = 1.f; }
    const bool base_b = f == MPB_FEAT_B || f == MPB_FEAT_BC, base_c = f == MPB_FEAT_C;
    const bool dir_ac = f == MPB_FEAT_CA, dir_bc = f == MPB_FEAT_BC;
    const float qx = base_b ? bpx : (base_c ? cpx : apx), qy = base_b ? bpy : (base_c ? cpy : apy), qz = base_b ? bpz : (base_c ? cpz : apz);
    const float e1x = dir_bc ? bcx : (dir_ac ? acx : abx), e1y = dir_bc ? bcy : (dir_ac ? acy : aby), e1z = dir_bc ? bcz : (dir_ac ? acz : abz);
    const float inv = __fdiv_rn(1.0f, den);
    const float u = fminf(fmaxf(nu * inv, 0.f), 1.f);
    const float w = fminf(fmaxf(nw * inv, 0.f), 1.f - u);
    rx = fmaf(-w, acx, fmaf(-u, e1x, qx));
    ry = fmaf(-w, acy, fmaf(-u, e1y, qy));
    rz = fmaf(-w, acz, fmaf(-u, e1z, qz));
    feat = f;
    return mesh_dot(rx, ry, rz, rx, ry, rz);
}

// squared distance from p to the nearest (FAR: the farthest) point of a box
template <bool FAR>
__device__ __forceinline__ float mesh_box_dist2(const float* __restrict__ Bx, float px, float py, float pz) {
    const float lx = Bx[0], ly = Bx[1], lz = Bx[2], hx = Bx[4], hy = Bx[5], hz = Bx[6];
    float ex, ey, ez;
    if (FAR) {
        ex = fmaxf(fabsf(px - lx), fabsf(hx - px)), ey = fmaxf(fabsf(py - ly), fabsf(hy - py)), ez = fmaxf(fabsf(pz - lz), fabsf(hz - pz));
    } else {
        ex = fmaxf(fmaxf(lx - px, px - hx), 0.f), ey = fmaxf(fmaxf(ly - py, py - hy), 0.f), ez = fmaxf(fmaxf(lz - pz, pz - hz), 0.f);
    }
    return mesh_dot(ex, ey, ez, ex, ey, ez);
}

// the launcher read the dims from the SDF header and n_tri / n_groups / the offsets from the mesh header; the kernel forms every
// address from ITS numbers and writes nothing when either header has changed since
__global__ __launch_bounds__(256) void mesh_dist_kernel(const float* __restrict__ mesh, float* __restrict__ sdfb, MeshPose pose, int nx, int ny,
                                                        int nz, int n_tri, int n_groups, int off_tris, int off_boxes, int flags, float slack) {
    const int* si = reinterpret_cast<const int*>(sdfb);
    const int* mi = reinterpret_cast<const int*>(mesh);
    const bool ok = si[MPB_DW_MAGIC] == MPB_SDF_MAGIC && si[MPB_DW_DIMS] == nx && si[MPB_DW_DIMS + 1] == ny && si[MPB_DW_DIMS + 2] == nz &&
                    mi[MPB_MW_MAGIC] == MPB_MESH_MAGIC && mi[MPB_MW_N_TRI] == n_tri && mi[MPB_MW_N_GROUPS] == n_groups &&
                    mi[MPB_MW_OFF_TRIS] == off_tris && mi[MPB_MW_OFF_BOXES] == off_boxes;
    if (!ok) return;                                            // (grid-uniform)
    const bool planar = nz == 1;
    const int ex = planar ? 8 : 4, ey = planar ? 8 : 4;          // nodes of a wave's block along x, y (z: 64 / (ex * ey))
    const int ez = planar ? 1 : 4;
    const unsigned bx = (unsigned)(nx + ex - 1) / (unsigned)ex, by = (unsigned)(ny + ey - 1) / (unsigned)ey, bz = (unsigned)(nz + ez - 1) / (unsigned)ez;
    const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (wave >= bx * by * bz) return;                           // (wave-uniform; bx * by * bz <= 256^3)
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wx = wave % bx, wyz = wave / bx, wy = wyz % by, wz = wyz / by;
    const int li = planar ? (int)(lane & 7u) : (int)(lane & 3u), lj = planar ? (int)(lane >> 3) : (int)((lane >> 2) & 3u), lk = planar ? 0 : (int)(lane >> 4);
    const int i = (int)wx * ex + li, j = (int)wy * ey + lj, k = (int)wz * ez + lk;
    const bool live = i < nx && j < ny && k < nz;
    const int ic = min(i, nx - 1), jc = min(j, ny - 1), kc = min(k, nz - 1);
    const float cell = sdfb[MPB_DW_CELL];
    float px = fmaf((float)ic, cell, sdfb[MPB_DW_LO]), py = fmaf((float)jc, cell, sdfb[MPB_DW_LO + 1]), pz = fmaf((float)kc, cell, sdfb[MPB_DW_LO + 2]);
    if (pose.on) {                                              // p' = R^T (p - t)
        const float dx = px - pose.r[3], dy = py - pose.r[7], dz = pz - pose.r[11];
        px = fmaf(pose.r[8], dz, fmaf(pose.r[4], dy, pose.r[0] * dx));
        py = fmaf(pose.r[9], dz, fmaf(pose.r[5], dy, pose.r[1] * dx));
        pz = fmaf(pose.r[10], dz, fmaf(pose.r[6], dy, pose.r[2] * dx));
    }
    const float* tris = mesh + off_tris;
    const float* boxes = mesh + off_boxes;
    const bool cull = (flags & MPB_MESH_NO_CULL) == 0;
    // pass 1: an upper bound of this node's smallest dist2 -- every box contains a triangle
    float bound = 3.0e38f;
    if (cull)
        for (int g = 0; g < n_groups; ++g) bound = fminf(bound, mesh_box_dist2<true>(boxes + (size_t)g * MPB_MESH_BOX_WORDS, px, py, pz));
    // pass 2
    float best = 3.0e38f, brx = 0.f, bry = 0.f, brz = 0.f;
    int best_t = 0, best_f = MPB_FEAT_FACE;
    for (int g = 0; g < n_groups; ++g) {
        if (cull) {
            const float near2 = mesh_box_dist2<false>(boxes + (size_t)g * MPB_MESH_BOX_WORDS, px, py, pz);
            if (__ballot(near2 <= fminf(best, bound) + slack) == 0ull) continue;     // (wave-uniform)
        }
        const int t0 = g * MPB_MESH_GROUP;
        for (int t = t0; t < t0 + MPB_MESH_GROUP; ++t) {
            float rx, ry, rz;
            int f;
            const float dist2 = mesh_tri_dist2(tris + (size_t)t * MPB_MESH_TRI_WORDS, px, py, pz, rx, ry, rz, f);
            const bool better = dist2 < best;
            best = better ? dist2 : best;
            brx = better ? rx : brx, bry = better ? ry : bry, brz = better ? rz : brz;
            best_t = better ? t : best_t;
            best_f = better ? f : best_f;
        }
    }
    if (!live) return;
    float v = __fsqrt_rn(best);
    if (mi[MPB_MW_SIGNED] != 0) {
        const float* n = tris + (size_t)best_t * MPB_MESH_TRI_WORDS + MPB_TRI_N_FACE + 3 * best_f;      // (best_t < n_groups * 64, best_f < 7: inside the record)
        const float s = mesh_dot(brx, bry, brz, n[0], n[1], n[2]);
        v = s < 0.f ? -v : v;
    } else {
        v = v - mesh[MPB_MW_THICKNESS];
    }
    float* node = sdfb + si[MPB_DW_OFF_NODES] + ((size_t)k * (unsigned)ny + (unsigned)j) * (unsigned)nx + (unsigned)i;
    *node = (flags & MPB_MESH_MIN) ? fminf(*node, v) : v;
}

// ---- host side ------------------------------------------------------------------------------------------------------
// (by the bits and never optimised: the library is compiled with -ffinite-math-only, under which a comparison -- and a bit test the
// compiler recognises as one -- is assumed to see no NaN or infinity)
__attribute__((optnone, noinline)) static bool mesh_finite(float v) {
    uint32_t b;
    memcpy(&b, &v, 4);
    return (b & 0x7F800000u) != 0x7F800000u;
}

// header, offsets and limits (n_words < 0: the total is not compared with a word count); max_abs: the largest absolute coordinate of the box
static int mesh_header_check(const int32_t* mi, long long n_words, float& max_abs, const char* who) {
    if (mi[MPB_MW_MAGIC] != MPB_MESH_MAGIC || mi[MPB_MW_VERSION] != MPB_MESH_VERSION) return mpb_failf(MPB_E_INVALID, "%s: bad magic/version of the mesh buffer", who);
    const int n_tri = mi[MPB_MW_N_TRI], n_groups = mi[MPB_MW_N_GROUPS];
    if (n_tri < 1 || n_tri > MPB_MESH_MAX_TRIS) return mpb_failf(MPB_E_UNSUPPORTED, "%s: %d triangles outside 1..MPB_MESH_MAX_TRIS = %d", who, n_tri, MPB_MESH_MAX_TRIS);
    if (n_groups != (n_tri + MPB_MESH_GROUP - 1) / MPB_MESH_GROUP) return mpb_failf(MPB_E_INVALID, "%s: n_groups must be ceil(n_tri / %d)", who, MPB_MESH_GROUP);
    if (mi[MPB_MW_SIGNED] != 0 && mi[MPB_MW_SIGNED] != 1) return mpb_failf(MPB_E_INVALID, "%s: signed must be 0 or 1", who);
    const int off_tris = mi[MPB_MW_OFF_TRIS], off_boxes = mi[MPB_MW_OFF_BOXES], total = mi[MPB_MW_TOTAL];
    if (off_tris != MPB_MESH_HEADER_WORDS || off_boxes != off_tris + n_groups * MPB_MESH_GROUP * MPB_MESH_TRI_WORDS ||
        total != off_boxes + n_groups * MPB_MESH_BOX_WORDS || (n_words >= 0 && total != n_words))
        return mpb_failf(MPB_E_INVALID, "%s: inconsistent section offsets / total of the mesh buffer", who);
    const float* mf = reinterpret_cast<const float*>(mi);
    if (!(mf[MPB_MW_THICKNESS] >= 0.f) || !mesh_finite(mf[MPB_MW_THICKNESS])) return mpb_failf(MPB_E_INVALID, "%s: thickness must be finite and >= 0", who);
    max_abs = 0.f;
    for (int a = 0; a < 3; ++a) {
        const float lo = mf[MPB_MW_BB_LO + a], hi = mf[MPB_MW_BB_HI + a];
        if (!mesh_finite(lo) || !mesh_finite(hi) || !(lo <= hi)) return mpb_failf(MPB_E_INVALID, "%s: the mesh's box must be finite with lo <= hi", who);
        max_abs = fmaxf(max_abs, fmaxf(fabsf(lo), fabsf(hi)));
    }
    return MPB_OK;
}

extern "C" int mpb_mesh_check(const float* m, int n_words) {
    if (!m || n_words < MPB_MESH_HEADER_WORDS) return mpb_failf(MPB_E_INVALID, "%s: mesh buffer too small", __func__);
    const int32_t* mi = reinterpret_cast<const int32_t*>(m);
    float max_abs;
    const int rc = mesh_header_check(mi, n_words, max_abs, __func__);
    if (rc) return rc;
    for (int w = MPB_MESH_HEADER_WORDS; w < n_words; ++w)
        if (!mesh_finite(m[w])) return mpb_failf(MPB_E_INVALID, "%s: word %d of the mesh buffer is not finite", __func__, w);
    const float* tris = m + mi[MPB_MW_OFF_TRIS];
    const float* boxes = m + mi[MPB_MW_OFF_BOXES];
    for (int g = 0; g < mi[MPB_MW_N_GROUPS]; ++g) {
        const float* B = boxes + (size_t)g * MPB_MESH_BOX_WORDS;
        for (int a = 0; a < 3; ++a)
            if (!(m[MPB_MW_BB_LO + a] <= B[a] && B[a] <= B[4 + a] && B[4 + a] <= m[MPB_MW_BB_HI + a]))
                return mpb_failf(MPB_E_INVALID, "%s: the box of group %d is empty or outside the mesh's box", __func__, g);
        for (int t = g * MPB_MESH_GROUP; t < (g + 1) * MPB_MESH_GROUP; ++t)
            for (int c = 0; c < 9; ++c) {
                const float x = tris[(size_t)t * MPB_MESH_TRI_WORDS + c];
                if (!(B[c % 3] <= x && x <= B[4 + c % 3])) return mpb_failf(MPB_E_INVALID, "%s: triangle record %d lies outside the box of its group %d", __func__, t, g);
            }
    }
    return MPB_OK;
}

static int mesh_shape(const float* mesh, MeshShape& out, const char* who) {
    return g_mesh_cache.get(mesh, out, who, "mesh", [who](const int32_t* hdr, MeshShape& M) {
        M.n_tri = hdr[MPB_MW_N_TRI], M.n_groups = hdr[MPB_MW_N_GROUPS], M.is_signed = hdr[MPB_MW_SIGNED];
        M.off_tris = hdr[MPB_MW_OFF_TRIS], M.off_boxes = hdr[MPB_MW_OFF_BOXES];
        M.thickness = reinterpret_cast<const float*>(hdr)[MPB_MW_THICKNESS];
        return mesh_header_check(hdr, -1, M.max_abs, who);
    });
}

extern "C" int mpb_sdf_grid_build_mesh(const float* mesh, const float* pose_host, float* sdfb, int flags, void* stream) {
    if (!mesh || !sdfb) return mpb_failf(MPB_E_INVALID, "%s: null pointer", __func__);
    if (mpb_misaligned16(mesh, sdfb)) return mpb_failf(MPB_E_INVALID, "%s: the mesh and the SDF-grid buffer must be 16-byte aligned", __func__);
    SdfShape S;
    int rc = sdf_shape(sdfb, S, __func__);
    if (rc) return rc;
    MeshShape M;
    if ((rc = mesh_shape(mesh, M, __func__))) return rc;
    if (flags & ~(MPB_MESH_MIN | MPB_MESH_NO_CULL)) return mpb_failf(MPB_E_INVALID, "%s: unknown flag bits 0x%X", __func__, flags & ~(MPB_MESH_MIN | MPB_MESH_NO_CULL));
    MeshPose P = {};
    if (pose_host) {
        for (int w = 0; w < 12; ++w) {
            if (!mesh_finite(pose_host[w])) return mpb_failf(MPB_E_INVALID, "%s: the pose is not finite", __func__);
            P.r[w] = pose_host[w];
        }
        P.on = 1;
    }
    // M of the slack: the largest absolute coordinate among the nodes in the mesh frame (a node is a convex combination of the grid's
    // eight corners, so are its coordinates there) and the mesh's box; in fp64, then 2^-14 M^2 rounded up
    double big = M.max_abs;
    for (int c = 0; c < 8; ++c) {
        const double p[3] = {(double)S.lo[0] + ((c & 1) ? (double)(S.nx - 1) * S.cell : 0.0), (double)S.lo[1] + ((c & 2) ? (double)(S.ny - 1) * S.cell : 0.0),
                             (double)S.lo[2] + ((c & 4) ? (double)(S.nz - 1) * S.cell : 0.0)};
        for (int m = 0; m < 3; ++m) {
            const double q = P.on ? P.r[m] * (p[0] - P.r[3]) + P.r[4 + m] * (p[1] - P.r[7]) + P.r[8 + m] * (p[2] - P.r[11]) : p[m];
            big = fmax(big, fabs(q));
        }
    }
    const float slack = (float)(big * big * (1.0 + 1e-6) / 16384.0);
    const bool planar = S.nz == 1;
    const unsigned ex = planar ? 8u : 4u, ez = planar ? 1u : 4u;
    const unsigned waves = (((unsigned)S.nx + ex - 1) / ex) * (((unsigned)S.ny + ex - 1) / ex) * (((unsigned)S.nz + ez - 1) / ez);
    hipLaunchKernelGGL(mesh_dist_kernel, dim3((waves + 3u) / 4u), dim3(256), 0, (hipStream_t)stream, mesh, sdfb, P, S.nx, S.ny, S.nz, M.n_tri, M.n_groups,
                       M.off_tris, M.off_boxes, flags, slack);
    return mpb_check_launch(__func__);
}
