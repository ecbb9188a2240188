// mpb_sdf_grid.hip -- a precomputed grid of signed distances as a collision field: build, sample, cost, gradient and predicate of a
// GridSDFField (geometry.py; build-defined; the reference's precompute_sdf_obj_fixed=True).  The grid is a lattice of
// (nx, ny, nz) fp32 nodes, node (i, j, k) at lo + (i, j, k) * cell, word (k * ny + j) * nx + i of the node section of the packed SDF
// buffer (include/mpb_sdf_layout.h); nz == 1 is a planar grid (z ignored).
//
// Sampling s(x), per axis:  u = (x - lo) * inv_cell, clamped to [0, n - 1];  i0 = min(floor(u), n - 2);  f = u - i0;  lerp form
// fmaf(f, v1 - v0, v0) along x, then y, then z.  The gradient is the exact derivative of that interpolant (piecewise constant along its own
// axis), 0 along an axis the point lies outside the box on, from the same eight (planar: four) node loads as the value.
// Per waypoint  c(q) = sum_l relu(margin + r_l - s(x_l(q)))  over the robot's collision spheres (FKState / fk_advance of mpb_geom.h through
// a GeomView filled from the SDF buffer; a point robot has its one sphere at q).
//
// Mapping: one wave per trajectory (a workgroup IS one wave: no barrier, no LDS), one lane per waypoint, trips of 64 for H > 64; the
// predicate and the sampler give one lane per configuration / point; the builder one thread per node (the builder from occupancy voxels
// is a distance transform with LDS tiles of its own, described where it stands; the builder from triangle meshes is mpb_sdf_mesh.hip).  The node gathers are what
// the kernels wait for (a lane's eight nodes are four pairs of adjacent words anywhere in a grid of tens of MB), so the spheres go in groups of
// MPB_SDF_GROUP: the chain walk places the group, every load of the group is issued, then the hinges are taken.  With gradients the force
// -grad s of an active sphere is pulled through J^T at once from the joint axes / origins the same walk has kept (FKState<true>,
// joint_term), skipped wave-wide when a ballot finds the sphere active in no lane.
// Order of the sums: spheres in table order in fp32 per waypoint, a lane's waypoints in ascending order, then the fixed-order wave
// reduction of mpb_common.h: every run gives the same bits.  Every node index is clamped into the grid whatever the input (NaN included).
#include <algorithm>

#include "mpb_common.h"
#include "mpb_host.h"
#include "mpb_sdf_host.h"
#include "mpb_geom.h"
#include "mpb_member_cost.h"
#include "mpb_sdf.h"
#include "../../include/mpb_sdf_layout.h"

template <bool GRAD>
__global__ __launch_bounds__(64) void sdf_cost_kernel(const float* __restrict__ trajs, const float* __restrict__ sdfb, float* __restrict__ out,
                                                      float* __restrict__ per_wp, float* __restrict__ grad, int H, int d, int h_begin,
                                                      float k_sigma, float weight, int accumulate, int D, int L, int nx, int ny, int nz) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const GeomView G = sdf_robot_view(sdfb);
    const SdfLattice S = sdf_lattice(sdfb, nx, ny, nz);
    const bool ok = sdf_header_matches(sdfb, D, L, nx, ny, nz);        // (D: the launcher's n_dof, which it held d against)
    const float sc = weight * k_sigma;
    float csum = 0.f;
    for (int h0 = 0; h0 < H; h0 += 64) {
        const int h = h0 + lane;
        const bool live = ok && h < H && h >= h_begin;
        float q[MPB_MAX_DOF], dq[MPB_MAX_DOF];
#pragma unroll
        for (int i = 0; i < MPB_MAX_DOF; ++i) { q[i] = 0.f; dq[i] = 0.f; }
        float c = 0.f;
        if (__ballot(live) != 0ull) {
            // (a lane that is not live walks along at q = 0 -- its loads stay inside the grid -- and its result is dropped: the ballots of
            // the walk then see whole waves)
            if (live) {
                const float* row = trajs + ((size_t)b * H + h) * d;
#pragma unroll
                for (int i = 0; i < MPB_MAX_DOF; ++i) q[i] = (i < D) ? row[i] : 0.f;
            }
            c = sdf_waypoint_cost<GRAD>(G, S, L, q, dq);
            if (!live) c = 0.f;
        }
        if (!ok) c = __uint_as_float(0x7FC00000u);
        if (h < H) {
            if (per_wp) per_wp[(size_t)b * H + h] = c;
            if (GRAD) {
                float* grow = grad + ((size_t)b * H + h) * d;
#pragma unroll
                for (int i = 0; i < MPB_MAX_DOF; ++i) {
                    if (i < D) {
                        const float g = ok ? (live ? sc * dq[i] : 0.f) : c;
                        grow[i] = accumulate ? add_rounded(grow[i], g) : g;
                    }
                }
                if (!accumulate)
                    for (int i = D; i < d; ++i) grow[i] = 0.f;   // the velocity channels
            }
        }
        csum += c;
    }
    member_store_out(out, b, lane, csum, k_sigma, weight, accumulate);
}

__global__ __launch_bounds__(64) void sdf_check_kernel(const float* __restrict__ q_in, const float* __restrict__ sdfb,
                                                       unsigned char* __restrict__ in_collision, float* __restrict__ gap, int N, int D,
                                                       int or_into, int L, int nx, int ny, int nz) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    const bool have = i < (size_t)N;
    const GeomView G = sdf_robot_view(sdfb);
    const SdfLattice S = sdf_lattice(sdfb, nx, ny, nz);
    float q[MPB_MAX_DOF], dq[MPB_MAX_DOF];
#pragma unroll
    for (int k = 0; k < MPB_MAX_DOF; ++k) q[k] = (have && k < D) ? q_in[i * D + k] : 0.f;
    float c = __uint_as_float(0x7FC00000u);
    if (sdf_header_matches(sdfb, D, L, nx, ny, nz)) c = sdf_waypoint_cost<false>(G, S, L, q, dq);
    if (have) member_store_hit(in_collision, gap, i, c, or_into);
}

// the interpolant alone: one lane per point
__global__ __launch_bounds__(256) void sdf_sample_kernel(const float* __restrict__ pts, const float* __restrict__ sdfb, float* __restrict__ s_out,
                                                         float* __restrict__ g_out, int N, int nx, int ny, int nz) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)N) return;
    const int* si = reinterpret_cast<const int*>(sdfb);
    const bool ok = si[MPB_DW_MAGIC] == MPB_SDF_MAGIC && si[MPB_DW_DIMS] == nx && si[MPB_DW_DIMS + 1] == ny && si[MPB_DW_DIMS + 2] == nz;
    const SdfLattice S = sdf_lattice(sdfb, nx, ny, nz);
    const float nan = __uint_as_float(0x7FC00000u);
    float s = nan, gx = nan, gy = nan, gz = nan;
    if (ok) {
        SdfTaps T;
        sdf_load(S, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], T);
        s = sdf_gradient(T, S.inv, gx, gy, gz);
    }
    s_out[i] = s;
    if (g_out) { g_out[3 * i] = gx; g_out[3 * i + 1] = gy; g_out[3 * i + 2] = gz; }
}

// the builder: one thread per node, min over the spheres and boxes of ONE packed CollisionField (sphere_sd / box_sd of mpb_geom.h: the
// distances every cost kernel takes), the obstacle index wave-uniform
__global__ __launch_bounds__(256) void sdf_build_kernel(const float* __restrict__ geom, float* __restrict__ sdfb, int nx, int ny, int nz,
                                                        int n_sph, int n_box) {
    const unsigned n = blockIdx.x * 256u + threadIdx.x;
    const unsigned n_nodes = (unsigned)nx * (unsigned)ny * (unsigned)nz;
    if (n >= n_nodes) return;
    const int* si = reinterpret_cast<const int*>(sdfb);
    const int* gi = reinterpret_cast<const int*>(geom);
    float* nodes = sdfb + si[MPB_DW_OFF_NODES];
    const bool ok = si[MPB_DW_MAGIC] == MPB_SDF_MAGIC && si[MPB_DW_DIMS] == nx && si[MPB_DW_DIMS + 1] == ny && si[MPB_DW_DIMS + 2] == nz &&
                    gi[MPB_GW_MAGIC] == MPB_GEOM_MAGIC && gi[MPB_GW_N_SPH] == n_sph && gi[MPB_GW_N_BOX] == n_box;
    if (!ok) return;                                           // (nothing is written through offsets the launcher has not read)
    const unsigned i = n % (unsigned)nx, jk = n / (unsigned)nx, j = jk % (unsigned)ny, k = jk / (unsigned)ny;
    const float cell = sdfb[MPB_DW_CELL];
    const float x = fmaf((float)i, cell, sdfb[MPB_DW_LO]), y = fmaf((float)j, cell, sdfb[MPB_DW_LO + 1]), z = fmaf((float)k, cell, sdfb[MPB_DW_LO + 2]);
    const float4* sp = reinterpret_cast<const float4*>(geom + gi[MPB_GW_OFF_SPH]);
    const float4* bp = reinterpret_cast<const float4*>(geom + gi[MPB_GW_OFF_BOX]);
    float best = 3.0e38f;
    for (int o = 0; o < n_sph; ++o) best = fminf(best, sphere_sd(x, y, z, sp[o]));
    for (int o = 0; o < n_box; ++o) best = fminf(best, box_sd(x, y, z, bp[2 * o], bp[2 * o + 1]));
    nodes[n] = best;
}

// ---- the grid from occupancy voxels: exact squared Euclidean distance transform, one pass per axis (include/mpb.h has the definition) --
// The partial squared index distances live IN the node section as one signed int32 per node until the last pass writes fp32 over them:
// a free node holds +(partial distance to the occupied class), an occupied node -(partial distance to the free class).  A node is at
// distance 0 from its own class in every partial transform, so a word w reads as max(w, 0) towards the occupied class and max(-w, 0)
// towards the free class; 0 is never stored and the sign is the class.  "None in this line" is MPB_EDT_NONE: two more passes add at
// most 2 * 1023^2 to it, which stays below 2^31; the last pass clamps whatever is >= MPB_EDT_NONE to D2_none.
// A pass loads a tile of WHOLE lines into LDS, then writes the tile back: in place is safe, no other workgroup touches those lines.
// The minimum  min_j f(j) + (i - j)^2  is taken by scanning outward from i in both directions until delta^2 >= the best so far (what
// remains cannot win: exact); integer minima do not depend on order, no atomics: the same bits on every run.
#define MPB_EDT_NONE (1 << 30)
#define MPB_EDT_X_TILE 1024                          // nodes of an x tile: whole lines, max(1, 1024 / nx) of them
#define MPB_EDT_T 32                                 // x positions of a y / z tile: rows of 128 bytes, a wave's lanes in consecutive banks

__device__ __forceinline__ bool edt_header_matches(const float* __restrict__ s, int nx, int ny, int nz) {
    const int* si = reinterpret_cast<const int*>(s);
    return si[MPB_DW_MAGIC] == MPB_SDF_MAGIC && si[MPB_DW_DIMS] == nx && si[MPB_DW_DIMS + 1] == ny && si[MPB_DW_DIMS + 2] == nz;
}

// along x, from the occupancy bytes (read only): the squared distance to the nearest node of the OTHER class in the node's own line
__global__ __launch_bounds__(256) void occ_edt_x_kernel(const unsigned char* __restrict__ occ, float* __restrict__ sdfb, int nx, int ny, int nz) {
    __shared__ unsigned char line[MPB_EDT_X_TILE];
    if (!edt_header_matches(sdfb, nx, ny, nz)) return;           // (block-uniform: nothing is written through offsets the launcher has not read)
    int* nodes = reinterpret_cast<int*>(sdfb) + reinterpret_cast<const int*>(sdfb)[MPB_DW_OFF_NODES];
    const unsigned n_nodes = (unsigned)nx * (unsigned)ny * (unsigned)nz;
    const unsigned tile = (unsigned)max(1, MPB_EDT_X_TILE / nx) * (unsigned)nx;      // <= 1024 nodes, whole lines
    const unsigned base = blockIdx.x * tile;
    const unsigned cnt = min(tile, n_nodes - base);
    for (unsigned l = threadIdx.x; l < cnt; l += 256u) line[l] = occ[base + l] != 0 ? 1 : 0;
    __syncthreads();
    for (unsigned l = threadIdx.x; l < cnt; l += 256u) {
        const int i = (int)(l % (unsigned)nx);
        const unsigned char* row = line + (l - (unsigned)i);
        const unsigned char c = row[i];
        int g = MPB_EDT_NONE;
        for (int d = 1; i - d >= 0 || i + d < nx; ++d) {
            const bool lo = i - d >= 0 && row[i - d] != c, hi = i + d < nx && row[i + d] != c;
            if (lo || hi) { g = d * d; break; }
        }
        nodes[base + l] = c ? -g : g;
    }
}

// cell * (sqrt(D2) - 0.5) in three separately rounded fp32 operations.  D2 < 2^24 is exact in fp32 and in fp64; the fp64 root is
// correctly rounded and rounding it to fp32 is the correctly rounded fp32 root (53 >= 2 * 24 + 2 bits: double rounding is innocuous)
__device__ __forceinline__ float edt_value(int d2, float cell) {
#pragma clang fp contract(off)
    const float root = (float)sqrt((double)d2);
    return __fmul_rn(cell, __fsub_rn(root, 0.5f));
}

// along y (axis 1) or z (axis 2): a tile is MPB_EDT_T consecutive x positions by the whole line, laid out [position along the axis][T];
// blockIdx.y is the other of the two axes.  LAST: the pass that turns D2 into the node value.
template <bool LAST>
__global__ __launch_bounds__(1024) void occ_edt_axis_kernel(float* __restrict__ sdfb, int nx, int ny, int nz, int axis) {
    extern __shared__ int edt_tile[];
    if (!edt_header_matches(sdfb, nx, ny, nz)) return;           // (block-uniform)
    int* nodes = reinterpret_cast<int*>(sdfb) + reinterpret_cast<const int*>(sdfb)[MPB_DW_OFF_NODES];
    const int n = axis == 1 ? ny : nz;
    const unsigned stride = axis == 1 ? (unsigned)nx : (unsigned)nx * (unsigned)ny;
    const int col = threadIdx.x & (MPB_EDT_T - 1), row0 = threadIdx.x / MPB_EDT_T, rows = blockDim.x / MPB_EDT_T;
    const int x = blockIdx.x * MPB_EDT_T + col;
    const bool live = x < nx;
    const unsigned base = (axis == 1 ? blockIdx.y * (unsigned)nx * (unsigned)ny : blockIdx.y * (unsigned)nx) + (unsigned)x;
    if (live)
        for (int r = row0; r < n; r += rows) edt_tile[r * MPB_EDT_T + col] = nodes[base + (unsigned)r * stride];
    __syncthreads();
    if (!live) return;
    const float cell = sdfb[MPB_DW_CELL];
    const int d2_none = (nx - 1) * (nx - 1) + (ny - 1) * (ny - 1) + (nz - 1) * (nz - 1) + 1;
    for (int r = row0; r < n; r += rows) {
        const int w = edt_tile[r * MPB_EDT_T + col];
        const int sgn = w < 0 ? -1 : 1;                          // the node's class; f(j) = max(sgn * word(j), 0): towards the other class
        int best = sgn * w;
        for (int d = 1; d * d < best && (r - d >= 0 || r + d < n); ++d) {
            if (r - d >= 0) best = min(best, max(sgn * edt_tile[(r - d) * MPB_EDT_T + col], 0) + d * d);
            if (r + d < n) best = min(best, max(sgn * edt_tile[(r + d) * MPB_EDT_T + col], 0) + d * d);
        }
        if (LAST) {
            const float v = edt_value(best >= MPB_EDT_NONE ? d2_none : best, cell);
            reinterpret_cast<float*>(nodes)[base + (unsigned)r * stride] = sgn < 0 ? -v : v;
        } else {
            nodes[base + (unsigned)r * stride] = sgn * best;
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
extern "C" int mpb_sdf_grid_check(const float* s, int n_words) {
    if (!s || n_words < MPB_SDF_HEADER_WORDS) return mpb_failf(MPB_E_INVALID, "%s: SDF-grid buffer too small", __func__);
    const int32_t* si = reinterpret_cast<const int32_t*>(s);
    const int rc = sdf_header_check(si, n_words, __func__);
    if (rc) return rc;
    if (si[MPB_DW_KIND] == MPB_KIND_CHAIN) {
        int prev = 1;
        for (int l = 0; l < si[MPB_DW_N_LINKS]; ++l) {
            const int f = si[si[MPB_DW_OFF_LINKS] + 8 * l];
            if (f < prev || f > si[MPB_DW_N_DOF] + 1) return mpb_failf(MPB_E_INVALID, "%s: link frames must be sorted in [1, n_dof+1]", __func__);
            prev = f;
        }
    }
    return MPB_OK;
}

extern "C" int mpb_sdf_grid_invalidate(const float* sdfb) {
    g_sdf_cache.drop(sdfb);
    g_mesh_cache.drop(sdfb);                                   // (a mesh buffer's address: mpb_sdf_grid_build_mesh reads it the same way)
    return MPB_OK;
}

extern "C" int mpb_sdf_grid_build(const float* geom, float* sdfb, void* stream) {
    if (!geom || !sdfb) return mpb_failf(MPB_E_INVALID, "%s: null pointer", __func__);
    if (mpb_misaligned16(geom, sdfb)) return mpb_failf(MPB_E_INVALID, "%s: the geometry and the SDF-grid buffer must be 16-byte aligned", __func__);
    SdfShape S;
    int rc = sdf_shape(sdfb, S, __func__);
    if (rc) return rc;
    int32_t gh[MPB_GEOM_HEADER_WORDS];
    const hipError_t e = hipMemcpy(gh, geom, sizeof(gh), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return mpb_failf(MPB_E_HIP, "%s: reading the geometry header failed: %s", __func__, hipGetErrorString(e));
    if (gh[MPB_GW_MAGIC] != MPB_GEOM_MAGIC || (gh[MPB_GW_VERSION] != MPB_GEOM_VERSION && gh[MPB_GW_VERSION] != MPB_GEOM_VERSION_LIST))
        return mpb_failf(MPB_E_INVALID, "%s: bad magic/version of the geometry buffer", __func__);
    if (gh[MPB_GW_NEXT] != 0) return mpb_failf(MPB_E_UNSUPPORTED, "%s: the grid is built from ONE CollisionField, this geometry buffer chains several", __func__);
    const int n_sph = gh[MPB_GW_N_SPH], n_box = gh[MPB_GW_N_BOX];
    if (n_sph < 0 || n_box < 0 || n_sph + n_box < 1) return mpb_failf(MPB_E_INVALID, "%s: the geometry buffer holds no obstacle", __func__);
    const unsigned n_nodes = (unsigned)S.nx * (unsigned)S.ny * (unsigned)S.nz;
    hipLaunchKernelGGL(sdf_build_kernel, dim3((n_nodes + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, geom, sdfb, S.nx, S.ny, S.nz, n_sph, n_box);
    return mpb_check_launch(__func__);
}

// LDS of a y / z pass: n rows of MPB_EDT_T words, 128 KB at n = MPB_SDF_MAX_DIM = 1 024; the kernel's limit is raised where that takes it
template <bool LAST>
static int edt_axis_launch(float* sdfb, const SdfShape& S, int axis, void* stream, const char* who) {
    const int n = axis == 1 ? S.ny : S.nz, other = axis == 1 ? S.nz : S.ny;
    const size_t bytes = (size_t)n * MPB_EDT_T * sizeof(int);
    const int rc = mpb_raise_lds_limit(reinterpret_cast<const void*>(occ_edt_axis_kernel<LAST>), S.dev, bytes, who);
    if (rc) return rc;
    const int threads = std::min(1024, (n * MPB_EDT_T + 63) / 64 * 64);          // one thread per node of the tile up to 1 024, whole waves
    hipLaunchKernelGGL(occ_edt_axis_kernel<LAST>, dim3((S.nx + MPB_EDT_T - 1) / MPB_EDT_T, other), dim3(threads), bytes, (hipStream_t)stream, sdfb,
                       S.nx, S.ny, S.nz, axis);
    return mpb_check_launch(who);
}

extern "C" int mpb_sdf_grid_build_occupancy(const unsigned char* occupancy, float* sdfb, void* stream) {
    if (!occupancy || !sdfb) return mpb_fail(MPB_E_INVALID, "mpb_sdf_grid_build_occupancy: null pointer");
    if (mpb_misaligned16(sdfb)) return mpb_failf(MPB_E_INVALID, "%s: the SDF-grid buffer must be 16-byte aligned", __func__);
    SdfShape S;
    int rc = sdf_shape(sdfb, S, __func__);
    if (rc) return rc;
    const unsigned n_nodes = (unsigned)S.nx * (unsigned)S.ny * (unsigned)S.nz;
    const unsigned tile = (unsigned)(MPB_EDT_X_TILE / S.nx > 1 ? MPB_EDT_X_TILE / S.nx : 1) * (unsigned)S.nx;
    hipLaunchKernelGGL(occ_edt_x_kernel, dim3((n_nodes + tile - 1) / tile), dim3(256), 0, (hipStream_t)stream, occupancy, sdfb, S.nx, S.ny, S.nz);
    rc = mpb_check_launch(__func__);
    if (rc) return rc;
    if (S.nz == 1) return edt_axis_launch<true>(sdfb, S, 1, stream, __func__);
    rc = edt_axis_launch<false>(sdfb, S, 1, stream, __func__);
    if (rc) return rc;
    return edt_axis_launch<true>(sdfb, S, 2, stream, __func__);
}

extern "C" int mpb_sdf_grid_sample(const float* points, const float* sdfb, float* s, float* grad, int N, void* stream) {
    if (N < 0) return mpb_failf(MPB_E_INVALID, "%s: bad shape", __func__);
    if (N == 0) return MPB_OK;
    if (!points || !sdfb || !s) return mpb_failf(MPB_E_INVALID, "%s: null pointer", __func__);
    if (mpb_misaligned16(sdfb)) return mpb_failf(MPB_E_INVALID, "%s: the SDF-grid buffer must be 16-byte aligned", __func__);
    SdfShape S;
    const int rc = sdf_shape(sdfb, S, __func__);
    if (rc) return rc;
    hipLaunchKernelGGL(sdf_sample_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, points, sdfb, s, grad, N, S.nx, S.ny, S.nz);
    return mpb_check_launch(__func__);
}

static int sdf_cost_launch(bool want_grad, const char* who, const float* trajs, const float* sdfb, float* out, float* per_wp, float* grad,
                           int B, int H, int d, int h_begin, float k_sigma, float weight, int accumulate, void* stream) {
    int rc = mpb_check_rows(who, "SDF-grid", trajs, sdfb, out, want_grad, grad, B, H, d, h_begin);
    if (rc || B == 0) return rc;
    SdfShape S;
    if ((rc = sdf_shape(sdfb, S, who))) return rc;
    if (d < S.n_dof) return mpb_failf(MPB_E_INVALID, "%s: rows of d = %d are narrower than the robot's %d coordinates", who, d, S.n_dof);
    hipLaunchKernelGGL(want_grad ? sdf_cost_kernel<true> : sdf_cost_kernel<false>, dim3(B), dim3(64), 0, (hipStream_t)stream, trajs, sdfb, out,
                       per_wp, grad, H, d, h_begin, k_sigma, weight, accumulate, S.n_dof, S.n_links, S.nx, S.ny, S.nz);
    return mpb_check_launch(who);
}

extern "C" int mpb_sdf_grid_eval(const float* trajs, const float* sdfb, float* out, float* per_waypoint, int B, int H, int d, int h_begin,
                                 float k_sigma, float weight, int accumulate, void* stream) {
    return sdf_cost_launch(false, __func__, trajs, sdfb, out, per_waypoint, nullptr, B, H, d, h_begin, k_sigma, weight, accumulate, stream);
}

extern "C" int mpb_sdf_grid_grad(const float* trajs, const float* sdfb, float* out, float* grad, int B, int H, int d, int h_begin, float k_sigma,
                                 float weight, int accumulate, void* stream) {
    return sdf_cost_launch(true, __func__, trajs, sdfb, out, nullptr, grad, B, H, d, h_begin, k_sigma, weight, accumulate, stream);
}

extern "C" int mpb_sdf_grid_collision_check(const float* q, const float* sdfb, unsigned char* in_collision, float* gap, int N, int D, int or_into,
                                            void* stream) {
    int rc = mpb_check_configs(__func__, "SDF-grid", q, sdfb, in_collision, N, D);
    if (rc || N == 0) return rc;
    SdfShape S;
    if ((rc = sdf_shape(sdfb, S, __func__))) return rc;
    if (D != S.n_dof) return mpb_failf(MPB_E_INVALID, "%s: D = %d, the robot has %d coordinates", __func__, D, S.n_dof);
    hipLaunchKernelGGL(sdf_check_kernel, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, q, sdfb, in_collision, gap, N, D, or_into, S.n_links,
                       S.nx, S.ny, S.nz);
    return mpb_check_launch(__func__);
}
