// mpb_rrt.h -- the pieces the sample-based planner kernels share (mpb_rrt_connect.hip, mpb_rrt_star.hip, mpb_strrt.hip,
// mpb_prm.hip, mpb_path_shortcut.hip; mpb_traj_validate.hip takes the predicate): the collision cost of one configuration
// per lane, the row loads, the two distances, torch.allclose's element, extend_path's point count and linspace point
// (utils.py:4-14), safe_path's scan for the first point in collision (utils.py:17-30), purge_duplicates_from_traj
// (utils.py:33-50) and the order-preserving deletion of a pool entry (rrt_base.py:59-63), and what the init kernels have
// in common.  Every function is block-uniform: all 64 lanes of the
// single-wave workgroup call it.  The workspace in numbers (status values, header word indices, the pool limit
// MPB_RRT_MAX_PRE_SAMPLES) is include/mpb_rrt_layout.h, generated from rrt_layout.py.
// Arithmetic: every function below that rounds carries #pragma clang fp contract(off) in its body and says what the device
// runs -- fmaf where one rounding is the definition, plain operators where every operation rounds; rrt_dist alone does
// not, and says why.  (The pragma is per function body, never at file scope: the collision walk of mpb_geom.h is compiled
// under the build's fast contraction.)
#pragma once
#include "../../include/mpb_rrt_layout.h"
#include "mpb_common.h"
#include "mpb_geom.h"
#include "mpb_model_panda.h"

#define RRT_MAX_PTS (1 << 20)    // points of one extension (dist / step_size + 2): far beyond any sane step size

// Collision cost of one configuration per lane, chained fields in turn.  Block-uniform control flow: every thread of the
// block calls it (a lane without work passes any valid configuration).  `staged` is the field whose grid sits in LDS.
template <int MODEL>
__device__ __forceinline__ float rrt_config_cost(const float* __restrict__ geom, unsigned* gridw, float4* otab,
                                                 const float*& staged, const float (&q)[MPB_MAX_DOF]) {
    float c = 0.f;
    for (const float* gp = geom; gp != nullptr; gp = geom_next(gp)) {
        const GeomView G = geom_view(gp);
        if (grid_usable(G)) {
            if (staged != gp) {
                __syncthreads();
                grid_stage(G, gridw, otab, threadIdx.x, blockDim.x);
                __syncthreads();
                staged = gp;
            }
            if (MODEL == PandaModel::ID && G.model == PandaModel::ID)
                c = fmaf(G.fscale, waypoint_cost_grid_model<PandaModel>(G, gridw, otab, q), c);
            else
                c = fmaf(G.fscale, waypoint_cost_grid(G, gridw, otab, q), c);
        } else {
            float dq[MPB_MAX_DOF];
            c = fmaf(G.fscale, waypoint_cost<false>(G, q, dq), c);
        }
    }
    return c;
}

// The predicate over the whole task (mpb_world.h, which defines both): obstacles, SDF grid and the robot against itself.  The
// functions below take WORLD as a compile-time switch and a WorldView; with WORLD == 0 they make the rrt_config_cost call above and
// nothing else, and the view is never looked at.
struct WorldView;
template <int MODEL, int WORLD>
__device__ __forceinline__ bool world_in_collision(const WorldView& W, unsigned* gridw, float4* otab, const float*& staged,
                                                   const float (&q)[MPB_MAX_DOF]);

// a configuration row of D floats into registers, zeros past D
template <int DM>
__device__ __forceinline__ void rrt_load_row(const float* p, int D, float (&q)[MPB_MAX_DOF]) {
#pragma unroll
    for (int k = 0; k < MPB_MAX_DOF; ++k) q[k] = (k < DM && k < D) ? p[k] : 0.f;
}

// a padded row (Dp floats, float4-aligned, zero padded) into registers
template <int DM>
__device__ __forceinline__ void rrt_load_row4(const float* row, int Dp, float (&q)[MPB_MAX_DOF]) {
    const float4* r = reinterpret_cast<const float4*>(row);
#pragma unroll
    for (int kk = 0; kk < (DM + 3) / 4; ++kk) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (4 * kk < Dp) v = r[kk];
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (4 * kk + c < MPB_MAX_DOF) q[4 * kk + c] = (4 * kk + c < DM) ? e[c] : 0.f;
    }
#pragma unroll
    for (int k = (DM + 3) / 4 * 4; k < MPB_MAX_DOF; ++k) q[k] = 0.f;
}

// RRT*'s distance: the squares summed in index order, symmetric in its arguments ((a - b)^2 == (b - a)^2); a distance between
// the same two bit patterns is the same number wherever it is computed.  The ONE expression of this file left under the
// build's contraction (plain operators, no pragma), because no single form is what the device runs: the compile-time-D
// instantiations of rrt_star_kernel take fma(df0, df0, fl(df1 df1)) and ONE fma per later term at every call, while in
// rrt_star_kernel<0, 0> the calls disagree (the informed test's two distances take that form, the nearest-node scan takes
// fl(df0 df0) and ONE fma per later term).  tests/test_gpu_sample_based_bits.py holds every instantiation to its bits.
template <int DM>
__device__ __forceinline__ float rrt_dist(const float (&x)[MPB_MAX_DOF], const float (&y)[MPB_MAX_DOF]) {
    float d2 = 0.f;
#pragma unroll
    for (int k = 0; k < DM; ++k) {
        const float df = x[k] - y[k];
        d2 = d2 + df * df;
    }
    return sqrtf(d2);
}

// The roadmap's and the shortcut pass's squared distance: the same sum rounded after every operation (tests/*_checks.py dist32)
template <int DM>
__device__ __forceinline__ float rrt_d2_rounded(const float (&x)[MPB_MAX_DOF], const float (&y)[MPB_MAX_DOF]) {
#pragma clang fp contract(off)
    float d2 = 0.f;
#pragma unroll
    for (int k = 0; k < DM; ++k) {
        const float df = x[k] - y[k];
        d2 = d2 + df * df;
    }
    return d2;
}

// torch.allclose(a, b) element: |a - b| <= atol + rtol |b| with the defaults rtol 1e-5, atol 1e-8; the right side is ONE fma
__device__ __forceinline__ bool rrt_close(float a, float b) {
#pragma clang fp contract(off)
    return fabsf(a - b) <= fmaf(1e-5f, fabsf(b), 1e-8f);
}

// extend_path's point count (utils.py:9-11), from the UNCLAMPED distance
__device__ __forceinline__ int rrt_point_count(float dist, float step) {
    return (int)fminf(dist / step, (float)(RRT_MAX_PTS - 2)) + 2;
}

// point p of  q1 + dl * linspace(0, 1, n_pts)  as ATen's CPU kernel walks the linspace (from the near end of each half),
// lstep = 1 / (n_pts - 1), with one rounding where ATen has two: 1 - lstep * j and q1 + dl * al are ONE fma each
template <int DM>
__device__ __forceinline__ void rrt_linspace_point(const float (&q1)[MPB_MAX_DOF], const float (&dl)[MPB_MAX_DOF], int n_pts,
                                                   float lstep, int p, float (&q)[MPB_MAX_DOF]) {
#pragma clang fp contract(off)
    const float al = (p < n_pts / 2) ? lstep * (float)p : fmaf(-lstep, (float)(n_pts - 1 - p), 1.0f);
#pragma unroll
    for (int k = 0; k < MPB_MAX_DOF; ++k) q[k] = (k < DM) ? fmaf(dl[k], al, q1[k]) : 0.f;
}

// safe_path's scan: the index of the first of the n_pts points of an extension that is in collision, -1 when none is;
// one lane per point, 64 points per trip, and the trips after the first hit are never evaluated
template <int DM, int MODEL, int WORLD = 0>
__device__ __forceinline__ int rrt_first_collision(const float* __restrict__ geom, unsigned* gridw, float4* otab,
                                                   const float*& staged, const float (&q1)[MPB_MAX_DOF],
                                                   const float (&dl)[MPB_MAX_DOF], int n_pts, float lstep, int lane,
                                                   const WorldView* W = nullptr) {
    for (int base = 0; base < n_pts; base += 64) {
        const int p = base + lane;
        float q[MPB_MAX_DOF];
        rrt_linspace_point<DM>(q1, dl, n_pts, lstep, min(p, n_pts - 1), q);
        unsigned long long m;
        if constexpr (WORLD == 0) {
            const float c = rrt_config_cost<MODEL>(geom, gridw, otab, staged, q);
            m = __ballot(p < n_pts && c > 0.f);
        } else {
            m = __ballot(world_in_collision<MODEL, WORLD>(*W, gridw, otab, staged, q) && p < n_pts);
        }
        if (m != 0ull) return base + (int)__builtin_ctzll(m);
    }
    return -1;
}

// rrt_base.py:59-63: delete entry idx of the LDS pool list of plen entries, keeping the order (a parallel shift)
__device__ __forceinline__ void rrt_pool_delete(unsigned short* pool, int idx, int plen, int lane) {
    for (int base = idx; base < plen - 1; base += 64) {
        const int i = base + lane;
        const unsigned short v = pool[min(i + 1, plen - 1)];
        __syncthreads();
        if (i < plen - 1) pool[i] = v;
        __syncthreads();
    }
}

// purge_duplicates_from_traj (utils.py:33-50) in place on the Lraw rows of path_b (row-major, D columns; lane k owns
// column k): returns the number of rows kept
__device__ __forceinline__ int rrt_purge(float* path_b, int Lraw, int D, int lane) {
    if (Lraw <= 2) return Lraw;
    const bool on = lane < D;
    const float row0 = on ? path_b[lane] : 0.f;
    const float last = on ? path_b[(size_t)(Lraw - 1) * D + lane] : 0.f;
    float cur = row0, lastsel = row0;
    int out = 0;
    bool any_sel = false;
    for (int j = 0; j + 1 < Lraw; ++j) {
        const float nxt = on ? path_b[(size_t)(j + 1) * D + lane] : 0.f;
        if (__ballot(on && fabsf(nxt - cur) > 1e-6f) != 0ull) {   // row j differs from row j + 1: selected
            if (!any_sel) {
                any_sel = true;
                if (j > 0 && __ballot(on && !rrt_close(cur, row0)) != 0ull) {
                    if (on) path_b[(size_t)out * D + lane] = row0;
                    ++out;
                }
            }
            if (on) path_b[(size_t)out * D + lane] = cur;
            ++out;
            lastsel = cur;
        }
        cur = nxt;
    }
    if (!any_sel) {                                 // (every row equals its successor: the first row stands for all)
        if (on) path_b[lane] = row0;
        out = 1;
    }
    if (__ballot(on && !rrt_close(lastsel, last)) != 0ull) {
        if (on) path_b[(size_t)out * D + lane] = last;
        ++out;
    }
    return out;
}

// What the init kernels of RRT-Connect and RRT* do alike, for problem b: the global words (block 0), the full pool list
// 0 .. n_pre - 1 at `pool`, and the collision check of the start (lane 0) and the goal (every other lane).  Returns the
// problem's first status word.
template <int MODEL, int WORLD = 0>
__device__ __forceinline__ int rrt_init_shared(int* __restrict__ ws, int magic, int B, int max_nodes, int n_pre, int D, int Dp,
                                               unsigned* __restrict__ pool, int pool_words, const float* __restrict__ start,
                                               const float* __restrict__ goal, const float* __restrict__ geom, unsigned* gridw,
                                               float4* otab, int b, int lane, const WorldView* W = nullptr) {
    if (b == 0 && lane < MPB_RRT_GLOBAL_WORDS) {
        int v = 0;
        if (lane == MPB_RRTG_MAGIC) v = magic;
        if (lane == MPB_RRTG_B) v = B;
        if (lane == MPB_RRTG_MAX_NODES) v = max_nodes;
        if (lane == MPB_RRTG_N_PRE) v = n_pre;
        if (lane == MPB_RRTG_D) v = D;
        if (lane == MPB_RRTG_DP) v = Dp;
        ws[lane] = v;
    }
    const float* row = (lane == 0 ? start : goal) + (size_t)b * D;
    float q[MPB_MAX_DOF];
    rrt_load_row<MPB_MAX_DOF>(row, D, q);
    const float* staged = nullptr;
    bool hit;
    if constexpr (WORLD == 0) {
        const float c = rrt_config_cost<MODEL>(geom, gridw, otab, staged, q);
        hit = __ballot(c > 0.f) != 0ull;
    } else {
        hit = __ballot(world_in_collision<MODEL, WORLD>(*W, gridw, otab, staged, q)) != 0ull;
    }
    for (int w = lane; w < pool_words; w += 64)
        pool[w] = (unsigned)(2 * w) | ((unsigned)(2 * w + 1) << MPB_RRT_POOL_INDEX_BITS);
    return hit ? MPB_RRT_START_OR_GOAL_IN_COLLISION : MPB_RRT_RUNNING;
}
