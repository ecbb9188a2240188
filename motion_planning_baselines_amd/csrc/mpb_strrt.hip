// mpb_strrt.hip -- space-time RRT-Connect among moving obstacles (planners.STRRTConnect; build-defined, DESIGN.md 10: the reference has
// nothing like it).  Time lives on the row grid of a packed moving-obstacle buffer (include/mpb_moving_layout.h): row h of R is the field's
// time t_start + h (t_end - t_start) / (R - 1), a tree node is (q, row, parent), tree 0 is rooted at (start, 0) and grows forward in time,
// tree 1 at (goal, R - 1) and grows backward.  Every collision check is made AT A ROW with the buffer's centres of that row -- obstacle
// positions are never interpolated -- which is the statement mpb_moving_collision_check makes of a trajectory; a finer clock is a larger R.
//
// Predicate of (q, row): the static cost of the task's geometry is positive (rrt_config_cost of mpb_rrt.h) OR the moving cost of that row
// is (moving_row_cost<false> of mpb_moving.h); one after the other in a lane, so the register need is the larger of the two.
// Metric from node n to a target (q_r, h_r) on the tree's growing side (dh = |h_r - h_n| >= 1), w_k the most joint k may move per row:
//   tau = max_k (|q_r[k] - q_n[k]| / w_k)    m = max(tau, (float)dh)       nearest: least m, lowest index on ties
// Extension from n towards the target: s = min(dh, max_step_rows) rows (a connect target: s = dh),
//   f = tau > dh ? dh / tau : 1     dl = (q_r - q_n) * f     point j = fma(dl, (float)j / (float)dh, q_n) at row h_n +- j, 1 <= j <= s,
//   and point j = dh with f == 1 is q_r's own bits.  One lane per point, trips of 64, the first colliding point j0 is the count of
//   trailing zeros of a ballot and the trips after it are never evaluated; j0 == 1 fails, otherwise point j0 - 1 (or s) is appended.
// Iteration `it`: tree it & 1 extends towards (pre_samples[idx], row) -- idx = mulhi(x, n_pre), row = 1 + mulhi(y, R - 2) of ONE Philox
//   call (problem_offset + b, it, MPB_STRRT_MAGIC, 0) --, then the other tree extends towards the new node; when it appends that very node
//   (same row, every coordinate rrt_close, and arrived at with f == 1 so that no edge of the plan exceeds w) the trees are joined: the
//   vertex list is tree 0's chain root -> its new node followed by tree 1's chain from the PARENT of its new node to the goal, the dense trajectory is q_a + (q_b - q_a) * ((h - h_a) / (h_b - h_a)) (one
//   fma) between consecutive vertices, the vertex rows their own bits, and every one of the R rows is checked again, one lane per row: the
//   interpolated rows are not the bits the extensions checked.  A row that fails discards the join (rejected_joins) and the search goes
//   on; FOUND therefore means every row of the output is free by this file's predicate, bit for bit.
// Mapping: one single-wave workgroup per problem; workgroups never wait on each other, there is no spin wait, every loop is bounded by
// n_iters, max_nodes, R or Lmax, and a finished problem returns at once.  The trees (configurations padded to float4s, int32 row, int32
// parent) live in the caller's workspace (include/mpb_strrt_layout.h, generated from strrt_layout.py).  The predicate strrt_collides, the
// metric strrt_tau and the scene record StMoving are in mpb_strrt.h, shared with mpb_st_shortcut.hip.
#include "mpb_common.h"
#include "mpb_rrt.h"
#include "mpb_rrt_host.h"
#include "mpb_moving.h"
#include "mpb_strrt.h"
#include "../../include/mpb_strrt_layout.h"

#define STRRT_WORDS_PER_NODE 32.0   // the size bound of the shape check: two trees, at most 12 + 2 words per node

struct StLayout {
    size_t hdr, nodes, rows, parents, total;   // offsets in 32-bit words
    int Dp;
};

__host__ __device__ static inline StLayout st_layout(int B, int max_nodes, int D) {
    StLayout L;
    L.Dp = (D + 3) & ~3;
    L.hdr = MPB_STRRT_GLOBAL_WORDS;
    L.nodes = L.hdr + (size_t)B * MPB_STRRT_HDR_WORDS;
    L.rows = L.nodes + (size_t)B * 2 * max_nodes * L.Dp;
    L.parents = L.rows + (size_t)B * 2 * max_nodes;
    L.total = L.parents + (size_t)B * 2 * max_nodes;
    return L;
}

// ---- workspace initialisation: global words, roots, counts, status (start at row 0, goal at row R - 1, the horizon) ----------------------
template <int MODEL>
__global__ __launch_bounds__(64) void strrt_init_kernel(int* __restrict__ ws, const float* __restrict__ start, const float* __restrict__ goal,
                                                        const float* __restrict__ wrow, const float* __restrict__ geom, const StMoving mv,
                                                        int B, int max_nodes, int D, int R) {
    __shared__ unsigned gridw[MPB_GRID_MAX_CELLS];
    __shared__ float4 otab[MPB_GRID_MAX_SPH + 1];
    const int b = blockIdx.x, lane = threadIdx.x;
    const StLayout L = st_layout(B, max_nodes, D);
    const GeomView G = moving_robot_view(mv.mob);
    const MovingTables T = moving_tables(mv.mob, R, mv.n_sph, mv.n_box);
    const bool ok = moving_header_matches(mv.mob, D, mv.L, R, mv.n_sph, mv.n_box);
    if (b == 0 && lane < MPB_STRRT_GLOBAL_WORDS) {
        int v = 0;
        if (lane == MPB_STG_MAGIC) v = MPB_STRRT_MAGIC;
        if (lane == MPB_STG_B) v = B;
        if (lane == MPB_STG_MAX_NODES) v = max_nodes;
        if (lane == MPB_STG_D) v = D;
        if (lane == MPB_STG_DP) v = L.Dp;
        if (lane == MPB_STG_N_ROWS) v = R;
        ws[lane] = v;
    }
    float qs[MPB_MAX_DOF], qg[MPB_MAX_DOF], w[MPB_MAX_DOF], q[MPB_MAX_DOF];
#pragma unroll
    for (int k = 0; k < MPB_MAX_DOF; ++k) {
        qs[k] = (k < D) ? start[(size_t)b * D + k] : 0.f;
        qg[k] = (k < D) ? goal[(size_t)b * D + k] : 0.f;
        w[k] = (k < D) ? wrow[k] : 1.f;
        q[k] = (lane == 0) ? qs[k] : qg[k];
    }
    const float* staged = nullptr;
    const bool hit = strrt_collides<MODEL>(geom, gridw, otab, staged, G, T, mv.L, ok, lane == 0 ? 0 : R - 1, q);
    int status = MPB_STRRT_RUNNING;
    if (strrt_tau(qg, qs, w) > (float)(R - 1)) status = MPB_STRRT_HORIZON_TOO_SHORT;
    if (__ballot(hit) != 0ull) status = MPB_STRRT_START_OR_GOAL_IN_COLLISION;
    float* nodes = reinterpret_cast<float*>(ws) + L.nodes + (size_t)b * 2 * max_nodes * L.Dp;
    int* rows = ws + L.rows + (size_t)b * 2 * max_nodes;
    int* parents = ws + L.parents + (size_t)b * 2 * max_nodes;
    if (lane < L.Dp) {
        nodes[lane] = (lane < D) ? start[(size_t)b * D + lane] : 0.f;
        nodes[(size_t)max_nodes * L.Dp + lane] = (lane < D) ? goal[(size_t)b * D + lane] : 0.f;
    }
    if (lane < 2) {
        parents[(size_t)lane * max_nodes] = -1;
        rows[(size_t)lane * max_nodes] = lane == 0 ? 0 : R - 1;
    }
    if (lane < MPB_STRRT_HDR_WORDS) {
        int* H = ws + L.hdr + (size_t)b * MPB_STRRT_HDR_WORDS;
        int v = 0;
        if (lane == MPB_STH_STATUS) v = status;
        if (lane == MPB_STH_COUNTS || lane == MPB_STH_COUNTS + 1) v = 1;
        H[lane] = v;
    }
}

struct StArgs {
    int* ws;
    const float* geom;
    StMoving mv;
    const float* w;
    const float* pre;
    size_t pre_stride;
    const int* sample_idx;
    const int* sample_row;
    float* trajs;
    float* vertex_q;
    int* vertex_row;
    int* n_vertices;
    int* status;
    int* log;
    int B, D, max_nodes, n_pre, R, Lmax, max_step, iter0, n_iters, total_iters;
    uint32_t seed_lo, seed_hi, problem_offset;
};

// ---- the persistent kernel -----------------------------------------------------------------------------------------------------------------
template <int DT, int MODEL>
__global__ __launch_bounds__(64) void strrt_kernel(const StArgs a) {
#pragma clang fp contract(off)
    __shared__ unsigned gridw[MPB_GRID_MAX_CELLS];
    __shared__ float4 otab[MPB_GRID_MAX_SPH + 1];
    constexpr int DM = DT ? DT : MPB_MAX_DOF;
    constexpr int DM4 = (DM + 3) / 4;
    const int D = DT ? DT : a.D;
    const int R = a.R;
    const int b = blockIdx.x, lane = threadIdx.x;
    const StLayout L = st_layout(a.B, a.max_nodes, D);
    int* H = a.ws + L.hdr + (size_t)b * MPB_STRRT_HDR_WORDS;
    int status = H[MPB_STH_STATUS];
    if (status != MPB_STRRT_RUNNING) {                     // block-uniform: a finished problem costs nothing
        if (lane == 0) a.status[b] = status;
        return;
    }
    int cnt[2] = {H[MPB_STH_COUNTS], H[MPB_STH_COUNTS + 1]};
    int rejected = H[MPB_STH_REJECTED_JOINS];
    float* nodes_b = reinterpret_cast<float*>(a.ws) + L.nodes + (size_t)b * 2 * a.max_nodes * L.Dp;
    int* rows_b = a.ws + L.rows + (size_t)b * 2 * a.max_nodes;
    int* parents_b = a.ws + L.parents + (size_t)b * 2 * a.max_nodes;
    const float* pre_b = a.pre + (size_t)b * a.pre_stride;
    float* tr = a.trajs + (size_t)b * R * D;
    float* vq = a.vertex_q + (size_t)b * a.Lmax * D;
    int* vr = a.vertex_row + (size_t)b * a.Lmax;
    const GeomView G = moving_robot_view(a.mv.mob);
    const MovingTables T = moving_tables(a.mv.mob, R, a.mv.n_sph, a.mv.n_box);
    const bool ok = moving_header_matches(a.mv.mob, D, a.mv.L, R, a.mv.n_sph, a.mv.n_box);
    float w[MPB_MAX_DOF];
#pragma unroll
    for (int k = 0; k < MPB_MAX_DOF; ++k) w[k] = (k < DM && k < D) ? a.w[k] : 1.f;
    const float* staged = nullptr;

    // (Of mpb_rrt.h this kernel calls the predicate and rrt_close only: with its loops behind shared helpers it measured 0.5 % slower
    // -- DESIGN.md, the RRT open items.)
    // one extension of tree t towards (tq, hr): nearest node by the time-like metric, the points at the rows between, the append.
    // Returns false when no node is eligible, the first point collides or the tree is full; leaves the appended node in (nq, nrow).
    float nq[MPB_MAX_DOF];
    int nrow = 0;
    bool arrived = false;                                  // the appended node is the target's own bits (f == 1 and nothing collided)
    auto extend = [&](int t, const float (&tq)[MPB_MAX_DOF], int hr, bool connect, int* rec) -> bool {
        const float* nd = nodes_b + (size_t)t * a.max_nodes * L.Dp;
        const int* rw = rows_b + (size_t)t * a.max_nodes;
        const int n = cnt[t];
        float best = 3.0e38f;
        int bi = 0x7FFFFFFF;
        for (int i = lane; i < n; i += 64) {
            const int hn = rw[i];
            const int dhs = (t == 0) ? hr - hn : hn - hr;
            if (dhs < 1) continue;                         // (not on the growing side of the node; no wave-wide call below)
            const float4* r = reinterpret_cast<const float4*>(nd + (size_t)i * L.Dp);
            float tau = 0.f;
#pragma unroll
            for (int kk = 0; kk < DM4; ++kk) {
                if (4 * kk < L.Dp) {
                    const float4 v = r[kk];
                    const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (4 * kk + c < DM) tau = fmaxf(tau, fabsf(tq[4 * kk + c] - e[c]) / w[4 * kk + c]);
                }
            }
            const float m = fmaxf(tau, (float)dhs);
            if (m < best) { best = m; bi = i; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float od = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (od < best || (od == best && oi < bi)) { best = od; bi = oi; }
        }
        if (rec != nullptr && lane == 0) { rec[MPB_STL_TREE] = t; rec[MPB_STL_NEAREST] = bi == 0x7FFFFFFF ? -1 : bi; }
        if (bi == 0x7FFFFFFF) {
            if (rec != nullptr && lane == 0) { rec[MPB_STL_DH] = 0; rec[MPB_STL_S] = 0; rec[MPB_STL_FIRST] = -1; rec[MPB_STL_APPENDED] = -1; }
            return false;
        }
        const int hn = rw[bi];
        const int dh = (t == 0) ? hr - hn : hn - hr;
        const int s = connect ? dh : min(dh, a.max_step);
        float q1[MPB_MAX_DOF], dl[MPB_MAX_DOF];
#pragma unroll
        for (int k = 0; k < MPB_MAX_DOF; ++k) q1[k] = (k < DM && k < D) ? nd[(size_t)bi * L.Dp + k] : 0.f;
        const float tau = strrt_tau(tq, q1, w);
        const float dhf = (float)dh;
        const bool whole = !(tau > dhf);
        const float f = whole ? 1.0f : dhf / tau;
#pragma unroll
        for (int k = 0; k < MPB_MAX_DOF; ++k) dl[k] = (tq[k] - q1[k]) * f;
        auto point = [&](int j, float (&q)[MPB_MAX_DOF]) {
            const float al = (float)j / dhf;
            const bool target = whole && j == dh;
#pragma unroll
            for (int k = 0; k < MPB_MAX_DOF; ++k) q[k] = (k < DM) ? (target ? tq[k] : fmaf(dl[k], al, q1[k])) : 0.f;
        };
        int first = -1;
        for (int base = 1; base <= s; base += 64) {
            const int j = base + lane, jc = min(j, s);
            float q[MPB_MAX_DOF];
            point(jc, q);
            const bool hit = strrt_collides<MODEL>(a.geom, gridw, otab, staged, G, T, a.mv.L, ok, (t == 0) ? hn + jc : hn - jc, q);
            const unsigned long long m = __ballot(j <= s && hit);
            if (m != 0ull) { first = base + (int)__builtin_ctzll(m); break; }
        }
        if (rec != nullptr && lane == 0) { rec[MPB_STL_DH] = dh; rec[MPB_STL_S] = s; rec[MPB_STL_FIRST] = first; rec[MPB_STL_APPENDED] = -1; }
        if (first == 1) return false;
        const int jend = first < 0 ? s : first - 1;
        point(jend, nq);
        arrived = whole && jend == dh;
        nrow = (t == 0) ? hn + jend : hn - jend;
        if (n >= a.max_nodes) {
            status = MPB_STRRT_TREE_FULL;
            return false;
        }
        float* dst = nodes_b + ((size_t)t * a.max_nodes + n) * L.Dp;
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < DM; ++k) v = (lane == k) ? nq[k] : v;
        if (lane < L.Dp) dst[lane] = v;
        if (lane == 0) {
            parents_b[(size_t)t * a.max_nodes + n] = bi;
            rows_b[(size_t)t * a.max_nodes + n] = nrow;
            if (rec != nullptr) rec[MPB_STL_APPENDED] = n;
        }
        cnt[t] = n + 1;
        __syncthreads();                                   // the node is read back by the next nearest-node scan
        return true;
    };

    int it = a.iter0;
    const int it_end = min(a.iter0 + a.n_iters, a.total_iters);
    for (; it < it_end && status == MPB_STRRT_RUNNING; ++it) {
        const int t1 = it & 1, t2 = t1 ^ 1;
        int* rec = a.log != nullptr ? a.log + ((size_t)b * a.total_iters + it) * MPB_STRRT_LOG_WORDS : nullptr;
        int idx, hs;
        if (a.sample_idx != nullptr) {
            idx = a.sample_idx[(size_t)b * a.total_iters + it];
            hs = a.sample_row[(size_t)b * a.total_iters + it];
        } else {
            const uint4 r = philox4x32_10(make_uint4(a.problem_offset + (uint32_t)b, (uint32_t)it, MPB_STRRT_MAGIC, 0u),
                                          make_uint2(a.seed_lo, a.seed_hi));
            idx = (int)__umulhi(r.x, (uint32_t)a.n_pre);
            hs = 1 + (int)__umulhi(r.y, (uint32_t)(R - 2));
        }
        idx = min(max(idx, 0), a.n_pre - 1);
        hs = min(max(hs, 1), R - 2);
        const float* trow = pre_b + (size_t)idx * D;
        float tq[MPB_MAX_DOF];
#pragma unroll
        for (int k = 0; k < MPB_MAX_DOF; ++k) tq[k] = (k < DM && k < D) ? trow[k] : 0.f;
        if (!extend(t1, tq, hs, false, rec)) continue;
        float n1[MPB_MAX_DOF];
#pragma unroll
        for (int k = 0; k < MPB_MAX_DOF; ++k) n1[k] = nq[k];
        const int h1 = nrow;
        if (!extend(t2, n1, h1, true, rec != nullptr ? rec + MPB_STRRT_LOG_EXT_WORDS : nullptr)) continue;
        // joined: the other tree appended the new node itself.  Beyond the allclose of every coordinate the extension must have ARRIVED
        // (tau <= dh, the node is the target's bits): a near miss with tau slightly above dh is allclose too, but the vertex list would
        // then link the target to that extension's parent over an edge faster than w
        bool joined = nrow == h1 && arrived;
#pragma unroll
        for (int k = 0; k < MPB_MAX_DOF; ++k)
            if (k < DM && k < D) joined = joined && rrt_close(n1[k], nq[k]);
        if (!joined) continue;
        // ---- the join: vertex list, dense rows, the re-check of every row
        const float* nd0 = nodes_b;
        const float* nd1 = nodes_b + (size_t)a.max_nodes * L.Dp;
        const int* rw0 = rows_b;
        const int* rw1 = rows_b + a.max_nodes;
        const int* pa0 = parents_b;
        const int* pa1 = parents_b + a.max_nodes;
        const int e0 = cnt[0] - 1, e1 = pa1[cnt[1] - 1];
        int lenA = 0, lenB = 0;
        for (int j = e0; j >= 0 && lenA < cnt[0]; j = pa0[j]) ++lenA;
        for (int j = e1; j >= 0 && lenB < cnt[1]; j = pa1[j]) ++lenB;
        const int nv = lenA + lenB;
        if (nv > a.Lmax) { status = MPB_STRRT_PATH_TOO_LONG; ++it; break; }
        {
            int pos = lenA - 1;
            for (int j = e0; j >= 0 && pos >= 0; j = pa0[j], --pos) {
                if (lane < D) vq[(size_t)pos * D + lane] = nd0[(size_t)j * L.Dp + lane];
                if (lane == 0) vr[pos] = rw0[j];
            }
            pos = lenA;
            for (int j = e1; j >= 0 && pos < nv; j = pa1[j], ++pos) {
                if (lane < D) vq[(size_t)pos * D + lane] = nd1[(size_t)j * L.Dp + lane];
                if (lane == 0) vr[pos] = rw1[j];
            }
        }
        __syncthreads();
        for (int i = 0; i + 1 < nv; ++i) {
            const int ha = vr[i], hb = vr[i + 1];
            if (ha < 0 || hb > R - 1) continue;            // (rows of a workspace this kernel wrote never are: keeps every store inside tr)
            const float span = (float)(hb - ha);
            for (int h = ha + lane; h < hb; h += 64) {
                const float al = (float)(h - ha) / span;
                for (int k = 0; k < D; ++k) {
                    const float qa = vq[(size_t)i * D + k], qb = vq[(size_t)(i + 1) * D + k];
                    tr[(size_t)h * D + k] = (h == ha) ? qa : fmaf(qb - qa, al, qa);
                }
            }
        }
        if (lane < D) tr[(size_t)(R - 1) * D + lane] = vq[(size_t)(nv - 1) * D + lane];
        __syncthreads();
        int bad = -1;
        for (int base = 0; base < R; base += 64) {
            const int h = base + lane, hc = min(h, R - 1);
            float q[MPB_MAX_DOF];
#pragma unroll
            for (int k = 0; k < MPB_MAX_DOF; ++k) q[k] = (k < DM && k < D) ? tr[(size_t)hc * D + k] : 0.f;
            const bool hit = strrt_collides<MODEL>(a.geom, gridw, otab, staged, G, T, a.mv.L, ok, hc, q);
            const unsigned long long m = __ballot(h < R && hit);
            if (m != 0ull) { bad = base + (int)__builtin_ctzll(m); break; }
        }
        if (rec != nullptr && lane == 0) rec[MPB_STRRT_LOG_JOIN] = bad;
        if (bad >= 0) {                                    // the join is discarded; both trees keep their nodes
            ++rejected;
            __syncthreads();                               // (tr is written again by the next join)
            continue;
        }
        if (lane == 0) a.n_vertices[b] = nv;
        status = MPB_STRRT_FOUND;
        ++it;
        break;
    }
    if (status == MPB_STRRT_RUNNING && it >= a.total_iters) status = MPB_STRRT_EXHAUSTED_ITERS;
    if (lane == 0) {
        H[MPB_STH_STATUS] = status; H[MPB_STH_ITERS] = it; H[MPB_STH_COUNTS] = cnt[0]; H[MPB_STH_COUNTS + 1] = cnt[1];
        H[MPB_STH_REJECTED_JOINS] = rejected;
        a.status[b] = status;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------
static int strrt_shape_check(const char* who, int B, int max_nodes, int D, int R) {
    if (D > MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "%s: D = %d exceeds MPB_MAX_DOF = %d", who, D, MPB_MAX_DOF);
    if (R > MPB_STRRT_MAX_ROWS) return mpb_failf(MPB_E_UNSUPPORTED, "%s: n_rows = %d exceeds MPB_STRRT_MAX_ROWS = %d", who, R, MPB_STRRT_MAX_ROWS);
    if (R < MPB_STRRT_MIN_ROWS) return mpb_failf(MPB_E_INVALID, "%s: n_rows = %d, the time grid needs at least MPB_STRRT_MIN_ROWS = %d rows", who, R, MPB_STRRT_MIN_ROWS);
    if (B < 0 || max_nodes < 2 || D < 1) return mpb_failf(MPB_E_INVALID, "%s: bad shape (B %d, max_nodes %d, D %d)", who, B, max_nodes, D);
    if ((double)B * max_nodes * STRRT_WORDS_PER_NODE > 2.0e9 || (double)B * R * D > 2.0e9) return mpb_failf(MPB_E_UNSUPPORTED, "%s: B x max_nodes or B x n_rows too large", who);
    return MPB_OK;
}

// the checks *_init and *_run share after the shapes; fills the moving half of the scene from the buffer's cached header
static int strrt_scene_check(const char* who, bool any_null, const void* workspace, const void* geom, const float* mob, size_t workspace_bytes,
                             size_t need, int D, int R, StMoving& mv) {
    if (any_null) return mpb_failf(MPB_E_INVALID, "%s: null pointer", who);
    if (mpb_misaligned16(workspace, geom) || mpb_misaligned16(mob)) return mpb_failf(MPB_E_INVALID, "%s: workspace, geom and moving must be 16-byte aligned", who);
    if (workspace_bytes < need) return mpb_failf(MPB_E_INVALID, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    MovingShape S;
    const int rc = mpb_moving_shape_cached(mob, S, who);
    if (rc != MPB_OK) return rc;
    if (S.n_rows != R) return mpb_failf(MPB_E_INVALID, "%s: n_rows = %d, the moving-obstacle buffer was packed for n_rows = %d", who, R, S.n_rows);
    if (S.n_dof != D) return mpb_failf(MPB_E_INVALID, "%s: D = %d, the moving-obstacle buffer's robot has n_dof = %d", who, D, S.n_dof);
    mv.mob = mob; mv.L = S.n_links; mv.n_sph = S.n_sph; mv.n_box = S.n_box;
    return MPB_OK;
}

extern "C" size_t mpb_strrt_workspace_bytes(int B, int max_nodes, int D) {
    if (strrt_shape_check("mpb_strrt_workspace_bytes", B, max_nodes, D, MPB_STRRT_MIN_ROWS) != MPB_OK) return 0;
    return 4 * st_layout(B, max_nodes, D).total;
}

extern "C" int mpb_strrt_init(void* workspace, size_t workspace_bytes, const float* start, const float* goal, const float* w, const float* geom,
                              int geom_flags, const float* moving, int B, int max_nodes, int D, int n_rows, void* stream) {
    const char* who = "mpb_strrt_init";
    int rc = strrt_shape_check(who, B, max_nodes, D, n_rows);
    if (rc != MPB_OK || B == 0) return rc;
    StMoving mv;
    rc = strrt_scene_check(who, !workspace || !start || !goal || !w || !geom || !moving, workspace, geom, moving, workspace_bytes,
                           4 * st_layout(B, max_nodes, D).total, D, n_rows, mv);
    if (rc != MPB_OK) return rc;
    if (rrt_use_model(geom_flags, D))
        hipLaunchKernelGGL(strrt_init_kernel<PandaModel::ID>, dim3(B), dim3(64), 0, (hipStream_t)stream, (int*)workspace, start, goal, w, geom, mv, B, max_nodes, D, n_rows);
    else
        hipLaunchKernelGGL(strrt_init_kernel<0>, dim3(B), dim3(64), 0, (hipStream_t)stream, (int*)workspace, start, goal, w, geom, mv, B, max_nodes, D, n_rows);
    return mpb_check_launch(who);
}

extern "C" int mpb_strrt_run(void* workspace, size_t workspace_bytes, const float* geom, int geom_flags, const float* moving, const float* w,
                             const float* pre_samples, size_t pre_stride, const int* sample_idx, const int* sample_row, float* trajs,
                             float* vertex_q, int* vertex_row, int* n_vertices, int* status, int* log, int B, int max_nodes, int n_pre, int D,
                             int n_rows, int Lmax, int max_step_rows, int iter0, int n_iters, int total_iters, uint64_t seed,
                             uint32_t problem_offset, void* stream) {
    const char* who = "mpb_strrt_run";
    int rc = strrt_shape_check(who, B, max_nodes, D, n_rows);
    if (rc != MPB_OK) return rc;
    if (n_pre < 1 || n_pre > MPB_STRRT_MAX_PRE_SAMPLES) return mpb_failf(MPB_E_INVALID, "%s: n_pre = %d outside 1..MPB_STRRT_MAX_PRE_SAMPLES = %d", who, n_pre, MPB_STRRT_MAX_PRE_SAMPLES);
    if (Lmax < 2 || max_step_rows < 1 || iter0 < 0 || n_iters < 0 || total_iters < 0 || iter0 > total_iters || (double)B * Lmax * D > 2.0e9 ||
        (double)B * total_iters * MPB_STRRT_LOG_WORDS > 2.0e9)
        return mpb_failf(MPB_E_INVALID, "%s: bad Lmax / max_step_rows / iteration range", who);
    if ((sample_idx == nullptr) != (sample_row == nullptr)) return mpb_failf(MPB_E_INVALID, "%s: sample_idx and sample_row are given together or not at all", who);
    if (B == 0) return MPB_OK;
    StMoving mv;
    rc = strrt_scene_check(who, !workspace || !geom || !moving || !w || !pre_samples || !trajs || !vertex_q || !vertex_row || !n_vertices || !status,
                           workspace, geom, moving, workspace_bytes, 4 * st_layout(B, max_nodes, D).total, D, n_rows, mv);
    if (rc != MPB_OK) return rc;
    const StArgs a = {(int*)workspace, geom, mv, w, pre_samples, pre_stride, sample_idx, sample_row, trajs, vertex_q, vertex_row, n_vertices,
                      status, log, B, D, max_nodes, n_pre, n_rows, Lmax, max_step_rows, iter0, n_iters, total_iters, (uint32_t)seed,
                      (uint32_t)(seed >> 32), problem_offset};
    return rrt_dispatch<2, 3, 7>(geom_flags, D, [&](auto dt, auto model) {
        hipLaunchKernelGGL((strrt_kernel<dt.value, model.value>), dim3(B), dim3(64), 0, (hipStream_t)stream, a);
        return mpb_check_launch(who);
    });
}
