// mpb_prm.hip -- the roadmap planner's three kernels (PRM: one graph of collision-free configurations, many start / goal queries;
// the reference has no roadmap planner -- the semantics are build-defined, include/mpb.h and DESIGN.md 10):
//   mpb_prm_knn         the K nearest nodes of every query row, brute force: one single-wave workgroup per query, the node rows staged
//                       through LDS in tiles of 64, the query's M distance keys in LDS, K rounds of a wave arg-min over (d2, index);
//   mpb_prm_edge_check  one wave per edge, one lane per point: the segment scan of mpb_path_shortcut (the sequential fp32 distance,
//                       dist / check_step + 2 points, rrt_linspace_point, rrt_first_collision with rrt_config_cost > 0: mpb_rrt.h);
//   mpb_prm_query       one workgroup per query: the M tentative costs in LDS, sweeps of both-way relaxations to the fixed point,
//                       then the predecessors from the converged costs alone and the walk back.  No geometry.
//   - workgroups never wait on each other; every loop is bounded by M, K, Lmax or the point count of one edge;
//   - the distances are ordered and the costs relaxed as unsigned integers on their bits: a non-negative float orders as its bits do, the
//     build assumes finite math and +inf is a value here, and an LDS atomic min on the bits is exact.  The relaxation order of a sweep is
//     not fixed, the fixed point is: fl(d + w) is monotone in d, so every run ends with the same bits;
//   - the arithmetic of this file is rounded after every operation: plain operators under #pragma clang fp contract(off) (what it calls
//     in mpb_rrt.h is what stands there: rrt_d2_rounded rounds alike, rrt_linspace_point says fmaf where it takes one rounding).
#include "mpb_common.h"
#include "mpb_rrt.h"
#include "mpb_rrt_host.h"

#define PRM_INF_BITS 0x7F800000u                             // +inf; a weight or a cost is FINITE iff its bits are below this (sign clear)
#define PRM_QUERY_THREADS 256
#define PRM_NO_PRED 0xFFFFFFFFu

// the key a d2 (rrt_d2_rounded of mpb_rrt.h) is ordered by: its bits (d2 is a sum of squares: never negative), a NaN as +inf
__device__ __forceinline__ unsigned prm_key(float d2) { return min(__float_as_uint(d2) & 0x7FFFFFFFu, PRM_INF_BITS); }

// ---- 1. k nearest nodes ---------------------------------------------------------------------------------------------------------------
struct PrmKnnArgs {
    const float* queries;
    const float* nodes;
    int* idx;
    float* dist;
    int M, D, K, exclude_self;
};

template <int DT>
__global__ __launch_bounds__(64) void prm_knn_kernel(const PrmKnnArgs a) {
#pragma clang fp contract(off)
    __shared__ float tile[64 * MPB_MAX_DOF];                // 64 node rows as they lie in memory
    extern __shared__ unsigned prm_keys[];                  // (M,) the query's distance keys
    constexpr int DM = DT ? DT : MPB_MAX_DOF;
    const int D = DT ? DT : a.D;
    const int i = blockIdx.x, lane = threadIdx.x, M = a.M;
    float q[MPB_MAX_DOF], x[MPB_MAX_DOF];
    rrt_load_row<DM>(a.queries + (size_t)i * D, D, q);
    for (int base = 0; base < M; base += 64) {
        const int rows = min(64, M - base);
        __syncthreads();
        for (int t = lane; t < rows * D; t += 64) tile[t] = a.nodes[(size_t)base * D + t];
        __syncthreads();
        const int j = base + lane;
        if (lane < rows) {
            rrt_load_row<DM>(tile + lane * D, D, x);
            prm_keys[j] = (a.exclude_self && j == i) ? 0xFFFFFFFFu : prm_key(rrt_d2_rounded<DM>(q, x));
        }
    }
    __syncthreads();
    // round r: the smallest (key, index) not below `from`, the one after round r - 1's; lane r keeps it
    unsigned long long from = 0ull, mine = 0ull;
    for (int r = 0; r < a.K; ++r) {
        unsigned long long best = ~0ull;
        for (int j = lane; j < M; j += 64) {
            const unsigned long long c = ((unsigned long long)prm_keys[j] << 32) | (unsigned)j;
            best = (c >= from && c < best) ? c : best;
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const unsigned long long o = __shfl_xor(best, s, 64);
            best = o < best ? o : best;
        }
        mine = (lane == r) ? best : mine;
        from = best + 1ull;
    }
    if (lane < a.K) {
        a.idx[(size_t)i * a.K + lane] = (int)(unsigned)(mine & 0xFFFFFFFFull);
        a.dist[(size_t)i * a.K + lane] = sqrtf(__uint_as_float((unsigned)(mine >> 32)));
    }
}

// ---- 2. edge check --------------------------------------------------------------------------------------------------------------------
struct PrmEdgeArgs {
    const float* pts;
    const int* pairs;
    const float* geom;
    int* flag;
    int* first;
    int P, E, D;
    float step;
};

template <int DT, int MODEL>
__global__ __launch_bounds__(64) void prm_edge_kernel(const PrmEdgeArgs a) {
#pragma clang fp contract(off)
    __shared__ unsigned gridw[MPB_GRID_MAX_CELLS];
    __shared__ float4 otab[MPB_GRID_MAX_SPH + 1];
    constexpr int DM = DT ? DT : MPB_MAX_DOF;
    const int D = DT ? DT : a.D;
    const int lane = threadIdx.x;
    const float* staged = nullptr;                          // (the grid stays staged from one edge of the workgroup to the next)
    for (int e = blockIdx.x; e < a.E; e += gridDim.x) {    // (block-uniform: every value below is the same in all 64 lanes)
        const int ia = a.pairs[2 * (size_t)e], ib = a.pairs[2 * (size_t)e + 1];
        int code = MPB_PRM_EDGE_FREE, first = -1;
        if (ia < 0 || ia >= a.P || ib < 0 || ib >= a.P) {
            code = MPB_PRM_EDGE_BAD_INDEX;
        } else {
            float p1[MPB_MAX_DOF], p2[MPB_MAX_DOF], dl[MPB_MAX_DOF];
            rrt_load_row<DM>(a.pts + (size_t)min(ia, ib) * D, D, p1);
            rrt_load_row<DM>(a.pts + (size_t)max(ia, ib) * D, D, p2);
            const float cntf = sqrtf(rrt_d2_rounded<DM>(p1, p2)) / a.step;
            // (on the bits: cntf is never negative, and a NaN or +inf counts as too long)
            if (!(__float_as_uint(cntf) < __float_as_uint((float)(RRT_MAX_PTS - 1)))) {
                code = MPB_PRM_EDGE_TOO_LONG;
            } else {
                const int n_pts = (int)cntf + 2;
                const float lstep = 1.0f / (float)(n_pts - 1);
#pragma unroll
                for (int k = 0; k < MPB_MAX_DOF; ++k) dl[k] = p2[k] - p1[k];
                first = rrt_first_collision<DM, MODEL>(a.geom, gridw, otab, staged, p1, dl, n_pts, lstep, lane);
                code = first >= 0 ? MPB_PRM_EDGE_BLOCKED : MPB_PRM_EDGE_FREE;
            }
        }
        if (lane == 0) {
            a.flag[e] = code;
            a.first[e] = first;
        }
    }
}

// ---- 3. queries against the roadmap ---------------------------------------------------------------------------------------------------
struct PrmQueryArgs {
    const float* nodes;
    const int* nbr;
    const float* w;
    const float* starts;
    const float* goals;
    const int* cs;
    const float* ws;
    const int* cg;
    const float* wg;
    const float* direct;
    float* paths;
    int* lengths;
    float* costs;
    int* status;
    int M, K, Kc, D, Lmax;
};

__device__ __forceinline__ bool prm_entry(unsigned wbits, int v, int M) { return wbits < PRM_INF_BITS && v >= 0 && v < M; }

// init[v]: the smallest finite ws entry that names v, +inf when none does (bits)
__device__ __forceinline__ unsigned prm_init_of(const int* __restrict__ cs, const float* __restrict__ ws, int Kc, int M, int v) {
    unsigned best = PRM_INF_BITS;
    for (int k = 0; k < Kc; ++k) {
        const unsigned wb = __float_as_uint(ws[k]);
        if (prm_entry(wb, cs[k], M) && cs[k] == v) best = min(best, wb);
    }
    return best;
}

__global__ __launch_bounds__(PRM_QUERY_THREADS) void prm_query_kernel(const PrmQueryArgs a) {
#pragma clang fp contract(off)
    extern __shared__ unsigned prm_lds[];                   // d (M,) the tentative costs' bits, then pred (M,)
    __shared__ int sh_status, sh_len;
    __shared__ unsigned sh_cost;
    unsigned* d = prm_lds;
    unsigned* pred = prm_lds + a.M;
    const int q = blockIdx.x, tid = threadIdx.x, M = a.M, K = a.K, Kc = a.Kc, D = a.D;
    const int* cs = a.cs + (size_t)q * Kc;
    const int* cg = a.cg + (size_t)q * Kc;
    const float* ws = a.ws + (size_t)q * Kc;
    const float* wg = a.wg + (size_t)q * Kc;
    float* path = a.paths + (size_t)q * a.Lmax * D;
    const unsigned direct = __float_as_uint(a.direct[q]);

    for (int v = tid; v < M; v += PRM_QUERY_THREADS) {
        d[v] = PRM_INF_BITS;
        pred[v] = PRM_NO_PRED;
    }
    if (tid == 0) {
        bool any_s = false, any_g = false;
        for (int k = 0; k < Kc; ++k) {
            any_s = any_s || prm_entry(__float_as_uint(ws[k]), cs[k], M);
            any_g = any_g || prm_entry(__float_as_uint(wg[k]), cg[k], M);
        }
        sh_status = direct < PRM_INF_BITS ? MPB_PRM_OK : !any_s ? MPB_PRM_NO_START : !any_g ? MPB_PRM_NO_GOAL : -1;
        sh_len = direct < PRM_INF_BITS ? 2 : 0;
        sh_cost = direct < PRM_INF_BITS ? direct : PRM_INF_BITS;
    }
    __syncthreads();
    if (sh_status < 0) {                                    // (block-uniform) the roadmap has to answer
        if (tid == 0)
            for (int k = 0; k < Kc; ++k) {
                const unsigned wb = __float_as_uint(ws[k]);
                if (prm_entry(wb, cs[k], M)) d[cs[k]] = min(d[cs[k]], wb);
            }
        __syncthreads();
        // sweeps: every finite table entry (i, nbr[i][k], w) relaxes both ways, until a sweep changes nothing (at most M of them)
        for (int sweep = 0; sweep < M; ++sweep) {
            int changed = 0;
            for (int t = tid; t < M * K; t += PRM_QUERY_THREADS) {
                const int i = t / K, j = a.nbr[t];
                const unsigned wb = __float_as_uint(a.w[t]);
                if (!prm_entry(wb, j, M)) continue;
                const float wf = __uint_as_float(wb);
                const unsigned di = d[i], dj = d[j];
                if (dj < PRM_INF_BITS) {
                    const unsigned c = __float_as_uint(__uint_as_float(dj) + wf);
                    if (c < di && atomicMin(&d[i], c) > c) changed = 1;
                }
                if (di < PRM_INF_BITS) {
                    const unsigned c = __float_as_uint(__uint_as_float(di) + wf);
                    if (c < dj && atomicMin(&d[j], c) > c) changed = 1;
                }
            }
            if (!__syncthreads_or(changed)) break;
        }
        // the predecessors, from the converged costs alone: the smallest-index neighbour u with fl(d[u] + w) == d[v] and d[u] < d[v]
        for (int t = tid; t < M * K; t += PRM_QUERY_THREADS) {
            const int i = t / K, j = a.nbr[t];
            const unsigned wb = __float_as_uint(a.w[t]);
            if (!prm_entry(wb, j, M)) continue;
            const float wf = __uint_as_float(wb);
            const unsigned di = d[i], dj = d[j];
            if (dj < di && __float_as_uint(__uint_as_float(dj) + wf) == di) atomicMin(&pred[i], (unsigned)j);
            if (di < dj && __float_as_uint(__uint_as_float(di) + wf) == dj) atomicMin(&pred[j], (unsigned)i);
        }
        __syncthreads();
        if (tid == 0) {
            // the goal's cost: min_k fl(d[cg_k] + wg_k), ties to the smallest k
            unsigned c = PRM_INF_BITS;
            int g = -1;
            for (int k = 0; k < Kc; ++k) {
                const unsigned wb = __float_as_uint(wg[k]);
                if (!prm_entry(wb, cg[k], M) || d[cg[k]] >= PRM_INF_BITS) continue;
                const unsigned ck = __float_as_uint(__uint_as_float(d[cg[k]]) + __uint_as_float(wb));
                if (ck < c) {
                    c = ck;
                    g = cg[k];
                }
            }
            int st = MPB_PRM_OK, n = 0;
            if (g < 0) {
                st = MPB_PRM_DISCONNECTED;
            } else if (a.Lmax < 3) {                        // (start, one node, goal)
                st = MPB_PRM_PATH_TOO_LONG;
            } else {
                // the walk back, twice: counted, then written (d falls strictly along it: it cannot loop, and Lmax bounds it)
                for (int pass = 0; pass < 2 && st == MPB_PRM_OK; ++pass) {
                    int v = g, pos = 1;
                    for (;;) {
                        if (pass == 1) {
                            const float* row = a.nodes + (size_t)v * D;
                            for (int k = 0; k < D; ++k) path[(size_t)(n - pos + 1) * D + k] = row[k];
                        }
                        if (prm_init_of(cs, ws, Kc, M, v) == d[v]) break;
                        const unsigned u = pred[v];
                        if (u == PRM_NO_PRED) {
                            st = MPB_PRM_DEGENERATE;
                            break;
                        }
                        if (pos + 3 > a.Lmax) {
                            st = MPB_PRM_PATH_TOO_LONG;
                            break;
                        }
                        v = (int)u;
                        ++pos;
                    }
                    n = pos;                                // nodes of the roadmap on the path
                }
            }
            sh_status = st;
            sh_len = st == MPB_PRM_OK ? n + 2 : 0;
            sh_cost = st == MPB_PRM_OK ? c : PRM_INF_BITS;
        }
        __syncthreads();
    }
    const int L = sh_len;
    // the start, the goal, and zeros at and past the length (the rows between are the walk's)
    for (int t = tid; t < a.Lmax * D; t += PRM_QUERY_THREADS) {
        const int r = t / D, k = t - r * D;
        if (r >= L) path[t] = 0.f;
        else if (r == 0) path[t] = a.starts[(size_t)q * D + k];
        else if (r == L - 1) path[t] = a.goals[(size_t)q * D + k];
    }
    if (tid == 0) {
        a.lengths[q] = L;
        a.costs[q] = __uint_as_float(sh_cost);
        a.status[q] = sh_status;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
// the shape and limit refusals the entry points share, in the order include/mpb.h gives them (rows: the count that may be 0)
static int prm_shape_check(const char* who, int rows, int D, int M, int K) {
    if (rows < 0 || D < 1) return mpb_failf(MPB_E_INVALID, "%s: bad shape (rows %d, D %d)", who, rows, D);
    if (D > MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "%s: D = %d exceeds MPB_MAX_DOF = %d", who, D, MPB_MAX_DOF);
    if (M > MPB_PRM_MAX_NODES) return mpb_failf(MPB_E_UNSUPPORTED, "%s: M = %d exceeds MPB_PRM_MAX_NODES = %d", who, M, MPB_PRM_MAX_NODES);
    if (K > MPB_PRM_MAX_K) return mpb_failf(MPB_E_UNSUPPORTED, "%s: K = %d exceeds MPB_PRM_MAX_K = %d", who, K, MPB_PRM_MAX_K);
    if (M < 2) return mpb_failf(MPB_E_INVALID, "%s: M = %d, a roadmap has at least 2 nodes", who, M);
    return MPB_OK;
}

extern "C" int mpb_prm_knn(const float* queries, const float* nodes, int* idx, float* dist, int Q, int M, int D, int K, int exclude_self,
                           void* stream) {
    const int rc = prm_shape_check("mpb_prm_knn", Q, D, M, K);
    if (rc) return rc;
    if (exclude_self != 0 && Q != M) return mpb_failf(MPB_E_INVALID, "mpb_prm_knn: exclude_self needs Q == M (Q %d, M %d)", Q, M);
    if (K < 1 || K > M - (exclude_self ? 1 : 0))
        return mpb_failf(MPB_E_INVALID, "mpb_prm_knn: K = %d outside 1 .. %d", K, M - (exclude_self ? 1 : 0));
    if (!queries || !nodes || !idx || !dist) return mpb_fail(MPB_E_INVALID, "mpb_prm_knn: null pointer");
    if (Q == 0) return MPB_OK;
    const PrmKnnArgs a = {queries, nodes, idx, dist, M, D, K, exclude_self ? 1 : 0};
    const size_t lds = (size_t)M * sizeof(unsigned);
    return rrt_dispatch<2, 3, 7>(0, D, [&](auto dt, auto) {                  // (no geometry: DT alone, never the model's branch)
        const int rl = mpb_raise_lds_limit(prm_knn_kernel<dt.value>, lds, "mpb_prm_knn");
        if (rl) return rl;
        hipLaunchKernelGGL((prm_knn_kernel<dt.value>), dim3(Q), dim3(64), lds, (hipStream_t)stream, a);
        return mpb_check_launch("mpb_prm_knn");
    });
}

extern "C" int mpb_prm_edge_check(const float* pts, const int* pairs, int* flag, int* first, const float* geom, int geom_flags, int P, int E,
                                  int D, float check_step, void* stream) {
    if (E < 0 || P < 1 || D < 1) return mpb_failf(MPB_E_INVALID, "mpb_prm_edge_check: bad shape (P %d, E %d, D %d)", P, E, D);
    if (D > MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "mpb_prm_edge_check: D = %d exceeds MPB_MAX_DOF = %d", D, MPB_MAX_DOF);
    if (mpb_bad_step(check_step)) return mpb_fail(MPB_E_INVALID, "mpb_prm_edge_check: check_step must be finite and positive");
    if (!pts || !pairs || !flag || !first || !geom) return mpb_fail(MPB_E_INVALID, "mpb_prm_edge_check: null pointer");
    if (mpb_misaligned16(geom)) return mpb_fail(MPB_E_INVALID, "mpb_prm_edge_check: geom must be 16-byte aligned");
    if (E == 0) return MPB_OK;
    const PrmEdgeArgs a = {pts, pairs, geom, flag, first, P, E, D, check_step};
    const int blocks = min(E, 8 * mpb_device_cu_count());
    return rrt_dispatch<2, 3, 7>(geom_flags, D, [&](auto dt, auto model) {
        hipLaunchKernelGGL((prm_edge_kernel<dt.value, model.value>), dim3(blocks), dim3(64), 0, (hipStream_t)stream, a);
        return mpb_check_launch("mpb_prm_edge_check");
    });
}

extern "C" int mpb_prm_query(const float* nodes, const int* nbr, const float* w, const float* starts, const float* goals, const int* cs,
                             const float* ws, const int* cg, const float* wg, const float* direct, float* paths, int* lengths, float* costs,
                             int* status, int Q, int M, int K, int Kc, int D, int Lmax, void* stream) {
    const int rc = prm_shape_check("mpb_prm_query", Q, D, M, K > Kc ? K : Kc);
    if (rc) return rc;
    if (K < 1 || Kc < 1) return mpb_failf(MPB_E_INVALID, "mpb_prm_query: K = %d and Kc = %d must be at least 1", K, Kc);
    if (Lmax < 2 || Lmax > MPB_PRM_MAX_PATH_ROWS) return mpb_failf(MPB_E_INVALID, "mpb_prm_query: Lmax = %d outside 2 .. %d", Lmax, MPB_PRM_MAX_PATH_ROWS);
    if (!nodes || !nbr || !w || !starts || !goals || !cs || !ws || !cg || !wg || !direct || !paths || !lengths || !costs || !status)
        return mpb_fail(MPB_E_INVALID, "mpb_prm_query: null pointer");
    if (Q == 0) return MPB_OK;
    const PrmQueryArgs a = {nodes, nbr, w, starts, goals, cs, ws, cg, wg, direct, paths, lengths, costs, status, M, K, Kc, D, Lmax};
    const size_t lds = 2 * (size_t)M * sizeof(unsigned);
    const int rl = mpb_raise_lds_limit(prm_query_kernel, lds, "mpb_prm_query");
    if (rl) return rl;
    hipLaunchKernelGGL(prm_query_kernel, dim3(Q), dim3(PRM_QUERY_THREADS), lds, (hipStream_t)stream, a);
    return mpb_check_launch("mpb_prm_query");
}
