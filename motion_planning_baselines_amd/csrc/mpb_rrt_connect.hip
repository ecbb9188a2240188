// mpb_rrt_connect.hip -- batched RRT-Connect (rrt_connect.py:93-192 over rrt_base.py:94-119 and utils.py:4-50) and the
// stand-alone collision predicate it rests on.
//
// The reference fans n_trajectories independent RRT-Connect planners out over a process pool
// (multi_sample_based_planner.py); independent tree pairs are batch-parallel.  Here ONE persistent launch runs up to
// n_iters iterations for B problems, one single-wave workgroup per problem:
//   - workgroups never wait on each other, there is no spin wait, and every loop is bounded by n_iters, max_nodes, the
//     pool length or the point count of one extension;
//   - nearest node: the lanes stride over the tree's nodes, (distance, index) is reduced lexicographically (the lowest
//     index wins a tie, as torch.argmin does);
//   - extension (utils.py:4-14): one lane per point of the linspace, 64 points per trip, the first point in collision is
//     the count of trailing zeros of a ballot -- and the trips after it are never evaluated (safe_path only needs the
//     first one, utils.py:25-30);
//   - the trees (configurations padded to float4s, int32 parents) live in a caller-allocated global workspace; tree 0 is
//     rooted at the start, tree 1 at the goal, and the reference's name swap is one bit per problem (Q15: `continue`
//     leaves an iteration BEFORE the swap-back, so the roles do not simply alternate and a path can run goal -> start);
//   - the sample pool is a uint16 indirection list in LDS over the read-only pre_samples array; a reached target is
//     deleted order-preserving (rrt_base.py:59-63) by a parallel shift.
// Collision predicate (build-defined, torch_robotics being absent): a configuration is in collision iff the package's
// per-waypoint collision cost  sum_f s_f sum_l relu(margin + r_l - min_o sdf_o(x_l))  is positive; evaluated with the
// evaluators of mpb_geom.h (broad-phase grid where the field has one, the compile-time Panda model where geom_flags
// allows, the exhaustive walk otherwise; chained fields in turn).
#include "mpb_common.h"
#include "mpb_rrt.h"
#include "mpb_rrt_host.h"

#define RRT_WORDS_PER_NODE 32.0  // the size bound of rrt_shape_check: two trees, 16 words per node

struct RrtLayout {
    size_t hdr, nodes, parents, pool, total;   // offsets in 32-bit words
    int Dp, pool_words;
};

__host__ __device__ static inline RrtLayout rrt_layout(int B, int max_nodes, int n_pre, int D) {
    RrtLayout L;
    L.Dp = (D + 3) & ~3;
    L.pool_words = (n_pre + 1) / 2;
    L.hdr = MPB_RRT_GLOBAL_WORDS;
    L.nodes = L.hdr + (size_t)B * MPB_RRT_CONNECT_HDR_WORDS;
    L.parents = L.nodes + (size_t)B * 2 * max_nodes * L.Dp;
    L.pool = L.parents + (size_t)B * 2 * max_nodes;
    L.total = L.pool + (size_t)B * L.pool_words;
    return L;
}

// ---- stand-alone predicate: N configurations (N, D) -> flag (N) [and the hinge sum] --------------------------------
template <int MODEL>
__global__ __launch_bounds__(256) void collision_check_kernel(const float* __restrict__ q_in, const float* __restrict__ geom,
                                                              unsigned char* __restrict__ flag, float* __restrict__ gap, int N,
                                                              int D) {
    __shared__ unsigned gridw[MPB_GRID_MAX_CELLS];
    __shared__ float4 otab[MPB_GRID_MAX_SPH + 1];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const float* row = q_in + (size_t)min(i, N - 1) * D;
    float q[MPB_MAX_DOF];
    rrt_load_row<MPB_MAX_DOF>(row, D, q);
    const float* staged = nullptr;
    const float c = rrt_config_cost<MODEL>(geom, gridw, otab, staged, q);
    if (i < N) {
        flag[i] = (c > 0.f) ? 1 : 0;
        if (gap != nullptr) gap[i] = c;
    }
}

// ---- workspace initialisation: roots, counts, pool lists, status, start / goal collision check ---------------------
template <int MODEL>
__global__ __launch_bounds__(64) void rrt_init_kernel(int* __restrict__ ws, const float* __restrict__ start,
                                                      const float* __restrict__ goal, const float* __restrict__ geom, int B,
                                                      int max_nodes, int n_pre, int D) {
    __shared__ unsigned gridw[MPB_GRID_MAX_CELLS];
    __shared__ float4 otab[MPB_GRID_MAX_SPH + 1];
    const int b = blockIdx.x, lane = threadIdx.x;
    const RrtLayout L = rrt_layout(B, max_nodes, n_pre, D);
    unsigned* pool = reinterpret_cast<unsigned*>(ws) + L.pool + (size_t)b * L.pool_words;
    const int status = rrt_init_shared<MODEL>(ws, MPB_RRT_CONNECT_MAGIC, B, max_nodes, n_pre, D, L.Dp, pool, L.pool_words, start, goal,
                                              geom, gridw, otab, b, lane);
    float* nodes = reinterpret_cast<float*>(ws) + L.nodes + (size_t)b * 2 * max_nodes * L.Dp;
    int* parents = ws + L.parents + (size_t)b * 2 * max_nodes;
    if (lane < L.Dp) {
        nodes[lane] = (lane < D) ? start[(size_t)b * D + lane] : 0.f;
        nodes[(size_t)max_nodes * L.Dp + lane] = (lane < D) ? goal[(size_t)b * D + lane] : 0.f;
    }
    if (lane < 2) parents[(size_t)lane * max_nodes] = -1;
    if (lane < MPB_RRT_CONNECT_HDR_WORDS) {
        int* H = ws + L.hdr + (size_t)b * MPB_RRT_CONNECT_HDR_WORDS;
        int v = 0;
        if (lane == MPB_RRTC_STATUS) v = status;
        if (lane == MPB_RRTC_COUNTS || lane == MPB_RRTC_COUNTS + 1) v = 1;
        if (lane == MPB_RRTC_POOL_LEN) v = n_pre;
        H[lane] = v;
    }
}

// The squared distance of the padded tree row `row` to tq (node minus target, index order): RRT-Connect's nearest-node metric.
// Left under the build's contraction like rrt_dist of mpb_rrt.h (plain operators, no pragma): the compile-time-D instantiations
// of rrt_connect_kernel round the first product and take ONE fma per later term; rrt_connect_kernel<0, 0> fuses the first product
// onto the rounded second, fma(df0, df0, fl(df1 df1)), and takes ONE fma per later term.
template <int DM>
__device__ __forceinline__ float rrtc_row_d2(const float* row, int Dp, const float (&tq)[MPB_MAX_DOF]) {
    const float4* r = reinterpret_cast<const float4*>(row);
    float d2 = 0.f;
#pragma unroll
    for (int kk = 0; kk < (DM + 3) / 4; ++kk) {
        if (4 * kk < Dp) {
            const float4 v = r[kk];
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (4 * kk + c < DM) {
                    const float df = e[c] - tq[4 * kk + c];
                    d2 = d2 + df * df;
                }
            }
        }
    }
    return d2;
}

struct RrtArgs {
    int* ws;
    const float* geom;
    const float* pre;
    size_t pre_stride;
    const int* sample_idx;
    float* paths;
    int* lengths;
    int* status;
    int B, D, max_nodes, n_pre, Lmax, iter0, n_iters, total_iters;
    float step, radius;
    uint32_t seed_lo, seed_hi, problem_offset;
};

// ---- the persistent kernel ------------------------------------------------------------------------------------------
template <int DT, int MODEL>
__global__ __launch_bounds__(64) void rrt_connect_kernel(const RrtArgs a) {
#pragma clang fp contract(off)
    __shared__ unsigned gridw[MPB_GRID_MAX_CELLS];
    __shared__ float4 otab[MPB_GRID_MAX_SPH + 1];
    __shared__ unsigned short pool[MPB_RRT_MAX_PRE_SAMPLES];
    constexpr int DM = DT ? DT : MPB_MAX_DOF;
    const int D = DT ? DT : a.D;
    const int b = blockIdx.x, lane = threadIdx.x;
    const RrtLayout L = rrt_layout(a.B, a.max_nodes, a.n_pre, D);
    int* H = a.ws + L.hdr + (size_t)b * MPB_RRT_CONNECT_HDR_WORDS;
    int status = H[MPB_RRTC_STATUS];
    if (status != MPB_RRT_RUNNING) {                       // block-uniform: a finished problem costs nothing
        if (lane == 0) a.status[b] = status;
        return;
    }
    int cnt[2] = {H[MPB_RRTC_COUNTS], H[MPB_RRTC_COUNTS + 1]};
    int bit = H[MPB_RRTC_SWAP], plen = H[MPB_RRTC_POOL_LEN];
    float* nodes_b = reinterpret_cast<float*>(a.ws) + L.nodes + (size_t)b * 2 * a.max_nodes * L.Dp;
    int* parents_b = a.ws + L.parents + (size_t)b * 2 * a.max_nodes;
    unsigned short* pool_g = reinterpret_cast<unsigned short*>(a.ws + L.pool + (size_t)b * L.pool_words);
    for (int i = lane; i < plen; i += 64) pool[i] = pool_g[i];
    const float* pre_b = a.pre + (size_t)b * a.pre_stride;
    float* path_b = a.paths + (size_t)b * a.Lmax * D;
    const float* staged = nullptr;
    __syncthreads();

    // one extension (extend_path + safe_path + the append): grows tree t from its node nearest to `tq` towards `tq`;
    // returns false when the extension's first point is in collision (safe_path's []) or the tree is full
    float nq[MPB_MAX_DOF];
    auto extend = [&](int t, const float (&tq)[MPB_MAX_DOF]) -> bool {
        const float* nd = nodes_b + (size_t)t * a.max_nodes * L.Dp;
        const int n = cnt[t];
        float best = 3.0e38f;
        int bi = 0x7FFFFFFF;
        for (int i = lane; i < n; i += 64) {
            const float ds = sqrtf(rrtc_row_d2<DM>(nd + (size_t)i * L.Dp, L.Dp, tq));
            if (ds < best) { best = ds; bi = i; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float od = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (od < best || (od == best && oi < bi)) { best = od; bi = oi; }
        }
        const float dist = best;
        float q1[MPB_MAX_DOF], dl[MPB_MAX_DOF];
        const float f = (dist > a.radius) ? a.radius / dist : 1.0f;
#pragma unroll
        for (int k = 0; k < MPB_MAX_DOF; ++k) {
            q1[k] = (k < DM && k < D) ? nd[(size_t)bi * L.Dp + k] : 0.f;
            const float df = tq[k] - q1[k];
            // (utils.py:7-8: the far end clamped to n_radius; the point count below is from the UNCLAMPED distance)
            const float q2 = (dist > a.radius) ? fmaf(df, f, q1[k]) : tq[k];
            dl[k] = q2 - q1[k];
        }
        const int n_pts = rrt_point_count(dist, a.step);
        const float lstep = 1.0f / (float)(n_pts - 1);
        const int first = rrt_first_collision<DM, MODEL>(a.geom, gridw, otab, staged, q1, dl, n_pts, lstep, lane);
        if (first == 0) return false;
        rrt_linspace_point<DM>(q1, dl, n_pts, lstep, first < 0 ? n_pts - 1 : first - 1, nq);
        if (n >= a.max_nodes) {
            status = MPB_RRT_TREE_FULL;
            return false;
        }
        float* dst = nodes_b + ((size_t)t * a.max_nodes + n) * L.Dp;
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < DM; ++k) v = (lane == k) ? nq[k] : v;
        if (lane < L.Dp) dst[lane] = v;
        if (lane == 0) parents_b[(size_t)t * a.max_nodes + n] = bi;
        cnt[t] = n + 1;
        __syncthreads();                                   // the node is read back by the next nearest-node scan
        return true;
    };

    int it = a.iter0;
    const int it_end = min(a.iter0 + a.n_iters, a.total_iters);
    for (; it < it_end && status == MPB_RRT_RUNNING; ++it) {
        if (plen == 0) { status = MPB_RRT_POOL_EMPTY; break; }
        bit ^= 1;                                          // rrt_connect.py:126-128
        const int t1 = bit, t2 = bit ^ 1;
        int idx;
        if (a.sample_idx != nullptr) {
            idx = a.sample_idx[(size_t)b * a.total_iters + it];
            idx = min(max(idx, 0), plen - 1);
        } else {
            const uint4 r = philox4x32_10(make_uint4(a.problem_offset + (uint32_t)b, (uint32_t)it, MPB_RRT_CONNECT_MAGIC, 0u),
                                          make_uint2(a.seed_lo, a.seed_hi));
            idx = (int)__umulhi(r.x, (uint32_t)plen);
        }
        const float* trow = pre_b + (size_t)pool[idx] * D;
        float tq[MPB_MAX_DOF];
#pragma unroll
        for (int k = 0; k < MPB_MAX_DOF; ++k) tq[k] = (k < DM && k < D) ? trow[k] : 0.f;
        if (!extend(t1, tq)) continue;                     // :142-143 -- BEFORE the swap-back (Q15)
        float n1[MPB_MAX_DOF];
        bool reached = true;
#pragma unroll
        for (int k = 0; k < MPB_MAX_DOF; ++k) {
            n1[k] = nq[k];
            if (k < DM && k < D) reached = reached && rrt_close(n1[k], tq[k]);
        }
        if (reached) {                                     // :149-150, rrt_base.py:59-63: delete entry idx, keep the order
            rrt_pool_delete(pool, idx, plen, lane);
            --plen;
        }
        if (!extend(t2, n1)) continue;                     // :161-162
        bit ^= 1;                                          // :168-170
        bool joined = true;
#pragma unroll
        for (int k = 0; k < MPB_MAX_DOF; ++k)
            if (k < DM && k < D) joined = joined && rrt_close(n1[k], nq[k]);
        if (!joined) continue;
        // ---- :173-185: retrace(n2)[:-1] + reversed(retrace(n1)), then purge_duplicates_from_traj (utils.py:33-50)
        const float* ndA = nodes_b + (size_t)t2 * a.max_nodes * L.Dp;
        const float* ndB = nodes_b + (size_t)t1 * a.max_nodes * L.Dp;
        const int* paA = parents_b + (size_t)t2 * a.max_nodes;
        const int* paB = parents_b + (size_t)t1 * a.max_nodes;
        int lenA = 0, lenB = 0;
        for (int j = paA[cnt[t2] - 1]; j >= 0 && lenA < cnt[t2]; j = paA[j]) ++lenA;
        for (int j = cnt[t1] - 1; j >= 0 && lenB < cnt[t1]; j = paB[j]) ++lenB;
        const int Lraw = lenA + lenB;
        ++it;
        if (Lraw > a.Lmax) { status = MPB_RRT_PATH_TOO_LONG; break; }
        {
            int pos = lenA - 1;
            for (int j = paA[cnt[t2] - 1]; j >= 0 && pos >= 0; j = paA[j], --pos)
                if (lane < D) path_b[(size_t)pos * D + lane] = ndA[(size_t)j * L.Dp + lane];
            pos = lenA;
            for (int j = cnt[t1] - 1; j >= 0 && pos < Lraw; j = paB[j], ++pos)
                if (lane < D) path_b[(size_t)pos * D + lane] = ndB[(size_t)j * L.Dp + lane];
        }
        __syncthreads();
        const int len = rrt_purge(path_b, Lraw, D, lane);
        if (lane == 0) a.lengths[b] = len;
        status = MPB_RRT_FOUND;
        break;
    }
    if (status == MPB_RRT_RUNNING && it >= a.total_iters) status = MPB_RRT_EXHAUSTED_ITERS;
    __syncthreads();
    for (int i = lane; i < plen; i += 64) pool_g[i] = pool[i];
    if (lane == 0) {
        H[MPB_RRTC_STATUS] = status; H[MPB_RRTC_ITERS] = it; H[MPB_RRTC_COUNTS] = cnt[0]; H[MPB_RRTC_COUNTS + 1] = cnt[1];
        H[MPB_RRTC_SWAP] = bit; H[MPB_RRTC_POOL_LEN] = plen;
        a.status[b] = status;
    }
}

// ---- host side (the checks: mpb_rrt_host.h) -------------------------------------------------------------------------
extern "C" size_t mpb_rrt_connect_workspace_bytes(int B, int max_nodes, int n_pre, int D) {
    if (rrt_shape_check("mpb_rrt_connect_workspace_bytes", RRT_WORDS_PER_NODE, B, max_nodes, n_pre, D) != MPB_OK) return 0;
    return 4 * rrt_layout(B, max_nodes, n_pre, D).total;
}

extern "C" int mpb_rrt_connect_init(void* workspace, size_t workspace_bytes, const float* start, const float* goal,
                                    const float* geom, int geom_flags, int B, int max_nodes, int n_pre, int D, void* stream) {
    const int rc = rrt_init_check("mpb_rrt_connect_init", RRT_WORDS_PER_NODE, B, max_nodes, n_pre, D, !workspace || !start || !goal || !geom, false,
                                  workspace, geom, workspace_bytes, 4 * rrt_layout(B, max_nodes, n_pre, D).total);
    if (rc != MPB_OK || B == 0) return rc;
    if (rrt_use_model(geom_flags, D))
        hipLaunchKernelGGL(rrt_init_kernel<PandaModel::ID>, dim3(B), dim3(64), 0, (hipStream_t)stream, (int*)workspace, start, goal, geom, B, max_nodes, n_pre, D);
    else
        hipLaunchKernelGGL(rrt_init_kernel<0>, dim3(B), dim3(64), 0, (hipStream_t)stream, (int*)workspace, start, goal, geom, B, max_nodes, n_pre, D);
    return mpb_check_launch("mpb_rrt_connect_init");
}

extern "C" int mpb_rrt_connect_run(void* workspace, size_t workspace_bytes, const float* geom, int geom_flags,
                                   const float* pre_samples, size_t pre_stride, const int* sample_idx, float* paths,
                                   int* lengths, int* status, int B, int max_nodes, int n_pre, int D, int Lmax, int iter0,
                                   int n_iters, int total_iters, float step_size, float n_radius, uint64_t seed,
                                   uint32_t problem_offset, void* stream) {
    int rc = rrt_init_check("mpb_rrt_connect_run", RRT_WORDS_PER_NODE, B, max_nodes, n_pre, D, !workspace || !geom || !pre_samples || !paths || !lengths || !status,
                            false, workspace, geom, workspace_bytes, 4 * rrt_layout(B, max_nodes, n_pre, D).total);
    if (rc == MPB_OK) rc = rrt_run_check("mpb_rrt_connect_run", Lmax, iter0, n_iters, total_iters, true, step_size, n_radius);
    if (rc != MPB_OK || B == 0) return rc;
    const RrtArgs a = {(int*)workspace, geom, pre_samples, pre_stride, sample_idx, paths, lengths, status, B, D, max_nodes, n_pre, Lmax,
                       iter0, n_iters, total_iters, step_size, n_radius, (uint32_t)seed, (uint32_t)(seed >> 32), problem_offset};
    return rrt_dispatch<2, 3, 7>(geom_flags, D, [&](auto dt, auto model) {
        hipLaunchKernelGGL((rrt_connect_kernel<dt.value, model.value>), dim3(B), dim3(64), 0, (hipStream_t)stream, a);
        return mpb_check_launch("mpb_rrt_connect_run");
    });
}

extern "C" int mpb_collision_check(const float* q, const float* geom, int geom_flags, unsigned char* in_collision, float* gap,
                                   int N, int D, void* stream) {
    if (D > MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "mpb_collision_check: D = %d exceeds MPB_MAX_DOF = %d", D, MPB_MAX_DOF);
    if (N < 0 || D < 1) return mpb_fail(MPB_E_INVALID, "mpb_collision_check: bad shape");
    if (N == 0) return MPB_OK;
    if (!q || !geom || !in_collision) return mpb_fail(MPB_E_INVALID, "mpb_collision_check: null pointer");
    if (mpb_misaligned16(geom)) return mpb_fail(MPB_E_INVALID, "mpb_collision_check: geom must be 16-byte aligned");
    const dim3 grid((N + 255) / 256);
    if (rrt_use_model(geom_flags, D))
        hipLaunchKernelGGL(collision_check_kernel<PandaModel::ID>, grid, dim3(256), 0, (hipStream_t)stream, q, geom, in_collision, gap, N, D);
    else
        hipLaunchKernelGGL(collision_check_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, q, geom, in_collision, gap, N, D);
    return mpb_check_launch("mpb_collision_check");
}
