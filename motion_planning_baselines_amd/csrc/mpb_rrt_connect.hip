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
// On a world (mpb_world.h: obstacles OR SDF grid OR the robot against itself) the same tree is grown by rrtc_world_init_kernel /
// rrtc_world_kernel, and world_check_kernel is the world predicate stand-alone: the *_world entries at the end of this file.
#include "mpb_common.h"
#include "mpb_rrt.h"
#include "mpb_rrt_host.h"
#include "mpb_world.h"
#include "mpb_world_host.h"

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

// ---- the world predicate (mpb_world.h) stand-alone: flag (N) and the three parts (N, 3) = (c_obs, c_sdf, c_self), one lane per
// configuration, single-wave workgroups (the self block is per wave).  WORLD == 0 serves a call without either buffer.
template <int MODEL, int WORLD>
__global__ __launch_bounds__(64) void world_check_kernel(const float* __restrict__ q_in, const float* __restrict__ geom, const WorldArgs w,
                                                         unsigned char* __restrict__ flag, float* __restrict__ parts, int N, int D) {
    __shared__ unsigned gridw[MPB_GRID_MAX_CELLS];
    __shared__ float4 otab[MPB_GRID_MAX_SPH + 1];
    extern __shared__ __align__(16) float world_lds[];
    const int i = blockIdx.x * 64 + threadIdx.x;
    const float* row = q_in + (size_t)min(i, N - 1) * D;
    float q[MPB_MAX_DOF];
    rrt_load_row<MPB_MAX_DOF>(row, D, q);
    const float* staged = nullptr;
    const WorldView W = world_view(geom, w, world_lds);
    const WorldCost c = world_config_cost<MODEL, WORLD>(W, gridw, otab, staged, q);
    if (i < N) {
        flag[i] = world_hit(c) ? 1 : 0;
        if (parts != nullptr) {
            parts[3 * (size_t)i] = c.obs;
            parts[3 * (size_t)i + 1] = c.sdf;
            parts[3 * (size_t)i + 2] = c.self;
        }
    }
}

// ---- workspace initialisation: roots, counts, pool lists, status, start / goal collision check ---------------------
// (the body of rrt_init_kernel and of its world form rrtc_world_init_kernel; W: null with WORLD == 0)
template <int MODEL, int WORLD>
__device__ __forceinline__ void rrt_init_body(int* __restrict__ ws, const float* __restrict__ start, const float* __restrict__ goal,
                                              const float* __restrict__ geom, int B, int max_nodes, int n_pre, int D, const WorldView* W) {
    __shared__ unsigned gridw[MPB_GRID_MAX_CELLS];
    __shared__ float4 otab[MPB_GRID_MAX_SPH + 1];
    const int b = blockIdx.x, lane = threadIdx.x;
    const RrtLayout L = rrt_layout(B, max_nodes, n_pre, D);
    unsigned* pool = reinterpret_cast<unsigned*>(ws) + L.pool + (size_t)b * L.pool_words;
    const int status = rrt_init_shared<MODEL, WORLD>(ws, MPB_RRT_CONNECT_MAGIC, B, max_nodes, n_pre, D, L.Dp, pool, L.pool_words, start, goal,
                                                     geom, gridw, otab, b, lane, W);
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

template <int MODEL>
__global__ __launch_bounds__(64) void rrt_init_kernel(int* __restrict__ ws, const float* __restrict__ start,
                                                      const float* __restrict__ goal, const float* __restrict__ geom, int B,
                                                      int max_nodes, int n_pre, int D) {
    rrt_init_body<MODEL, 0>(ws, start, goal, geom, B, max_nodes, n_pre, D, nullptr);
}

// the same on a world: the start / goal check is the world predicate (a refused header puts every problem in START_OR_GOAL_IN_COLLISION)
template <int MODEL>
__global__ __launch_bounds__(64) void rrtc_world_init_kernel(int* __restrict__ ws, const float* __restrict__ start,
                                                             const float* __restrict__ goal, const float* __restrict__ geom, int B,
                                                             int max_nodes, int n_pre, int D, const WorldArgs w) {
    extern __shared__ __align__(16) float world_lds[];
    const WorldView W = world_view(geom, w, world_lds);
    rrt_init_body<MODEL, 1>(ws, start, goal, geom, B, max_nodes, n_pre, D, &W);
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
// (its body is mpb_rrt_connect_loop.h, which says why it is text included by both kernels)
template <int DT, int MODEL>
__global__ __launch_bounds__(64) void rrt_connect_kernel(const RrtArgs a) {
    const WorldView* W = nullptr;
    {
#define RRT_WORLD 0
#include "mpb_rrt_connect_loop.h"
#undef RRT_WORLD
    }
}

// the same tree on a world: every extension point is decided by the world predicate (mpb_world.h); the self blocks are dynamic LDS
template <int DT, int MODEL>
__global__ __launch_bounds__(64) void rrtc_world_kernel(const RrtArgs a, const WorldArgs w) {
    extern __shared__ __align__(16) float world_lds[];
    const WorldView Wv = world_view(a.geom, w, world_lds);
    const WorldView* W = &Wv;
    {
#define RRT_WORLD 1
#include "mpb_rrt_connect_loop.h"
#undef RRT_WORLD
    }
}

// ---- host side (the checks: mpb_rrt_host.h) -------------------------------------------------------------------------
extern "C" size_t mpb_rrt_connect_workspace_bytes(int B, int max_nodes, int n_pre, int D) {
    if (rrt_shape_check("mpb_rrt_connect_workspace_bytes", RRT_WORDS_PER_NODE, B, max_nodes, n_pre, D) != MPB_OK) return 0;
    return 4 * rrt_layout(B, max_nodes, n_pre, D).total;
}

// both forms of *_init and *_run: the old entry's checks under the name `who`, then (a buffer given) world_args and the world kernels
static int rrt_connect_init_impl(const char* who, void* workspace, size_t workspace_bytes, const float* start, const float* goal,
                                 const float* geom, int geom_flags, const float* sdfb, const float* selfb, int B, int max_nodes, int n_pre,
                                 int D, void* stream) {
    int rc = rrt_init_check(who, RRT_WORDS_PER_NODE, B, max_nodes, n_pre, D, !workspace || !start || !goal || !geom, false, workspace, geom,
                            workspace_bytes, 4 * rrt_layout(B, max_nodes, n_pre, D).total);
    if (rc != MPB_OK || B == 0) return rc;
    if (!world_present(sdfb, selfb)) {
        if (rrt_use_model(geom_flags, D))
            hipLaunchKernelGGL(rrt_init_kernel<PandaModel::ID>, dim3(B), dim3(64), 0, (hipStream_t)stream, (int*)workspace, start, goal, geom, B, max_nodes, n_pre, D);
        else
            hipLaunchKernelGGL(rrt_init_kernel<0>, dim3(B), dim3(64), 0, (hipStream_t)stream, (int*)workspace, start, goal, geom, B, max_nodes, n_pre, D);
        return mpb_check_launch(who);
    }
    WorldArgs w;
    if ((rc = world_args(who, sdfb, selfb, D, w))) return rc;
    const size_t lds = world_self_lds_bytes(w, 1);
    return rrt_dispatch<>(geom_flags, D, [&](auto, auto model) {
        const int rl = mpb_raise_lds_limit(rrtc_world_init_kernel<model.value>, lds, who);
        if (rl) return rl;
        hipLaunchKernelGGL(rrtc_world_init_kernel<model.value>, dim3(B), dim3(64), lds, (hipStream_t)stream, (int*)workspace, start, goal, geom, B,
                           max_nodes, n_pre, D, w);
        return mpb_check_launch(who);
    });
}

static int rrt_connect_run_impl(const char* who, void* workspace, size_t workspace_bytes, const float* geom, int geom_flags, const float* sdfb,
                                const float* selfb, const float* pre_samples, size_t pre_stride, const int* sample_idx, float* paths,
                                int* lengths, int* status, int B, int max_nodes, int n_pre, int D, int Lmax, int iter0, int n_iters,
                                int total_iters, float step_size, float n_radius, uint64_t seed, uint32_t problem_offset, void* stream) {
    int rc = rrt_init_check(who, RRT_WORDS_PER_NODE, B, max_nodes, n_pre, D, !workspace || !geom || !pre_samples || !paths || !lengths || !status,
                            false, workspace, geom, workspace_bytes, 4 * rrt_layout(B, max_nodes, n_pre, D).total);
    if (rc == MPB_OK) rc = rrt_run_check(who, Lmax, iter0, n_iters, total_iters, true, step_size, n_radius);
    if (rc != MPB_OK || B == 0) return rc;
    const RrtArgs a = {(int*)workspace, geom, pre_samples, pre_stride, sample_idx, paths, lengths, status, B, D, max_nodes, n_pre, Lmax,
                       iter0, n_iters, total_iters, step_size, n_radius, (uint32_t)seed, (uint32_t)(seed >> 32), problem_offset};
    if (!world_present(sdfb, selfb))
        return rrt_dispatch<2, 3, 7>(geom_flags, D, [&](auto dt, auto model) {
            hipLaunchKernelGGL((rrt_connect_kernel<dt.value, model.value>), dim3(B), dim3(64), 0, (hipStream_t)stream, a);
            return mpb_check_launch(who);
        });
    WorldArgs w;
    if ((rc = world_args(who, sdfb, selfb, D, w))) return rc;
    const size_t lds = world_self_lds_bytes(w, 1);
    // (the world kernel is instantiated for the compile-time Panda and for run-time D: DESIGN.md 10)
    return rrt_dispatch<>(geom_flags, D, [&](auto dt, auto model) {
        const int rl = mpb_raise_lds_limit(rrtc_world_kernel<dt.value, model.value>, lds, who);
        if (rl) return rl;
        hipLaunchKernelGGL((rrtc_world_kernel<dt.value, model.value>), dim3(B), dim3(64), lds, (hipStream_t)stream, a, w);
        return mpb_check_launch(who);
    });
}

extern "C" int mpb_rrt_connect_init(void* workspace, size_t workspace_bytes, const float* start, const float* goal,
                                    const float* geom, int geom_flags, int B, int max_nodes, int n_pre, int D, void* stream) {
    return rrt_connect_init_impl(__func__, workspace, workspace_bytes, start, goal, geom, geom_flags, nullptr, nullptr, B, max_nodes, n_pre, D, stream);
}

extern "C" int mpb_rrt_connect_init_world(void* workspace, size_t workspace_bytes, const float* start, const float* goal,
                                          const float* geom, int geom_flags, const float* sdfb, const float* selfb, int B, int max_nodes,
                                          int n_pre, int D, void* stream) {
    return rrt_connect_init_impl(__func__, workspace, workspace_bytes, start, goal, geom, geom_flags, sdfb, selfb, B, max_nodes, n_pre, D, stream);
}

extern "C" int mpb_rrt_connect_run(void* workspace, size_t workspace_bytes, const float* geom, int geom_flags,
                                   const float* pre_samples, size_t pre_stride, const int* sample_idx, float* paths,
                                   int* lengths, int* status, int B, int max_nodes, int n_pre, int D, int Lmax, int iter0,
                                   int n_iters, int total_iters, float step_size, float n_radius, uint64_t seed,
                                   uint32_t problem_offset, void* stream) {
    return rrt_connect_run_impl(__func__, workspace, workspace_bytes, geom, geom_flags, nullptr, nullptr, pre_samples, pre_stride, sample_idx, paths,
                                lengths, status, B, max_nodes, n_pre, D, Lmax, iter0, n_iters, total_iters, step_size, n_radius, seed,
                                problem_offset, stream);
}

extern "C" int mpb_rrt_connect_run_world(void* workspace, size_t workspace_bytes, const float* geom, int geom_flags, const float* sdfb,
                                         const float* selfb, const float* pre_samples, size_t pre_stride, const int* sample_idx,
                                         float* paths, int* lengths, int* status, int B, int max_nodes, int n_pre, int D, int Lmax,
                                         int iter0, int n_iters, int total_iters, float step_size, float n_radius, uint64_t seed,
                                         uint32_t problem_offset, void* stream) {
    return rrt_connect_run_impl(__func__, workspace, workspace_bytes, geom, geom_flags, sdfb, selfb, pre_samples, pre_stride, sample_idx, paths,
                                lengths, status, B, max_nodes, n_pre, D, Lmax, iter0, n_iters, total_iters, step_size, n_radius, seed,
                                problem_offset, stream);
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

extern "C" int mpb_world_collision_check(const float* q, const float* geom, int geom_flags, const float* sdfb, const float* selfb,
                                         unsigned char* in_collision, float* parts, int N, int D, void* stream) {
    if (D > MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "%s: D = %d exceeds MPB_MAX_DOF = %d", __func__, D, MPB_MAX_DOF);
    if (N < 0 || D < 1) return mpb_failf(MPB_E_INVALID, "%s: bad shape", __func__);
    if (N == 0) return MPB_OK;
    if (!q || !geom || !in_collision) return mpb_failf(MPB_E_INVALID, "%s: null pointer", __func__);
    if (mpb_misaligned16(geom)) return mpb_failf(MPB_E_INVALID, "%s: geom must be 16-byte aligned", __func__);
    WorldArgs w = {};
    w.n_dof = D;
    const dim3 grid((N + 63) / 64);
    if (!world_present(sdfb, selfb))
        return rrt_dispatch<>(geom_flags, D, [&](auto, auto model) {
            hipLaunchKernelGGL((world_check_kernel<model.value, 0>), grid, dim3(64), 0, (hipStream_t)stream, q, geom, w, in_collision, parts, N, D);
            return mpb_check_launch("mpb_world_collision_check");
        });
    const int rc = world_args(__func__, sdfb, selfb, D, w);
    if (rc) return rc;
    const size_t lds = world_self_lds_bytes(w, 1);
    return rrt_dispatch<>(geom_flags, D, [&](auto, auto model) {
        const int rl = mpb_raise_lds_limit(world_check_kernel<model.value, 1>, lds, "mpb_world_collision_check");
        if (rl) return rl;
        hipLaunchKernelGGL((world_check_kernel<model.value, 1>), grid, dim3(64), lds, (hipStream_t)stream, q, geom, w, in_collision, parts, N, D);
        return mpb_check_launch("mpb_world_collision_check");
    });
}
