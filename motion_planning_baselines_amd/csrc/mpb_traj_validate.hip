// mpb_traj_validate.hip -- which trajectories of a batch are collision-free, and where the others are not: what the
// reference's examples ask the planning task after a planner has run (task.get_trajs_collision_and_free,
// compute_fraction_free_trajs, compute_collision_intensity_trajs, compute_success_free_trajs; panda_spheres_CHOMP.py:126,
// :146-148; provider: torch_robotics, absent -- the semantics are build-defined).
//
// One launch, one workgroup of 256 threads per trajectory.  The threads stride over the P = (H - 1)(n_interp + 1) + 1
// dense points of the trajectory -- the points mpb_traj_interpolate defines, formed in registers from the two waypoints
// they lie between, never stored -- and evaluate the collision cost of each with rrt_config_cost (mpb_rrt.h): the
// predicate and the evaluators of mpb_collision_check.  The rows are read in place with the caller's stride (the (N, H, 2D)
// state output of a planner is read as it is; the columns past D are never touched).
//   - The waypoints are NOT staged in LDS: a point reads two rows of D floats, neighbouring lanes read the same or
//     the next row (one or two cache lines per wave, re-read from L1 by the next wave), and the evaluation that follows
//     -- forward kinematics and the obstacle walk -- is two orders of magnitude more work than the read.  A tile of H x D
//     floats would bound H by the LDS left over next to the 17 KB of the staged grid and buy nothing measurable.
//   - The trip count of the stride loop is block-uniform (rrt_config_cost holds __syncthreads() when it stages a grid; with
//     chained fields it restages on every trip); a lane past the last point evaluates the last point and is masked out.
//   - Reduction without atomics: ballot / popcount / count of trailing zeros per wave and trip, a wave max of the hinge
//     sums, then the four waves through LDS in wave order.  Integer sums and min / max of floats do not depend on the
//     order: the outputs are the same bits on every run.
//   - On a world (mpb_world.h) traj_stats_world_kernel runs the same body with the world predicate: 256 threads, or 64 where the world
//     holds a self buffer (one LDS block of sphere centres per wave; four of 64 spheres do not fit beside the staged grid).
#include <climits>

#include "mpb_common.h"
#include "mpb_rrt.h"
#include "mpb_rrt_host.h"
#include "mpb_world.h"
#include "mpb_world_host.h"

// (the body of traj_collision_stats_kernel and of its world form traj_stats_world_kernel.  WORLD == 0: 256 threads, W null.  On a world
// the workgroup has NT = blockDim.x threads -- 256, or 64 where the world holds a self buffer, whose LDS block is per wave: four blocks of
// 64 spheres would not fit beside the staged grid -- and max_gap is the largest SUM of the three parts.)
template <int MODEL, int WORLD>
__device__ __forceinline__ void traj_collision_stats_body(const float* __restrict__ trajs, size_t row_stride, const float* __restrict__ geom,
                                                          int* __restrict__ n_coll, int* __restrict__ first_coll,
                                                          float* __restrict__ max_gap, unsigned char* __restrict__ flag, int H, int D, int n1,
                                                          int P, const WorldView* W) {
    __shared__ unsigned gridw[MPB_GRID_MAX_CELLS];
    __shared__ float4 otab[MPB_GRID_MAX_SPH + 1];
    __shared__ int w_cnt[4], w_first[4];
    __shared__ float w_gap[4];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* T = trajs + (size_t)n * H * row_stride;
    const float* staged = nullptr;
    int cnt = 0, first = INT_MAX;                                 // (wave-uniform)
    float gmax = 0.f;                                             // (per lane)
    const unsigned NT = WORLD ? blockDim.x : 256u;
    for (unsigned base = 0; base < (unsigned)P; base += NT) {     // (unsigned: P may come within 256 of INT_MAX)
        const unsigned p = base + tid;
        const int pc = (int)min(p, (unsigned)P - 1u);
        const int seg = pc / n1, k = pc - seg * n1;               // pc = seg*(n+1) + k; the last point is seg = H-1, k = 0
        const float* row = T + (size_t)seg * row_stride;
        float q[MPB_MAX_DOF];
#pragma unroll
        for (int i = 0; i < MPB_MAX_DOF; ++i) {
            float v = 0.f;
            if (i < D) {
                const float x0 = row[i];
                v = x0;
                if (k > 0) v = x0 + ((float)k / (float)n1) * (row[row_stride + i] - x0);   // traj_interpolate_kernel's expression
            }
            q[i] = v;
        }
        float c;
        bool hit;
        if constexpr (WORLD == 0) {
            c = rrt_config_cost<MODEL>(geom, gridw, otab, staged, q);
            hit = p < (unsigned)P && c > 0.f;
        } else {
            const WorldCost wc = world_config_cost<MODEL, WORLD>(*W, gridw, otab, staged, q);
            c = wc.refused ? 3.0e38f : world_gap(wc);      // (a refused buffer: every point in collision, the largest finite gap)
            hit = p < (unsigned)P && world_hit(wc);
        }
        const unsigned long long m = __ballot(hit);
        if (m != 0ull && first == INT_MAX) first = (int)(base + wave * 64 + (unsigned)__builtin_ctzll(m));
        cnt += __popcll(m);
        if (p < (unsigned)P) {
            gmax = fmaxf(gmax, c);
            if (flag != nullptr) flag[(size_t)n * P + p] = hit ? 1 : 0;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) gmax = fmaxf(gmax, __shfl_xor(gmax, off, 64));
    if (lane == 0) {
        w_cnt[wave] = cnt;
        w_first[wave] = first;
        w_gap[wave] = gmax;
    }
    __syncthreads();
    if constexpr (WORLD == 0) {
        if (tid == 0) {
            const int f = min(min(w_first[0], w_first[1]), min(w_first[2], w_first[3]));
            n_coll[n] = w_cnt[0] + w_cnt[1] + w_cnt[2] + w_cnt[3];
            first_coll[n] = (f == INT_MAX) ? -1 : f;
            max_gap[n] = fmaxf(fmaxf(w_gap[0], w_gap[1]), fmaxf(w_gap[2], w_gap[3]));
        }
    } else {
        if (tid == 0) {
            int f = INT_MAX, c = 0;
            float g = 0.f;
            for (unsigned wv = 0; wv < NT / 64u; ++wv) {
                f = min(f, w_first[wv]);
                c += w_cnt[wv];
                g = fmaxf(g, w_gap[wv]);
            }
            n_coll[n] = c;
            first_coll[n] = (f == INT_MAX) ? -1 : f;
            max_gap[n] = g;
        }
    }
}

template <int MODEL>
__global__ __launch_bounds__(256) void traj_collision_stats_kernel(const float* __restrict__ trajs, size_t row_stride,
                                                                   const float* __restrict__ geom, int* __restrict__ n_coll,
                                                                   int* __restrict__ first_coll, float* __restrict__ max_gap,
                                                                   unsigned char* __restrict__ flag, int H, int D, int n1, int P) {
    traj_collision_stats_body<MODEL, 0>(trajs, row_stride, geom, n_coll, first_coll, max_gap, flag, H, D, n1, P, nullptr);
}

template <int MODEL>
__global__ __launch_bounds__(256) void traj_stats_world_kernel(const float* __restrict__ trajs, size_t row_stride,
                                                               const float* __restrict__ geom, int* __restrict__ n_coll,
                                                               int* __restrict__ first_coll, float* __restrict__ max_gap,
                                                               unsigned char* __restrict__ flag, int H, int D, int n1, int P, const WorldArgs w) {
    extern __shared__ __align__(16) float world_lds[];
    const WorldView W = world_view(geom, w, world_lds);
    traj_collision_stats_body<MODEL, 1>(trajs, row_stride, geom, n_coll, first_coll, max_gap, flag, H, D, n1, P, &W);
}

// ---- host side ------------------------------------------------------------------------------------------------------
static int traj_collision_stats_impl(const char* who, const float* trajs, size_t row_stride, const float* geom, int geom_flags, const float* sdfb,
                                     const float* selfb, int n_interp, int* n_in_collision, int* first_in_collision, float* max_gap,
                                     unsigned char* point_in_collision, int N, int H, int D, void* stream) {
    if (D > MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "%s: D = %d exceeds MPB_MAX_DOF = %d", who, D, MPB_MAX_DOF);
    if (N < 0 || H < 2 || D < 1 || n_interp < 0 || row_stride < (size_t)D) return mpb_failf(MPB_E_INVALID, "%s: bad shape", who);
    const long long P = (long long)(H - 1) * ((long long)n_interp + 1) + 1;
    if (P > INT_MAX) return mpb_failf(MPB_E_INVALID, "%s: bad shape ((H - 1)(n_interp + 1) + 1 dense points do not fit an int)", who);
    if (N == 0) return MPB_OK;
    if (!trajs || !geom || !n_in_collision || !first_in_collision || !max_gap) return mpb_failf(MPB_E_INVALID, "%s: null pointer", who);
    if (mpb_misaligned16(geom)) return mpb_failf(MPB_E_INVALID, "%s: geom must be 16-byte aligned", who);
    if (!world_present(sdfb, selfb)) {
        if (rrt_use_model(geom_flags, D))
            hipLaunchKernelGGL(traj_collision_stats_kernel<PandaModel::ID>, dim3(N), dim3(256), 0, (hipStream_t)stream, trajs, row_stride, geom,
                               n_in_collision, first_in_collision, max_gap, point_in_collision, H, D, n_interp + 1, (int)P);
        else
            hipLaunchKernelGGL(traj_collision_stats_kernel<0>, dim3(N), dim3(256), 0, (hipStream_t)stream, trajs, row_stride, geom,
                               n_in_collision, first_in_collision, max_gap, point_in_collision, H, D, n_interp + 1, (int)P);
        return mpb_check_launch(who);
    }
    WorldArgs w;
    const int rc = world_args(who, sdfb, selfb, D, w);
    if (rc) return rc;
    const int threads = selfb != nullptr ? 64 : 256;          // (one self block: the 64-thread form)
    const size_t lds = world_self_lds_bytes(w, threads / 64);
    return rrt_dispatch<>(geom_flags, D, [&](auto, auto model) {
        const int rl = mpb_raise_lds_limit(traj_stats_world_kernel<model.value>, lds, who);
        if (rl) return rl;
        hipLaunchKernelGGL(traj_stats_world_kernel<model.value>, dim3(N), dim3(threads), lds, (hipStream_t)stream, trajs, row_stride, geom,
                           n_in_collision, first_in_collision, max_gap, point_in_collision, H, D, n_interp + 1, (int)P, w);
        return mpb_check_launch(who);
    });
}

extern "C" int mpb_traj_collision_stats(const float* trajs, size_t row_stride, const float* geom, int geom_flags, int n_interp,
                                        int* n_in_collision, int* first_in_collision, float* max_gap,
                                        unsigned char* point_in_collision, int N, int H, int D, void* stream) {
    return traj_collision_stats_impl(__func__, trajs, row_stride, geom, geom_flags, nullptr, nullptr, n_interp, n_in_collision, first_in_collision,
                                     max_gap, point_in_collision, N, H, D, stream);
}

extern "C" int mpb_traj_collision_stats_world(const float* trajs, size_t row_stride, const float* geom, int geom_flags, const float* sdfb,
                                              const float* selfb, int n_interp, int* n_in_collision, int* first_in_collision,
                                              float* max_gap, unsigned char* point_in_collision, int N, int H, int D, void* stream) {
    return traj_collision_stats_impl(__func__, trajs, row_stride, geom, geom_flags, sdfb, selfb, n_interp, n_in_collision, first_in_collision,
                                     max_gap, point_in_collision, N, H, D, stream);
}
