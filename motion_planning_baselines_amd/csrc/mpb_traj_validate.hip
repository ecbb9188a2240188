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
#include <climits>

#include "mpb_common.h"
#include "mpb_rrt.h"
#include "mpb_rrt_host.h"

template <int MODEL>
__global__ __launch_bounds__(256) void traj_collision_stats_kernel(const float* __restrict__ trajs, size_t row_stride,
                                                                   const float* __restrict__ geom, int* __restrict__ n_coll,
                                                                   int* __restrict__ first_coll, float* __restrict__ max_gap,
                                                                   unsigned char* __restrict__ flag, int H, int D, int n1, int P) {
    __shared__ unsigned gridw[MPB_GRID_MAX_CELLS];
    __shared__ float4 otab[MPB_GRID_MAX_SPH + 1];
    __shared__ int w_cnt[4], w_first[4];
    __shared__ float w_gap[4];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* T = trajs + (size_t)n * H * row_stride;
    const float* staged = nullptr;
    int cnt = 0, first = INT_MAX;                                 // (wave-uniform)
    float gmax = 0.f;                                             // (per lane)
    for (unsigned base = 0; base < (unsigned)P; base += 256) {    // (unsigned: P may come within 256 of INT_MAX)
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
        const float c = rrt_config_cost<MODEL>(geom, gridw, otab, staged, q);
        const bool hit = p < (unsigned)P && c > 0.f;
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
    if (tid == 0) {
        const int f = min(min(w_first[0], w_first[1]), min(w_first[2], w_first[3]));
        n_coll[n] = w_cnt[0] + w_cnt[1] + w_cnt[2] + w_cnt[3];
        first_coll[n] = (f == INT_MAX) ? -1 : f;
        max_gap[n] = fmaxf(fmaxf(w_gap[0], w_gap[1]), fmaxf(w_gap[2], w_gap[3]));
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
extern "C" int mpb_traj_collision_stats(const float* trajs, size_t row_stride, const float* geom, int geom_flags, int n_interp,
                                        int* n_in_collision, int* first_in_collision, float* max_gap,
                                        unsigned char* point_in_collision, int N, int H, int D, void* stream) {
    if (D > MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "mpb_traj_collision_stats: D = %d exceeds MPB_MAX_DOF = %d", D, MPB_MAX_DOF);
    if (N < 0 || H < 2 || D < 1 || n_interp < 0 || row_stride < (size_t)D) return mpb_fail(MPB_E_INVALID, "mpb_traj_collision_stats: bad shape");
    const long long P = (long long)(H - 1) * ((long long)n_interp + 1) + 1;
    if (P > INT_MAX) return mpb_fail(MPB_E_INVALID, "mpb_traj_collision_stats: bad shape ((H - 1)(n_interp + 1) + 1 dense points do not fit an int)");
    if (N == 0) return MPB_OK;
    if (!trajs || !geom || !n_in_collision || !first_in_collision || !max_gap) return mpb_fail(MPB_E_INVALID, "mpb_traj_collision_stats: null pointer");
    if (mpb_misaligned16(geom)) return mpb_fail(MPB_E_INVALID, "mpb_traj_collision_stats: geom must be 16-byte aligned");
    if (rrt_use_model(geom_flags, D))
        hipLaunchKernelGGL(traj_collision_stats_kernel<PandaModel::ID>, dim3(N), dim3(256), 0, (hipStream_t)stream, trajs, row_stride, geom,
                           n_in_collision, first_in_collision, max_gap, point_in_collision, H, D, n_interp + 1, (int)P);
    else
        hipLaunchKernelGGL(traj_collision_stats_kernel<0>, dim3(N), dim3(256), 0, (hipStream_t)stream, trajs, row_stride, geom,
                           n_in_collision, first_in_collision, max_gap, point_in_collision, H, D, n_interp + 1, (int)P);
    return mpb_check_launch("mpb_traj_collision_stats");
}
