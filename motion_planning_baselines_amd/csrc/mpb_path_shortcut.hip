// mpb_path_shortcut.hip -- batched path shortcutting: the pass a sample-based stack runs between the tree and the optimiser
// (pybullet-planning's smooth_path, OMPL's PathSimplifier; the reference's RRT code did not carry it over -- the semantics are
// build-defined).  It edits the (paths (N, Lmax, D), lengths (N,)) batch the RRT planners emit and
// mpb_traj_resample consumes.
//
// ONE launch, one single-wave workgroup per path, the path in LDS as (Lmax, Dp) floats (Dp = D rounded up to 4) for the
// whole launch.  Per iteration: two uniforms pick two positions on the polyline, the segment between them is checked exactly
// as the RRT kernels check an extension without the max_dist clamp (the rounded fp32 distance, dist / check_step + 2
// points, rrt_linspace_point, rrt_first_collision with rrt_config_cost > 0: mpb_rrt.h), and a free segment replaces the
// nodes between the two positions; the tail moves in LDS by a parallel shift, as rrt_pool_delete moves its list.
//   - workgroups never wait on each other, every loop is bounded by n_iters, Lmax or the point count of one candidate;
//   - no atomics, a fixed order: the same bits on every run, and a path's bits depend on its own inputs only;
//   - the arithmetic of this file is rounded after every operation: plain operators under #pragma clang fp contract(off).  What
//     it calls in mpb_rrt.h is what stands there: rrt_d2_rounded rounds after every operation too, rrt_linspace_point and
//     rrt_close say fmaf where they take one rounding;
//   - every value that steers control flow (the length, the positions, the verdicts) is computed alike by all 64 lanes
//     from LDS broadcasts: the control flow is block-uniform, as rrt_config_cost's __syncthreads() needs.
// On a world (mpb_world.h) shortcut_world_kernel runs the same body with the world predicate; its self block sits behind the path.
#include "mpb_common.h"
#include "mpb_rrt.h"
#include "mpb_rrt_host.h"
#include "mpb_world.h"
#include "mpb_world_host.h"

#define SC_TAG 0x53484354u                                   // the Philox stream of this kernel (the RRT kernels': their magics)
#define SC_STAGING_BYTES (4 * MPB_GRID_MAX_CELLS + 16 * (MPB_GRID_MAX_SPH + 1))   // gridw + otab, static LDS
#define SC_LDS_BYTES (160 * 1024)                            // LDS of one workgroup on gfx950

struct ScArgs {
    const float* paths_in;
    const int* lengths_in;
    float* paths_out;
    int* lengths_out;
    float* stats;
    int* log;
    const float* geom;
    const float* draws;
    int Lmax, D, n_iters;
    float step;
    uint32_t seed_lo, seed_hi, problem_offset;
};

// a recorded draw into [0, 1): NaN reads as 0 (tested on the bits: the build assumes finite math)
__device__ __forceinline__ float sc_unit(float u) {
    if ((__float_as_uint(u) & 0x7FFFFFFFu) > 0x7F800000u) return 0.f;
    return fminf(fmaxf(u, 0.f), 0x1.fffffep-1f);
}

template <int DM>
__device__ __forceinline__ bool sc_allclose(const float (&x)[MPB_MAX_DOF], const float (&y)[MPB_MAX_DOF], int D) {
    bool c = true;
#pragma unroll
    for (int k = 0; k < DM; ++k)
        if (k < D) c = c && rrt_close(x[k], y[k]);
    return c;
}

// the polyline's joint-space length: the segments' distances (the square root of rrt_d2_rounded) summed in fp32 in path order
// (every lane the whole sum)
template <int DM>
__device__ __forceinline__ float sc_length(const float* P, int Dp, int D, int L) {
#pragma clang fp contract(off)
    float len = 0.f, x[MPB_MAX_DOF], y[MPB_MAX_DOF];
    if (L > 0) rrt_load_row<DM>(P, D, x);
    for (int j = 1; j < L; ++j) {
        rrt_load_row<DM>(P + j * Dp, D, y);
        len = len + sqrtf(rrt_d2_rounded<DM>(x, y));
#pragma unroll
        for (int k = 0; k < MPB_MAX_DOF; ++k) x[k] = y[k];
    }
    return len;
}

// the position a uniform picks on a polyline of L >= 3 nodes: segment a, parameter t in [0, 1)
__device__ __forceinline__ void sc_position(float u, int L, int& a, float& t) {
#pragma clang fp contract(off)
    const float s = u * (float)(L - 1);
    a = min((int)s, L - 2);
    t = s - (float)a;
}

// The shortcut point of position (a, t) and the node rows that stay on its outer side.  t == 0, or a point allclose to node
// a, IS node a (its bits, nothing to insert); a point allclose to node a + 1 is that node.  Returns whether a row is inserted;
// `node`: the index of the node the point is, else -1.
template <int DM>
__device__ __forceinline__ bool sc_point(const float* P, int Dp, int D, int a, float t, float (&pt)[MPB_MAX_DOF], int& node) {
#pragma clang fp contract(off)
    float q0[MPB_MAX_DOF], q1[MPB_MAX_DOF];
    rrt_load_row<DM>(P + a * Dp, D, q0);
    rrt_load_row<DM>(P + (a + 1) * Dp, D, q1);
#pragma unroll
    for (int k = 0; k < MPB_MAX_DOF; ++k) pt[k] = q0[k] + t * (q1[k] - q0[k]);
    const bool at0 = t == 0.f || sc_allclose<DM>(pt, q0, D);
    const bool at1 = !at0 && sc_allclose<DM>(pt, q1, D);
#pragma unroll
    for (int k = 0; k < MPB_MAX_DOF; ++k) pt[k] = at0 ? q0[k] : at1 ? q1[k] : pt[k];
    node = at0 ? a : at1 ? a + 1 : -1;
    return !at0 && !at1;
}

// (the body of path_shortcut_kernel and of its world form shortcut_world_kernel; W: null with WORLD == 0, whose self block sits in the
// dynamic LDS behind the path)
template <int DT, int MODEL, int WORLD>
__device__ __forceinline__ void path_shortcut_body(const ScArgs& a, const WorldView* W) {
#pragma clang fp contract(off)
    __shared__ unsigned gridw[MPB_GRID_MAX_CELLS];
    __shared__ float4 otab[MPB_GRID_MAX_SPH + 1];
    extern __shared__ float sc_path[];                     // (Lmax, Dp), zero padded columns
    constexpr int DM = DT ? DT : MPB_MAX_DOF;
    const int D = DT ? DT : a.D;
    const int Dp = (D + 3) & ~3;
    const int b = blockIdx.x, lane = threadIdx.x;
    const float* in_b = a.paths_in + (size_t)b * a.Lmax * D;
    float* out_b = a.paths_out + (size_t)b * a.Lmax * D;
    float* P = sc_path;
    int L = a.lengths_in[b];
    const bool bad = L < 0 || L > a.Lmax;                  // flagged: length 0, NaN stats, a zeroed path
    if (bad) L = 0;
    for (int i = lane; i < L * Dp; i += 64) {
        const int r = i / Dp, k = i - r * Dp;
        P[i] = (k < D) ? in_b[(size_t)r * D + k] : 0.f;
    }
    __syncthreads();
    const float len_before = sc_length<DM>(P, Dp, D, L);
    const float* staged = nullptr;
    int tested = 0, accepted = 0;

    for (int it = 0; it < a.n_iters; ++it) {
        int code = MPB_SHORTCUT_IDLE, first = 0;
        if (L >= 3) {                                      // (block-uniform)
            float u1, u2;
            if (a.draws != nullptr) {
                const float* d = a.draws + ((size_t)b * a.n_iters + it) * 2;
                u1 = sc_unit(d[0]);
                u2 = sc_unit(d[1]);
            } else {
                const uint4 r = philox4x32_10(make_uint4(a.problem_offset + (uint32_t)b, (uint32_t)it, SC_TAG, 0u),
                                              make_uint2(a.seed_lo, a.seed_hi));
                u1 = (float)(r.x >> 8) * 0x1p-24f;
                u2 = (float)(r.y >> 8) * 0x1p-24f;
            }
            int a1, a2;
            float t1, t2;
            sc_position(u1, L, a1, t1);
            sc_position(u2, L, a2, t2);
            if (a2 < a1 || (a2 == a1 && t2 < t1)) {
                const int ai = a1; a1 = a2; a2 = ai;
                const float ti = t1; t1 = t2; t2 = ti;
            }
            code = MPB_SHORTCUT_SKIP;
            if (a1 != a2) {
                float p1[MPB_MAX_DOF], p2[MPB_MAX_DOF], dl[MPB_MAX_DOF];
                int n1, n2;
                const bool ins1 = sc_point<DM>(P, Dp, D, a1, t1, p1, n1);
                const bool ins2 = sc_point<DM>(P, Dp, D, a2, t2, p2, n2);
                const int lo = ins1 ? a1 : n1;             // the last node kept before the shortcut
                const int hi = ins2 ? a2 + 1 : n2;         // the first node kept after it
                const float dist = sqrtf(rrt_d2_rounded<DM>(p1, p2));
                const float cntf = dist / a.step;
                // (hi - lo < 2: after the snap to nodes both points lie on one segment)
                if (hi - lo >= 2 && !sc_allclose<DM>(p1, p2, D) && cntf < (float)(RRT_MAX_PTS - 1)) {
                    const int n_pts = (int)cntf + 2;
                    const float lstep = 1.0f / (float)(n_pts - 1);
#pragma unroll
                    for (int k = 0; k < MPB_MAX_DOF; ++k) dl[k] = p2[k] - p1[k];
                    first = rrt_first_collision<DM, MODEL, WORLD>(a.geom, gridw, otab, staged, p1, dl, n_pts, lstep, lane, W);
                    ++tested;
                    const int n_ins = (ins1 ? 1 : 0) + (ins2 ? 1 : 0);
                    const int new_len = lo + 1 + n_ins + (L - hi);
                    if (first >= 0) {
                        code = MPB_SHORTCUT_REJECT;
                    } else if (new_len > a.Lmax) {         // (the corner cut: one node replaced by two on a full path)
                        code = MPB_SHORTCUT_OVERFLOW;
                        first = 0;
                    } else {
                        code = MPB_SHORTCUT_ACCEPT;
                        first = 0;
                        ++accepted;
                        // the tail hi .. L - 1 moves to lo + 1 + n_ins: towards the front in ascending trips, one row towards the
                        // back in descending ones (a trip never writes what a later trip still reads)
                        const int src = hi * Dp, dst = (lo + 1 + n_ins) * Dp, cnt = (L - hi) * Dp;
                        if (dst != src) {
                            const int trips = (cnt + 63) / 64;
                            for (int tr = 0; tr < trips; ++tr) {
                                const int i = (dst < src ? tr : trips - 1 - tr) * 64 + lane;
                                const float v = P[src + min(i, cnt - 1)];
                                __syncthreads();
                                if (i < cnt) P[dst + i] = v;
                                __syncthreads();
                            }
                        }
                        float v1 = 0.f, v2 = 0.f;
#pragma unroll
                        for (int k = 0; k < DM; ++k) {
                            v1 = (lane == k) ? p1[k] : v1;
                            v2 = (lane == k) ? p2[k] : v2;
                        }
                        if (ins1 && lane < Dp) P[(lo + 1) * Dp + lane] = v1;
                        if (ins2 && lane < Dp) P[(lo + 1 + (ins1 ? 1 : 0)) * Dp + lane] = v2;
                        L = new_len;
                        __syncthreads();
                    }
                }
            }
        }
        if (a.log != nullptr && lane == 0) a.log[(size_t)b * a.n_iters + it] = code | (first << MPB_SHORTCUT_LOG_INDEX_SHIFT);
    }

    const float len_after = sc_length<DM>(P, Dp, D, L);
    for (int i = lane; i < a.Lmax * D; i += 64) {           // rows at and past the length: zeros
        const int r = i / D, k = i - r * D;
        out_b[i] = (r < L) ? P[r * Dp + k] : 0.f;
    }
    if (lane < 4) {
        const float s = lane == 0 ? (float)tested : lane == 1 ? (float)accepted : lane == 2 ? len_before : len_after;
        a.stats[(size_t)b * 4 + lane] = bad ? __uint_as_float(0x7FC00000u) : s;
    }
    if (lane == 0) a.lengths_out[b] = L;
}

template <int DT, int MODEL>
__global__ __launch_bounds__(64) void path_shortcut_kernel(const ScArgs a) {
    path_shortcut_body<DT, MODEL, 0>(a, nullptr);
}

// the same pass on a world: a candidate's points are decided by the world predicate (mpb_world.h)
template <int DT, int MODEL>
__global__ __launch_bounds__(64) void shortcut_world_kernel(const ScArgs a, const WorldArgs w) {
    extern __shared__ float sc_path[];
    const int Dp = ((DT ? DT : a.D) + 3) & ~3;
    const WorldView W = world_view(a.geom, w, sc_path + (size_t)a.Lmax * Dp);
    path_shortcut_body<DT, MODEL, 1>(a, &W);
}

// ---- host side ------------------------------------------------------------------------------------------------------
static int path_shortcut_impl(const char* who, const float* paths_in, const int* lengths_in, float* paths_out, int* lengths_out, float* stats,
                              int* log, const float* geom, int geom_flags, const float* sdfb, const float* selfb, const float* draws, int N,
                              int Lmax, int D, int n_iters, float check_step, uint64_t seed, uint32_t problem_offset, void* stream) {
    if (D > MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "%s: D = %d exceeds MPB_MAX_DOF = %d", who, D, MPB_MAX_DOF);
    if (N < 0 || D < 1) return mpb_failf(MPB_E_INVALID, "%s: bad shape (N %d, D %d)", who, N, D);
    const int Dp = (D + 3) & ~3;
    const int max_rows = (SC_LDS_BYTES - SC_STAGING_BYTES) / (4 * Dp);
    if (Lmax < 2 || Lmax > max_rows)
        return mpb_failf(MPB_E_INVALID, "%s: Lmax = %d outside 2 .. %d (the path of D = %d lives in LDS)", who, Lmax, max_rows, D);
    if (n_iters < 0 || n_iters > MPB_SHORTCUT_MAX_ITERS)
        return mpb_failf(MPB_E_INVALID, "%s: n_iters = %d outside 0 .. %d", who, n_iters, MPB_SHORTCUT_MAX_ITERS);
    if (mpb_bad_step(check_step)) return mpb_failf(MPB_E_INVALID, "%s: check_step must be finite and positive", who);
    if (!paths_in || !lengths_in || !paths_out || !lengths_out || !stats || !geom) return mpb_failf(MPB_E_INVALID, "%s: null pointer", who);
    if (mpb_misaligned16(geom)) return mpb_failf(MPB_E_INVALID, "%s: geom must be 16-byte aligned", who);
    if (N == 0) return MPB_OK;
    const ScArgs a = {paths_in, lengths_in, paths_out, lengths_out, stats, log, geom, draws, Lmax, D, n_iters, check_step,
                      (uint32_t)seed, (uint32_t)(seed >> 32), problem_offset};
    const size_t lds = (size_t)Lmax * Dp * sizeof(float);
    if (!world_present(sdfb, selfb))
        return rrt_dispatch<2, 3, 7>(geom_flags, D, [&](auto dt, auto model) {
            const int rl = mpb_raise_lds_limit(path_shortcut_kernel<dt.value, model.value>, lds, who);
            if (rl) return rl;
            hipLaunchKernelGGL((path_shortcut_kernel<dt.value, model.value>), dim3(N), dim3(64), lds, (hipStream_t)stream, a);
            return mpb_check_launch(who);
        });
    WorldArgs w;
    const int rc = world_args(who, sdfb, selfb, D, w);
    if (rc) return rc;
    const size_t lds_w = lds + world_self_lds_bytes(w, 1);
    if (lds_w > (size_t)(SC_LDS_BYTES - SC_STAGING_BYTES))
        return mpb_failf(MPB_E_INVALID, "%s: Lmax = %d rows of D = %d and the self block of %d spheres take %zu bytes of LDS, %d are there", who, Lmax,
                         D, w.self_links, lds_w, SC_LDS_BYTES - SC_STAGING_BYTES);
    return rrt_dispatch<>(geom_flags, D, [&](auto dt, auto model) {
        const int rl = mpb_raise_lds_limit(shortcut_world_kernel<dt.value, model.value>, lds_w, who);
        if (rl) return rl;
        hipLaunchKernelGGL((shortcut_world_kernel<dt.value, model.value>), dim3(N), dim3(64), lds_w, (hipStream_t)stream, a, w);
        return mpb_check_launch(who);
    });
}

extern "C" int mpb_path_shortcut(const float* paths_in, const int* lengths_in, float* paths_out, int* lengths_out, float* stats,
                                 int* log, const float* geom, int geom_flags, const float* draws, int N, int Lmax, int D,
                                 int n_iters, float check_step, uint64_t seed, uint32_t problem_offset, void* stream) {
    return path_shortcut_impl(__func__, paths_in, lengths_in, paths_out, lengths_out, stats, log, geom, geom_flags, nullptr, nullptr, draws, N,
                              Lmax, D, n_iters, check_step, seed, problem_offset, stream);
}

extern "C" int mpb_path_shortcut_world(const float* paths_in, const int* lengths_in, float* paths_out, int* lengths_out, float* stats,
                                       int* log, const float* geom, int geom_flags, const float* sdfb, const float* selfb,
                                       const float* draws, int N, int Lmax, int D, int n_iters, float check_step, uint64_t seed,
                                       uint32_t problem_offset, void* stream) {
    return path_shortcut_impl(__func__, paths_in, lengths_in, paths_out, lengths_out, stats, log, geom, geom_flags, sdfb, selfb, draws, N, Lmax,
                              D, n_iters, check_step, seed, problem_offset, stream);
}
