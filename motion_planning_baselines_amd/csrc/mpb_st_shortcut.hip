// mpb_st_shortcut.hip -- space-time shortcutting: the pass between a planner on the moving-obstacle clock (planners.STRRTConnect,
// PlanningTask.time_paths_moving) and the optimiser (ops.st_shortcut, PlanningTask.shortcut_trajs_moving; build-defined, DESIGN.md 10: the
// reference has nothing like it).  N dense trajectories of R rows each, row h at the time of row h of a packed moving-obstacle buffer
// (include/mpb_moving_layout.h: the clock of mpb_strrt.hip, mpb_path_timing.hip and mpb_moving_collision_check).  The row count never
// changes, so the clock is kept: an iteration replaces the rows BETWEEN two rows a < b by the constant-velocity straight piece, and keeps
// the replacement only when every new row is free at its own time and the piece respects the per-row velocity bound w.
//
// Predicate of (q, row): strrt_collides of mpb_strrt.h -- the static cost of the task's geometry is positive OR the moving cost of that
//   row is; at the rows only, obstacle positions are never interpolated.
// Input gate, before any iteration: all R rows by the predicate (INPUT_IN_COLLISION, first_bad = the first such row), then every step
//   strrt_tau(q[h+1], q[h], w) <= MPB_STS_GATE_LIMIT (INPUT_TOO_FAST, first_bad = h + 1 of the first step above it).  valid[n] == 0:
//   NOT_VALID; a buffer whose header differs from what the launcher read: BUFFER_CHANGED, and nothing of the buffer is read.  Only OK
//   trajectories are edited; every other one comes out with its input bits, NaN stats and an IDLE log.
// Iteration `it`: r0 = mulhi(x, R), r1 = mulhi(y, R) of ONE Philox call (problem_offset + n, it, MPB_STS_PHILOX_TAG, 0), key = seed -- or
//   the two recorded ints clamped into 0 .. R - 1 --, a = min, b = max, with max_span > 0: b = min(b, a + max_span).  Then
//   1 b - a < 2: SKIP_SHORT.   2 strrt_tau(q_b, q_a, w) > (float)(b - a): SKIP_FAST (STRRT's f == 1 condition).
//   3 candidate row a < h < b: fma(q_b - q_a, (float)(h - a) / (float)(b - a), q_a) -- the subtraction and the division rounded, ONE
//     fma: STRRT's dense-row expression; rows a and b keep their bits.
//   4 every candidate row rrt_close to the row it would replace, in every coordinate: SKIP_STRAIGHT, nothing is evaluated.
//   5 rows a + 1 .. b - 1 by the predicate at their own rows, ascending: a hit is REJECT | first colliding row << 8.
//   6 otherwise ACCEPT: the candidate rows replace the old ones.
// Mapping: one single-wave workgroup per trajectory, persistent over the iterations (STRRT's mapping and its block-uniform static
//   predicate with the staged broad-phase grid in LDS).  The trajectory lives in dynamic LDS as [row][Dp] floats for the whole launch.
//   The gate and every candidate run one lane per row in trips of 64, the first hit is the count of trailing zeros of a ballot and the
//   trips after it are never evaluated.  q_a and q_b are read from LDS (broadcasts) wherever a row is formed, so nothing but w and the
//   lane's own row is live across the predicate; on ACCEPT the lanes form their rows again -- the same bits -- and write them to LDS.
//   The last phase copies LDS to trajs_out coalesced (in place is served: a workgroup has read its trajectory before it writes it).
// No workgroup waits on another, no spin wait, no atomics; every loop is bounded by n_iters, R, the link count or the obstacle counts;
// every value that steers control flow is computed alike by all 64 lanes; the same bits on every run, and a trajectory's bits depend on
// its own inputs only.
#include "mpb_common.h"
#include "mpb_rrt.h"
#include "mpb_rrt_host.h"
#include "mpb_moving.h"
#include "mpb_strrt.h"
#include "../../include/mpb_st_shortcut_layout.h"

static_assert(MPB_STS_STATIC_LDS_BYTES == 4 * MPB_GRID_MAX_CELLS + 16 * (MPB_GRID_MAX_SPH + 1), "the staged grid's bytes");

struct StsArgs {
    const float* trajs_in;         // (N, R, D)
    float* trajs_out;              // (N, R, D); may be trajs_in
    const float* geom;
    StMoving mv;
    const float* w;                // (D)
    const unsigned char* valid;    // (N) or null
    const int* draws;              // (N, n_iters, 2) or null
    int* status;                   // (N)
    int* first_bad;                // (N)
    float* stats;                  // (N, 4)
    int* log;                      // (N, n_iters) or null
    int R, D, n_iters, max_span;
    uint32_t seed_lo, seed_hi, problem_offset;
};

// the joint-space length of the R rows in LDS: per-row distances in the rounded form (the square root of rrt_d2_rounded) summed in fp32
// in row order (every lane the whole sum)
template <int DM>
__device__ __forceinline__ float sts_length(const float* P, int Dp, int R) {
#pragma clang fp contract(off)
    float len = 0.f, x[MPB_MAX_DOF], y[MPB_MAX_DOF];
    rrt_load_row4<DM>(P, Dp, x);
    for (int h = 1; h < R; ++h) {
        rrt_load_row4<DM>(P + h * Dp, Dp, y);
        len = len + sqrtf(rrt_d2_rounded<DM>(x, y));
#pragma unroll
        for (int k = 0; k < MPB_MAX_DOF; ++k) x[k] = y[k];
    }
    return len;
}

template <int DT, int MODEL>
__global__ __launch_bounds__(64) void st_shortcut_kernel(const StsArgs a) {
#pragma clang fp contract(off)
    __shared__ unsigned gridw[MPB_GRID_MAX_CELLS];
    __shared__ float4 otab[MPB_GRID_MAX_SPH + 1];
    extern __shared__ __align__(16) float sts_traj[];      // [R][Dp], zero padded columns
    constexpr int DM = DT ? DT : MPB_MAX_DOF;
    const int D = DT ? DT : a.D;
    const int Dp = (D + 3) & ~3;
    const int R = a.R;
    const int n = blockIdx.x, lane = threadIdx.x;
    const float* in_n = a.trajs_in + (size_t)n * R * D;
    float* out_n = a.trajs_out + (size_t)n * R * D;
    float* P = sts_traj;
    for (int i = lane; i < R * Dp; i += 64) {
        const int r = i / Dp, k = i - r * Dp;
        P[i] = (k < D) ? in_n[(size_t)r * D + k] : 0.f;
    }
    __syncthreads();
    const GeomView G = moving_robot_view(a.mv.mob);
    const MovingTables T = moving_tables(a.mv.mob, R, a.mv.n_sph, a.mv.n_box);
    const bool ok = moving_header_matches(a.mv.mob, D, a.mv.L, R, a.mv.n_sph, a.mv.n_box);
    float w[MPB_MAX_DOF];
#pragma unroll
    for (int k = 0; k < MPB_MAX_DOF; ++k) w[k] = (k < DM && k < D) ? a.w[k] : 1.f;
    const float* staged = nullptr;

    // ---- the input gate (every branch below is block-uniform)
    int status = MPB_STS_OK, bad = -1;
    if (a.valid != nullptr && a.valid[n] == 0) status = MPB_STS_NOT_VALID;
    else if (!ok) status = MPB_STS_BUFFER_CHANGED;
    if (status == MPB_STS_OK) {
        for (int base = 0; base < R; base += 64) {
            const int h = base + lane, hc = min(h, R - 1);
            float q[MPB_MAX_DOF];
            rrt_load_row4<DM>(P + hc * Dp, Dp, q);
            const bool hit = strrt_collides<MODEL>(a.geom, gridw, otab, staged, G, T, a.mv.L, ok, hc, q);
            const unsigned long long m = __ballot(h < R && hit);
            if (m != 0ull) { bad = base + (int)__builtin_ctzll(m); break; }
        }
        if (bad >= 0) status = MPB_STS_INPUT_IN_COLLISION;
    }
    if (status == MPB_STS_OK) {
        for (int base = 0; base < R - 1; base += 64) {
            const int h = base + lane, hc = min(h, R - 2);
            float q0[MPB_MAX_DOF], q1[MPB_MAX_DOF];
            rrt_load_row4<DM>(P + hc * Dp, Dp, q0);
            rrt_load_row4<DM>(P + (hc + 1) * Dp, Dp, q1);
            const unsigned long long m = __ballot(h < R - 1 && strrt_tau(q1, q0, w) > MPB_STS_GATE_LIMIT);
            if (m != 0ull) { bad = base + (int)__builtin_ctzll(m) + 1; break; }
        }
        if (bad >= 0) status = MPB_STS_INPUT_TOO_FAST;
    }
    const bool run = status == MPB_STS_OK;
    const float len_before = run ? sts_length<DM>(P, Dp, R) : 0.f;
    int tested = 0, accepted = 0;

    for (int it = 0; it < a.n_iters; ++it) {
        int code = MPB_STS_LOG_IDLE, first = 0;
        if (run) {
            int r0, r1;
            if (a.draws != nullptr) {
                const int* d = a.draws + ((size_t)n * a.n_iters + it) * 2;
                r0 = d[0];
                r1 = d[1];
            } else {
                const uint4 r = philox4x32_10(make_uint4(a.problem_offset + (uint32_t)n, (uint32_t)it, MPB_STS_PHILOX_TAG, 0u),
                                              make_uint2(a.seed_lo, a.seed_hi));
                r0 = (int)__umulhi(r.x, (uint32_t)R);
                r1 = (int)__umulhi(r.y, (uint32_t)R);
            }
            r0 = min(max(r0, 0), R - 1);
            r1 = min(max(r1, 0), R - 1);
            const int ra = min(r0, r1);
            int rb = max(r0, r1);
            if (a.max_span > 0) rb = min(rb, ra + a.max_span);
            const float* Pa = P + ra * Dp;
            const float* Pb = P + rb * Dp;
            const float span = (float)(rb - ra);
            // the candidate row h, ra < h < rb (q_a, q_b: LDS broadcasts)
            auto candidate = [&](int h, float (&q)[MPB_MAX_DOF]) {
                float qa[MPB_MAX_DOF], qb[MPB_MAX_DOF];
                rrt_load_row4<DM>(Pa, Dp, qa);
                rrt_load_row4<DM>(Pb, Dp, qb);
                const float al = (float)(h - ra) / span;
#pragma unroll
                for (int k = 0; k < MPB_MAX_DOF; ++k) q[k] = (k < DM) ? fmaf(qb[k] - qa[k], al, qa[k]) : 0.f;
            };
            bool fast = false;
            if (rb - ra >= 2) {
                float qa[MPB_MAX_DOF], qb[MPB_MAX_DOF];
                rrt_load_row4<DM>(Pa, Dp, qa);
                rrt_load_row4<DM>(Pb, Dp, qb);
                fast = strrt_tau(qb, qa, w) > span;
            }
            if (rb - ra < 2) {
                code = MPB_STS_LOG_SKIP_SHORT;
            } else if (fast) {
                code = MPB_STS_LOG_SKIP_FAST;
            } else {
                const int cnt = rb - ra - 1;               // rows ra + 1 .. rb - 1
                bool straight = true;
                for (int base = 0; base < cnt && straight; base += 64) {
                    const int j = base + lane, h = ra + 1 + min(j, cnt - 1);
                    float q[MPB_MAX_DOF], old[MPB_MAX_DOF];
                    candidate(h, q);
                    rrt_load_row4<DM>(P + h * Dp, Dp, old);
                    bool c = true;
#pragma unroll
                    for (int k = 0; k < DM; ++k)
                        if (k < D) c = c && rrt_close(q[k], old[k]);
                    straight = __ballot(j < cnt && !c) == 0ull;
                }
                if (straight) {
                    code = MPB_STS_LOG_SKIP_STRAIGHT;
                } else {
                    int hit_row = -1;
                    for (int base = 0; base < cnt; base += 64) {
                        const int j = base + lane, h = ra + 1 + min(j, cnt - 1);
                        float q[MPB_MAX_DOF];
                        candidate(h, q);
                        const bool hit = strrt_collides<MODEL>(a.geom, gridw, otab, staged, G, T, a.mv.L, ok, h, q);
                        const unsigned long long m = __ballot(j < cnt && hit);
                        if (m != 0ull) { hit_row = ra + 1 + base + (int)__builtin_ctzll(m); break; }
                    }
                    ++tested;
                    if (hit_row >= 0) {
                        code = MPB_STS_LOG_REJECT;
                        first = hit_row;
                    } else {
                        code = MPB_STS_LOG_ACCEPT;
                        ++accepted;
                        for (int base = 0; base < cnt; base += 64) {
                            const int j = base + lane, h = ra + 1 + min(j, cnt - 1);
                            float q[MPB_MAX_DOF];
                            candidate(h, q);               // (rows ra and rb are not written: every lane reads the same q_a, q_b)
                            if (j < cnt) {
                                float4* dst = reinterpret_cast<float4*>(P + h * Dp);
#pragma unroll
                                for (int kk = 0; kk < (DM + 3) / 4; ++kk)
                                    if (4 * kk < Dp) dst[kk] = make_float4(q[4 * kk], q[4 * kk + 1], q[4 * kk + 2], q[4 * kk + 3]);   // (q is 0 past D)
                            }
                        }
                        __syncthreads();                   // the rows are read back by the next iteration
                    }
                }
            }
        }
        if (a.log != nullptr && lane == 0) a.log[(size_t)n * a.n_iters + it] = code | (first << MPB_STS_LOG_INDEX_SHIFT);
    }

    const float len_after = run ? sts_length<DM>(P, Dp, R) : 0.f;
    for (int i = lane; i < R * D; i += 64) {
        const int r = i / D, k = i - r * D;
        out_n[i] = P[r * Dp + k];
    }
    if (lane < 4) {
        const float s = lane == 0 ? (float)tested : lane == 1 ? (float)accepted : lane == 2 ? len_before : len_after;
        a.stats[(size_t)n * 4 + lane] = run ? s : __uint_as_float(0x7FC00000u);
    }
    if (lane == 0) {
        a.status[n] = status;
        a.first_bad[n] = bad;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------
static int sts_shape_check(const char* who, int N, int R, int D, int n_iters, int max_span) {
    if (D > MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "%s: D = %d exceeds MPB_MAX_DOF = %d", who, D, MPB_MAX_DOF);
    if (R > MPB_STS_MAX_ROWS) return mpb_failf(MPB_E_UNSUPPORTED, "%s: n_rows = %d exceeds MPB_STS_MAX_ROWS = %d", who, R, MPB_STS_MAX_ROWS);
    if (R < MPB_STS_MIN_ROWS) return mpb_failf(MPB_E_INVALID, "%s: n_rows = %d, a trajectory needs at least MPB_STS_MIN_ROWS = %d rows", who, R, MPB_STS_MIN_ROWS);
    if (N < 0 || D < 1) return mpb_failf(MPB_E_INVALID, "%s: bad shape (N %d, D %d)", who, N, D);
    if (n_iters < 0 || n_iters > MPB_STS_MAX_ITERS) return mpb_failf(MPB_E_INVALID, "%s: n_iters = %d outside 0 .. MPB_STS_MAX_ITERS = %d", who, n_iters, MPB_STS_MAX_ITERS);
    if (max_span < 0) return mpb_failf(MPB_E_INVALID, "%s: max_span = %d, 0 (no limit) or a positive row count", who, max_span);
    if ((double)N * R * D > 2.0e9 || (double)N * n_iters > 1.0e9) return mpb_failf(MPB_E_UNSUPPORTED, "%s: N x n_rows x D or N x n_iters too large", who);
    return MPB_OK;
}

// the checks after the shapes; fills the moving half of the scene from the buffer's cached header
static int sts_scene_check(const char* who, bool any_null, const void* geom, const float* mob, int D, int R, StMoving& mv, int& dev) {
    if (any_null) return mpb_failf(MPB_E_INVALID, "%s: null pointer", who);
    if (mpb_misaligned16(geom) || mpb_misaligned16(mob)) return mpb_failf(MPB_E_INVALID, "%s: geom and moving must be 16-byte aligned", who);
    MovingShape S;
    const int rc = mpb_moving_shape_cached(mob, S, who);
    if (rc != MPB_OK) return rc;
    if (S.n_rows != R) return mpb_failf(MPB_E_INVALID, "%s: n_rows = %d, the moving-obstacle buffer was packed for n_rows = %d", who, R, S.n_rows);
    if (S.n_dof != D) return mpb_failf(MPB_E_INVALID, "%s: D = %d, the moving-obstacle buffer's robot has n_dof = %d", who, D, S.n_dof);
    mv.mob = mob; mv.L = S.n_links; mv.n_sph = S.n_sph; mv.n_box = S.n_box;
    dev = S.dev;
    return MPB_OK;
}

extern "C" int mpb_st_shortcut(const float* trajs_in, float* trajs_out, const float* geom, int geom_flags, const float* moving, const float* w,
                               const unsigned char* valid, const int* draws, int* status, int* first_bad, float* stats, int* log, int N,
                               int n_rows, int D, int n_iters, int max_span, uint64_t seed, uint32_t problem_offset, void* stream) {
    const char* who = "mpb_st_shortcut";
    int rc = sts_shape_check(who, N, n_rows, D, n_iters, max_span);
    if (rc != MPB_OK || N == 0) return rc;
    StMoving mv;
    int dev = 0;
    rc = sts_scene_check(who, !trajs_in || !trajs_out || !geom || !moving || !w || !status || !first_bad || !stats, geom, moving, D, n_rows, mv, dev);
    if (rc != MPB_OK) return rc;
    const size_t need = (size_t)MPB_STS_LDS_BYTES(n_rows, D);
    if (need > MPB_STS_MAX_LDS_BYTES)
        return mpb_failf(MPB_E_UNSUPPORTED, "%s: %d rows of D = %d need %zu bytes of LDS, above MPB_STS_MAX_LDS_BYTES = %d", who, n_rows, D, need,
                         MPB_STS_MAX_LDS_BYTES);
    const size_t lds = need - MPB_STS_STATIC_LDS_BYTES;
    const StsArgs a = {trajs_in, trajs_out, geom, mv, w, valid, draws, status, first_bad, stats, log, n_rows, D, n_iters, max_span,
                       (uint32_t)seed, (uint32_t)(seed >> 32), problem_offset};
    return rrt_dispatch<2, 3, 7>(geom_flags, D, [&](auto dt, auto model) {
        const int rl = mpb_raise_lds_limit(reinterpret_cast<const void*>(st_shortcut_kernel<dt.value, model.value>), dev, lds, who);
        if (rl) return rl;
        hipLaunchKernelGGL((st_shortcut_kernel<dt.value, model.value>), dim3(N), dim3(64), lds, (hipStream_t)stream, a);
        return mpb_check_launch(who);
    });
}
