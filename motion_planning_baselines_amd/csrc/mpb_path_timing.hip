// mpb_path_timing.hip -- path-velocity decomposition among moving obstacles (ops.path_time_plan, PlanningTask.time_paths_moving;
// build-defined, DESIGN.md 10: the reference has nothing like it).  A geometric path P of S samples keeps its shape and gets its TIMING
// on the row grid of a packed moving-obstacle buffer of R rows (include/mpb_moving_layout.h; the clock of mpb_strrt.hip and
// mpb_moving_collision_check): at which row to stand on which sample, advancing or waiting, so that every row is free at its own time.
//   c(i)    = max_k fl(fl(|fl(P[i+1,k] - P[i,k])|) / w_k), from 0, no contraction (strrt_tau's form); cfix(i) = (uint32) ceilf(c(i) * 65536);
//             a term above 1 or not finite: SEGMENT_TOO_LONG.  C(i) = sum_{m < i} cfix(m) in integers.
//   advance   in one row from sample i to i' >= i iff C(i') - C(i) <= 65536; lo(i') = the smallest such i.
//   F[j][i] = !blocked[i] && !(the moving cost of P[i] at row j is positive): the predicate of mpb_moving_collision_check, the buffer's
//             centres of row j, nothing interpolated.
//   reach[0][i] = (i == 0) && F[0][0];  reach[j][i'] = F[j][i'] && OR_{i in [lo(i'), i']} reach[j-1][i].
//   hold[j] = F[j'][S-1] for every j' >= j; the arrival row j* = the least j with reach[j][S-1] && hold[j].
//   idx[j*] = S-1; idx[j-1] = the largest i in [lo(idx[j]), idx[j]] with reach[j-1][i]; idx[j] = S-1 for j > j*.  trajs[j] = P[idx[j]], its bits.
//   status: BUFFER_CHANGED, SEGMENT_TOO_LONG, START_BLOCKED (!F[0][0]), GOAL_NOT_HOLDABLE (!F[R-1][S-1]), NO_TIMING -- the first that
//             applies --, else FOUND.  Exact on this lattice: FOUND arrives at the earliest row any monotone timing can, NO_TIMING: none exists.
//
// Mapping: one workgroup of MPB_PT_THREADS threads per path, everything between the phases in its LDS (include/mpb_path_timing_layout.h).
//   (0) one thread per segment: cfix, a wave scan + the wave totals for C, a bisection of C for lo.
//   (A) one thread per sample walks the chain ONCE (FKState / fk_advance / link_centre through moving_robot_view) and leaves the sphere
//       centres as [link][xyz][sample] -- S walks per path where the predicate per cell would take S x R.
//   (B) one lane per row: a wave's task is 64 rows x the 32 samples of one word of the bit table, the tasks dealt round the waves (a
//       whole workgroup on one trip of rows would leave three waves in four idle at R = 64).  The samples and the groups of MPB_GROUP
//       spheres are wave-uniform loops (centres: LDS broadcasts), the obstacles of the lane's row stream past a group as in the other
//       moving kernels (moving_chunk_vs_obstacles: coalesced over the row axis, the same expressions, so the same bits as
//       mpb_moving_collision_check).  The 32 bits of a task gather in ONE word register, stored to the bit table [word][row]: no register
//       array to index.
//   (C) the recurrence over rows on the bit table in place (reach[j] is a subset of F[j]): one thread per sample i', one barrier per row;
//       the interval [lo(i'), i'] is eight word masks computed once, the OR over it eight ANDs of the previous row's words; the new row is
//       two ballot halves per wave.  Stops at the arrival row, or at a row nothing reaches.
//   (D) wave 0 walks back from the arrival row (uniform: every lane reads the same words), then all threads gather the rows.
// No atomics, no spin waits; every loop is bounded by S, R, n_links or the obstacle counts; every run gives the same bits.
#include <math.h>

#include "mpb_common.h"
#include "mpb_host.h"
#include "mpb_geom.h"
#include "mpb_member_cost.h"
#include "mpb_moving.h"
#include "../../include/mpb_path_timing_layout.h"

struct PtArgs {
    const float* paths;            // (N, S, D)
    const float* mob;
    const float* w;                // (D)
    const unsigned char* blocked;  // (N, S) or null
    float* trajs;                  // (N, R, D)
    int* idx;                      // (N, R) or null
    int* arrival;                  // (N) or null
    int* status;                   // (N)
    unsigned char* table;          // (N, R, S) or null
    int S, R, D, L, n_sph, n_box;
};

// bits a .. b (0 <= a <= b <= 31) of a word
__device__ __forceinline__ unsigned pt_bits(int a, int b) { return (0xFFFFFFFFu >> (31 - b)) & (0xFFFFFFFFu << a); }

// the part of the sample interval [l, i] that lies in word w
__device__ __forceinline__ unsigned pt_word_mask(int w, int l, int i) {
    const int a = max(l - 32 * w, 0), b = min(i - 32 * w, 31);
    return a <= b ? pt_bits(a, b) : 0u;
}

__global__ __launch_bounds__(MPB_PT_THREADS) void path_time_plan_kernel(const PtArgs a) {
    extern __shared__ __align__(16) float pt_lds[];
    const int S = a.S, R = a.R, D = a.D, L = a.L;
    const int W = (S + 31) >> 5;
    float* cen = pt_lds;                                                  // [L][3][S]
    unsigned* bits = reinterpret_cast<unsigned*>(cen + 3 * L * S);        // [W][R]
    int* Cp = reinterpret_cast<int*>(bits + W * R);                       // [S]
    int* lo = Cp + S;                                                     // [S]
    int* idxl = lo + S;                                                   // [R]
    int* red = idxl + R;                                                  // [MPB_PT_SCRATCH_WORDS]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = blockIdx.x;
    const float* P = a.paths + (size_t)n * S * D;
    const GeomView G = moving_robot_view(a.mob);
    const MovingTables T = moving_tables(a.mob, R, a.n_sph, a.n_box);
    const bool ok = moving_header_matches(a.mob, D, L, R, a.n_sph, a.n_box);

    // ---- (0) segment costs, prefix sums, interval starts
    unsigned cf = 0u;
    bool bad = false;
    if (tid < S - 1) {
#pragma clang fp contract(off)
        float c = 0.f;
        for (int k = 0; k < D; ++k) {
            const float t = fabsf(P[(size_t)(tid + 1) * D + k] - P[(size_t)tid * D + k]) / a.w[k];
            bad = bad || (__float_as_uint(t) & 0x7FFFFFFFu) > 0x3F800000u;   // above 1, infinite or NaN: on the bits (the build assumes finite math)
            c = fmaxf(c, t);
        }
        cf = bad ? 0u : (unsigned)ceilf(c * (float)MPB_PT_COST_ONE);
    }
    const bool seg_bad = __syncthreads_or(bad) != 0;
    {
        unsigned inc = cf;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned o = __shfl_up(inc, off, 64);
            if (lane >= off) inc += o;
        }
        if (lane == 63) red[wave] = (int)inc;
        __syncthreads();
        unsigned base = 0u;
        for (int v = 0; v < wave; ++v) base += (unsigned)red[v];
        if (tid < S) Cp[tid] = (int)(base + inc - cf);
        __syncthreads();
    }
    if (tid < S) {
        const int target = Cp[tid] - MPB_PT_COST_ONE;
        int lo_ = 0, hi_ = tid;
        for (int it = 0; it < 9 && lo_ < hi_; ++it) {                     // the smallest i with C(i) >= C(tid) - 1: C ascends
            const int mid = (lo_ + hi_) >> 1;
            if (Cp[mid] >= target) hi_ = mid; else lo_ = mid + 1;
        }
        lo[tid] = lo_;
    }

    // ---- (A) sphere centres of every sample, one walk of the chain each
    const bool point = G.kind == MPB_KIND_POINT;
    if (tid < S && ok) {
        float q[MPB_MAX_DOF];
#pragma unroll
        for (int k = 0; k < MPB_MAX_DOF; ++k) q[k] = (k < D) ? P[(size_t)tid * D + k] : 0.f;
        if (point) {
            cen[tid] = q[0]; cen[S + tid] = q[1]; cen[2 * S + tid] = (G.n_dof > 2) ? q[2] : 0.f;
        } else {
            FKState<false> F;
            fk_identity(F);
            F.frame = 0;
            for (int l = 0; l < L; ++l) {
                const float4 lk = *reinterpret_cast<const float4*>(G.links + 8 * l);      // frame, ox, oy, oz
                const int f = min(__float_as_int(lk.x), G.n_tf);                          // (a checked buffer never clamps: keeps the walk inside tf)
                while (F.frame < f) fk_advance<false>(G, F, q);
                float x, y, z;
                link_centre(F, lk, x, y, z);
                float* c = cen + (size_t)3 * l * S + tid;
                c[0] = x; c[S] = y; c[2 * S] = z;
            }
        }
    }
    __syncthreads();

    // ---- (B) the free table: one lane per row; F[j][i] as bit i & 31 of bits[i >> 5][j]
    const bool dead = !ok || (seg_bad && a.table == nullptr);             // nothing of the table is used: every cell reads as not free
    int jh = 0;                                                           // hold[j] <=> j >= jh: one past the last row that refuses the goal sample
    const int trips = (R + 63) >> 6;
    for (int task = wave; task < trips * W; task += MPB_PT_THREADS / 64) {   // a wave's task: 64 rows x the 32 samples of one word
        const int wd = task / trips, j = (task - wd * trips) * 64 + lane, jc = min(j, R - 1);
        const int i_end = min(32 * wd + 32, S);
        unsigned word = 0u;
        bool free_ = false;
        for (int i = 32 * wd; i < i_end; ++i) {
            free_ = false;
            if (!dead && !(a.blocked != nullptr && a.blocked[(size_t)n * S + i] != 0)) {       // (uniform)
                bool hit = false;
                if (point) {
                    LinkChunk<false> C;
                    C.x[0] = cen[i]; C.y[0] = cen[S + i]; C.z[0] = cen[2 * S + i];
                    C.best[0] = 3.0e38f;
                    moving_chunk_vs_obstacles<false, 1>(T, jc, C);
                    hit = fmaxf(G.margin + G.links[4] - C.best[0], 0.f) > 0.f;
                } else {
                    constexpr int N = LinkChunk<false>::N;
                    for (int l0 = 0; l0 < L; l0 += N) {
                        LinkChunk<false> C;
                        float thr[N];
#pragma unroll
                        for (int s = 0; s < N; ++s) {
                            C.best[s] = 3.0e38f;
                            if (l0 + s < L) {                                                  // (uniform)
                                const float* c = cen + (size_t)3 * (l0 + s) * S + i;
                                C.x[s] = c[0]; C.y[s] = c[S]; C.z[s] = c[2 * S];
                                thr[s] = G.margin + G.links[8 * (l0 + s) + 4];
                            } else {
                                C.x[s] = C.y[s] = C.z[s] = 1.0e9f;                             // parked slot: farther than any obstacle, hinge 0
                                thr[s] = 0.f;
                            }
                        }
                        moving_chunk_vs_obstacles<false, N>(T, jc, C);
#pragma unroll
                        for (int s = 0; s < N; ++s) hit = hit || fmaxf(thr[s] - C.best[s], 0.f) > 0.f;
                        if (__ballot(!hit) == 0ull) break;                                     // every row of the wave already collides here
                    }
                }
                free_ = !hit;
            }
            word |= (free_ ? 1u : 0u) << (i & 31);
        }
        if (j < R) {
            bits[wd * R + j] = word;
            if (i_end == S && !free_) jh = max(jh, j + 1);                // (free_: of sample S - 1)
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) jh = max(jh, __shfl_xor(jh, off, 64));
    if (lane == 0) red[4 + wave] = jh;
    __syncthreads();
    jh = max(max(red[4], red[5]), max(red[6], red[7]));
    const bool f00 = (bits[0] & 1u) != 0u;
    if (a.table != nullptr) {
        unsigned char* tb = a.table + (size_t)n * R * S;
        for (int e = tid; e < R * S; e += MPB_PT_THREADS) {
            const int j = e / S, i = e - j * S;
            tb[e] = (unsigned char)((bits[(i >> 5) * R + j] >> (i & 31)) & 1u);
        }
    }
    int status = MPB_PT_FOUND;
    if (!ok) status = MPB_PT_BUFFER_CHANGED;
    else if (seg_bad) status = MPB_PT_SEGMENT_TOO_LONG;
    else if (!f00) status = MPB_PT_START_BLOCKED;
    else if (jh >= R) status = MPB_PT_GOAL_NOT_HOLDABLE;

    // ---- (C) reachability over the rows, in place
    int jstar = -1;
    if (status == MPB_PT_FOUND) {                                         // (block-uniform)
        __syncthreads();                                                  // (the table was read above)
        if (tid < W) bits[tid * R] = (tid == 0) ? 1u : 0u;                // reach[0]: the start alone
        unsigned m[8];
        const int myl = tid < S ? lo[tid] : 0;
#pragma unroll
        for (int w = 0; w < 8; ++w) m[w] = (tid < S && w < W) ? pt_word_mask(w, myl, tid) : 0u;
        const int gw = (S - 1) >> 5, gb = (S - 1) & 31;
        __syncthreads();
        for (int j = 1; j < R; ++j) {
            unsigned any = 0u, all = 0u;
#pragma unroll
            for (int w = 0; w < 8; ++w) {
                if (w < W) {
                    const unsigned r = bits[w * R + j - 1];                // (a broadcast: every thread reads the same word)
                    any |= r & m[w];
                    all |= r;
                }
            }
            if (all == 0u) break;                                         // (uniform) nothing is reached any more
            const bool f = tid < S && any != 0u && ((bits[(tid >> 5) * R + j] >> (tid & 31)) & 1u) != 0u;
            const unsigned long long b = __ballot(f);
            if (lane == 0) {
                if (2 * wave < W) bits[(2 * wave) * R + j] = (unsigned)b;
                if (2 * wave + 1 < W) bits[(2 * wave + 1) * R + j] = (unsigned)(b >> 32);
            }
            __syncthreads();
            if (j >= jh && ((bits[gw * R + j] >> gb) & 1u) != 0u) { jstar = j; break; }   // (uniform)
        }
        if (jstar < 0) status = MPB_PT_NO_TIMING;
    }

    // ---- (D) the walk back from the arrival row, the gather
    const bool found = status == MPB_PT_FOUND;
    if (found) {
        if (wave == 0) {
            int cur = S - 1;
            if (lane == 0) idxl[jstar] = cur;
            for (int j = jstar; j >= 1; --j) {
                const int l = lo[cur];
                int hit = l;                                              // (reach[j][cur] holds, so a predecessor exists: l is never taken)
                for (int w = cur >> 5; w >= (l >> 5); --w) {
                    const unsigned r = bits[w * R + j - 1] & pt_word_mask(w, l, cur);
                    if (r != 0u) { hit = 32 * w + 31 - __clz((int)r); break; }
                }
                cur = hit;
                if (lane == 0) idxl[j - 1] = cur;
            }
        }
        for (int j = jstar + 1 + tid; j < R; j += MPB_PT_THREADS) idxl[j] = S - 1;
    }
    __syncthreads();
    float* tr = a.trajs + (size_t)n * R * D;
    for (int e = tid; e < R * D; e += MPB_PT_THREADS) {
        const int j = e / D, k = e - j * D;
        tr[e] = found ? P[(size_t)idxl[j] * D + k] : 0.f;
    }
    if (a.idx != nullptr)
        for (int j = tid; j < R; j += MPB_PT_THREADS) a.idx[(size_t)n * R + j] = found ? idxl[j] : -1;
    if (tid == 0) {
        a.status[n] = status;
        if (a.arrival != nullptr) a.arrival[n] = found ? jstar : -1;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------
extern "C" int mpb_path_time_plan(const float* paths, const float* moving, const float* w, const unsigned char* blocked, float* trajs,
                                  int* idx, int* arrival_row, int* status, unsigned char* free_table, int N, int S, int D, int n_rows,
                                  void* stream) {
    const char* who = "mpb_path_time_plan";
    if (D > MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "%s: D = %d exceeds MPB_MAX_DOF = %d", who, D, MPB_MAX_DOF);
    if (S > MPB_PT_MAX_SAMPLES) return mpb_failf(MPB_E_UNSUPPORTED, "%s: n_samples = %d exceeds MPB_PT_MAX_SAMPLES = %d", who, S, MPB_PT_MAX_SAMPLES);
    if (n_rows > MPB_PT_MAX_ROWS) return mpb_failf(MPB_E_UNSUPPORTED, "%s: n_rows = %d exceeds MPB_PT_MAX_ROWS = %d", who, n_rows, MPB_PT_MAX_ROWS);
    if (S < MPB_PT_MIN_SAMPLES) return mpb_failf(MPB_E_INVALID, "%s: n_samples = %d, a path needs at least MPB_PT_MIN_SAMPLES = %d samples", who, S, MPB_PT_MIN_SAMPLES);
    if (n_rows < MPB_PT_MIN_ROWS) return mpb_failf(MPB_E_INVALID, "%s: n_rows = %d, the clock needs at least MPB_PT_MIN_ROWS = %d rows", who, n_rows, MPB_PT_MIN_ROWS);
    if (N < 0 || D < 1) return mpb_failf(MPB_E_INVALID, "%s: bad shape (N %d, D %d)", who, N, D);
    if ((double)N * n_rows * D > 2.0e9 || (double)N * n_rows * S > 2.0e9) return mpb_failf(MPB_E_UNSUPPORTED, "%s: N x n_rows x D or N x n_rows x n_samples too large", who);
    if (N == 0) return MPB_OK;
    if (!paths || !moving || !w || !trajs || !status) return mpb_failf(MPB_E_INVALID, "%s: null pointer", who);
    if (mpb_misaligned16(moving)) return mpb_failf(MPB_E_INVALID, "%s: the moving-obstacle buffer must be 16-byte aligned", who);
    MovingShape M;
    int rc = mpb_moving_shape_cached(moving, M, who);
    if (rc != MPB_OK) return rc;
    if (M.n_rows != n_rows) return mpb_failf(MPB_E_INVALID, "%s: n_rows = %d, the moving-obstacle buffer was packed for n_rows = %d", who, n_rows, M.n_rows);
    if (M.n_dof != D) return mpb_failf(MPB_E_INVALID, "%s: D = %d, the moving-obstacle buffer's robot has n_dof = %d", who, D, M.n_dof);
    const size_t lds = sizeof(float) * (size_t)MPB_PT_LDS_WORDS(M.n_links, S, n_rows);
    if (lds > MPB_PT_MAX_LDS_BYTES)
        return mpb_failf(MPB_E_UNSUPPORTED, "%s: %d collision spheres x %d samples over %d rows need %zu bytes of LDS, above MPB_PT_MAX_LDS_BYTES = %d",
                         who, M.n_links, S, n_rows, lds, MPB_PT_MAX_LDS_BYTES);
    if ((rc = mpb_raise_lds_limit(reinterpret_cast<const void*>(path_time_plan_kernel), M.dev, lds, who))) return rc;
    const PtArgs a = {paths, moving, w, blocked, trajs, idx, arrival_row, status, free_table, S, n_rows, D, M.n_links, M.n_sph, M.n_box};
    hipLaunchKernelGGL(path_time_plan_kernel, dim3(N), dim3(MPB_PT_THREADS), lds, (hipStream_t)stream, a);
    return mpb_check_launch(who);
}
