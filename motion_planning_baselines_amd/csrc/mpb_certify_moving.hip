// mpb_certify_moving.hip -- the clearance of a timed trajectory's rows against a moving-obstacle field, and the certificate that the
// trajectory is collision-free over the whole CONTINUUM of its clock: the bisection of mpb_certify.hip with a motion bound in which
// the obstacles move too.  Build-defined; the definition is in include/mpb.h, the proof in DESIGN.md 10.  Every other kernel of the
// moving-obstacle pipeline decides collisions at the rows of the clock; this file is new code beside them and beside mpb_certify.hip and
// changes nothing they compute (a shared bisection driver for both certifiers is a later deduplication).
//
// The continuum: segment h in 0 .. R - 2, s in [0, 1]: the robot at q_h + s (q_{h+1} - q_h), obstacle o centred on the CHORD
// c_{o,h} + s (c_{o,h+1} - c_{o,h}) of the packed buffer's own per-row centres; the static scene is the geometry chain.
//   eta(h, s) = min_l min( eta_static_l(q), min_o sd_o(x_l(q); c_o(h, s)) - (margin_moving + r_l) )
// Over a parameter half-width w the pair (robot sphere l, moving obstacle o) changes its distance by at most w (Lambda_l + V_{o,h}),
// V_{o,h} = |c_{o,h+1} - c_{o,h}| formed in the lane and inflated as Lambda_l is; a static pair by w Lambda_l.
//
// moving_clearance_kernel: one lane per (trajectory, row): eta, its robot sphere and its obstacle at the row's own time.
//
// traj_certify_moving_kernel: ONE launch, one single-wave workgroup per trajectory, the shape of path_certify_kernel: level -1 on the
// nodes, then the levels' intervals as packed words (segment << MPB_CERT_J_BITS | j) in two ping-pong queues in LDS, one lane per
// interval in trips of 64, children appended in order by ballot + prefix count.  Every value that steers control flow comes out of a
// ballot; no atomics, no waits on other workgroups; every loop is bounded by R, max_depth, max_intervals, the link count, the obstacle
// counts or MPB_MAX_FIELDS.  The minima are taken in a fixed order: the same bits on every run.
//
// Arithmetic: the code BELOW the pragma is compiled with contraction off and writes every fused multiply-add it wants as fmaf(), so the
// fp32 restatement (tests/st_certify_checks.py) follows it operation by operation.  The evaluators it calls -- sphere_sd, box_sd,
// clr_point_distance, fk_advance, link_centre -- sit in headers included ABOVE the pragma and are compiled as they are everywhere else:
// eta_static is the bits of mpb_clearance.
#include "mpb_clearance.h"
#include "mpb_host.h"
#include "mpb_moving.h"
#include "../../include/mpb_st_certify_layout.h"

#pragma clang fp contract(off)

struct STCArgs {
    const float* trajs;
    size_t row_stride;
    const float* geom;
    const float* mob;
    const float* reach;
    int* out_i;
    float* out_f;
    int R, D, L, n_sph, n_box, max_depth, max_intervals;
    float S, c_req;
};

// what a lane keeps of one (configuration, time): min eta with its robot sphere, that sphere's centre and its obstacle (o >= 0 moving,
// -1: the static scene), and the min over pairs of eta_pair - w bound_pair
struct STCEval {
    float eta, bound, x, y, z;
    int link, obst;
};

// min_o sd_o and min_o (sd_o - w (lam + V_o)) of the point (x, y, z) against every moving obstacle centred at
// fmaf(c_{o,h1} - c_{o,h0}, s, c_{o,h0}); spheres first, then boxes, a strict < keeps the first minimum.  moving_chunk_vs_obstacles of
// mpb_moving.h keeps only the first of the two and reads one row; this walk stands beside it.  h0, h1 < T.stride.
__device__ __forceinline__ void stc_moving_walk(const MovingTables& T, int h0, int h1, float s, float w, float lam, float x, float y, float z,
                                                float& best, int& arg, float& best_b) {
    const float* c0 = T.centres + h0;
    const float* c1 = T.centres + h1;
    const float4* hp = reinterpret_cast<const float4*>(T.half);
    const int n = T.n_sph + T.n_box;
    for (int o = 0; o < n; ++o) {
        const float ax = c0[0], ay = c0[T.stride], az = c0[2 * T.stride];
        const float dx = c1[0] - ax, dy = c1[T.stride] - ay, dz = c1[2 * T.stride] - az;
        const float4 c = make_float4(fmaf(dx, s, ax), fmaf(dy, s, ay), fmaf(dz, s, az), (o < T.n_sph) ? T.radii[min(o, max(T.n_sph - 1, 0))] : 0.f);
        const float V = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx))) * MPB_CERT_LAMBDA_INFLATE;
        const float sd = (o < T.n_sph) ? sphere_sd(x, y, z, c) : box_sd(x, y, z, c, hp[max(o - T.n_sph, 0)]);     // (o: wave-uniform)
        arg = (sd < best) ? o : arg;
        best = fminf(best, sd);
        best_b = fminf(best_b, fmaf(-w, lam + V, sd));
        c0 += 3 * T.stride;
        c1 += 3 * T.stride;
    }
}

// one configuration m at parameter s of segment h0 -> h1 (a node: h1 == h0 or s == 0, w == 0: no motion bound is formed), on the step of
// absolute joint differences ad
__device__ __forceinline__ STCEval stc_eval(const STCArgs& a, const MovingTables& T, const float (&m)[MPB_MAX_DOF], const float (&ad)[MPB_MAX_DOF],
                                            int h0, int h1, float s, float w, bool point) {
    STCEval e = {3.0e38f, 3.0e38f, 0.f, 0.f, 0.f, -1, -1};
    const float* rho = a.reach + MPB_REACH_HEADER_WORDS;
    const float margin_m = a.mob[MPB_VW_MARGIN];
    const GeomView G = geom_view(a.geom);
    float len = 0.f;
    if (point) {                                                 // a point robot: Lambda = |b - a|_2
#pragma unroll
        for (int i = 0; i < 3; ++i) len = fmaf(ad[i], ad[i], len);
        len = sqrtf(len);
    }
    auto per_sphere = [&](int l, float x, float y, float z, float r_l) {
        float lam = len;
        if (!point && w > 0.f) {
#pragma unroll
            for (int i = 0; i < MPB_MAX_DOF; ++i)
                if (i < a.D) lam = fmaf(ad[i], rho[i * a.L + l], lam);
        }
        lam *= MPB_CERT_LAMBDA_INFLATE;
        const float eta_s = clr_point_distance(a.geom, x, y, z) - r_l;
        float sd_m = 3.0e38f, sd_b = 3.0e38f;
        int o_m = -1;
        stc_moving_walk(T, h0, h1, s, w, lam, x, y, z, sd_m, o_m, sd_b);
        const float thr = margin_m + r_l;
        const float eta_m = sd_m - thr;                           // (its sign is the moving predicate's: thr - sd_m > 0)
        const float eta_l = fminf(eta_s, eta_m);
        const int o_l = (eta_m < eta_s) ? o_m : -1;               // (a tie: the static scene)
        const bool better = eta_l < e.eta;                        // (strict: the lowest sphere on a tie)
        e.link = better ? l : e.link;
        e.obst = better ? o_l : e.obst;
        e.x = better ? x : e.x; e.y = better ? y : e.y; e.z = better ? z : e.z;
        e.eta = fminf(e.eta, eta_l);
        e.bound = fminf(e.bound, fminf(fmaf(-w, lam, eta_s), sd_b - thr));
    };
    if (G.kind == MPB_KIND_POINT) {
        per_sphere(0, m[0], m[1], (G.n_dof > 2) ? m[2] : 0.f, G.links[4]);
        return e;
    }
    FKState<false> F;
    fk_identity(F);
    F.frame = 0;
    for (int l = 0; l < G.n_links; ++l) {
        const float4 lk = *reinterpret_cast<const float4*>(G.links + 8 * l);   // frame, ox, oy, oz
        const int f = min(__float_as_int(lk.x), G.n_tf);
        while (F.frame < f) fk_advance<false>(G, F, m);
        float x, y, z;
        link_centre(F, lk, x, y, z);
        per_sphere(l, x, y, z, G.links[8 * l + 4]);
    }
    return e;
}

// which chained field holds the static minimum at a point: arg min_f (sd_f - margin_f), the first on a tie (clr_point_distance keeps the
// value alone; asked once per witness / per row)
__device__ __forceinline__ int stc_static_field(const float* __restrict__ geom, float x, float y, float z) {
    float best = 3.0e38f;
    int arg = 0, n = 0;
    for (const float* gp = geom; gp != nullptr && n < MPB_MAX_FIELDS; gp = geom_next(gp), ++n) {
        const int* gi = reinterpret_cast<const int*>(gp);
        const int n_sph = gi[MPB_GW_N_SPH], n_box = gi[MPB_GW_N_BOX];
        const float4* sp = reinterpret_cast<const float4*>(gp + gi[MPB_GW_OFF_SPH]);
        const float4* bp = reinterpret_cast<const float4*>(gp + gi[MPB_GW_OFF_BOX]);
        float sd = 3.0e38f;
        for (int o = 0; o < n_sph; ++o) sd = fminf(sd, sphere_sd(x, y, z, sp[o]));
        for (int o = 0; o < n_box; ++o) sd = fminf(sd, box_sd(x, y, z, bp[2 * o], bp[2 * o + 1]));
        const float v = sd - gp[MPB_GW_MARGIN];
        arg = (v < best) ? n : arg;
        best = fminf(best, v);
    }
    return arg;
}

__device__ __forceinline__ bool stc_headers_ok(const STCArgs& a) {
    const int* rh = reinterpret_cast<const int*>(a.reach);
    return clr_headers_ok(a.geom, a.D, a.L) && moving_header_matches(a.mob, a.D, a.L, a.R, a.n_sph, a.n_box) && rh[0] == MPB_REACH_MAGIC &&
           rh[1] == a.D && rh[2] == a.L;
}

// ---- clearance of the rows at their own times ------------------------------------------------------------------------------------
// (a.reach is not read: w == 0 forms no motion bound; the header test is the geometry's and the moving buffer's)
__global__ __launch_bounds__(64) void moving_clearance_kernel(const STCArgs a, float* __restrict__ eta, int* __restrict__ link,
                                                              int* __restrict__ obstacle, int N) {
    const long long total = (long long)N * a.R;
    const long long idx = (long long)blockIdx.x * 64 + threadIdx.x;
    const long long ic = idx < total ? idx : total - 1;
    const int n = (int)(ic / a.R), h = (int)(ic % a.R);
    const bool ok = clr_headers_ok(a.geom, a.D, a.L) && moving_header_matches(a.mob, a.D, a.L, a.R, a.n_sph, a.n_box);   // (wave-uniform)
    float best = __uint_as_float(0x7FC00000u);
    int arg_l = -1, arg_o = MPB_STC_NO_OBSTACLE;
    if (ok) {
        const MovingTables T = moving_tables(a.mob, a.R, a.n_sph, a.n_box);
        const bool point = reinterpret_cast<const int*>(a.geom)[MPB_GW_KIND] == MPB_KIND_POINT;
        const float* row = a.trajs + ((size_t)n * a.R + h) * a.row_stride;
        float q[MPB_MAX_DOF], zero[MPB_MAX_DOF];
#pragma unroll
        for (int i = 0; i < MPB_MAX_DOF; ++i) { q[i] = (i < a.D) ? row[i] : 0.f; zero[i] = 0.f; }
        const STCEval e = stc_eval(a, T, q, zero, h, h, 0.f, 0.f, point);
        best = e.eta;
        arg_l = e.link;
        arg_o = (e.obst >= 0) ? e.obst : -1 - stc_static_field(a.geom, e.x, e.y, e.z);
    }
    if (idx < total) {
        eta[idx] = best;
        if (link != nullptr) link[idx] = arg_l;
        if (obstacle != nullptr) obstacle[idx] = arg_o;
    }
}

// ---- the certifier --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void traj_certify_moving_kernel(const STCArgs a) {
    extern __shared__ unsigned stc_queue[];                      // two arrays of max_intervals words
    const int b = blockIdx.x, lane = threadIdx.x;
    const int D = a.D, R = a.R;
    const float* P = a.trajs + (size_t)b * R * a.row_stride;
    int status = MPB_CERT_FREE, w_seg = -1, w_link = -1, w_obst = MPB_STC_NO_OBSTACLE, n_evals = 0, depth_max = -1;
    float w_s = 0.f, w_eta = 0.f, cert = 3.0e38f;

    const bool headers = stc_headers_ok(a);
    if (!headers) status = MPB_CERT_BUFFER_CHANGED;
    if (status == MPB_CERT_FREE) {                               // a non-finite coordinate, decided on the bits (the build assumes finite math)
        bool bad = false;
        for (int r = lane; r < R; r += 64)
            for (int i = 0; i < D; ++i) bad = bad || (__float_as_uint(P[(size_t)r * a.row_stride + i]) & 0x7F800000u) == 0x7F800000u;
        if (__any(bad)) status = MPB_CERT_BAD_INPUT;
    }
    const bool point = headers && reinterpret_cast<const int*>(a.geom)[MPB_GW_KIND] == MPB_KIND_POINT;
    const MovingTables T = moving_tables(a.mob, R, a.n_sph, a.n_box);      // (the launcher's counts: every centre index stays inside the section)
    const float thr_free = a.S, thr_coll = -a.S;
    float wx = 0.f, wy = 0.f, wz = 0.f;                          // the witness sphere's centre

    // level -1: the nodes, each against its own row of centres
    if (status == MPB_CERT_FREE) {
        float zero[MPB_MAX_DOF];
#pragma unroll
        for (int i = 0; i < MPB_MAX_DOF; ++i) zero[i] = 0.f;
        for (int base = 0; base < R; base += 64) {
            const int r = min(base + lane, R - 1);
            const bool active = base + lane < R;
            const float* row = P + (size_t)r * a.row_stride;
            float q[MPB_MAX_DOF];
#pragma unroll
            for (int i = 0; i < MPB_MAX_DOF; ++i) q[i] = (i < D) ? row[i] : 0.f;
            const STCEval e = stc_eval(a, T, q, zero, r, r, 0.f, 0.f, point);
            n_evals += min(64, R - base);
            const unsigned long long hit = __ballot(active && e.eta - a.c_req < thr_coll);
            if (hit != 0ull) {
                const int src = (int)__builtin_ctzll(hit);
                status = MPB_CERT_COLLISION;
                w_seg = base + src;
                w_s = 0.f;
                w_link = __shfl(e.link, src, 64);
                w_obst = __shfl(e.obst, src, 64);
                w_eta = __shfl(e.eta, src, 64);
                wx = __shfl(e.x, src, 64); wy = __shfl(e.y, src, 64); wz = __shfl(e.z, src, 64);
                break;
            }
            if (R == 1) cert = __shfl(e.eta, 0, 64) - a.c_req;   // a trajectory of one row: the continuum is its node
        }
    }

    // level 0: one interval per segment
    unsigned* cur = stc_queue;
    unsigned* nxt = stc_queue + a.max_intervals;
    int n_cur = 0;
    if (status == MPB_CERT_FREE && R >= 2) {
        if (R - 1 > a.max_intervals) {
            status = MPB_CERT_UNDECIDED_QUEUE;
        } else {
            n_cur = R - 1;
            for (int i = lane; i < n_cur; i += 64) cur[i] = (unsigned)i << MPB_CERT_J_BITS;
        }
    }
    __syncthreads();

    bool undecided = false;
    float lane_cert = 3.0e38f;
    for (int d = 0; d <= a.max_depth && status == MPB_CERT_FREE && n_cur > 0; ++d) {
        const float w = __uint_as_float((unsigned)(127 - (d + 1)) << 23);      // 2^-(d+1)
        int n_nxt = 0;
        bool overflow = false;
        depth_max = d;
        for (int base = 0; base < n_cur; base += 64) {
            const int idx = base + lane;
            const bool active = idx < n_cur;
            const unsigned word = cur[min(idx, n_cur - 1)];
            const int seg = min((int)(word >> MPB_CERT_J_BITS), R - 2);           // (a queue word never exceeds it: keeps row seg + 1 inside the table)
            const unsigned j = word & ((1u << MPB_CERT_J_BITS) - 1u);
            const float s = (float)(2u * j + 1u) * w;                             // exact: 2j + 1 < 2^21
            const float* r0 = P + (size_t)seg * a.row_stride;
            const float* r1 = r0 + a.row_stride;
            float m[MPB_MAX_DOF], ad[MPB_MAX_DOF];
#pragma unroll
            for (int i = 0; i < MPB_MAX_DOF; ++i) {
                const float x0 = (i < D) ? r0[i] : 0.f, x1 = (i < D) ? r1[i] : 0.f;
                const float dl = x1 - x0;
                m[i] = fmaf(dl, s, x0);
                ad[i] = fabsf(dl);
            }
            const STCEval e = stc_eval(a, T, m, ad, seg, seg + 1, s, w, point);
            n_evals += min(64, n_cur - base);
            const bool coll = e.eta - a.c_req < thr_coll;
            const bool is_free = e.bound - a.c_req > thr_free;
            const unsigned long long hit = __ballot(active && coll);
            if (hit != 0ull) {
                const int src = (int)__builtin_ctzll(hit);
                status = MPB_CERT_COLLISION;
                w_seg = __shfl(seg, src, 64);
                w_s = __shfl(s, src, 64);
                w_link = __shfl(e.link, src, 64);
                w_obst = __shfl(e.obst, src, 64);
                w_eta = __shfl(e.eta, src, 64);
                wx = __shfl(e.x, src, 64); wy = __shfl(e.y, src, 64); wz = __shfl(e.z, src, 64);
                break;
            }
            if (active && is_free) lane_cert = fminf(lane_cert, e.bound - a.c_req);
            const unsigned long long split = __ballot(active && !is_free);
            if (split != 0ull) {
                if (d == a.max_depth) {
                    undecided = true;
                } else if (!overflow) {
                    const int n_split = __popcll(split);
                    if (n_nxt + 2 * n_split > a.max_intervals) {
                        overflow = true;                         // the level is still walked to its end: a collision in it wins
                    } else {
                        if (active && !is_free) {
                            const int at = n_nxt + 2 * __popcll(split & ((1ull << lane) - 1ull));
                            const unsigned child = ((unsigned)seg << MPB_CERT_J_BITS) | (2u * j);
                            nxt[at] = child;
                            nxt[at + 1] = child + 1u;
                        }
                        n_nxt += 2 * n_split;
                    }
                }
            }
        }
        __syncthreads();
        if (status != MPB_CERT_FREE) break;
        if (overflow) {
            status = MPB_CERT_UNDECIDED_QUEUE;
            break;
        }
        unsigned* sw = cur; cur = nxt; nxt = sw;
        n_cur = n_nxt;
    }
    if (status == MPB_CERT_FREE && undecided) status = MPB_CERT_UNDECIDED_DEPTH;
    // the witness of the static scene names its field (wave-uniform: every lane holds the witness)
    if (status == MPB_CERT_COLLISION && w_obst < 0) w_obst = -1 - stc_static_field(a.geom, wx, wy, wz);

#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) lane_cert = fminf(lane_cert, __shfl_xor(lane_cert, off, 64));
    cert = fminf(cert, lane_cert);
    if (lane == 0) {
        int* oi = a.out_i + (size_t)b * MPB_STC_OUT_INTS;
        float* of = a.out_f + (size_t)b * MPB_STC_OUT_FLOATS;
        oi[0] = status; oi[1] = w_seg; oi[2] = w_link; oi[3] = w_obst; oi[4] = n_evals; oi[5] = depth_max;
        of[0] = w_s; of[1] = w_eta;
        of[2] = (status == MPB_CERT_FREE) ? cert : __uint_as_float(0xFF800000u);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static bool stc_not_finite(float v) {
    uint32_t bits;
    memcpy(&bits, &v, 4);
    return (bits & 0x7F800000u) == 0x7F800000u;
}

// the shape of the moving buffer against the launch: its robot, and exactly the row count the centres were evaluated for
static int stc_shape(const char* who, const float* mob, int R, int D, MovingShape& S) {
    int rc = mpb_moving_shape_cached(mob, S, who);
    if (rc) return rc;
    if (S.n_dof != D) return mpb_failf(MPB_E_INVALID, "%s: D = %d, the moving-obstacle buffer holds a robot of %d coordinates", who, D, S.n_dof);
    if (R != S.n_rows)
        return mpb_failf(MPB_E_INVALID, "%s: trajectories of R = %d rows, the moving-obstacle buffer was packed for n_rows = %d", who, R, S.n_rows);
    return MPB_OK;
}

extern "C" int mpb_moving_clearance(const float* trajs, size_t row_stride, const float* geom, const float* moving, float* eta, int* link,
                                    int* obstacle, int N, int R, int D, void* stream) {
    if (D > MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "mpb_moving_clearance: D = %d exceeds MPB_MAX_DOF = %d", D, MPB_MAX_DOF);
    if (R < 1 || R > MPB_MOVING_MAX_ROWS)
        return mpb_failf(MPB_E_UNSUPPORTED, "mpb_moving_clearance: R = %d outside 1 .. MPB_MOVING_MAX_ROWS = %d", R, MPB_MOVING_MAX_ROWS);
    if (N < 0 || D < 1 || row_stride < (size_t)D) return mpb_failf(MPB_E_INVALID, "mpb_moving_clearance: bad shape (N %d, D %d, row_stride %zu)", N, D, row_stride);
    if (N == 0) return MPB_OK;
    if (!trajs || !geom || !moving || !eta) return mpb_fail(MPB_E_INVALID, "mpb_moving_clearance: null pointer");
    if (mpb_misaligned16(geom, moving)) return mpb_fail(MPB_E_INVALID, "mpb_moving_clearance: geom and the moving-obstacle buffer must be 16-byte aligned");
    MovingShape S;
    const int rc = stc_shape("mpb_moving_clearance", moving, R, D, S);
    if (rc) return rc;
    const STCArgs a = {trajs, row_stride, geom, moving, nullptr, nullptr, nullptr, R, D, S.n_links, S.n_sph, S.n_box, 0, 0, 0.f, 0.f};
    const long long total = (long long)N * R;
    hipLaunchKernelGGL(moving_clearance_kernel, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a, eta, link, obstacle, N);
    return mpb_check_launch("mpb_moving_clearance");
}

extern "C" int mpb_traj_certify_moving(const float* trajs, size_t row_stride, const float* geom, const float* moving, const float* reach,
                                       int n_links, float S, float c_req, int max_depth, int max_intervals, int* out_i, float* out_f, int N,
                                       int R, int D, void* stream) {
    const char* who = "mpb_traj_certify_moving";
    if (D > MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "%s: D = %d exceeds MPB_MAX_DOF = %d", who, D, MPB_MAX_DOF);
    if (R < 1 || R > MPB_MOVING_MAX_ROWS)
        return mpb_failf(MPB_E_UNSUPPORTED, "%s: R = %d outside 1 .. MPB_MOVING_MAX_ROWS = %d (the rows of a moving-obstacle buffer)", who, R, MPB_MOVING_MAX_ROWS);
    if (max_depth < 0 || max_depth > MPB_CERT_MAX_DEPTH)
        return mpb_failf(MPB_E_UNSUPPORTED, "%s: max_depth = %d outside 0 .. MPB_CERT_MAX_DEPTH = %d (the j field of the interval word)", who, max_depth, MPB_CERT_MAX_DEPTH);
    if (max_intervals < 1 || max_intervals > MPB_CERT_MAX_INTERVALS)
        return mpb_failf(MPB_E_UNSUPPORTED, "%s: max_intervals = %d outside 1 .. MPB_CERT_MAX_INTERVALS = %d (the queue lives in LDS)", who, max_intervals, MPB_CERT_MAX_INTERVALS);
    if (n_links < 1 || n_links > MPB_MOVING_MAX_LINKS)
        return mpb_failf(MPB_E_UNSUPPORTED, "%s: n_links = %d outside 1 .. MPB_MOVING_MAX_LINKS = %d", who, n_links, MPB_MOVING_MAX_LINKS);
    if (N < 0 || D < 1 || row_stride < (size_t)D) return mpb_failf(MPB_E_INVALID, "%s: bad shape (N %d, D %d, row_stride %zu)", who, N, D, row_stride);
    if (stc_not_finite(S) || S < 0.f) return mpb_failf(MPB_E_INVALID, "%s: the slack S must be finite and >= 0", who);
    if (stc_not_finite(c_req)) return mpb_failf(MPB_E_INVALID, "%s: c_req must be finite", who);
    if (N == 0) return MPB_OK;
    if (!trajs || !geom || !moving || !reach || !out_i || !out_f) return mpb_failf(MPB_E_INVALID, "%s: null pointer", who);
    if (mpb_misaligned16(geom, moving, reach)) return mpb_failf(MPB_E_INVALID, "%s: geom, the moving-obstacle buffer and reach must be 16-byte aligned", who);
    MovingShape Sh;
    const int rc = stc_shape(who, moving, R, D, Sh);
    if (rc) return rc;
    if (Sh.n_links != n_links)
        return mpb_failf(MPB_E_INVALID, "%s: n_links = %d, the moving-obstacle buffer holds a robot of %d collision spheres", who, n_links, Sh.n_links);
    const STCArgs a = {trajs, row_stride, geom, moving, reach, out_i, out_f, R, D, n_links, Sh.n_sph, Sh.n_box, max_depth, max_intervals, S, c_req};
    hipLaunchKernelGGL(traj_certify_moving_kernel, dim3(N), dim3(64), 2 * sizeof(unsigned) * (size_t)max_intervals, (hipStream_t)stream, a);
    return mpb_check_launch(who);
}
