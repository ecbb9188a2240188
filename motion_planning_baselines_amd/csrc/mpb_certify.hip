// mpb_certify.hip -- the clearance op and the certificate that a joint-space polyline is collision-free BETWEEN its samples: adaptive
// dynamic collision checking (Schwarzer, Saha, Latombe) in its one-point form -- bisection with a motion bound.  Build-defined; the
// definition is in include/mpb.h, the proof in DESIGN.md 10.  Every other collision decision of this library is made at sample
// points; this file is new code beside those kernels and changes nothing they compute.
//
// clearance_kernel: one lane per configuration, the walk of mpb_clearance.h with a running minimum and its sphere.
//
// path_certify_kernel: ONE launch, one single-wave workgroup per path.
//   - level -1: the nodes in trips of 64, one lane per node; the first colliding lane of the first colliding trip is the witness;
//   - level d >= 0: the level's intervals are a queue of packed words (segment << MPB_CERT_J_BITS | j) in LDS, two ping-pong arrays of
//     max_intervals words; one lane per interval in trips of 64.  A lane forms its midpoint from the two rows of its segment (read in
//     place, the caller's stride), walks the chain once and keeps three things over the spheres: min eta_l with its sphere, min of
//     eta_l - w Lambda_l.  Lambda_l = sum_i |b_i - a_i| rho_il is formed per sphere from the reach table through wave-uniform loads.
//   - children are appended in order by ballot + prefix count, so the queue stays sorted by (segment, j): the first colliding lane
//     of the first colliding trip of a level is its smallest (segment, t), and a level stops there;
//   - every value that steers control flow comes out of a ballot: the control flow is wave-uniform.  No atomics, no waits on other
//     workgroups; every loop is bounded by the length, max_depth, max_intervals, the link count or MPB_MAX_FIELDS.  The minima are
//     taken in a fixed order: the same bits on every run, and a path's bits depend on its own inputs only.
#include "mpb_clearance.h"
#include "mpb_host.h"

// ---- clearance of configurations ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void clearance_kernel(const float* __restrict__ qs, const float* __restrict__ geom, float* __restrict__ eta,
                                                       int* __restrict__ link, int N, int D) {
    const int L = reinterpret_cast<const int*>(geom)[MPB_GW_N_LINKS];   // (the chained fields are held to the first one's link count)
    const int n = blockIdx.x * 64 + threadIdx.x;
    const int nc = min(n, N - 1);
    float q[MPB_MAX_DOF];
#pragma unroll
    for (int i = 0; i < MPB_MAX_DOF; ++i) q[i] = (i < D) ? qs[(size_t)nc * D + i] : 0.f;
    float best = __uint_as_float(0x7FC00000u);
    int arg = -1;
    if (clr_headers_ok(geom, D, L)) {                          // (wave-uniform)
        best = 3.0e38f;
        clearance_walk(geom, q, [&](int l, float e) {
            arg = (e < best) ? l : arg;                          // (strict: the lowest index on a tie)
            best = fminf(best, e);
        });
    }
    if (n < N) {
        eta[n] = best;
        if (link != nullptr) link[n] = arg;
    }
}

// ---- the certifier --------------------------------------------------------------------------------------------------------------
struct CertArgs {
    const float* paths;
    size_t row_stride;
    const int* lengths;
    const float* geom;
    const float* reach;
    int* out_i;
    float* out_f;
    int H, D, L, max_depth, max_intervals;
    float S, c_req;
};

// what a lane keeps of one configuration: min_l eta_l and its sphere, min_l (eta_l - w Lambda_l)
struct CertEval {
    float eta, bound;
    int link;
};

// one configuration m on the step of absolute joint differences ad, half-width w (0: a node, no motion bound is formed)
__device__ __forceinline__ CertEval cert_eval(const CertArgs& a, const float (&m)[MPB_MAX_DOF], const float (&ad)[MPB_MAX_DOF], float w,
                                              bool point) {
    CertEval e = {3.0e38f, 3.0e38f, -1};
    const float* rho = a.reach + MPB_REACH_HEADER_WORDS;
    float len = 0.f;
    if (point) {                                                 // a point robot: Lambda = |b - a|_2
#pragma unroll
        for (int i = 0; i < 3; ++i) len = fmaf(ad[i], ad[i], len);
        len = sqrtf(len);
    }
    clearance_walk(a.geom, m, [&](int l, float eta_l) {
        float lam = len;
        if (!point && w > 0.f) {
#pragma unroll
            for (int i = 0; i < MPB_MAX_DOF; ++i)
                if (i < a.D) lam = fmaf(ad[i], rho[i * a.L + l], lam);
        }
        lam *= MPB_CERT_LAMBDA_INFLATE;
        e.link = (eta_l < e.eta) ? l : e.link;
        e.eta = fminf(e.eta, eta_l);
        e.bound = fminf(e.bound, fmaf(-w, lam, eta_l));
    });
    return e;
}

__global__ __launch_bounds__(64) void path_certify_kernel(const CertArgs a) {
    extern __shared__ unsigned cert_queue[];                     // two arrays of max_intervals words
    const int b = blockIdx.x, lane = threadIdx.x;
    const int D = a.D;
    const float* P = a.paths + (size_t)b * a.H * a.row_stride;
    int status = MPB_CERT_FREE, w_seg = -1, w_link = -1, n_evals = 0, depth_max = -1;
    float w_t = 0.f, w_eta = 0.f, cert = 3.0e38f;

    const int* rh = reinterpret_cast<const int*>(a.reach);
    const bool headers = clr_headers_ok(a.geom, D, a.L) && rh[0] == MPB_REACH_MAGIC && rh[1] == D && rh[2] == a.L;
    const int Lp = (a.lengths != nullptr) ? a.lengths[b] : a.H;
    if (!headers) status = MPB_CERT_BUFFER_CHANGED;
    else if (Lp < 1 || Lp > a.H) status = MPB_CERT_BAD_INPUT;
    if (status == MPB_CERT_FREE) {                               // a non-finite coordinate, decided on the bits (the build assumes finite math)
        bool bad = false;
        for (int r = lane; r < Lp; r += 64)
            for (int i = 0; i < D; ++i) bad = bad || (__float_as_uint(P[(size_t)r * a.row_stride + i]) & 0x7F800000u) == 0x7F800000u;
        if (__any(bad)) status = MPB_CERT_BAD_INPUT;
    }
    const bool point = headers && reinterpret_cast<const int*>(a.geom)[MPB_GW_KIND] == MPB_KIND_POINT;
    const float thr_free = a.S, thr_coll = -a.S;

    // level -1: the nodes
    if (status == MPB_CERT_FREE) {
        float zero[MPB_MAX_DOF];
#pragma unroll
        for (int i = 0; i < MPB_MAX_DOF; ++i) zero[i] = 0.f;
        for (int base = 0; base < Lp; base += 64) {
            const int r = base + lane;
            const bool active = r < Lp;
            const float* row = P + (size_t)min(r, Lp - 1) * a.row_stride;
            float q[MPB_MAX_DOF];
#pragma unroll
            for (int i = 0; i < MPB_MAX_DOF; ++i) q[i] = (i < D) ? row[i] : 0.f;
            const CertEval e = cert_eval(a, q, zero, 0.f, point);
            n_evals += min(64, Lp - base);
            const unsigned long long hit = __ballot(active && e.eta - a.c_req < thr_coll);
            if (hit != 0ull) {
                const int src = (int)__builtin_ctzll(hit);
                status = MPB_CERT_COLLISION;
                w_seg = base + src;
                w_t = 0.f;
                w_link = __shfl(e.link, src, 64);
                w_eta = __shfl(e.eta, src, 64);
                break;
            }
            if (Lp == 1) cert = __shfl(e.eta, 0, 64) - a.c_req;  // a path of one row: the continuum is its node
        }
    }

    // level 0: one interval per segment
    unsigned* cur = cert_queue;
    unsigned* nxt = cert_queue + a.max_intervals;
    int n_cur = 0;
    if (status == MPB_CERT_FREE && Lp >= 2) {
        if (Lp - 1 > a.max_intervals) {
            status = MPB_CERT_UNDECIDED_QUEUE;
        } else {
            n_cur = Lp - 1;
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
            const int seg = (int)(word >> MPB_CERT_J_BITS);
            const unsigned j = word & ((1u << MPB_CERT_J_BITS) - 1u);
            const float t = (float)(2u * j + 1u) * w;                             // exact: 2j + 1 < 2^21
            const float* r0 = P + (size_t)seg * a.row_stride;
            const float* r1 = r0 + a.row_stride;
            float m[MPB_MAX_DOF], ad[MPB_MAX_DOF];
#pragma unroll
            for (int i = 0; i < MPB_MAX_DOF; ++i) {
                const float x0 = (i < D) ? r0[i] : 0.f, x1 = (i < D) ? r1[i] : 0.f;
                const float dl = x1 - x0;
                m[i] = fmaf(dl, t, x0);
                ad[i] = fabsf(dl);
            }
            const CertEval e = cert_eval(a, m, ad, w, point);
            n_evals += min(64, n_cur - base);
            const bool coll = e.eta - a.c_req < thr_coll;
            const bool is_free = e.bound - a.c_req > thr_free;
            const unsigned long long hit = __ballot(active && coll);
            if (hit != 0ull) {
                const int src = (int)__builtin_ctzll(hit);
                status = MPB_CERT_COLLISION;
                w_seg = __shfl(seg, src, 64);
                w_t = __shfl(t, src, 64);
                w_link = __shfl(e.link, src, 64);
                w_eta = __shfl(e.eta, src, 64);
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

#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) lane_cert = fminf(lane_cert, __shfl_xor(lane_cert, off, 64));
    cert = fminf(cert, lane_cert);
    if (lane == 0) {
        int* oi = a.out_i + (size_t)b * MPB_CERT_OUT_INTS;
        float* of = a.out_f + (size_t)b * MPB_CERT_OUT_FLOATS;
        oi[0] = status; oi[1] = w_seg; oi[2] = w_link; oi[3] = n_evals; oi[4] = depth_max;
        of[0] = w_t; of[1] = w_eta;
        of[2] = (status == MPB_CERT_FREE) ? cert : __uint_as_float(0xFF800000u);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static bool cert_not_finite(float v) {
    uint32_t bits;
    memcpy(&bits, &v, 4);
    return (bits & 0x7F800000u) == 0x7F800000u;
}

extern "C" int mpb_clearance(const float* q, const float* geom, float* eta, int* link, int N, int D, void* stream) {
    if (D > MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "mpb_clearance: D = %d exceeds MPB_MAX_DOF = %d", D, MPB_MAX_DOF);
    if (N < 0 || D < 1) return mpb_failf(MPB_E_INVALID, "mpb_clearance: bad shape (N %d, D %d)", N, D);
    if (N == 0) return MPB_OK;
    if (!q || !geom || !eta) return mpb_fail(MPB_E_INVALID, "mpb_clearance: null pointer");
    if (mpb_misaligned16(geom)) return mpb_fail(MPB_E_INVALID, "mpb_clearance: geom must be 16-byte aligned");
    hipLaunchKernelGGL(clearance_kernel, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, q, geom, eta, link, N, D);
    return mpb_check_launch("mpb_clearance");
}

extern "C" int mpb_path_certify(const float* paths, size_t row_stride, const int* lengths, const float* geom, const float* reach,
                                int n_links, float S, float c_req, int max_depth, int max_intervals, int* out_i, float* out_f, int N, int H,
                                int D, void* stream) {
    if (D > MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "mpb_path_certify: D = %d exceeds MPB_MAX_DOF = %d", D, MPB_MAX_DOF);
    if (H < 1 || H > MPB_CERT_MAX_ROWS)
        return mpb_failf(MPB_E_UNSUPPORTED, "mpb_path_certify: H = %d outside 1 .. MPB_CERT_MAX_ROWS = %d (the segment field of the interval word)", H, MPB_CERT_MAX_ROWS);
    if (max_depth < 0 || max_depth > MPB_CERT_MAX_DEPTH)
        return mpb_failf(MPB_E_UNSUPPORTED, "mpb_path_certify: max_depth = %d outside 0 .. MPB_CERT_MAX_DEPTH = %d (the j field of the interval word)", max_depth, MPB_CERT_MAX_DEPTH);
    if (max_intervals < 1 || max_intervals > MPB_CERT_MAX_INTERVALS)
        return mpb_failf(MPB_E_UNSUPPORTED, "mpb_path_certify: max_intervals = %d outside 1 .. MPB_CERT_MAX_INTERVALS = %d (the queue lives in LDS)", max_intervals, MPB_CERT_MAX_INTERVALS);
    if (n_links < 1 || n_links > MPB_CERT_MAX_LINKS)
        return mpb_failf(MPB_E_UNSUPPORTED, "mpb_path_certify: n_links = %d outside 1 .. MPB_CERT_MAX_LINKS = %d", n_links, MPB_CERT_MAX_LINKS);
    if (N < 0 || D < 1 || row_stride < (size_t)D) return mpb_failf(MPB_E_INVALID, "mpb_path_certify: bad shape (N %d, D %d, row_stride %zu)", N, D, row_stride);
    if (cert_not_finite(S) || S < 0.f) return mpb_fail(MPB_E_INVALID, "mpb_path_certify: the slack S must be finite and >= 0");
    if (cert_not_finite(c_req)) return mpb_fail(MPB_E_INVALID, "mpb_path_certify: c_req must be finite");
    if (N == 0) return MPB_OK;
    if (!paths || !geom || !reach || !out_i || !out_f) return mpb_fail(MPB_E_INVALID, "mpb_path_certify: null pointer");
    if (mpb_misaligned16(geom, reach)) return mpb_fail(MPB_E_INVALID, "mpb_path_certify: geom and reach must be 16-byte aligned");
    const CertArgs a = {paths, row_stride, lengths, geom, reach, out_i, out_f, H, D, n_links, max_depth, max_intervals, S, c_req};
    hipLaunchKernelGGL(path_certify_kernel, dim3(N), dim3(64), 2 * sizeof(unsigned) * (size_t)max_intervals, (hipStream_t)stream, a);
    return mpb_check_launch("mpb_path_certify");
}
