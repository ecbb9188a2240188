// mpb_self_collision.hip -- the robot against itself: cost, gradient and predicate of a SelfCollisionField (geometry.py; build-defined,
// DESIGN.md 10).  Per waypoint  c(q) = sum over pairs (a, b) of relu(T_ab - |x_a(q) - x_b(q)|)  with the collision-sphere centres x_l of
// the chain walk every kernel here uses (FKState / fk_advance of mpb_geom.h, unchanged, through a GeomView filled from the self buffer)
// and the pair table (a | b << 16, T_ab) of the packed self buffer (include/mpb_self_layout.h).
//
// Mapping: one wave per trajectory (a workgroup IS one wave: no barrier anywhere), one lane per waypoint; the predicate gives one lane
// per configuration of the flattened N.  Indexing 31-64 sphere centres by a run-time pair index from registers would go to scratch
// memory, so a trip of 64 waypoints runs in phases:
//   1. the lane walks the chain and stores each centre to LDS as [link][xyz][lane]: a wave's access is one bank per lane;
//   2. the pair loop runs on a wave-uniform pair index (the pair words are scalar loads), each lane reads its own column; with gradients
//      an ACTIVE pair (rare: most waypoints are free) adds -+u into a second LDS array of the same shape.  A lane owns its column: no
//      races, no atomics;
//   3. (gradient) a second walk, fk_advance<true>, applies J^T to that array as fk_points_vjp_kernel does -- skipped wave-wide when a
//      ballot says that no lane had an active pair.
// LDS is sized at launch from n_links: 768 B per link (1536 B with gradients) -- the Panda's 31 spheres take 23.8 KB / 47.6 KB, the
// limit of MPB_SELF_MAX_LINKS = 64 takes 48 KB / 96 KB of the 160 KB a workgroup may have.
// Order of the sums: pairs in table order in fp32 per waypoint, a lane's waypoints in ascending order, then the fixed-order wave
// reduction of mpb_common.h: every run gives the same bits.
#include "mpb_common.h"
#include "mpb_host.h"
#include "mpb_geom.h"
#include "mpb_member_cost.h"
#include "../../include/mpb_self_layout.h"

// the chain of a self buffer as the GeomView fk_advance reads (tf, n_dof) and the walks below read (links, n_links); no obstacles
__device__ __forceinline__ GeomView self_view(const float* __restrict__ s) {
    const int* si = reinterpret_cast<const int*>(s);
    GeomView v = {};
    v.kind = MPB_KIND_CHAIN;
    v.n_dof = si[MPB_SW_N_DOF];
    v.n_tf = si[MPB_SW_N_TF];
    v.n_links = si[MPB_SW_N_LINKS];
    v.margin = s[MPB_SW_MARGIN];
    v.tf = s + si[MPB_SW_OFF_TF];
    v.links = s + si[MPB_SW_OFF_LINKS];
    return v;
}

// phase 1: centres of the L collision spheres of configuration q into this lane's column of pos ([link][xyz][lane]); GRAD: zero the
// lane's column of the force array
template <bool GRAD>
__device__ __forceinline__ void self_store_centres(const GeomView& G, int L, const float (&q)[MPB_MAX_DOF], float* __restrict__ pos,
                                                   float* __restrict__ frc, int lane) {
    FKState<false> F;
    fk_identity(F);
    F.frame = 0;
    for (int l = 0; l < L; ++l) {
        const float4 lk = *reinterpret_cast<const float4*>(G.links + 8 * l);   // frame, ox, oy, oz
        const int f = min(__float_as_int(lk.x), G.n_tf);                       // (a checked buffer never clamps: keeps the walk inside tf)
        while (F.frame < f) fk_advance<false>(G, F, q);
        float* p = pos + l * 192 + lane;
        p[0] = mad3(F.r00, lk.y, F.r01, lk.z, F.r02, lk.w, F.tx);
        p[64] = mad3(F.r10, lk.y, F.r11, lk.z, F.r12, lk.w, F.ty);
        p[128] = mad3(F.r20, lk.y, F.r21, lk.z, F.r22, lk.w, F.tz);
        if (GRAD) {
            float* g = frc + l * 192 + lane;
            g[0] = g[64] = g[128] = 0.f;
        }
    }
}

// phase 2: sum of the hinges over the pair table (table order, fp32); GRAD: d c / d x_a = -(x_a - x_b) / n, d c / d x_b = +(x_a - x_b) / n
// of every active pair into frc; a pair with n == 0 contributes no force (the oracle's safe-norm sub-gradient).  Returns c; `any` is set
// when a force was written.
template <bool GRAD>
__device__ __forceinline__ float self_pair_sum(const float* __restrict__ pairs, int n_pairs, int L, const float* __restrict__ pos,
                                               float* __restrict__ frc, int lane, bool& any) {
    float c = 0.f;
    for (int p = 0; p < n_pairs; ++p) {
        const unsigned w = __float_as_uint(pairs[MPB_SELF_PAIR_WORDS * p]);
        const float T = pairs[MPB_SELF_PAIR_WORDS * p + 1];
        const int a = min((int)(w & MPB_SELF_PAIR_A_MASK), L - 1), b = min((int)(w >> MPB_SELF_PAIR_B_SHIFT), L - 1);   // (wave-uniform; a checked buffer never clamps)
        const float* pa = pos + a * 192 + lane;
        const float* pb = pos + b * 192 + lane;
        const float dx = pa[0] - pb[0], dy = pa[64] - pb[64], dz = pa[128] - pb[128];
        const float n = fast_sqrt(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
        const float hng = T - n;
        if (hng > 0.f) {
            c += hng;
            if (GRAD && n > 0.f) {
                const float ux = dx / n, uy = dy / n, uz = dz / n;
                float* ga = frc + a * 192 + lane;
                float* gb = frc + b * 192 + lane;
                ga[0] -= ux; ga[64] -= uy; ga[128] -= uz;
                gb[0] += ux; gb[64] += uy; gb[128] += uz;
                any = true;
            }
        }
    }
    return c;
}

// phase 3: dq = J^T frc by a second walk (d x_l / d q_i = z_i x (x_l - p_i) for the joints upstream of the sphere's frame)
__device__ __forceinline__ void self_apply_jt(const GeomView& G, int L, const float (&q)[MPB_MAX_DOF], const float* __restrict__ frc,
                                              int lane, float (&dq)[MPB_MAX_DOF]) {
    FKState<true> F;
    fk_identity(F);
    F.frame = 0;
#pragma unroll
    for (int i = 0; i < MPB_MAX_DOF; ++i) { F.zx[i] = F.zy[i] = F.zz[i] = F.px[i] = F.py[i] = F.pz[i] = 0.f; }
    for (int l = 0; l < L; ++l) {
        const float4 lk = *reinterpret_cast<const float4*>(G.links + 8 * l);
        const int f = min(__float_as_int(lk.x), G.n_tf);
        while (F.frame < f) fk_advance<true>(G, F, q);
        const float* g = frc + l * 192 + lane;
        const float fx = g[0], fy = g[64], fz = g[128];
        float x, y, z;
        link_centre(F, lk, x, y, z);
#pragma unroll
        for (int i = 0; i < MPB_MAX_DOF; ++i)
            if (i < f && i < G.n_dof) dq[i] += joint_term(F.zx[i], F.zy[i], F.zz[i], F.px[i], F.py[i], F.pz[i], x, y, z, fx, fy, fz);
    }
}

// the launcher read n_dof / n_links / n_pairs from the header to size the LDS and to check the row width; the kernels use ITS numbers
// for every LDS address and every row index and refuse (NaN outputs) a buffer whose header has changed since
__device__ __forceinline__ bool self_header_matches(const float* __restrict__ s, int n_dof, int L, int n_pairs) {
    const int* si = reinterpret_cast<const int*>(s);
    return si[MPB_SW_MAGIC] == MPB_SELF_MAGIC && si[MPB_SW_N_DOF] == n_dof && si[MPB_SW_N_LINKS] == L && si[MPB_SW_N_PAIRS] == n_pairs;
}

template <bool GRAD>
__global__ __launch_bounds__(64) void self_cost_kernel(const float* __restrict__ trajs, const float* __restrict__ selfb,
                                                       float* __restrict__ out, float* __restrict__ per_wp, float* __restrict__ grad,
                                                       int H, int d, int h_begin, float k_sigma, float weight, int accumulate, int D,
                                                       int L, int n_pairs) {
    extern __shared__ __align__(16) float self_lds[];
    float* pos = self_lds;                 // [L][3][64]
    float* frc = self_lds + L * 192;       // [L][3][64] (GRAD)
    const int lane = threadIdx.x, b = blockIdx.x;
    const GeomView G = self_view(selfb);
    const float* pairs = selfb + reinterpret_cast<const int*>(selfb)[MPB_SW_OFF_PAIRS];
    const bool ok = self_header_matches(selfb, D, L, n_pairs);        // (D: the launcher's n_dof, which it held d against)
    const float sc = weight * k_sigma;
    float csum = 0.f;
    for (int h0 = 0; h0 < H; h0 += 64) {
        const int h = h0 + lane;
        const bool live = ok && h < H && h >= h_begin;
        float q[MPB_MAX_DOF], dq[MPB_MAX_DOF];
#pragma unroll
        for (int i = 0; i < MPB_MAX_DOF; ++i) dq[i] = 0.f;
        float c = 0.f;
        bool any = false;
        if (live) {
            const float* row = trajs + ((size_t)b * H + h) * d;      // (element loads: the 8-byte form of load_row_prefix costs this kernel 21 spilled SGPRs)
#pragma unroll
            for (int i = 0; i < MPB_MAX_DOF; ++i) q[i] = (i < D) ? row[i] : 0.f;
            self_store_centres<GRAD>(G, L, q, pos, frc, lane);
            c = self_pair_sum<GRAD>(pairs, n_pairs, L, pos, frc, lane, any);
        }
        if (GRAD) {
            if (__ballot(any) != 0ull && live) self_apply_jt(G, L, q, frc, lane, dq);
        }
        if (!ok) c = __uint_as_float(0x7FC00000u);
        if (h < H) {
            if (per_wp) per_wp[(size_t)b * H + h] = c;
            if (GRAD) {
                float* grow = grad + ((size_t)b * H + h) * d;
#pragma unroll
                for (int i = 0; i < MPB_MAX_DOF; ++i) {
                    if (i < D) {
                        const float g = ok ? sc * dq[i] : c;
                        grow[i] = accumulate ? add_rounded(grow[i], g) : g;
                    }
                }
                if (!accumulate)
                    for (int i = D; i < d; ++i) grow[i] = 0.f;   // the velocity channels
            }
        }
        csum += c;
    }
    member_store_out(out, b, lane, csum, k_sigma, weight, accumulate);
}

__global__ __launch_bounds__(64) void self_check_kernel(const float* __restrict__ q_in, const float* __restrict__ selfb,
                                                        unsigned char* __restrict__ in_collision, float* __restrict__ gap, int N, int D,
                                                        int or_into, int L, int n_pairs) {
    extern __shared__ __align__(16) float self_lds[];
    const int lane = threadIdx.x;
    const size_t i = (size_t)blockIdx.x * 64 + lane;
    if (i >= (size_t)N) return;
    const GeomView G = self_view(selfb);
    const float* pairs = selfb + reinterpret_cast<const int*>(selfb)[MPB_SW_OFF_PAIRS];
    float q[MPB_MAX_DOF];
#pragma unroll
    for (int k = 0; k < MPB_MAX_DOF; ++k) q[k] = (k < D) ? q_in[i * D + k] : 0.f;
    float c = __uint_as_float(0x7FC00000u);
    if (self_header_matches(selfb, D, L, n_pairs)) {
        bool any = false;
        self_store_centres<false>(G, L, q, self_lds, nullptr, lane);
        c = self_pair_sum<false>(pairs, n_pairs, L, self_lds, nullptr, lane, any);
    }
    member_store_hit(in_collision, gap, i, c, or_into);
}

// ---- host side ------------------------------------------------------------------------------------------------------
static int self_header_check(const int32_t* si, int n_words, const char* who) {
    if (si[MPB_SW_MAGIC] != MPB_SELF_MAGIC || si[MPB_SW_VERSION] != MPB_SELF_VERSION) return mpb_failf(MPB_E_INVALID, "%s: bad magic/version of the self-collision buffer", who);
    const int n_dof = si[MPB_SW_N_DOF], n_tf = si[MPB_SW_N_TF], n_links = si[MPB_SW_N_LINKS], n_pairs = si[MPB_SW_N_PAIRS];
    if (n_dof < 1 || n_dof > MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "%s: n_dof = %d outside 1..MPB_MAX_DOF = %d", who, n_dof, MPB_MAX_DOF);
    if (n_links < 2 || n_links > MPB_SELF_MAX_LINKS) return mpb_failf(MPB_E_UNSUPPORTED, "%s: %d collision spheres outside 2..MPB_SELF_MAX_LINKS = %d", who, n_links, MPB_SELF_MAX_LINKS);
    if (n_pairs < 0 || n_pairs > MPB_SELF_MAX_PAIRS) return mpb_failf(MPB_E_UNSUPPORTED, "%s: %d pairs outside 0..MPB_SELF_MAX_PAIRS = %d", who, n_pairs, MPB_SELF_MAX_PAIRS);
    if (n_tf != n_dof + 1) return mpb_failf(MPB_E_INVALID, "%s: a chain needs n_dof + 1 transforms", who);
    const int off_tf = si[MPB_SW_OFF_TF], off_links = si[MPB_SW_OFF_LINKS], off_pairs = si[MPB_SW_OFF_PAIRS], total = si[MPB_SW_TOTAL];
    if (off_tf != MPB_SELF_HEADER_WORDS || off_links != off_tf + 12 * n_tf || off_pairs != off_links + 8 * n_links ||
        total != off_pairs + MPB_SELF_PAIR_WORDS * n_pairs || (n_words >= 0 && total != n_words))
        return mpb_failf(MPB_E_INVALID, "%s: inconsistent section offsets / total of the self-collision buffer", who);
    return MPB_OK;
}

extern "C" int mpb_self_check(const float* s, int n_words) {
    if (!s || n_words < MPB_SELF_HEADER_WORDS) return mpb_failf(MPB_E_INVALID, "%s: self-collision buffer too small", __func__);
    const int32_t* si = reinterpret_cast<const int32_t*>(s);
    const int rc = self_header_check(si, n_words, __func__);
    if (rc) return rc;
    const int n_dof = si[MPB_SW_N_DOF], n_links = si[MPB_SW_N_LINKS], n_pairs = si[MPB_SW_N_PAIRS];
    int prev = 1;
    for (int l = 0; l < n_links; ++l) {
        const int f = si[si[MPB_SW_OFF_LINKS] + 8 * l];
        if (f < prev || f > n_dof + 1) return mpb_failf(MPB_E_INVALID, "%s: link frames must be sorted in [1, n_dof+1]", __func__);
        prev = f;
    }
    for (int p = 0; p < n_pairs; ++p) {
        const uint32_t w = (uint32_t)si[si[MPB_SW_OFF_PAIRS] + MPB_SELF_PAIR_WORDS * p];
        const int a = (int)(w & MPB_SELF_PAIR_A_MASK), b = (int)(w >> MPB_SELF_PAIR_B_SHIFT);
        const float T = s[si[MPB_SW_OFF_PAIRS] + MPB_SELF_PAIR_WORDS * p + 1];
        if (!(a < b && b < n_links)) return mpb_failf(MPB_E_INVALID, "%s: pair %d = (%d, %d) needs a < b < n_links = %d", __func__, p, a, b, n_links);
        if (!(T > 0.f && T < 3.0e38f)) return mpb_failf(MPB_E_INVALID, "%s: pair %d has no positive finite threshold", __func__, p);
    }
    return MPB_OK;
}

// what a launch needs of a device buffer's header (LDS bytes come from n_links), through the cache of mpb_host.h (its contract is stated
// there); memory that gets ANOTHER buffer at an address an earlier call has seen must be announced with mpb_self_invalidate
struct SelfShape { const void* ptr; int dev, n_dof, n_links, n_pairs; };
static MpbHeaderCache<SelfShape, MPB_SELF_HEADER_WORDS> g_self_cache;

extern "C" int mpb_self_invalidate(const float* selfb) {
    g_self_cache.drop(selfb);
    return MPB_OK;
}

static int self_shape(const float* selfb, SelfShape& out, const char* who) {
    return g_self_cache.get(selfb, out, who, "self-collision", [who](const int32_t* hdr, SelfShape& S) {
        S.n_dof = hdr[MPB_SW_N_DOF], S.n_links = hdr[MPB_SW_N_LINKS], S.n_pairs = hdr[MPB_SW_N_PAIRS];
        return self_header_check(hdr, -1, who);
    });
}

// LDS of a launch ([L][3][64] words, twice with gradients), the kernel's limit raised where that takes it
static int self_lds_bytes(const void* kernel, const SelfShape& S, bool grad, size_t& bytes, const char* who) {
    bytes = (size_t)S.n_links * 192 * sizeof(float) * (grad ? 2 : 1);
    return mpb_raise_lds_limit(kernel, S.dev, bytes, who);
}

static int self_cost_launch(bool want_grad, const char* who, const float* trajs, const float* selfb, float* out, float* per_wp, float* grad,
                            int B, int H, int d, int h_begin, float k_sigma, float weight, int accumulate, void* stream) {
    int rc = mpb_check_rows(who, "self-collision", trajs, selfb, out, want_grad, grad, B, H, d, h_begin);
    if (rc || B == 0) return rc;
    SelfShape S;
    if ((rc = self_shape(selfb, S, who))) return rc;
    if (d < S.n_dof) return mpb_failf(MPB_E_INVALID, "%s: rows of d = %d are narrower than the chain's %d joints", who, d, S.n_dof);
    const auto kernel = want_grad ? self_cost_kernel<true> : self_cost_kernel<false>;
    size_t lds;
    if ((rc = self_lds_bytes(reinterpret_cast<const void*>(kernel), S, want_grad, lds, who))) return rc;
    hipLaunchKernelGGL(kernel, dim3(B), dim3(64), lds, (hipStream_t)stream, trajs, selfb, out, per_wp, grad, H, d, h_begin, k_sigma, weight,
                       accumulate, S.n_dof, S.n_links, S.n_pairs);
    return mpb_check_launch(who);
}

extern "C" int mpb_self_collision_eval(const float* trajs, const float* selfb, float* out, float* per_waypoint, int B, int H, int d,
                                       int h_begin, float k_sigma, float weight, int accumulate, void* stream) {
    return self_cost_launch(false, __func__, trajs, selfb, out, per_waypoint, nullptr, B, H, d, h_begin, k_sigma, weight, accumulate, stream);
}

extern "C" int mpb_self_collision_grad(const float* trajs, const float* selfb, float* out, float* grad, int B, int H, int d, int h_begin,
                                       float k_sigma, float weight, int accumulate, void* stream) {
    return self_cost_launch(true, __func__, trajs, selfb, out, nullptr, grad, B, H, d, h_begin, k_sigma, weight, accumulate, stream);
}

extern "C" int mpb_self_collision_check(const float* q, const float* selfb, unsigned char* in_collision, float* gap, int N, int D,
                                        int or_into, void* stream) {
    int rc = mpb_check_configs(__func__, "self-collision", q, selfb, in_collision, N, D);
    if (rc || N == 0) return rc;
    SelfShape S;
    if ((rc = self_shape(selfb, S, __func__))) return rc;
    if (D != S.n_dof) return mpb_failf(MPB_E_INVALID, "%s: D = %d, the chain has %d joints", __func__, D, S.n_dof);
    size_t lds;
    if ((rc = self_lds_bytes(reinterpret_cast<const void*>(self_check_kernel), S, false, lds, __func__))) return rc;
    hipLaunchKernelGGL(self_check_kernel, dim3((N + 63) / 64), dim3(64), lds, (hipStream_t)stream, q, selfb, in_collision, gap, N, D, or_into,
                       S.n_links, S.n_pairs);
    return mpb_check_launch(__func__);
}
