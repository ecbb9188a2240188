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
#include "mpb_self_host.h"
#include "mpb_geom.h"
#include "mpb_member_cost.h"
#include "mpb_self.h"
#include "../../include/mpb_self_layout.h"

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

extern "C" int mpb_self_invalidate(const float* selfb) {
    g_self_cache.drop(selfb);
    return MPB_OK;
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
