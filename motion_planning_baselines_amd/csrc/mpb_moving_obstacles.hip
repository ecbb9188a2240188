// mpb_moving_obstacles.hip -- obstacles that move: cost, gradient and predicate of a MovingObstacleField (geometry.py; build-defined,
// DESIGN.md 10).  Row h of a trajectory sees the world at the field's time t_h: spheres and axis-aligned boxes whose centres c_{o,h} the
// host has evaluated per row in fp64 (piecewise linear between keyframes) and packed as [obstacle][x|y|z][row] (include/mpb_moving_layout.h).
//   c_h(q) = sum_l relu(margin + r_l - min_o sd_{o,h}(x_l(q)))
// over the robot's collision spheres (FKState / fk_advance of mpb_geom.h through a GeomView filled from the buffer; a point robot has its
// one sphere at q), sd the expressions of exact_sphere / exact_box (mpb_geom.h: what the static CollisionField kernels take), spheres in
// the given order, then boxes, a strict < keeps the first minimum.  Time is fixed per row: the obstacles' velocity is no part of d c / d q.
//
// Mapping: one wave per trajectory (a workgroup IS one wave: no barrier, no LDS), one lane per row, trips of 64 for R > 64.  The robot's
// spheres go in groups of MPB_GROUP held in registers (LinkChunk); the obstacles stream past a group in order.  The obstacle index is
// wave-uniform -- radii and half extents are uniform loads --, the centre is one coalesced load per component: the row axis is padded to
// whole trips with the last row, so the lanes of a trip read 64 consecutive words and never past the table.  With gradients the force of
// an active sphere is pulled through J^T at once from the joint axes / origins the walk has kept (joint_term), skipped wave-wide when a
// ballot finds the sphere active in no lane.  No broad phase: a conservative cull would need keys per row.
// Order of the sums: spheres in table order in fp32 per row, a lane's rows in ascending order, then the fixed-order wave reduction of
// mpb_common.h: every run gives the same bits.
#include <math.h>

#include "mpb_common.h"
#include "mpb_host.h"
#include "mpb_geom.h"
#include "mpb_member_cost.h"
#include "mpb_moving.h"

template <bool GRAD>
__global__ __launch_bounds__(64) void moving_cost_kernel(const float* __restrict__ trajs, const float* __restrict__ mob, float* __restrict__ out,
                                                         float* __restrict__ per_wp, float* __restrict__ grad, int H, int d, int h_begin,
                                                         float k_sigma, float weight, int accumulate, int D, int L, int n_sph, int n_box) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const GeomView G = moving_robot_view(mob);
    const MovingTables T = moving_tables(mob, H, n_sph, n_box);
    const bool ok = moving_header_matches(mob, D, L, H, n_sph, n_box);      // (D: the launcher's n_dof, which it held d against)
    const float sc = weight * k_sigma;
    float csum = 0.f;
    for (int h0 = 0; h0 < H; h0 += 64) {
        const int h = h0 + lane;                                            // (< T.stride: the padded rows)
        const bool live = ok && h < H && h >= h_begin;
        float q[MPB_MAX_DOF], dq[MPB_MAX_DOF];
#pragma unroll
        for (int i = 0; i < MPB_MAX_DOF; ++i) { q[i] = 0.f; dq[i] = 0.f; }
        float c = 0.f;
        if (__ballot(live) != 0ull) {
            // (a lane that is not live walks along at q = 0 against its own -- possibly padded -- row and its result is dropped: the
            // ballots of the walk then see whole waves)
            if (live) {
                const float* row = trajs + ((size_t)b * H + h) * d;
#pragma unroll
                for (int i = 0; i < MPB_MAX_DOF; ++i) q[i] = (i < D) ? row[i] : 0.f;
            }
            c = moving_row_cost<GRAD>(G, T, L, h, q, dq);
            if (!live) c = 0.f;
        }
        if (!ok) c = __uint_as_float(0x7FC00000u);
        if (h < H) {
            if (per_wp) per_wp[(size_t)b * H + h] = c;
            if (GRAD) {
                float* grow = grad + ((size_t)b * H + h) * d;
#pragma unroll
                for (int i = 0; i < MPB_MAX_DOF; ++i) {
                    if (i < D) {
                        const float g = ok ? (live ? sc * dq[i] : 0.f) : c;
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

// the predicate per ROW (it needs the row's time): in collision iff c_h(q_h) > 0
__global__ __launch_bounds__(64) void moving_check_kernel(const float* __restrict__ trajs, const float* __restrict__ mob,
                                                          unsigned char* __restrict__ in_collision, float* __restrict__ gap, int H, int d,
                                                          int or_into, int D, int L, int n_sph, int n_box) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const GeomView G = moving_robot_view(mob);
    const MovingTables T = moving_tables(mob, H, n_sph, n_box);
    const bool ok = moving_header_matches(mob, D, L, H, n_sph, n_box);
    for (int h0 = 0; h0 < H; h0 += 64) {
        const int h = h0 + lane;
        const bool have = h < H;
        float q[MPB_MAX_DOF], dq[MPB_MAX_DOF];
#pragma unroll
        for (int i = 0; i < MPB_MAX_DOF; ++i) q[i] = 0.f;
        if (have) {
            const float* row = trajs + ((size_t)b * H + h) * d;
#pragma unroll
            for (int i = 0; i < MPB_MAX_DOF; ++i) q[i] = (i < D) ? row[i] : 0.f;
        }
        if (ok) {
            const float c = moving_row_cost<false>(G, T, L, h, q, dq);
            if (have) member_store_hit(in_collision, gap, (size_t)b * H + h, c, or_into);
        } else if (have) {
            // a refused buffer reads as in collision with a NaN gap: stored as bits (the build assumes finite math: a NaN constant taken
            // through member_store_hit's comparison may be folded away)
            in_collision[(size_t)b * H + h] = 1;
            if (gap) reinterpret_cast<unsigned*>(gap)[(size_t)b * H + h] = 0x7FC00000u;
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
static inline int moving_up(int n, int m) { return (n + m - 1) / m * m; }

static int moving_header_check(const int32_t* si, int n_words, const char* who) {
    if (si[MPB_VW_MAGIC] != MPB_MOVING_MAGIC || si[MPB_VW_VERSION] != MPB_MOVING_VERSION)
        return mpb_failf(MPB_E_INVALID, "%s: bad magic/version of the moving-obstacle buffer", who);
    const int n_dof = si[MPB_VW_N_DOF], n_tf = si[MPB_VW_N_TF], n_links = si[MPB_VW_N_LINKS], n_rows = si[MPB_VW_N_ROWS];
    const int n_sph = si[MPB_VW_N_SPHERES], n_box = si[MPB_VW_N_BOXES];
    if (n_dof < 1 || n_dof > MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "%s: n_dof = %d outside 1..MPB_MAX_DOF = %d", who, n_dof, MPB_MAX_DOF);
    if (n_links < 1 || n_links > MPB_MOVING_MAX_LINKS)
        return mpb_failf(MPB_E_UNSUPPORTED, "%s: %d collision spheres outside 1..MPB_MOVING_MAX_LINKS = %d", who, n_links, MPB_MOVING_MAX_LINKS);
    if (n_rows < 1 || n_rows > MPB_MOVING_MAX_ROWS) return mpb_failf(MPB_E_UNSUPPORTED, "%s: n_rows = %d outside 1..MPB_MOVING_MAX_ROWS = %d", who, n_rows, MPB_MOVING_MAX_ROWS);
    if (n_sph < 0 || n_sph > MPB_MOVING_MAX_SPHERES)
        return mpb_failf(MPB_E_UNSUPPORTED, "%s: n_spheres = %d outside 0..MPB_MOVING_MAX_SPHERES = %d", who, n_sph, MPB_MOVING_MAX_SPHERES);
    if (n_box < 0 || n_box > MPB_MOVING_MAX_BOXES) return mpb_failf(MPB_E_UNSUPPORTED, "%s: n_boxes = %d outside 0..MPB_MOVING_MAX_BOXES = %d", who, n_box, MPB_MOVING_MAX_BOXES);
    if (n_sph + n_box < 1) return mpb_failf(MPB_E_INVALID, "%s: the moving-obstacle buffer holds no obstacle", who);
    if (n_tf == 0) {
        if (n_dof < 2 || n_dof > 3 || n_links != 1) return mpb_failf(MPB_E_INVALID, "%s: a point robot (n_tf = 0) has 2 or 3 coordinates and one sphere", who);
    } else if (n_tf != n_dof + 1) {
        return mpb_failf(MPB_E_INVALID, "%s: a chain needs n_dof + 1 transforms", who);
    }
    const int off_tf = MPB_MOVING_HEADER_WORDS, off_links = off_tf + 12 * n_tf, off_radii = off_links + 8 * n_links;
    const int off_half = off_radii + moving_up(n_sph, MPB_MOVING_ALIGN), off_centres = off_half + 4 * n_box;
    const int total = off_centres + 3 * (n_sph + n_box) * moving_up(n_rows, MPB_MOVING_ROW_PAD);
    if (si[MPB_VW_OFF_TF] != off_tf || si[MPB_VW_OFF_LINKS] != off_links || si[MPB_VW_OFF_RADII] != off_radii || si[MPB_VW_OFF_HALF] != off_half ||
        si[MPB_VW_OFF_CENTRES] != off_centres || si[MPB_VW_TOTAL] != total || (n_words >= 0 && total != n_words))
        return mpb_failf(MPB_E_INVALID, "%s: inconsistent section offsets / total of the moving-obstacle buffer", who);
    return MPB_OK;
}

// finite by the exponent bits (the build compiles with -ffinite-math-only: a floating-point comparison against NaN may be folded away)
static inline bool moving_finite(const float* p) { return (*reinterpret_cast<const uint32_t*>(p) & 0x7F800000u) != 0x7F800000u; }

extern "C" int mpb_moving_check(const float* s, int n_words) {
    if (!s || n_words < MPB_MOVING_HEADER_WORDS) return mpb_failf(MPB_E_INVALID, "%s: moving-obstacle buffer too small", __func__);
    const int32_t* si = reinterpret_cast<const int32_t*>(s);
    const int rc = moving_header_check(si, n_words, __func__);
    if (rc) return rc;
    const int n_dof = si[MPB_VW_N_DOF], n_tf = si[MPB_VW_N_TF], n_links = si[MPB_VW_N_LINKS], n_rows = si[MPB_VW_N_ROWS];
    const int n_sph = si[MPB_VW_N_SPHERES], n_box = si[MPB_VW_N_BOXES];
    if (!moving_finite(s + MPB_VW_MARGIN)) return mpb_failf(MPB_E_INVALID, "%s: the margin is not finite", __func__);
    if (n_tf > 0) {
        int prev = 1;
        for (int l = 0; l < n_links; ++l) {
            const int f = si[si[MPB_VW_OFF_LINKS] + 8 * l];
            if (f < prev || f > n_dof + 1) return mpb_failf(MPB_E_INVALID, "%s: link frames must be sorted in [1, n_dof+1]", __func__);
            prev = f;
        }
    }
    for (int o = 0; o < n_sph; ++o) {
        const float r = s[si[MPB_VW_OFF_RADII] + o];
        if (!moving_finite(s + si[MPB_VW_OFF_RADII] + o) || !(r > 0.f)) return mpb_failf(MPB_E_INVALID, "%s: sphere %d has no positive finite radius", __func__, o);
    }
    for (int o = 0; o < n_box; ++o)
        for (int k = 0; k < 3; ++k) {
            const float h = s[si[MPB_VW_OFF_HALF] + 4 * o + k];
            if (!moving_finite(s + si[MPB_VW_OFF_HALF] + 4 * o + k) || !(h > 0.f)) return mpb_failf(MPB_E_INVALID, "%s: box %d has no positive finite half extents", __func__, o);
        }
    const int stride = moving_up(n_rows, MPB_MOVING_ROW_PAD);
    const float* cp = s + si[MPB_VW_OFF_CENTRES];
    for (int o = 0; o < n_sph + n_box; ++o)
        for (int k = 0; k < 3; ++k) {
            const float* line = cp + ((size_t)o * 3 + k) * stride;
            for (int h = 0; h < stride; ++h) {
                if (!moving_finite(line + h)) return mpb_failf(MPB_E_INVALID, "%s: the centre of obstacle %d at row %d is not finite", __func__, o, h);
                if (h >= n_rows && line[h] != line[n_rows - 1])
                    return mpb_failf(MPB_E_INVALID, "%s: the padding rows of obstacle %d must repeat row %d", __func__, o, n_rows - 1);
            }
        }
    return MPB_OK;
}

// what a launch needs of a device buffer's header, through the cache of mpb_host.h (its contract is stated there); memory that gets ANOTHER
// buffer at an address an earlier call has seen must be announced with mpb_moving_invalidate
static MpbHeaderCache<MovingShape, MPB_MOVING_HEADER_WORDS> g_moving_cache;

extern "C" int mpb_moving_invalidate(const float* mob) {
    g_moving_cache.drop(mob);
    return MPB_OK;
}

static int moving_shape(const float* mob, MovingShape& out, const char* who) {
    return g_moving_cache.get(mob, out, who, "moving-obstacle", [who](const int32_t* hdr, MovingShape& S) {
        S.n_dof = hdr[MPB_VW_N_DOF], S.n_links = hdr[MPB_VW_N_LINKS], S.n_rows = hdr[MPB_VW_N_ROWS];
        S.n_sph = hdr[MPB_VW_N_SPHERES], S.n_box = hdr[MPB_VW_N_BOXES];
        return moving_header_check(hdr, -1, who);
    });
}

int mpb_moving_shape_cached(const float* mob, MovingShape& out, const char* who) { return moving_shape(mob, out, who); }

// the rows of a launch against the buffer: wide enough for the robot, and exactly the row count the centres were evaluated for
static int moving_rows_fit(const MovingShape& S, int H, int d, const char* who) {
    if (d < S.n_dof) return mpb_failf(MPB_E_INVALID, "%s: rows of d = %d are narrower than the robot's %d coordinates", who, d, S.n_dof);
    if (H != S.n_rows)
        return mpb_failf(MPB_E_INVALID, "%s: trajectories of H = %d rows, the moving-obstacle buffer was packed for n_rows = %d", who, H, S.n_rows);
    return MPB_OK;
}

static int moving_cost_launch(bool want_grad, const char* who, const float* trajs, const float* mob, float* out, float* per_wp, float* grad,
                              int B, int H, int d, int h_begin, float k_sigma, float weight, int accumulate, void* stream) {
    int rc = mpb_check_rows(who, "moving-obstacle", trajs, mob, out, want_grad, grad, B, H, d, h_begin);
    if (rc || B == 0) return rc;
    MovingShape S;
    if ((rc = moving_shape(mob, S, who))) return rc;
    if ((rc = moving_rows_fit(S, H, d, who))) return rc;
    hipLaunchKernelGGL(want_grad ? moving_cost_kernel<true> : moving_cost_kernel<false>, dim3(B), dim3(64), 0, (hipStream_t)stream, trajs, mob, out,
                       per_wp, grad, H, d, h_begin, k_sigma, weight, accumulate, S.n_dof, S.n_links, S.n_sph, S.n_box);
    return mpb_check_launch(who);
}

extern "C" int mpb_moving_collision_eval(const float* trajs, const float* mob, float* out, float* per_waypoint, int B, int H, int d, int h_begin,
                                         float k_sigma, float weight, int accumulate, void* stream) {
    return moving_cost_launch(false, __func__, trajs, mob, out, per_waypoint, nullptr, B, H, d, h_begin, k_sigma, weight, accumulate, stream);
}

extern "C" int mpb_moving_collision_grad(const float* trajs, const float* mob, float* out, float* grad, int B, int H, int d, int h_begin,
                                         float k_sigma, float weight, int accumulate, void* stream) {
    return moving_cost_launch(true, __func__, trajs, mob, out, nullptr, grad, B, H, d, h_begin, k_sigma, weight, accumulate, stream);
}

extern "C" int mpb_moving_collision_check(const float* trajs, const float* mob, unsigned char* in_collision, float* gap, int B, int H, int d,
                                          int or_into, void* stream) {
    int rc = mpb_check_rows(__func__, "moving-obstacle", trajs, mob, in_collision, false, nullptr, B, H, d, 0);
    if (rc || B == 0) return rc;
    MovingShape S;
    if ((rc = moving_shape(mob, S, __func__))) return rc;
    if ((rc = moving_rows_fit(S, H, d, __func__))) return rc;
    hipLaunchKernelGGL(moving_check_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, trajs, mob, in_collision, gap, H, d, or_into, S.n_dof,
                       S.n_links, S.n_sph, S.n_box);
    return mpb_check_launch(__func__);
}
