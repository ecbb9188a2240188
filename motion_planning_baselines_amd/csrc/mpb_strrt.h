// mpb_strrt.h -- what the kernels on the space-time clock share (mpb_strrt.hip, mpb_st_shortcut.hip): the moving half of a scene as a
// launcher read it from a packed moving-obstacle buffer's header, the predicate of (q, row) and the time-like metric tau.  The definitions
// are at the head of mpb_strrt.hip and in include/mpb.h.
#pragma once
#include "mpb_common.h"
#include "mpb_rrt.h"
#include "mpb_moving.h"

// the moving half of the scene as the launcher read it from the buffer's header
struct StMoving {
    const float* mob;
    int L, n_sph, n_box;
};

// the predicate of (q, row), row < R: block-uniform (every lane of the workgroup calls it; a lane without work passes any valid pair)
template <int MODEL>
__device__ __forceinline__ bool strrt_collides(const float* __restrict__ geom, unsigned* gridw, float4* otab, const float*& staged,
                                               const GeomView& G, const MovingTables& T, int L, bool ok, int row,
                                               const float (&q)[MPB_MAX_DOF]) {
    const float cs = rrt_config_cost<MODEL>(geom, gridw, otab, staged, q);
    const bool hs = cs > 0.f;
    float dq[MPB_MAX_DOF];
    const float cm = moving_row_cost<false>(G, T, L, row, q, dq);
    return !ok || hs || cm > 0.f;          // (a buffer whose header changed since the launcher read it: everything collides)
}

// tau of the definition between two configurations held in registers
__device__ __forceinline__ float strrt_tau(const float (&qr)[MPB_MAX_DOF], const float (&qn)[MPB_MAX_DOF], const float (&w)[MPB_MAX_DOF]) {
#pragma clang fp contract(off)
    float tau = 0.f;
#pragma unroll
    for (int k = 0; k < MPB_MAX_DOF; ++k) tau = fmaxf(tau, fabsf(qr[k] - qn[k]) / w[k]);
    return tau;
}
