// mpb_member_cost.h -- device pieces shared by the cost members with kernels of their own (mpb_self_collision.hip, mpb_sdf_grid.hip;
// mpb_ee_cost.hip takes add_rounded): where a collision sphere sits, and the epilogues that write a trajectory's sum and a
// configuration's predicate.  Everything is forced inline, and a piece is here only where every kernel that calls it compiles to the
// instructions it had with the text written out.  That is why three copies stay where they are: the cost kernels' row store (through a
// function the compiler folds the two selects of sdf_cost_kernel<true> into one), the zeroing of FKState<true>'s joint arrays (mpb_geom.h
// says the same of its own) and the centre stores of self_store_centres come out as other code.
// Kept out of mpb_common.h / mpb_geom.h, which every planner kernel's counter summary is fingerprinted with (build.PMC_SOURCES).
#pragma once
#include "mpb_common.h"
#include "mpb_geom.h"

// a + b in one rounding whatever produced b: without this the compiler contracts  old + scale * x  into one fma, and accumulating onto
// a buffer would not equal the buffer plus a fresh evaluation bit for bit
__device__ __forceinline__ float add_rounded(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

// centre of a collision sphere: the offset (lk.y, lk.z, lk.w) of its link-table row in the frame F stands at
template <bool G>
__device__ __forceinline__ void link_centre(const FKState<G>& F, const float4& lk, float& x, float& y, float& z) {
    x = mad3(F.r00, lk.y, F.r01, lk.z, F.r02, lk.w, F.tx);
    y = mad3(F.r10, lk.y, F.r11, lk.z, F.r12, lk.w, F.ty);
    z = mad3(F.r20, lk.y, F.r21, lk.z, F.r22, lk.w, F.tz);
}

// out[b] (+)= weight * k_sigma * (the wave's sum of csum, in the fixed order of wave_sum_f32)
__device__ __forceinline__ void member_store_out(float* out, int b, int lane, float csum, float k_sigma, float weight, int accumulate) {
    csum = wave_sum_f32(csum);
    if (lane == 0) {
        const float v = weight * (k_sigma * csum);
        out[b] = accumulate ? add_rounded(out[b], v) : v;
    }
}

// configuration i of a predicate: in collision iff its hinge sum c is positive (a refused buffer's NaN reads as in collision); or_into:
// ORed into the flag and added onto the gap that are there
__device__ __forceinline__ void member_store_hit(unsigned char* in_collision, float* gap, size_t i, float c, int or_into) {
    const bool hit = !(c <= 0.f);
    in_collision[i] = (hit || (or_into && in_collision[i] != 0)) ? 1 : 0;
    if (gap) gap[i] = or_into ? add_rounded(gap[i], c) : c;
}
