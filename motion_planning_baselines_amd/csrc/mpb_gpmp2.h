// mpb_gpmp2.h -- what the two forms of the GPMP2 solve (mpb_gpmp2.hip: block elimination; mpb_gpmp2_lr.hip: low-rank form) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// precisions 1 / sigma^2 of the factors, damping and step of one Gauss-Newton iteration (gpmp2.py:308-368)
struct GpConst { double dt, ks, kgp, kg, kc, delta, step; int trust; };
// ... from the sigmas of the C-ABI: the only place the precisions are formed (sigma_goal <= 0: no goal factor, precision 0)
static inline GpConst gp_const(float dt, float s_start, float s_gp, float s_goal, float s_coll, float delta = 0.f, int trust = 0, float step = 0.f) {
    const auto prec = [](float sigma) { return 1.0 / ((double)sigma * sigma); };
    return {dt, prec(s_start), prec(s_gp), s_goal > 0.f ? prec(s_goal) : 0.0, prec(s_coll), delta, step, trust};
}

// The workspace of a call: byte offsets of its sections from the 256-byte aligned base (mpb_gpmp2_workspace_bytes is `total`).
//   jac        (MPB_MAX_FIELDS, B, H, D + 1) floats, (h_t, c_t) per chained field.  AT OFFSET 0, sized for MPB_MAX_FIELDS whatever the call
//              chains, and the ONLY section the linearisation writes: ops.gpmp2_collision_rows hands mpb_gpmp2_linearize this section alone
//   diag_sum   (H, 2D) doubles, diag(A^T K A) summed over the particles; diag_mean right behind it: their mean, the damping; solve: see gp_layout
struct GpLayout { size_t jac, diag_sum, diag_mean, solve, total; };
GpLayout gp_layout(int B, int H, int D);

// One GPMP2 call as the C-ABI hands it over (what an entry point is not given is 0)
struct GpCall {
    char* workspace;             // 256-byte aligned; its sections are at workspace + at.<section> once gp_check has passed the call
    int B, H, D, n_fields, n_interp, geom_flags;
    hipStream_t stream;
    GpConst K;
    float *x, *costs_out;
    const float *geom, *start, *goal;
    const double* diag_mean;     // the caller's (all-reduced) damping, or NULL: the workspace's
    GpLayout at;
    const double* damping() const { return !K.trust ? nullptr : diag_mean ? diag_mean : (const double*)(workspace + at.diag_mean); }
};

// the low-rank form (mpb_gpmp2_lr.hip): whether it takes the shape, the doubles of GpLayout::solve it needs, its launches with their launch check
bool mpb_gpmp2_lr_ok(int H, int D, int n_fields);
size_t mpb_gpmp2_lr_ws_doubles(int B, int H, int D);
int mpb_gpmp2_lr_launch(const GpCall& c);
