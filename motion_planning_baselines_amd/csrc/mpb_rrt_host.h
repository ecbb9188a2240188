// mpb_rrt_host.h -- the host side the launchers of the sample-based planners share (RRT-Connect, RRT*, STRRT, PRM, the shortcut pass, the
// trajectory validation): the shape check, the model predicate, the <DT, MODEL> dispatch and the argument checks of *_init and *_run.
// Every check reports under the entry point's name `who`; the order of the checks is part of the ABI (a call wrong in two ways gets the
// earlier message).  No device code.
#pragma once
#include <type_traits>

#include "mpb_host.h"
#include "mpb_model_panda.h"

// the shapes a workspace is served for; words_per_node: what one node of one problem takes at most, for the bound that keeps every
// offset a kernel forms within 32-bit indexing
static int rrt_shape_check(const char* who, double words_per_node, int B, int max_nodes, int n_pre, int D) {
    if (n_pre > MPB_RRT_MAX_PRE_SAMPLES) return mpb_failf(MPB_E_UNSUPPORTED, "%s: n_pre = %d exceeds the %d pool entries the kernel keeps in LDS", who, n_pre, MPB_RRT_MAX_PRE_SAMPLES);
    if (D > MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "%s: D = %d exceeds MPB_MAX_DOF = %d", who, D, MPB_MAX_DOF);
    if (B < 0 || max_nodes < 2 || n_pre < 1 || D < 1) return mpb_failf(MPB_E_INVALID, "%s: bad shape (B %d, max_nodes %d, n_pre %d, D %d)", who, B, max_nodes, n_pre, D);
    if ((double)B * max_nodes * words_per_node > 2.0e9) return mpb_failf(MPB_E_UNSUPPORTED, "%s: B x max_nodes too large", who);
    return MPB_OK;
}

// may a launcher pick the kernels instantiated for the compile-time Panda?
static bool rrt_use_model(int geom_flags, int D) { return mpb_flags_model_on_grids(geom_flags, PandaModel::ID) && D == PandaModel::N_DOF; }

// The <DT, MODEL> instantiation a launcher picks -- the compile-time Panda where rrt_use_model allows, else the D among DTS... a kernel is
// instantiated for, else the run-time-D form <0, 0>: returns launch(DT, MODEL), both handed over as std::integral_constant values.
template <int... DTS, class Launch>
static int rrt_dispatch(int geom_flags, int D, Launch launch) {
    using std::integral_constant;
    if (rrt_use_model(geom_flags, D)) return launch(integral_constant<int, PandaModel::N_DOF>{}, integral_constant<int, PandaModel::ID>{});
    int rc = MPB_OK;
    if (((D == DTS && (rc = launch(integral_constant<int, DTS>{}, integral_constant<int, 0>{}), true)) || ...)) return rc;
    return launch(integral_constant<int, 0>{}, integral_constant<int, 0>{});
}

// what every *_init checks, and every *_run first: the shapes, the pointers (any_null: one of the call's required pointers is null;
// draws_unpaired: RRT*'s two recorded-draw arrays, one given without the other), the alignment, the workspace's size (need: the bytes
// the planner's layout takes for these shapes)
static int rrt_init_check(const char* who, double words_per_node, int B, int max_nodes, int n_pre, int D, bool any_null, bool draws_unpaired,
                          const void* workspace, const void* geom, size_t workspace_bytes, size_t need) {
    const int rc = rrt_shape_check(who, words_per_node, B, max_nodes, n_pre, D);
    if (rc != MPB_OK) return rc;
    if (any_null) return mpb_failf(MPB_E_INVALID, "%s: null pointer", who);
    if (draws_unpaired) return mpb_failf(MPB_E_INVALID, "%s: sample_idx and goal_draw are given together or not at all", who);
    if (mpb_misaligned16(workspace, geom)) return mpb_failf(MPB_E_INVALID, "%s: workspace and geom must be 16-byte aligned", who);
    if (workspace_bytes < need) return mpb_failf(MPB_E_INVALID, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    return MPB_OK;
}

// ... and what every *_run checks after that (limits_ok: the planner's own iteration limits are in range)
static int rrt_run_check(const char* who, int Lmax, int iter0, int n_iters, int total_iters, bool limits_ok, float step_size, float n_radius) {
    if (Lmax < 2 || iter0 < 0 || n_iters < 0 || total_iters < 0 || iter0 > total_iters || !limits_ok) return mpb_failf(MPB_E_INVALID, "%s: bad Lmax / iteration range / iteration limits", who);
    if (!(step_size > 0.f) || !(n_radius > 0.f)) return mpb_failf(MPB_E_INVALID, "%s: step_size and n_radius must be positive", who);
    return MPB_OK;
}
