// mpb_world_host.h -- host side the *_world launchers share (mpb_world.hip, mpb_rrt_connect.hip, mpb_path_shortcut.hip,
// mpb_traj_validate.hip): the two optional buffers of a world checked and their headers read into the WorldArgs a kernel is launched
// with, and the LDS the self blocks take.  A *_world entry makes its old entry's checks first, under its own name and in the old order,
// then world_args: alignment, the SDF header, the self header (both through the caches of mpb_sdf_host.h / mpb_self_host.h), each
// buffer's n_dof against D.  With both buffers null nothing here runs and the old kernels are launched.  Included after mpb_world.h
// (WorldArgs).
#pragma once
#include "mpb_rrt_host.h"
#include "mpb_sdf_host.h"
#include "mpb_self_host.h"

static inline bool world_present(const float* sdfb, const float* selfb) { return sdfb != nullptr || selfb != nullptr; }

// `w` for a launch with D coordinates on the current device; a buffer packed for another robot width is refused
static int world_args(const char* who, const float* sdfb, const float* selfb, int D, WorldArgs& w) {
    w = WorldArgs{};
    w.sdfb = sdfb;
    w.selfb = selfb;
    w.n_dof = D;
    if (mpb_misaligned16(sdfb, selfb)) return mpb_failf(MPB_E_INVALID, "%s: the SDF-grid and the self-collision buffer must be 16-byte aligned", who);
    int rc;
    if (sdfb != nullptr) {
        SdfShape S;
        if ((rc = sdf_shape(sdfb, S, who))) return rc;
        if (S.n_dof != D) return mpb_failf(MPB_E_INVALID, "%s: D = %d, the SDF-grid buffer's robot has %d coordinates", who, D, S.n_dof);
        w.sdf_links = S.n_links, w.nx = S.nx, w.ny = S.ny, w.nz = S.nz;
    }
    if (selfb != nullptr) {
        SelfShape S;
        if ((rc = self_shape(selfb, S, who))) return rc;
        if (S.n_dof != D) return mpb_failf(MPB_E_INVALID, "%s: D = %d, the self-collision buffer's chain has %d joints", who, D, S.n_dof);
        w.self_links = S.n_links, w.self_pairs = S.n_pairs;
    }
    return MPB_OK;
}

// dynamic LDS of the self blocks of a workgroup of `waves` waves ([L][3][64] words each; 0 without a self buffer)
static inline size_t world_self_lds_bytes(const WorldArgs& w, int waves) {
    return w.selfb != nullptr ? (size_t)w.self_links * 192 * sizeof(float) * (size_t)waves : 0;
}
