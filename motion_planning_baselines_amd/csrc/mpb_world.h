// mpb_world.h -- ONE in-kernel collision predicate over the whole planning task, "the world" (build-defined): a
// configuration is in collision iff  c_obs(q) > 0  or  c_sdf(q) > 0  or  c_self(q) > 0,  the three costs exactly what the stand-alone
// predicates compute:
//   c_obs   rrt_config_cost (mpb_rrt.h) on the packed geometry: mpb_collision_check's gap;
//   c_sdf   sdf_waypoint_cost<false> (mpb_sdf.h) on a packed SDF-grid buffer: mpb_sdf_grid_collision_check's gap;
//   c_self  self_store_centres<false> + self_pair_sum<false> (mpb_self.h) on a packed self buffer: mpb_self_collision_check's gap.
// This is PlanningTask._in_collision's answer (three launches ORed) in one call per lane, for the kernels that decide collisions inside a
// loop: the RRT-Connect tree, the shortcut pass, the trajectory validation, and the stand-alone world predicate (mpb_world.hip).
//
// WORLD is a compile-time switch: with WORLD == 0 world_config_cost is the rrt_config_cost call and nothing else (the view's geom is all
// it reads); everything else sits under `if constexpr`.  With WORLD != 0 either buffer may still be absent at run time (a null pointer,
// block-uniform): an absent part costs one scalar branch and no LDS.
// Self-collision needs its [link][xyz][lane] column block in LDS, 768 B per sphere PER WAVE: the launcher sizes it from the header it
// read (world_self_lds_bytes of mpb_world_host.h) and the kernel hands every wave its own block (world_view).  A lane reads and writes its
// own column only: no barrier, and the block is dead between two calls.
// A buffer whose header no longer holds what the launcher read (sdf_header_matches / self_header_matches false) puts EVERY configuration
// in collision, the stand-alone predicates' rule; its part reads NaN.  No kernel forms an address from a header word the launcher has
// not checked.
// Block-uniformity: rrt_config_cost holds __syncthreads() -- every thread of the block calls world_config_cost on every trip (a lane
// without work passes any valid configuration); the two new parts hold no barrier.
#pragma once
#include "mpb_rrt.h"
#include "mpb_sdf.h"
#include "mpb_self.h"

// what a launcher hands a world kernel next to the geometry: the two buffers (null: absent) with the shapes IT read from their headers
struct WorldArgs {
    const float* sdfb;
    const float* selfb;
    int n_dof;                    // the D the launcher held both headers against
    int sdf_links, nx, ny, nz;
    int self_links, self_pairs;
};

struct WorldView {
    const float* geom;            // the chained obstacle fields (rrt_config_cost)
    WorldArgs a;
    float* self_lds;              // THIS wave's [link][xyz][lane] block (null without a self buffer)
};

struct WorldCost {
    float obs, sdf, self;         // the three hinge sums; a refused buffer's part is NaN
    bool refused;                 // a header has changed since the launcher read it (decided on integers: the build assumes finite math)
};

// the view of a thread: `lds` is the dynamic LDS left for the self blocks, one of self_links * 192 words per wave of the block
__device__ __forceinline__ WorldView world_view(const float* geom, const WorldArgs& a, float* lds) {
    WorldView W;
    W.geom = geom;
    W.a = a;
    W.self_lds = (a.selfb != nullptr) ? lds + (size_t)(threadIdx.x >> 6) * a.self_links * 192 : nullptr;
    return W;
}

template <int MODEL, int WORLD>
__device__ __forceinline__ WorldCost world_config_cost(const WorldView& W, unsigned* gridw, float4* otab, const float*& staged,
                                                       const float (&q)[MPB_MAX_DOF]) {
    WorldCost c = {rrt_config_cost<MODEL>(W.geom, gridw, otab, staged, q), 0.f, 0.f, false};
    if constexpr (WORLD != 0) {
        const float nan = __uint_as_float(0x7FC00000u);
        if (W.a.sdfb != nullptr) {                                              // (block-uniform)
            if (sdf_header_matches(W.a.sdfb, W.a.n_dof, W.a.sdf_links, W.a.nx, W.a.ny, W.a.nz)) {
                const GeomView G = sdf_robot_view(W.a.sdfb);
                const SdfLattice S = sdf_lattice(W.a.sdfb, W.a.nx, W.a.ny, W.a.nz);
                float dq[MPB_MAX_DOF];
                c.sdf = sdf_waypoint_cost<false>(G, S, W.a.sdf_links, q, dq);
            } else {
                c.sdf = nan;
                c.refused = true;
            }
        }
        if (W.a.selfb != nullptr) {                                             // (block-uniform)
            if (self_header_matches(W.a.selfb, W.a.n_dof, W.a.self_links, W.a.self_pairs)) {
                const GeomView G = self_view(W.a.selfb);
                const float* pairs = W.a.selfb + reinterpret_cast<const int*>(W.a.selfb)[MPB_SW_OFF_PAIRS];
                const int lane = threadIdx.x & 63;
                bool any = false;
                self_store_centres<false>(G, W.a.self_links, q, W.self_lds, nullptr, lane);
                c.self = self_pair_sum<false>(pairs, W.a.self_pairs, W.a.self_links, W.self_lds, nullptr, lane, any);
            } else {
                c.self = nan;
                c.refused = true;
            }
        }
    }
    return c;
}

__device__ __forceinline__ bool world_hit(const WorldCost& c) { return c.refused || c.obs > 0.f || c.sdf > 0.f || c.self > 0.f; }

// the sum validation reports as max_gap: obstacles, then grid, then self, every addition rounded
__device__ __forceinline__ float world_gap(const WorldCost& c) {
#pragma clang fp contract(off)
    return (c.obs + c.sdf) + c.self;
}

template <int MODEL, int WORLD>
__device__ __forceinline__ bool world_in_collision(const WorldView& W, unsigned* gridw, float4* otab, const float*& staged,
                                                   const float (&q)[MPB_MAX_DOF]) {
    return world_hit(world_config_cost<MODEL, WORLD>(W, gridw, otab, staged, q));
}
