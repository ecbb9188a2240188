// mpb_stomp_host.h -- the host side of a STOMP call, between the C-ABI (mpb_stomp_api.hip) and the kernel files: the record
// every entry point packs its arguments into once, and the launchers the kernel files export for it.  Host code only.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "mpb_host.h"

#define MPB_MAX_D 16       // channels of a STOMP rollout (one matrix-core tile of channels): D <= 8 with velocities, D <= 12 position only

// What is constant over the iterations of a call (include/mpb.h, mpb_stomp_step, for the meaning of each).  Entry points that
// take fewer arguments (mpb_stomp_sample, mpb_stomp_update) leave the rest zero.
struct StompCall {
    float* means;
    const float* eps;        // injected noise of the call's first iteration, or NULL: device noise
    float *samples, *costs, *weights;
    const float *L, *Sigma, *geom;
    int geom_flags;
    int P, S, H, d, D;
    float k_sigma, weight, lr, temperature;
    uint64_t seed;
    uint32_t particle_offset;
};

// Measurement aids: a launch that is given a pair records it on the dispatch itself (hipExtLaunchKernelGGL: kernel begin / end
// timestamps, the quantity rocprofv3 --kernel-trace reports).
struct StompEvents { hipEvent_t start, stop; };
#define MPB_LAUNCH(ev, kernel, grid, block, lds, st, ...)                                                                   \
    do {                                                                                                                    \
        if ((ev) != nullptr) hipExtLaunchKernelGGL(kernel, grid, block, lds, st, (ev)->start, (ev)->stop, 0, __VA_ARGS__);  \
        else hipLaunchKernelGGL(kernel, grid, block, lds, st, __VA_ARGS__);                                                 \
    } while (0)

// What varies from one launch of a call to the next.
struct StompLaunch {
    int n_iters;
    uint32_t iter0;
    float* means_copy;          // (persistent kernels) second destination of the final means, or NULL
    hipStream_t stream;
    const StompEvents* events;  // NULL outside the measurement aids
};

// How a persistent launch is laid out over the chip and how it reports (fused_plan and mpb_stomp_run_checked, mpb_stomp_api.hip).
struct StompFusedGrid {
    float* workspace;
    int nc;                     // workgroups per particle (exchange layout)
    int nb;                     // H = 64 kernel: 2 = one workgroup per particle runs two batches of 16; generalised kernel: passes per iteration
    uint32_t tag0;              // per-call epoch of the granules and the status words
    unsigned long long timeout; // bound of every wait for a partner, in ticks of s_memrealtime
    unsigned* status_dev;       // device address of the caller's status block, or NULL
};

// ---- mpb_kernels.hip: the two kernels of one iteration (c.geom == NULL: samples without costs).  None checks its arguments.
void mpb_stomp_launch_sample(const StompCall& c, const float* eps_it, uint32_t iter, hipStream_t st, const StompEvents* ev);
bool mpb_stomp_launch_update(const StompCall& c, hipStream_t st, const StompEvents* ev);   // false: outside mpb_update_envelope
// ---- mpb_stomp_fused.hip: the persistent H = 64 kernel (d in 2, 3, 4, 6, 7, 14; S <= 64; compact grids) and its exchange area
size_t mpb_fused_ws_floats(int P, int nc);
int mpb_fused_launch(const StompCall& c, const StompLaunch& l, const StompFusedGrid& g);
// ---- mpb_stomp_fused_hx.hip: the generalised kernel (any H <= 128, d <= 16, S <= 128) and the shapes it serves
bool mpb_fused_hx_plan(int geom_flags, int n_cu, int P, int S, int H, int d, int* nc_out, int* nb_out, size_t* ws_bytes);
int mpb_fused_hx_launch(const StompCall& c, const StompLaunch& l, const StompFusedGrid& g);
