// mpb_stomp_api.hip -- the STOMP part of the C-ABI (include/mpb.h): every entry point packs its arguments into one
// StompCall (mpb_stomp_host.h) and from there on only the record travels -- through the one argument check, the planner
// that picks the form of the loop, and the launchers the kernel files export.  No kernel.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <atomic>
#include <chrono>

#include "mpb_stomp_host.h"
#include "mpb_stomp_fused.h"

// ------------------------------------------------------------------------------------------------
// the argument check of the entry points that take a whole call
// ------------------------------------------------------------------------------------------------
// Where the entry points differ, they differ by one of these options.
struct StompCheck {
    const char* who;         // the name the message carries
    int n_iters;             // of this launch (mpb_stomp_plan_create has none yet: 0)
    // The call may run the two-kernel loop, whose kernels have an envelope of their own: H in [3, MPB_MAX_H], D in
    // [1, MPB_MAX_DOF] joints and the update kernel's LDS budget.  A persistent launch is checked WITHOUT it: fused_plan has
    // admitted the horizon and the channel count by then (or has sent the call to the two-kernel loop and this check with
    // the option set), and the persistent kernels never see D.
    bool two_kernel;
    // mpb_stomp_step_profile averages over its iterations: it refuses an empty batch and n_iters outside [1, 1024], where the
    // other entry points return at once for P = 0 and take any n_iters >= 0.
    bool profile;
    // The buffers named in the alignment message; `extra` are those beyond the record (workspace, means_copy).  NULL: no
    // alignment test -- mpb_stomp_step_profile has never had one (ops.stomp_step_profile hands it whole tensors).
    const char* aligned;
    const void *extra0 = nullptr, *extra1 = nullptr;
};

static int stomp_check(const StompCall& c, const StompCheck& k) {
    if (!c.means || !c.samples || !c.costs || !c.weights || !c.L || !c.Sigma || !c.geom) return mpb_failf(MPB_E_INVALID, "%s: null pointer", k.who);
    bool bad = c.P < (k.profile ? 1 : 0) || c.S < 1 || !(c.d == c.D || c.d == 2 * c.D) || k.n_iters < (k.profile ? 1 : 0) || (k.profile && k.n_iters > 1024);
    if (k.two_kernel) bad = bad || c.H < 3 || c.H > MPB_MAX_H || c.D < 1 || c.D > MPB_MAX_DOF;
    if (bad) return mpb_failf(MPB_E_INVALID, "%s: bad shape", k.who);
    if (!(c.temperature > 0.f)) return mpb_failf(MPB_E_INVALID, "%s: temperature must be > 0", k.who);
    if (k.aligned && (mpb_misaligned16(c.means, c.eps, c.samples, c.L, c.Sigma, c.geom) || mpb_misaligned16(k.extra0, k.extra1)))
        return mpb_failf(MPB_E_INVALID, "%s: %s must be 16-byte aligned", k.who, k.aligned);
    return k.two_kernel ? mpb_update_envelope(c.S, c.H, c.d, k.who) : MPB_OK;   // (its shape test cannot fail here: the LDS budget)
}

// ------------------------------------------------------------------------------------------------
// the two-kernel loop
// ------------------------------------------------------------------------------------------------
extern "C" int mpb_stomp_sample(const float* means, const float* eps, float* samples, const float* L,
                                const float* geom, int geom_flags, float* costs, int P, int S, int H, int d, float k_sigma,
                                float weight, uint64_t seed, uint32_t iter, uint32_t particle_offset, void* stream) {
    if (P == 0) return MPB_OK;
    if (!means || !samples || !L) return mpb_failf(MPB_E_INVALID, "%s: null pointer", __func__);
    if ((geom == nullptr) != (costs == nullptr)) return mpb_failf(MPB_E_INVALID, "%s: geom and costs must be given together", __func__);
    if (P < 0 || S < 1 || H < 3 || H > MPB_MAX_H || d < 1 || d > MPB_MAX_D) return mpb_failf(MPB_E_INVALID, "%s: bad shape", __func__);
    if (mpb_misaligned16(means, eps, samples, L, geom)) return mpb_failf(MPB_E_INVALID, "%s: means / eps / samples / L / geom must be 16-byte aligned", __func__);
    StompCall c = {};        // (the means are only read; without geom the kernel takes no flags, k_sigma or weight)
    c.means = const_cast<float*>(means); c.eps = eps; c.samples = samples; c.costs = costs; c.L = L; c.geom = geom;
    c.P = P; c.S = S; c.H = H; c.d = d; c.seed = seed; c.particle_offset = particle_offset;
    if (geom) { c.geom_flags = geom_flags; c.k_sigma = k_sigma; c.weight = weight; }
    mpb_stomp_launch_sample(c, eps, iter, (hipStream_t)stream, nullptr);
    return mpb_check_launch(__func__);
}

extern "C" int mpb_stomp_update(float* means, const float* samples, const float* costs, float* weights,
                                const float* Sigma, int P, int S, int H, int d, float lr, float temperature,
                                void* stream) {
    if (P == 0) return MPB_OK;
    if (!means || !samples || !costs || !weights) return mpb_failf(MPB_E_INVALID, "%s: null pointer", __func__);
    if (P < 0) return mpb_failf(MPB_E_INVALID, "%s: bad shape", __func__);
    if (const int rc = mpb_update_envelope(S, H, d, __func__)) return rc;
    if (!(temperature > 0.f)) return mpb_failf(MPB_E_INVALID, "%s: temperature must be > 0", __func__);
    if (mpb_misaligned16(means, samples, Sigma)) return mpb_failf(MPB_E_INVALID, "%s: means / samples / Sigma must be 16-byte aligned", __func__);
    StompCall c = {};        // (samples and costs are only read)
    c.means = means; c.samples = const_cast<float*>(samples); c.costs = const_cast<float*>(costs); c.weights = weights; c.Sigma = Sigma;
    c.P = P; c.S = S; c.H = H; c.d = d; c.lr = lr; c.temperature = temperature;
    mpb_stomp_launch_update(c, (hipStream_t)stream, nullptr);   // (within the envelope)
    return mpb_check_launch(__func__);
}

static int stomp_step(const StompCall& c, const StompLaunch& l) {
    if (c.P == 0) return MPB_OK;
    if (const int rc = stomp_check(c, {"mpb_stomp_step", l.n_iters, true, false, "means / eps / samples / L / Sigma / geom"})) return rc;
    const size_t eps_stride = (size_t)c.S * c.d * c.P * c.H;
    // Launch-queue throttle: long runs keep at most two chunks of MPB_CHUNK iterations queued ahead of the
    // GPU (before queueing chunk k+2 the host waits on an event recorded after chunk k), so the host never
    // sits on thousands of pending launches.  Short calls (<= 2 chunks) and calls made while the stream is
    // being captured into a graph never wait.
    constexpr int MPB_CHUNK = 128;
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const bool throttle = l.n_iters > 2 * MPB_CHUNK &&
                          hipStreamIsCapturing(l.stream, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone;
    for (int it = 0; it < l.n_iters; ++it) {
        if (throttle && it % MPB_CHUNK == 0) {
            const int k = (it / MPB_CHUNK) & 1;
            if (ev[k]) (void)hipEventSynchronize(ev[k]);                 // chunk it/MPB_CHUNK - 2 has finished
            else (void)hipEventCreateWithFlags(&ev[k], hipEventDisableTiming);
        }
        mpb_stomp_launch_sample(c, c.eps ? c.eps + (size_t)it * eps_stride : nullptr, l.iter0 + (uint32_t)it, l.stream, nullptr);
        mpb_stomp_launch_update(c, l.stream, nullptr);
        if (throttle && it % MPB_CHUNK == MPB_CHUNK - 1) (void)hipEventRecord(ev[(it / MPB_CHUNK) & 1], l.stream);
    }
    for (int k = 0; k < 2; ++k)
        if (ev[k]) (void)hipEventDestroy(ev[k]);
    return mpb_check_launch("mpb_stomp_step");
}

extern "C" int mpb_stomp_step(float* means, const float* eps, float* samples, float* costs, float* weights,
                              const float* L, const float* Sigma, const float* geom, int geom_flags, int P, int S, int H, int d, int D,
                              float k_sigma, float weight, float lr, float temperature, int n_iters, uint64_t seed,
                              uint32_t iter0, uint32_t particle_offset, void* stream) {
    const StompCall c = {means, eps, samples, costs, weights, L, Sigma, geom, geom_flags, P, S, H, d, D,
                         k_sigma, weight, lr, temperature, seed, particle_offset};
    return stomp_step(c, {n_iters, iter0, nullptr, (hipStream_t)stream, nullptr});
}

extern "C" int mpb_stomp_step_profile(float* means, float* samples, float* costs, float* weights, const float* L,
                                      const float* Sigma, const float* geom, int geom_flags, int P, int S, int H, int d, int D,
                                      float k_sigma, float weight, float lr, float temperature, int n_iters, uint64_t seed,
                                      uint32_t iter0, uint32_t particle_offset, void* stream, float* sample_kernel_ms,
                                      float* update_kernel_ms) {
    const StompCall c = {means, nullptr, samples, costs, weights, L, Sigma, geom, geom_flags, P, S, H, d, D,
                         k_sigma, weight, lr, temperature, seed, particle_offset};
    if (!sample_kernel_ms || !update_kernel_ms) return mpb_failf(MPB_E_INVALID, "%s: null pointer", __func__);
    if (const int rc = stomp_check(c, {__func__, n_iters, true, true, nullptr})) return rc;
    hipStream_t st = (hipStream_t)stream;
    StompEvents* ev = new StompEvents[2 * (size_t)n_iters]();      // per iteration: the sample launch's pair, the update launch's
    int rc = MPB_OK;
    for (int i = 0; i < 2 * n_iters && rc == MPB_OK; ++i)
        if (hipEventCreate(&ev[i].start) != hipSuccess || hipEventCreate(&ev[i].stop) != hipSuccess)
            rc = mpb_failf(MPB_E_HIP, "%s: hipEventCreate failed", __func__);
    if (rc == MPB_OK) {
        for (int it = 0; it < n_iters; ++it) {
            mpb_stomp_launch_sample(c, nullptr, iter0 + (uint32_t)it, st, &ev[2 * it]);
            mpb_stomp_launch_update(c, st, &ev[2 * it + 1]);
        }
        rc = mpb_check_launch(__func__);
    }
    if (rc == MPB_OK && hipStreamSynchronize(st) != hipSuccess) rc = mpb_failf(MPB_E_HIP, "%s: synchronize failed", __func__);
    double sa = 0.0, sb = 0.0;
    for (int it = 0; it < n_iters && rc == MPB_OK; ++it) {
        float ma = 0.f, mb = 0.f;
        if (hipEventElapsedTime(&ma, ev[2 * it].start, ev[2 * it].stop) != hipSuccess ||
            hipEventElapsedTime(&mb, ev[2 * it + 1].start, ev[2 * it + 1].stop) != hipSuccess)
            rc = mpb_failf(MPB_E_HIP, "%s: hipEventElapsedTime failed", __func__);
        sa += ma;
        sb += mb;
    }
    for (int i = 0; i < 2 * n_iters; ++i) {
        if (ev[i].start) (void)hipEventDestroy(ev[i].start);
        if (ev[i].stop) (void)hipEventDestroy(ev[i].stop);
    }
    delete[] ev;
    if (rc != MPB_OK) return rc;
    *sample_kernel_ms = (float)(sa / n_iters);
    *update_kernel_ms = (float)(sb / n_iters);
    return MPB_OK;
}

// ------------------------------------------------------------------------------------------------
// the persistent loop: which form serves a call, its workspace, the call itself
// ------------------------------------------------------------------------------------------------
// which form of the loop serves a call, and the workspace it needs
struct FusedPlan {
    int path;            // MPB_STOMP_PATH_*: 0 two-kernel loop, 1 persistent with exchange, 2 persistent one workgroup per particle
    int nc;              // workgroups per particle (exchange layout)
    bool hx;             // served by the generalised kernel (any H <= 128, d <= 16, S <= 128)
    int nb;              // (H = 64 kernel) 2: one workgroup per particle runs two batches of 16 samples; (generalised kernel) passes per workgroup and iteration
    size_t ws_bytes;     // workspace the persistent kernel needs (header only when nothing is exchanged)
};
static FusedPlan fused_plan(int geom_flags, int P, int S, int H, int d) {
    FusedPlan f = {MPB_STOMP_PATH_TWO_KERNEL, 1, false, 1, 0};
    if (P < 1 || S < 1) return f;
    const int n_cu = mpb_device_cu_count();
    // MPB_STOMP_HX = 1 sends every shape to the generalised kernel (a test aid: it is compared with the H = 64 kernel)
    const char* hx_env = getenv("MPB_STOMP_HX");
    const int force_hx = hx_env ? atoi(hx_env) : 0;
    const bool v1 = !force_hx && H == 64 && S <= FUSED_WAVES * FUSED_MAX_CHUNKS && mpb_flags_all_grids(geom_flags) &&
                    (d == 2 || d == 3 || d == 4 || d == 6 || d == 7 || d == 14);
    if (!v1) {
        if (!mpb_fused_hx_plan(geom_flags, n_cu, P, S, H, d, &f.nc, &f.nb, &f.ws_bytes)) return f;
        f.hx = true;
        f.path = f.nc > 1 ? MPB_STOMP_PATH_PERSISTENT_EXCHANGE : MPB_STOMP_PATH_PERSISTENT;
        return f;
    }
    f.nc = (S + FUSED_WAVES - 1) / FUSED_WAVES;
    // layout: one workgroup per (particle, chunk of 16 samples) with the exchange -- or, when there are at least as many
    // particles as CUs and S <= 32, one workgroup per particle running two batches of 16 (no exchange; same bits).
    // MPB_STOMP_BATCHES = 1 / 2 forces one or the other (2 only where it applies).
    static const int force_nb = [] { const char* e = getenv("MPB_STOMP_BATCHES"); return e ? atoi(e) : 0; }();
    // rounds of workgroups either layout needs on this chip: the two-batch workgroup takes ~1.88 x as long per iteration
    const long r1 = (2L * P + n_cu - 1) / n_cu, r2 = ((long)P + n_cu - 1) / n_cu;
    const bool two_batches = f.nc == 2 && force_nb != 1 && (force_nb == 2 || 188 * r2 < 100 * r1);
    f.nb = two_batches ? 2 : 1;
    const bool exchange = f.nc > 1 && !two_batches;
    f.path = exchange ? MPB_STOMP_PATH_PERSISTENT_EXCHANGE : MPB_STOMP_PATH_PERSISTENT;
    f.ws_bytes = (exchange ? mpb_fused_ws_floats(P, f.nc) : FUSED_HDR_WORDS) * sizeof(float);
    return f;
}

extern "C" size_t mpb_stomp_workspace_bytes(int P, int S, int H, int d) {
    if (P < 1 || S < 1) return 0;
    // what the layout the launcher will pick needs (grid-backed fields assumed; a call the persistent kernel cannot
    // serve needs none): the exchange area only when partner workgroups exchange partials, else just the header
    const FusedPlan f = fused_plan(MPB_GEOM_FLAG_ALL_GRIDS, P, S, H, d);
    // (a scene packed with LIST grids -- geometry version 7, MPB_GEOM_FLAG_ALL_LISTS -- goes to the generalised kernel even at H = 64, whose
    // exchange slots are larger: the workspace serves whichever of the two the geometry will select)
    const FusedPlan fl = fused_plan(MPB_GEOM_FLAG_ALL_LISTS, P, S, H, d);
    size_t b = f.path == MPB_STOMP_PATH_TWO_KERNEL ? FUSED_HDR_WORDS * sizeof(float) : f.ws_bytes;
    if (fl.path != MPB_STOMP_PATH_TWO_KERNEL && fl.ws_bytes > b) b = fl.ws_bytes;
    return b;
}

extern "C" int mpb_stomp_workspace_init(float* workspace, size_t workspace_bytes, void* stream) {
    if (!workspace || workspace_bytes < FUSED_HDR_WORDS * sizeof(float)) return mpb_fail(MPB_E_INVALID, "mpb_stomp_workspace_init: workspace too small");
    if (hipMemsetAsync(workspace, 0, FUSED_HDR_WORDS * sizeof(float), (hipStream_t)stream) != hipSuccess) return mpb_fail(MPB_E_HIP, "mpb_stomp_workspace_init: memset failed");
    return MPB_OK;
}

extern "C" int mpb_stomp_run_path(int geom_flags, size_t workspace_bytes, int P, int S, int H, int d) {
    const FusedPlan f = fused_plan(geom_flags, P, S, H, d);
    return (f.path != MPB_STOMP_PATH_TWO_KERNEL && workspace_bytes >= f.ws_bytes) ? f.path : MPB_STOMP_PATH_TWO_KERNEL;
}

// mpb_stomp_run_checked behind its packing (status: the caller's host-visible block or NULL; tag_out: NULL or where the call's tag goes)
static int stomp_run(const StompCall& c, float* workspace, size_t workspace_bytes, uint32_t* status, const StompLaunch& l, uint32_t* tag_out) {
    if (tag_out) *tag_out = 0u;
    if (c.P == 0) return MPB_OK;
    const FusedPlan f = fused_plan(c.geom_flags, c.P, c.S, c.H, c.d);
    if (l.n_iters == 0 || !workspace || f.path == MPB_STOMP_PATH_TWO_KERNEL || workspace_bytes < f.ws_bytes) {
        const int rc = l.n_iters == 0 ? MPB_OK : stomp_step(c, l);
        if (rc == MPB_OK && l.means_copy && c.means &&
            hipMemcpyAsync(l.means_copy, c.means, sizeof(float) * (size_t)c.P * c.H * c.d, hipMemcpyDeviceToDevice, l.stream) != hipSuccess)
            return mpb_fail(MPB_E_HIP, "mpb_stomp_run: copy of the means failed");
        return rc;
    }
    if (const int rc = stomp_check(c, {"mpb_stomp_run", l.n_iters, false, false, "means / eps / samples / L / Sigma / geom / workspace / means_copy",
                                       workspace, l.means_copy}))
        return rc;
    StompFusedGrid g = {workspace, f.nc, f.nb, 0u, 0ull, nullptr};
    // the status block is host memory the device can write (pinned + mapped): its device address
    if (status) {
        static thread_local uint32_t* seen_host = nullptr;      // (a planner passes the same block every call: asked once)
        static thread_local unsigned* seen_dev = nullptr;
        if (status != seen_host) {
            unsigned* dp = nullptr;
            if (hipHostGetDevicePointer(reinterpret_cast<void**>(&dp), status, 0) != hipSuccess) {
                (void)hipGetLastError();
                return mpb_fail(MPB_E_INVALID, "mpb_stomp_run: status is not pinned, device-mapped host memory");
            }
            seen_host = status;
            seen_dev = dp;
        }
        g.status_dev = seen_dev;
    }
    // the granules' tags and the error word carry a per-call epoch (process-wide counter scrambled over 32 bits), so
    // whatever an earlier call left in the exchange area does not match.  Header: word 0 = tag of the call in which a
    // workgroup gave up, word 1 = tag of the last call; "lost" <=> word 0 == word 1 != 0.  Not capturable in a HIP
    // graph: a replay would reuse the tag.
    static std::atomic<uint32_t> epoch{(uint32_t)std::chrono::steady_clock::now().time_since_epoch().count()};
    g.tag0 = (epoch.fetch_add(1u) + 1u) * 0x9E3779B9u;
    if (g.tag0 == 0u) g.tag0 = 0x9E3779B9u;      // 0 means "none" in the header and the status block
    if (tag_out) *tag_out = g.tag0;
    // bound of every wait for a partner; MPB_STOMP_TIMEOUT_US overrides it (a test aid)
    g.timeout = FUSED_TIMEOUT_TICKS + FUSED_TIMEOUT_PER_ITER * (unsigned long long)l.n_iters;
    if (const char* e = getenv("MPB_STOMP_TIMEOUT_US")) { const long long us = atoll(e); if (us > 0) g.timeout = 100ull * (unsigned long long)us; }
    return f.hx ? mpb_fused_hx_launch(c, l, g) : mpb_fused_launch(c, l, g);
}

extern "C" int mpb_stomp_run_checked(float* means, const float* eps, float* samples, float* costs, float* weights,
                                     const float* L, const float* Sigma, const float* geom, int geom_flags, float* workspace,
                                     size_t workspace_bytes, int P, int S, int H, int d, int D, float k_sigma, float weight, float lr,
                                     float temperature, int n_iters, uint64_t seed, uint32_t iter0, uint32_t particle_offset,
                                     uint32_t* status, uint32_t* tag_out, float* means_copy, void* stream) {
    const StompCall c = {means, eps, samples, costs, weights, L, Sigma, geom, geom_flags, P, S, H, d, D,
                         k_sigma, weight, lr, temperature, seed, particle_offset};
    return stomp_run(c, workspace, workspace_bytes, status, {n_iters, iter0, means_copy, (hipStream_t)stream, nullptr}, tag_out);
}

extern "C" int mpb_stomp_run(float* means, const float* eps, float* samples, float* costs, float* weights,
                             const float* L, const float* Sigma, const float* geom, int geom_flags, float* workspace,
                             size_t workspace_bytes, int P, int S, int H, int d, int D, float k_sigma, float weight, float lr,
                             float temperature, int n_iters, uint64_t seed, uint32_t iter0, uint32_t particle_offset,
                             void* stream) {
    const StompCall c = {means, eps, samples, costs, weights, L, Sigma, geom, geom_flags, P, S, H, d, D,
                         k_sigma, weight, lr, temperature, seed, particle_offset};
    return stomp_run(c, workspace, workspace_bytes, nullptr, {n_iters, iter0, nullptr, (hipStream_t)stream, nullptr}, nullptr);
}

/* A call of mpb_stomp_run_checked with everything but (n_iters, iter0, means_copy, stream) fixed, kept on the library's side:
   a planner whose buffers do not change between optimize() calls hands over four values per call instead of twenty-eight
   (the foreign-function marshalling of the long form is ~3 us of the ~11 us host side of a call).  Device noise only (eps = NULL). */
struct mpb_stomp_plan_s {
    StompCall call;
    float* workspace;
    size_t workspace_bytes;
    uint32_t* status;
};

extern "C" int mpb_stomp_plan_create(mpb_stomp_plan** plan, float* means, float* samples, float* costs, float* weights, const float* L,
                                     const float* Sigma, const float* geom, int geom_flags, float* workspace, size_t workspace_bytes,
                                     int P, int S, int H, int d, int D, float k_sigma, float weight, float lr, float temperature,
                                     uint64_t seed, uint32_t particle_offset, uint32_t* status) {
    if (!plan) return mpb_failf(MPB_E_INVALID, "%s: null pointer", __func__);
    *plan = nullptr;
    const StompCall c = {means, nullptr, samples, costs, weights, L, Sigma, geom, geom_flags, P, S, H, d, D,
                         k_sigma, weight, lr, temperature, seed, particle_offset};
    if (const int rc = stomp_check(c, {__func__, 0, false, false, "means / samples / L / Sigma / geom / workspace", workspace})) return rc;
    mpb_stomp_plan_s* q = static_cast<mpb_stomp_plan_s*>(malloc(sizeof(mpb_stomp_plan_s)));
    if (!q) return mpb_failf(MPB_E_HIP, "%s: out of host memory", __func__);
    *q = mpb_stomp_plan_s{c, workspace, workspace_bytes, status};
    *plan = q;
    return MPB_OK;
}

extern "C" int mpb_stomp_plan_launch(mpb_stomp_plan* plan, int n_iters, uint32_t iter0, float* means_copy, void* stream, uint32_t* tag_out) {
    if (!plan) return mpb_fail(MPB_E_INVALID, "mpb_stomp_plan_launch: null plan");
    return stomp_run(plan->call, plan->workspace, plan->workspace_bytes, plan->status, {n_iters, iter0, means_copy, (hipStream_t)stream, nullptr}, tag_out);
}

extern "C" int mpb_stomp_plan_destroy(mpb_stomp_plan* plan) {
    free(plan);
    return MPB_OK;
}

/* measurement aid for bench.py: mpb_stomp_run_checked with the kernel's begin / end timestamps recorded on the dispatch
   itself; synchronises the stream and returns the kernel's duration (0 when the call ran the two-kernel loop) */
extern "C" int mpb_stomp_run_timed(float* means, const float* eps, float* samples, float* costs, float* weights,
                                   const float* L, const float* Sigma, const float* geom, int geom_flags, float* workspace,
                                   size_t workspace_bytes, int P, int S, int H, int d, int D, float k_sigma, float weight, float lr,
                                   float temperature, int n_iters, uint64_t seed, uint32_t iter0, uint32_t particle_offset,
                                   uint32_t* status, uint32_t* tag_out, float* means_copy, void* stream, float* kernel_ms) {
    if (!kernel_ms) return mpb_failf(MPB_E_INVALID, "%s: null pointer", __func__);
    *kernel_ms = 0.f;
    StompEvents ev = {nullptr, nullptr};
    if (hipEventCreate(&ev.start) != hipSuccess || hipEventCreate(&ev.stop) != hipSuccess) {
        if (ev.start) (void)hipEventDestroy(ev.start);
        return mpb_failf(MPB_E_HIP, "%s: hipEventCreate failed", __func__);
    }
    const StompCall c = {means, eps, samples, costs, weights, L, Sigma, geom, geom_flags, P, S, H, d, D,
                         k_sigma, weight, lr, temperature, seed, particle_offset};
    uint32_t tag = 0;
    int rc = stomp_run(c, workspace, workspace_bytes, status, {n_iters, iter0, means_copy, (hipStream_t)stream, &ev}, &tag);
    if (tag_out) *tag_out = tag;
    if (rc == MPB_OK && hipStreamSynchronize((hipStream_t)stream) != hipSuccess) rc = mpb_failf(MPB_E_HIP, "%s: synchronize failed", __func__);
    if (rc == MPB_OK && tag != 0u && hipEventElapsedTime(kernel_ms, ev.start, ev.stop) != hipSuccess) {
        (void)hipGetLastError();
        rc = mpb_failf(MPB_E_HIP, "%s: hipEventElapsedTime failed", __func__);
    }
    (void)hipEventDestroy(ev.start);
    (void)hipEventDestroy(ev.stop);
    return rc;
}

/* state of the last persistent launch on this workspace (host-side read of the header: synchronises the stream):
   0 = fine (or no persistent launch yet), 1 = a workgroup gave up waiting for its partner, 2 = header not initialised */
extern "C" int mpb_stomp_run_status(const float* workspace, void* stream, int* timed_out) {
    if (!workspace || !timed_out) return mpb_failf(MPB_E_INVALID, "%s: null pointer", __func__);
    uint32_t w[4] = {0u};
    if (hipMemcpyAsync(w, workspace, sizeof(w), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
        return mpb_failf(MPB_E_HIP, "%s: copy failed", __func__);
    *timed_out = (w[FUSED_HDR_ERR] == w[FUSED_HDR_TAG] && w[FUSED_HDR_TAG] != 0u) ? (w[FUSED_HDR_WHY] == 2u ? 2 : 1) : 0;
    return MPB_OK;
}
