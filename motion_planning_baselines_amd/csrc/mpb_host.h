// mpb_host.h -- host-only helpers shared by the translation units: the last-error buffer, the error returns and the
// argument checks of the C-ABI, and what the launchers of the cost members with kernels of their own share (the cached read of a device
// buffer's header, the dynamic-LDS limit, the checks of rows against a packed robot buffer).  No device code, and no kernel's counters
// depend on it (build.PMC_SOURCES does not list it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <mutex>

#include "../../include/mpb.h"

// thread-local last-error string (512 bytes) of the library the file is linked into: the product library's is defined in
// mpb_lib.hip, the test-aid library's in mpb_debug.hip
char* mpb_err_buf();
// `msg` as it stands (it may come from anywhere: never read as a format)
static inline int mpb_fail(int code, const char* msg) {
    snprintf(mpb_err_buf(), 512, "%s", msg);
    return code;
}
__attribute__((format(printf, 2, 3))) static inline int mpb_failf(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(mpb_err_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}
static inline int mpb_check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return mpb_failf(MPB_E_HIP, "%s: HIP launch failed: %s", what, hipGetErrorString(e));
    return MPB_OK;
}
// the STOMP kernels read eps / L / Sigma / the means and write the samples as 16-byte vectors: a pointer the C-ABI is handed must
// be 16-byte aligned (a view at a 4-byte offset into an allocation would be misaligned dwordx4 accesses)
static inline bool mpb_misaligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr,
                                    const void* e = nullptr, const void* f = nullptr) {
    return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d) | ((uintptr_t)e) | ((uintptr_t)f)) & 15u) != 0;
}
static inline bool mpb_misaligned256(const void* a) { return (((uintptr_t)a) & 255u) != 0; }   // (a workspace carved at 256-byte steps)
// compute units of the current device, 256 where it cannot be asked (every GPU of a node is the same part: asked once per translation unit)
static inline int mpb_device_cu_count() {
    static const int n_cu = [] {
        int dev = 0, n = 0;
        return hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0 ? n : 256;
    }();
    return n_cu;
}
// what the geom_flags of mpb_geom_flags (MPB_GEOM_FLAG_* of include/mpb_geom_layout.h; include/mpb.h says what each promises) tell a
// launcher: the compile-time robot model every chained field is tagged with (0: none) ...
static inline int mpb_flags_model(int geom_flags) { return geom_flags & MPB_GEOM_FLAG_MODEL_MASK; }
// ... every chained field backed by a compact grid / by a list grid; ONE field; a point robot with a small obstacle set in one field
static inline bool mpb_flags_all_grids(int geom_flags) { return (geom_flags & MPB_GEOM_FLAG_ALL_GRIDS) != 0; }
static inline bool mpb_flags_all_lists(int geom_flags) { return (geom_flags & MPB_GEOM_FLAG_ALL_LISTS) != 0; }
static inline bool mpb_flags_one_field(int geom_flags) { return (geom_flags & MPB_GEOM_FLAG_ONE_FIELD) != 0; }
static inline bool mpb_flags_point_small(int geom_flags) { return (geom_flags & MPB_GEOM_FLAG_POINT_SMALL) != 0; }
// ... a point robot in ONE field that has a compact grid, and the cells of the chain's largest grid (what staging it in LDS takes)
static inline bool mpb_flags_point_on_one_grid(int geom_flags) {
    const int need = MPB_GEOM_FLAG_POINT | MPB_GEOM_FLAG_ONE_FIELD | MPB_GEOM_FLAG_ALL_GRIDS;
    return (geom_flags & need) == need;
}
static inline int mpb_flags_cells(int geom_flags) { return (geom_flags >> MPB_GEOM_FLAG_CELLS_SHIFT) & MPB_GEOM_FLAG_CELLS_MASK; }
// ... the model `model_id` AND compact grids throughout: only then may a launcher pick the kernel instantiated for that model
static inline bool mpb_flags_model_on_grids(int geom_flags, int model_id) {
    return mpb_flags_model(geom_flags) == model_id && mpb_flags_all_grids(geom_flags);
}

// ---- the cost members with kernels of their own (self-collision, SDF grid, end-effector pose): what their launchers share -----------
// What a launch needs of a DEVICE buffer's header -- the numbers that size its LDS and bound its row / node indices -- is read once per
// (buffer address, device): one synchronous copy of WORDS header words on the first call with that pointer, kept in a table of 16
// entries that are replaced round-robin.  THE CONTRACT: every kernel is launched with the numbers of the entry, forms every address from
// them, and compares them with the header it finds; where they differ it answers NaN (nothing converged).  So an entry that outlived its
// buffer -- an allocator hands a freed block out again -- costs a wrong answer that says so, never an access outside what the launch
// was sized for; a caller that puts ANOTHER buffer at an address drops the entry first (the members' *_invalidate).
// Shape: a struct that begins { const void* ptr; int dev; ... }; the cache fills those two, the caller's parser the rest.
template <class Shape, int WORDS>
struct MpbHeaderCache {
    std::mutex mu;
    Shape table[16] = {};
    int next = 0;

    // The shape of `buf` (never null) on the current device.  An entry that `keep` accepts is returned as it stands; otherwise the header
    // is read (`noun` names the buffer in the refusal), parse(hdr, out) fills `out` -- or refuses: its code is returned, nothing is
    // stored -- and `out` is stored: over the entry `keep` turned down, else in the next slot of the round.
    template <class Parse, class Keep = bool (*)(const Shape&)>
    int get(const void* buf, Shape& out, const char* who, const char* noun, Parse parse, Keep keep = [](const Shape&) { return true; }) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return mpb_failf(MPB_E_HIP, "%s: hipGetDevice failed", who);
        std::lock_guard<std::mutex> lock(mu);
        int slot = 0;
        while (slot < 16 && !(table[slot].ptr == buf && table[slot].dev == dev)) ++slot;
        if (slot < 16 && keep(table[slot])) { out = table[slot]; return MPB_OK; }
        int32_t hdr[WORDS];
        const hipError_t e = hipMemcpy(hdr, buf, sizeof(hdr), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return mpb_failf(MPB_E_HIP, "%s: reading the %s header failed: %s", who, noun, hipGetErrorString(e));
        out.ptr = buf;
        out.dev = dev;
        const int rc = parse(hdr, out);
        if (rc) return rc;
        if (slot == 16) {
            slot = next;
            next = (next + 1) % 16;
        }
        table[slot] = out;
        return MPB_OK;
    }
    // forget `buf` on every device (the caller names an address)
    void drop(const void* buf) {
        std::lock_guard<std::mutex> lock(mu);
        for (Shape& s : table)
            if (s.ptr == buf) s.ptr = nullptr;
    }
};

// A launch with `bytes` of dynamic LDS: beyond the default limit of 48 KB the kernel's limit is raised to `bytes` -- once per (kernel,
// device) and size reached, remembered here so that a planner's per-iteration launches make no runtime call for it.
static inline int mpb_raise_lds_limit(const void* kernel, int dev, size_t bytes, const char* who) {
    static std::mutex mu;
    static struct { const void* kernel; int dev; size_t bytes; } raised[64];          // what the limits stand at; filled from the front
    if (bytes <= 48 * 1024) return MPB_OK;
    std::lock_guard<std::mutex> lock(mu);
    int slot = 0;
    while (slot < 64 && raised[slot].kernel && !(raised[slot].kernel == kernel && raised[slot].dev == dev)) ++slot;
    if (slot < 64 && raised[slot].bytes >= bytes) return MPB_OK;                     // (an empty slot holds 0 bytes)
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return mpb_failf(MPB_E_HIP, "%s: raising the LDS limit to %zu bytes failed: %s", who, bytes, hipGetErrorString(e));
    if (slot < 64) raised[slot] = {kernel, dev, bytes};                               // (a full table only costs the call again)
    return MPB_OK;
}
// ... on the current device, as a launcher asks for it (at or below 48 KB no runtime call is made)
template <class Kernel>
static inline int mpb_raise_lds_limit(Kernel kernel, size_t bytes, const char* who) {
    if (bytes <= 48 * 1024) return MPB_OK;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return mpb_failf(MPB_E_HIP, "%s: hipGetDevice failed", who);
    return mpb_raise_lds_limit(reinterpret_cast<const void*>(kernel), dev, bytes, who);
}

// a step size a launcher refuses: not finite or not positive, decided on the bits (the build assumes finite math)
static inline bool mpb_bad_step(float step) {
    uint32_t bits;
    memcpy(&bits, &step, 4);
    return (bits >> 31) != 0u || (bits << 1) == 0u || (bits & 0x7F800000u) == 0x7F800000u;
}

// Trajectory rows (B, H, d) against a packed robot buffer, "the <noun> buffer": the refusals that need no header, in the order
// include/mpb.h gives them.  An empty batch passes before its pointers are looked at: the caller returns on `rc || B == 0`.
static inline int mpb_check_rows(const char* who, const char* noun, const void* trajs, const void* buf, const void* out, bool want_grad,
                                 const void* grad, int B, int H, int d, int h_begin) {
    if (d > 2 * MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "%s: rows of d = %d exceed positions + velocities of MPB_MAX_DOF = %d joints", who, d, MPB_MAX_DOF);
    if (B < 0 || H < 1 || d < 1 || h_begin < 0) return mpb_failf(MPB_E_INVALID, "%s: bad shape", who);
    if (B == 0) return MPB_OK;
    if (!trajs || !buf || !out || (want_grad && !grad)) return mpb_failf(MPB_E_INVALID, "%s: null pointer", who);
    if (mpb_misaligned16(buf)) return mpb_failf(MPB_E_INVALID, "%s: the %s buffer must be 16-byte aligned", who, noun);
    return MPB_OK;
}
// the same for the predicate's (N, D) configurations: the caller returns on `rc || N == 0`
static inline int mpb_check_configs(const char* who, const char* noun, const void* q, const void* buf, const void* in_collision, int N, int D) {
    if (D > MPB_MAX_DOF) return mpb_failf(MPB_E_UNSUPPORTED, "%s: D = %d exceeds MPB_MAX_DOF = %d", who, D, MPB_MAX_DOF);
    if (N < 0 || D < 1) return mpb_failf(MPB_E_INVALID, "%s: bad shape", who);
    if (N == 0) return MPB_OK;
    if (!q || !buf || !in_collision) return mpb_failf(MPB_E_INVALID, "%s: null pointer", who);
    if (mpb_misaligned16(buf)) return mpb_failf(MPB_E_INVALID, "%s: the %s buffer must be 16-byte aligned", who, noun);
    return MPB_OK;
}

// the shapes and LDS budget mpb_stomp_update takes (defined beside the update kernels in mpb_kernels.hip): MPB_OK, or the code and
// message (under the name `who`) of the refusal -- for callers that enqueue the update behind other stages and must refuse before
// the first launch
int mpb_update_envelope(int S, int H, int d, const char* who);
