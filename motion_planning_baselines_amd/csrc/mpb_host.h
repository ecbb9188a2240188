// mpb_host.h -- host-only helpers shared by the translation units: the last-error buffer, the error returns and the
// argument checks of the C-ABI.  No device code, and no kernel's counters depend on it (build.PMC_SOURCES does not list it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

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
// the shapes and LDS budget mpb_stomp_update takes (defined beside the update kernels in mpb_kernels.hip): MPB_OK, or the code and
// message (under the name `who`) of the refusal -- for callers that enqueue the update behind other stages and must refuse before
// the first launch
int mpb_update_envelope(int S, int H, int d, const char* who);
