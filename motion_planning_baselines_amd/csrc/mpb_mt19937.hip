// mpb_mt19937.hip -- mpb_mt19937_normals: n_calls successive torch CPU normal_() draws of n fp32 elements each, on the device
// (the kernels and their layout: mpb_mt19937.h; the host tables and torch's state: motion_planning_baselines_amd/mt19937.py).
#include <hip/hip_runtime.h>

#include "mpb_common.h"
#include "mpb_host.h"
#include "mpb_mt19937.h"
#include "../../include/mpb.h"

extern "C" int mpb_mt19937_normals(float* out, int n, int n_calls, const uint32_t* state_in, int pos, int final_idx, uint32_t* state_out,
                                   const uint16_t* jump_idx, const int* jump_cnt, int jump_stride, const int* segs, int n_segs,
                                   uint32_t* work, void* stream) {
    if (!out || !state_in || !state_out || !jump_idx || !jump_cnt || !segs || !work)
        return mpb_fail(MPB_E_INVALID, "mpb_mt19937_normals: null pointer");
    if (const char* why = mt19937_bad_args(n, n_calls, pos, final_idx, jump_stride, n_segs)) return mpb_failf(MPB_E_INVALID, "mpb_mt19937_normals: %s", why);
    if (((uintptr_t)jump_idx & 15u) || ((uintptr_t)work & 15u)) return mpb_fail(MPB_E_INVALID, "mpb_mt19937_normals: jump_idx / work must be 16-byte aligned");
    hipError_t e = mt19937_launch<false>(out, n, state_in, pos, final_idx, state_out, jump_idx, jump_cnt, jump_stride, segs, n_segs, work,
                                         nullptr, (hipStream_t)stream);
    if (e != hipSuccess) return mpb_failf(MPB_E_HIP, "mpb_mt19937_normals: HIP launch failed: %s", hipGetErrorString(e));
    return MPB_OK;
}
