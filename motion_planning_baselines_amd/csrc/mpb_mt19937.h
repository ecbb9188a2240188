// mpb_mt19937.h -- torch's CPU Mersenne Twister (mt19937) on the device, in parallel by jump ahead; shared by the product library
// (mpb_mt19937.hip: normal_() blocks) and the test aids (mpb_debug.hip: uniform_() blocks, to check the words bit for bit).
//
// The raw word stream x[] continues torch's 624-word array by x[k+624] = x[k+397] ^ twist(x[k], x[k+1]) (the host restatement,
// motion_planning_baselines_amd/mt19937.py, states the correspondence and the jump).  A draw of T words is cut into SEGMENTS of
// whole 16-chunks (Box-Muller pairs word j with word j + 8 of a chunk), one workgroup each:
//   mt19937_prefix    one workgroup twists from the start array: the PREFIX x[s .. s + 20 559] from the first word drawn, x[s];
//   mt19937_jump      one workgroup per segment (and one for the final state): the segment's first 624 words, as the XOR of the
//                     prefix windows x[s + i ..] over the set coefficients i of t^offset mod phi (host tables: the list of i,
//                     padded to a multiple of 8 with MT_JUMP_PAD, whose window is zero).  The prefix sits in LDS;
//   mt19937_generate  one workgroup per segment twists on from its window in an LDS ring of two 624-word blocks (three dependent
//                     phases of 208 words per block: word m needs m - 227, m - 624, m - 623), tempers, and writes the 16-chunks
//                     that END in the block just made.  The last workgroup writes torch's array after the draw.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define MT_N 624
#define MT_PREFIX 20560               // 19 937 + 623: the windows x[s + i .. s + i + 623], i < 19 937
#define MT_JUMP_PAD MT_PREFIX         // a padding index of the jump lists: the window there is zero
#define MT_WINDOWS_AT 20608           // work buffer: prefix at 0, the windows (n_segs + 1) x 624 from here (16-byte aligned)
#define MT_JUMP_THREADS 640           // one word of the window per thread (10 waves keep the LDS busy)
#define MT_GEN_THREADS 320            // 312 = 39 chunks x 8 Box-Muller pairs of a 624-word block, + the 8 pairs of a tail chunk
#define MT_PREFIX_THREADS 256

__device__ __forceinline__ uint32_t mt_twist(uint32_t a, uint32_t b) {
    return (((a & 0x80000000u) | (b & 0x7FFFFFFFu)) >> 1) ^ ((b & 1u) ? 0x9908B0DFu : 0u);
}

__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9D2C5680u;
    y ^= (y << 15) & 0xEFC60000u;
    y ^= y >> 18;
    return y;
}

// uniform_() in fp32: (w & 0xFFFFFF) * 2^-24, exact
__device__ __forceinline__ float mt_uniform(uint32_t raw) { return (float)(mt_temper(raw) & 0xFFFFFFu) * 0x1p-24f; }

// one 624-word block of the ring: word m (ring slot m mod 1248) from m - 624, m - 623 (the previous block, or this block's first
// word for m = 624k + 623) and m - 227 (an earlier phase)
__device__ __forceinline__ void mt_ring_block(uint32_t* ring, int k) {
    const int base = (k & 1) * MT_N, prev = ((k - 1) & 1) * MT_N;
    for (int ph = 0; ph < 3; ++ph) {
        const int t = ph * 208 + (int)threadIdx.x;
        if (threadIdx.x < 208) {
            const uint32_t a = ring[prev + t];
            const uint32_t b = (t + 1 < MT_N) ? ring[prev + t + 1] : ring[base];
            const uint32_t c = (t >= 227) ? ring[base + t - 227] : ring[prev + t + 397];
            ring[base + t] = c ^ mt_twist(a, b);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(MT_PREFIX_THREADS) mt19937_prefix(const uint32_t* __restrict__ state, int pos,
                                                                    uint32_t* __restrict__ prefix) {
    __shared__ uint32_t ring[2 * MT_N];
    for (int i = threadIdx.x; i < MT_N; i += blockDim.x) ring[i] = state[i];
    __syncthreads();
    // x[m], m from the array's first word: the prefix is x[pos .. pos + MT_PREFIX - 1], pos in [1, 624]
    const int blocks = (pos + MT_PREFIX + MT_N - 1) / MT_N;
    for (int k = 0; k < blocks; ++k) {
        if (k > 0) mt_ring_block(ring, k);
        for (int t = threadIdx.x; t < MT_N; t += blockDim.x) {
            const int m = k * MT_N + t;
            if (m >= pos && m < pos + MT_PREFIX) prefix[m - pos] = ring[(k & 1) * MT_N + t];
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(MT_JUMP_THREADS) mt19937_jump(const uint32_t* __restrict__ prefix, const uint16_t* __restrict__ idx,
                                                                const int* __restrict__ cnt, int stride, uint32_t* __restrict__ windows) {
    extern __shared__ __attribute__((aligned(16))) uint32_t xs[];        // MT_PREFIX + MT_N words: the prefix, then a zero window
    for (int i = threadIdx.x; i < MT_PREFIX + MT_N; i += blockDim.x) xs[i] = i < MT_PREFIX ? prefix[i] : 0u;
    __syncthreads();
    const int seg = blockIdx.x;
    const uint16_t* __restrict__ li = idx + (size_t)seg * stride;
    const int n = cnt[seg];                                                  // a multiple of 8
    const int j = threadIdx.x < MT_N ? (int)threadIdx.x : 0;                 // (the 16 lanes past the window read word 0..15, unused)
    uint32_t acc = 0;
    for (int e = 0; e < n; e += 8) {
        // eight coefficients per step: eight independent LDS reads in flight per wave
        const uint4 q = *reinterpret_cast<const uint4*>(li + e);
        acc ^= xs[(q.x & 0xFFFFu) + j] ^ xs[(q.x >> 16) + j] ^ xs[(q.y & 0xFFFFu) + j] ^ xs[(q.y >> 16) + j]
             ^ xs[(q.z & 0xFFFFu) + j] ^ xs[(q.z >> 16) + j] ^ xs[(q.w & 0xFFFFu) + j] ^ xs[(q.w >> 16) + j];
    }
    if (threadIdx.x < MT_N) windows[(size_t)seg * MT_N + threadIdx.x] = acc;
}

// segs: (call, first full chunk q0, full chunks nq, last segment of its call) per segment.  UNIFORM: the words of uniform_() calls
// (n words a call; the n % 16 words after the last full chunk are the tail); else normal_() calls (n + 16 [n % 16 != 0] words: the
// tail chunk is 16 fresh words at n and writes out[n - 16 .. n - 1], which the full chunks then leave alone).
// Block n_segs: torch's array after the draw, the 624 words at final_idx of the final window and the block after it
// (final_idx < 0: the draw does not twist the array -- copied).
template <bool UNIFORM>
__global__ void __launch_bounds__(MT_GEN_THREADS) mt19937_generate(float* __restrict__ out, int n, const int* __restrict__ segs, int n_segs,
                                                                   const uint32_t* __restrict__ windows, const uint32_t* state_in,
                                                                   int final_idx, uint32_t* state_out) {
    __shared__ uint32_t ring[2 * MT_N];
    const int seg = blockIdx.x;
    const int tid = threadIdx.x;
    if (seg == n_segs) {
        if (final_idx < 0) {
            if (state_out != state_in)
                for (int i = tid; i < MT_N; i += blockDim.x) state_out[i] = state_in[i];
            return;
        }
        for (int i = tid; i < MT_N; i += blockDim.x) ring[i] = windows[(size_t)seg * MT_N + i];
        __syncthreads();
        mt_ring_block(ring, 1);
        for (int i = tid; i < MT_N; i += blockDim.x) state_out[i] = ring[final_idx + i];
        return;
    }
    const int c = segs[4 * seg], q0 = segs[4 * seg + 1], nq = segs[4 * seg + 2];
    const int rem = n & 15;
    const bool tail = segs[4 * seg + 3] && rem != 0;
    const int Q = n >> 4;
    // the tail chunk: its first word (from the segment's), its length in words, its first output element
    const int tw = UNIFORM ? 16 * (Q - q0) : n - 16 * q0;
    const int tlen = UNIFORM ? rem : 16;
    const int tout = UNIFORM ? 16 * Q : n - 16;
    const int clip = (!UNIFORM && rem != 0) ? n - 16 : n;     // full chunks write elements below clip
    const int words = tail ? tw + tlen : 16 * nq;
    const int blocks = (words + MT_N - 1) / MT_N;
    float* __restrict__ o = out + (size_t)c * n;
    for (int i = tid; i < MT_N; i += blockDim.x) ring[i] = windows[(size_t)seg * MT_N + i];
    __syncthreads();
    for (int k = 0; k < blocks; ++k) {
        if (k > 0) mt_ring_block(ring, k);
        int w0 = -1, e0 = 0, lim = 0;                         // this thread's pair: words w0, w0 + 8 -> elements e0, e0 + 8 (< lim)
        if (tid < 312) {
            const int qq = 39 * k + (tid >> 3);
            if (qq < nq) { w0 = 16 * qq + (tid & 7); e0 = 16 * (q0 + qq) + (tid & 7); lim = clip; }
        } else if (tail) {
            const int end = tw + tlen;
            if (end > k * MT_N && end <= (k + 1) * MT_N) { w0 = tw + (tid - 312); e0 = tout + (tid - 312); lim = tout + tlen; }
        }
        if (w0 >= 0) {
            const uint32_t ra = ring[w0 % (2 * MT_N)], rb = ring[(w0 + 8) % (2 * MT_N)];
            const float ua = mt_uniform(ra), ub = mt_uniform(rb);
            float va, vb;
            if (UNIFORM) {
                va = ua; vb = ub;
            } else {
                // normal_fill_16: u1 = 1 - u[j], u2 = u[j + 8], radius sqrt(-2 log u1), theta = fl32(2 pi) u2
                const float r = sqrtf(-2.0f * logf(1.0f - ua));
                const float th = 6.28318548202514648f * ub;
                float s, co;
                sincosf(th, &s, &co);
                va = r * co; vb = r * s;
            }
            if (e0 < lim) o[e0] = va;
            if (e0 + 8 < lim) o[e0 + 8] = vb;
        }
        __syncthreads();
    }
}

// the three launches of a draw (work: prefix at 0, windows at MT_WINDOWS_AT); ev: NULL or four events recorded around them
template <bool UNIFORM>
static inline hipError_t mt19937_launch(float* out, int n, const uint32_t* state_in, int pos, int final_idx, uint32_t* state_out,
                                        const uint16_t* jump_idx, const int* jump_cnt, int jump_stride, const int* segs, int n_segs,
                                        uint32_t* work, hipEvent_t* ev, hipStream_t stream) {
    const size_t lds = (size_t)(MT_PREFIX + MT_N) * sizeof(uint32_t);
    // (83 KB of dynamic LDS: above the 64 KB a launch gets without asking; per device, so asked every time -- a host call)
    hipError_t e = hipFuncSetAttribute((const void*)mt19937_jump, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    if (ev) (void)hipEventRecord(ev[0], stream);
    hipLaunchKernelGGL(mt19937_prefix, dim3(1), dim3(MT_PREFIX_THREADS), 0, stream, state_in, pos, work);
    if (ev) (void)hipEventRecord(ev[1], stream);
    hipLaunchKernelGGL(mt19937_jump, dim3(n_segs + 1), dim3(MT_JUMP_THREADS), lds, stream, (const uint32_t*)work, jump_idx, jump_cnt,
                       jump_stride, work + MT_WINDOWS_AT);
    if (ev) (void)hipEventRecord(ev[2], stream);
    hipLaunchKernelGGL(mt19937_generate<UNIFORM>, dim3(n_segs + 1), dim3(MT_GEN_THREADS), 0, stream, out, n, segs, n_segs,
                       (const uint32_t*)(work + MT_WINDOWS_AT), state_in, final_idx, state_out);
    if (ev) (void)hipEventRecord(ev[3], stream);
    return hipGetLastError();
}

static inline const char* mt19937_bad_args(int n, int n_calls, int pos, int final_idx, int jump_stride, int n_segs) {
    if (n < 16) return "n must be >= 16 (the vectorised normal_() path)";
    if (n_calls < 1 || n_segs < n_calls || n_segs > n_calls * ((n >> 4) > 0 ? (n >> 4) : 1)) return "bad n_calls / n_segs";
    if (pos < 1 || pos > MT_N) return "pos must be in [1, 624]";
    if (final_idx < -1 || final_idx > MT_N) return "final_idx must be in [-1, 624]";
    if (jump_stride < 8 || (jump_stride & 7)) return "jump_stride must be a positive multiple of 8";
    return nullptr;
}
