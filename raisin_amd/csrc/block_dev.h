// block_dev.h -- what a workgroup of any codec's batch kernels ends and scans with (the LZSS units through lzss_enc_body.h and
// lzss_dec_body.h, the Huffman units through huff_small_body.h): its last store, the word the host polls, and the exclusive scan of a value
// a thread.
#pragma once

#include "rsn_common.h"

namespace rsn {

#ifdef __HIPCC__
// A block's last act: its stores to host memory made visible, then ONE word the host is polling (the host does not wait for the stream: a
// hipStreamSynchronize is 5-10 us of wake-up, the kernel is as long).
__device__ __forceinline__ void block_done(uint32_t *flag, uint32_t value) {
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(flag, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// exclusive scan of one value per thread over a workgroup of T threads; *total: the sum
template <int T>
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t *s_wave /*[T / 64 + 1]*/, uint32_t *total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d, 64); if (lane >= (uint32_t)d) inc += o; }
    __syncthreads();                                                      // (the previous scan's readers are done with s_wave)
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    if (threadIdx.x < 64) {
        uint32_t w = threadIdx.x < T / 64 ? s_wave[threadIdx.x] : 0u, wi = w;
#pragma unroll
        for (int d = 1; d < T / 64; d <<= 1) { const uint32_t o = __shfl_up(wi, d, 64); if (lane >= (uint32_t)d) wi += o; }
        if (threadIdx.x < T / 64) s_wave[threadIdx.x] = wi - w;
        if (threadIdx.x == T / 64 - 1) s_wave[T / 64] = wi;
    }
    __syncthreads();
    *total = s_wave[T / 64];
    return s_wave[wave] + inc - v;
}
#endif

}  // namespace rsn
