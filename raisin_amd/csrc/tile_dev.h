// tile_dev.h -- what the kernels of the tiled batch classes share on the device ("the tiled classes' common shape"): a tile's
// own bytes out of its image, and the member's answer by the last of its tiles.  Every kernel keeps its own launch bounds and LDS.
#pragma once

#include "rsn_common.h"
#include "tile_layout.h"

namespace rsn {

// The bytes [lo, hi) of the member's output at dst, from the tile's image: img[0] is the output's byte `origin` (tile_layout.h:
// tile_store).  The whole workgroup of THREADS calls it, behind the barrier that ends the image's writes; img is 16-byte aligned.
template <int THREADS>
__device__ __forceinline__ void tile_store_out(uint8_t *dst, const uint8_t *img, uint32_t origin, uint32_t lo, uint32_t hi) {
    for (uint32_t u = threadIdx.x; origin + 16 * u < hi; u += THREADS) {
        const TileStore st = tile_store(origin, lo, hi, u);
        if (st.whole) *reinterpret_cast<uint4 *>(dst + st.lo) = reinterpret_cast<const uint4 *>(img)[u];
        else for (uint32_t x = st.lo; x < st.hi; x++) dst[x] = img[x - origin];
    }
}

// The end of a tile's workgroup, called by all of it: a fence behind every thread's stores, a barrier, and one more on the member's
// agent-scope counter *done (zeroed by an earlier launch), acquire-release.  True in thread 0 of the LAST of the member's `tiles` tiles
// to get here: every byte of the member is then in place, and the caller stores its status word(s), the last as an agent-scope release.
__device__ __forceinline__ bool tile_finish(uint32_t *done, uint32_t tiles) {
    __threadfence();
    __syncthreads();
    return threadIdx.x == 0 && __hip_atomic_fetch_add(done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) + 1 == tiles;
}

}  // namespace rsn
