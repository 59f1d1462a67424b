// tile_layout.h -- the arithmetic the tiled batch classes share ("the tiled classes' common shape") as plain code: no HIP
// include, so the CPU tests of the classes' layout headers compile it (tests/lzss_tile_layout_test.cpp sweeps tile_store).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define RSN_HD_FN __host__ __device__ __forceinline__
#else
#define RSN_HD_FN inline
#endif

namespace rsn {

// `bytes` in tiles of `tile`, the last one shorter
RSN_HD_FN uint32_t tile_count(uint32_t bytes, uint32_t tile) { return (bytes + tile - 1) / tile; }
RSN_HD_FN uint32_t tile_len(uint32_t bytes, uint32_t tile, uint32_t t) { return bytes - t * tile < tile ? bytes - t * tile : tile; }   // t < tile_count(bytes, tile)

// ---- which tile stores which byte.  A tile owns the bytes [lo, hi) of its member's output, and its image begins at `origin`, a 16-byte
// unit's first byte at or before lo.  Unit u of the image -- the output's bytes [origin + 16u, origin + 16u + 16) -- goes out as one
// 16-byte store when it lies inside [lo, hi); of a unit shared with a neighbour only the bytes inside the range go out, one by one.
RSN_HD_FN uint32_t tile_origin(uint32_t off) { return off & ~15u; }
struct TileStore { uint32_t lo, hi; bool whole; };                            // the bytes [lo, hi) of the output; whole: as one 16-byte store
RSN_HD_FN TileStore tile_store(uint32_t origin, uint32_t lo, uint32_t hi, uint32_t u) {
    const uint32_t x0 = origin + 16 * u, x1 = x0 + 16;
    TileStore s;
    s.lo = x0 > lo ? x0 : lo;
    s.hi = x1 < hi ? x1 : hi;
    if (s.hi < s.lo) s.hi = s.lo;
    s.whole = x0 >= lo && x1 <= hi;
    return s;
}

}  // namespace rsn
