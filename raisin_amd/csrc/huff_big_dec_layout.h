// huff_big_dec_layout.h -- the arithmetic of the tiled class of the Huffman decompress batch (huff_big_dec.hip) as plain code:
// no HIP include, so a CPU test (tests/huff_big_dec_plan_test.cpp) holds it against naive loops and runs the three phases as a model.
// A stream that promises more than HUFF_MID_OUT_MAX bytes does not fit a workgroup's LDS (huff_mid.hip).  It is one bit string without an
// index, so it is cut in the PAYLOAD:
//   tiles      a tile is BIGD_LANES lanes of BIGD_S code bits, counted from the stream's first code bit: BIGD_TILE_BITS bits, 7680 bytes of
//              payload, a workgroup (the tiled classes' common shape).  A stream of `span` code bits has bigd_lanes(span)
//              lanes and bigd_tiles(span) tiles, the last one shorter;
//   scratch    BIGD_SCR_WORDS words a member of the group (Slot::GD_BIG_DEC): per tile its 32-entry map -- "entered at bit c of the tile,
//              the codewords that start in it number n and the last one ends at bit c' of the next tile": c' << 24 | n, BIGD_OFF_BAD for
//              c' where the path is lost or runs off the payload -- then per tile its true entry, its first output byte and its symbols,
//              and four words of the member's own (verdict, decoded length, tiles done);
//   chain      bigd_chain composes the maps from the stream's first code bit (tile 0 is entered at its bit 0) and gives every verdict a
//              one-workgroup decoder gives: a lost tile, an exit that is none, a stream that ends inside a codeword, more symbols than the
//              header promises, a tile of more symbols than the emit kernel's image holds (BIGD_OUT_CAP);
//   ownership  tile t stores exactly the output bytes [base_t, base_t + count_t): no byte twice, none left out.
#pragma once

#include <cstddef>
#include <cstdint>

#include "huff_plan_small.h"

namespace rsn {

// the class's limits: codecs.h names the first two HUFF_BIG_OUT_MAX / HUFF_BIG_PAY_MAX
constexpr uint32_t BIGD_OUT_MAX = 262144;                                    // decoded bytes of a member at most
constexpr uint32_t BIGD_PAY_MAX = 229376;                                    // payload bytes of a member at most: 7/8 of BIGD_OUT_MAX
constexpr uint32_t BIGD_LANES = 960;                                         // lanes of a tile: 15 wavefronts (the sixteenth answers the first lane's entries)
constexpr uint32_t BIGD_S = 64;                                              // code bits of a lane
constexpr uint32_t BIGD_TILE_BITS = BIGD_LANES * BIGD_S;                     // 61440: 7680 bytes of payload
constexpr uint32_t BIGD_TILES_MAX = (8 * BIGD_PAY_MAX + BIGD_TILE_BITS - 1) / BIGD_TILE_BITS;
constexpr uint32_t BIGD_OUT_CAP = 32768;                                     // bytes of the emit kernel's output image (with the 16 of the alignment shift)
constexpr uint32_t BIGD_OFF_BAD = 0xFF;                                      // OFF_BAD (huff_small_body.h)
static_assert(BIGD_TILES_MAX == 30 && BIGD_S % 32 == 0 && BIGD_S >= 64, "whole words a lane, 64 bits at least: an exit lies within 32 bits of the next lane's first");
static_assert(8ull * BIGD_PAY_MAX == 7ull * BIGD_OUT_MAX, "a byte alphabet codes in at most 7 bits a byte");

RSN_HD_FN uint32_t bigd_lanes(uint32_t span) { return (span + BIGD_S - 1) / BIGD_S; }
RSN_HD_FN uint32_t bigd_tiles(uint32_t span) { return (bigd_lanes(span) + BIGD_LANES - 1) / BIGD_LANES; }
// what parse_lanes (huff_parse_small.h) is asked for the class: BIGD_TILES_MAX tiles' lanes of at most BIGD_S bits -- it answers S = BIGD_S
// for every span the class takes, so a tile's bits do not depend on the stream
constexpr uint32_t BIGD_LANES_ALL = BIGD_TILES_MAX * BIGD_LANES;
static_assert((8ull * BIGD_PAY_MAX + BIGD_LANES_ALL - 1) / BIGD_LANES_ALL <= BIGD_S, "the largest payload in lanes of BIGD_S bits");

// ---- a member's scratch, in words
constexpr uint32_t BIGD_SCR_MAP = 0;                                         // [tile][32] exit << 24 | symbols
constexpr uint32_t BIGD_SCR_TILE = BIGD_SCR_MAP + BIGD_TILES_MAX * 32;       // [tile][4] true entry, first output byte, symbols, -
constexpr uint32_t BIGD_SCR_META = BIGD_SCR_TILE + BIGD_TILES_MAX * 4;       // verdict (0: taken, else handed back), decoded bytes, tiles done, -
constexpr uint32_t BIGD_SCR_WORDS = BIGD_SCR_META + 4;
static_assert(BIGD_SCR_WORDS % 4 == 0, "a member's scratch is whole 16-byte units");
constexpr uint32_t BIGD_META_VERDICT = 0, BIGD_META_TOTAL = 1, BIGD_META_DONE = 2;
constexpr uint32_t BIGD_TILE_ENTRY = 0, BIGD_TILE_BASE = 1, BIGD_TILE_COUNT = 2;

// The maps of a member's `tiles` tiles composed in order.  maps[t * 32 + c]: tile t's answer for entry c.  rec[t * 4 ..): tile t's true
// entry, first output byte and symbols.  out_max: the bytes the header promises (the output slot holds them).  Returns true with *total =
// the decoded bytes, or false: the member is handed back.  Bounded by the tiles.
RSN_HD_FN bool bigd_chain(const uint32_t *maps, uint32_t tiles, uint32_t out_max, uint32_t *rec, uint32_t *total) {
    uint32_t c = 0, base = 0;
    if (tiles == 0 || tiles > BIGD_TILES_MAX) return false;
    for (uint32_t t = 0; t < tiles; t++) {
        const uint32_t e = maps[t * 32 + c], exit_off = e >> 24, n = e & 0xFFFFFFu;
        if (exit_off >= 32) return false;                                    // lost (more than four phases, the rounds), off the payload, or no entry at all
        if (n + 16 > BIGD_OUT_CAP) return false;                             // more symbols than the emit image holds
        if (n > out_max - base) return false;                                // more symbols than the header promises (base <= out_max)
        rec[t * 4 + BIGD_TILE_ENTRY] = c; rec[t * 4 + BIGD_TILE_BASE] = base; rec[t * 4 + BIGD_TILE_COUNT] = n; rec[t * 4 + 3] = 0;
        base += n; c = exit_off;
    }
    if (c != 0) return false;                                                // the stream ends inside a codeword
    *total = base;
    return true;
}

}  // namespace rsn
