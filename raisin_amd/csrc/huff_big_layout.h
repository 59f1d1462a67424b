// huff_big_layout.h -- the arithmetic of the big class of the Huffman compress batch (huff_big.hip) as plain code: no HIP
// include, so a CPU test (tests/huff_big_plan_test.cpp) holds it against naive loops.  A member above HUFF_MID_IN_MAX bytes does not fit a
// workgroup's LDS, so it is cut into TILES of BIGL_TILE input bytes, a workgroup each (the tiled classes' common shape):
//   scratch    BIG_SCR_WORDS words a member of the group (Slot::GD_BIG_TILES): the tiles' 128 counts, a "byte >= 0x80" flag a tile, the 128
//              code table entries, the tiles' first bits and four words of the member's own (verdict, stream length, tiles done);
//   bit offsets  a tile's code bits are sum(count * code length) over its own counts; tile t's first bit is the header, the pad in front
//              (huffman.go:245-255) and the bits of the tiles before it -- big_tile_offsets;
//   ownership  an output byte belongs to the tile in which its FIRST bit lies (big_tile_first_byte / big_tile_end_byte): tile t codes on
//              into tile t + 1's first symbols until its last byte is full (at most 7 symbols: a code has a bit at least), and does not
//              store the byte its own first bit lies in when that bit is not the byte's first.  No two tiles store the same byte.
#pragma once

#include <cstddef>
#include <cstdint>

#include "huff_plan_small.h"
#include "tile_layout.h"

namespace rsn {

// the class's limits: codecs.h names them HUFF_BIG_IN_MAX / HUFF_BIG_TILE
constexpr uint32_t BIGL_IN_MAX = 1u << 18;
constexpr uint32_t BIGL_TILE = 16384;
constexpr uint32_t BIGL_TILES_MAX = BIGL_IN_MAX / BIGL_TILE;
static_assert(BIGL_IN_MAX % BIGL_TILE == 0 && BIGL_TILE % 16 == 0, "whole tiles, whole 16-byte units");

RSN_HD_FN uint32_t big_tiles(uint32_t n) { return tile_count(n, BIGL_TILE); }
RSN_HD_FN uint32_t big_tile_len(uint32_t n, uint32_t t) { return tile_len(n, BIGL_TILE, t); }   // t < big_tiles(n)

// ---- the header's bound.  The entries are "<count>|<byte>" (the newline's byte takes two), at most 128 of them, and the counts sum to
// the member's length, so not all of them can be long: a count of d digits is at least 10^(d-1).  Start from a symbols of one digit (a
// count of 1 each); giving a symbol one more digit costs 9 * 10^(d-1) more input, the same for every symbol and more for every further
// digit, so the most digits n bytes can buy are bought cheapest first.  The bound is the largest over every alphabet size.
constexpr uint32_t big_hdr_digits(uint32_t n, uint32_t a) {                  // the most count digits of a symbols whose counts sum to at most n (n >= a)
    uint64_t left = n - a, digits = a;
    for (uint64_t step = 9; step <= left; step *= 10) {
        const uint64_t k = left / step < a ? left / step : a;                // symbols that get this digit
        digits += k; left -= k * step;
        if (k < a) break;                                                    // (a further digit is dearer still)
    }
    return (uint32_t)digits;
}
constexpr uint32_t big_hdr_bound(uint32_t n) {
    uint32_t best = 0;
    for (uint32_t a = 2; a <= PLAN_SYMS_MAX && a <= n; a++) {
        const uint32_t h = big_hdr_digits(n, a) + 2 * a + 1 + 3;             // digits, '|' and a byte each, the newline's second byte, "\\\n" and the pad byte
        best = h > best ? h : best;
    }
    return best;
}
constexpr uint32_t HUFF_BIG_HDR_MAX = big_hdr_bound(BIGL_IN_MAX);
static_assert(HUFF_BIG_HDR_MAX == 786, "256 KiB buy 14 counts of five digits and 114 of four: 526 digits, 128 x 2, the newline's byte and 3");

// the output slot of a member of n bytes: the header and at most 7 bits a byte (the flat 7-bit code is a prefix code of a byte alphabet,
// and Huffman's is no longer than any), in whole 16-byte units
constexpr uint32_t huff_big_enc_out_slot(uint32_t n) { return (HUFF_BIG_HDR_MAX + (7 * n + 7) / 8 + 15) & ~15u; }

// ---- a member's scratch, in words
constexpr uint32_t BIG_SCR_HIST = 0;                                         // [tile][128] counts
constexpr uint32_t BIG_SCR_FLAG = BIG_SCR_HIST + BIGL_TILES_MAX * 128;       // [tile] 1: the tile holds a byte >= 0x80
constexpr uint32_t BIG_SCR_TAB = BIG_SCR_FLAG + BIGL_TILES_MAX;              // [128] len << 24 | code, 0 for a byte that does not occur
constexpr uint32_t BIG_SCR_OFF = BIG_SCR_TAB + 128;                          // [tile] its first bit, counted from the output slot's first; [tiles]: the stream's end
constexpr uint32_t BIG_SCR_META = BIG_SCR_OFF + BIGL_TILES_MAX + 4;          // verdict (0: taken, else the hand-back), stream length, tiles done, -
constexpr uint32_t BIG_SCR_WORDS = BIG_SCR_META + 4;
static_assert(BIG_SCR_WORDS % 4 == 0, "a member's scratch is whole 16-byte units");
constexpr uint32_t BIG_META_VERDICT = 0, BIG_META_TOTAL = 1, BIG_META_DONE = 2;

// ---- what the plan refuses once the tree is built: a code beyond the 24 bits of the emit table's entry, a header beyond its bound, a
// stream beyond the member's output slot (none of the last two can occur for n <= BIGL_IN_MAX: the slot is sized by the two bounds)
RSN_HD_FN bool big_plan_refuses(uint32_t max_len, uint32_t hdr, uint32_t total, uint32_t slot) {
    return max_len > 24 || hdr > HUFF_BIG_HDR_MAX || total > slot;
}

// the code bits of a tile: hist[128] its counts, tab[128] the code table
RSN_HD_FN uint32_t big_tile_bits(const uint32_t *hist, const uint32_t *tab) {
    uint32_t bits = 0;
    for (uint32_t b = 0; b < PLAN_SYMS_MAX; b++) bits += hist[b] * (tab[b] >> 24);
    return bits;
}
// off[t] = base + the bits of the tiles before t, for t in [0, tiles]; base: 8 * header + the pad in front
RSN_HD_FN void big_tile_offsets(const uint32_t *tile_bits, uint32_t tiles, uint32_t base, uint32_t *off) {
    uint32_t at = base;
    for (uint32_t t = 0; t < tiles; t++) { off[t] = at; at += tile_bits[t]; }
    off[tiles] = at;
}
// the bytes tile t stores: [first, end) -- b0 / b1: its first bit and the next tile's.  Tile 0 starts behind the pad, inside the first
// payload byte, which is its own.  The tile's image begins at the unit b0 lies in: for t > 0 and b0 inside the LAST byte of a unit the
// tile's first byte is the next unit's, and unit 0 of the image stores nothing
RSN_HD_FN uint32_t big_tile_origin(uint32_t b0) { return tile_origin(b0 >> 3); }
RSN_HD_FN uint32_t big_tile_first_byte(uint32_t t, uint32_t b0) { return t == 0 ? b0 >> 3 : (b0 + 7) >> 3; }
RSN_HD_FN uint32_t big_tile_end_byte(uint32_t b1) { return (b1 + 7) >> 3; }

}  // namespace rsn
