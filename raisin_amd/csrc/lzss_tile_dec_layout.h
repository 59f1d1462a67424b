// lzss_tile_dec_layout.h -- the arithmetic of the tiled class of the LZSS decompress batch (lzss_tile_dec.hip) as plain code:
// no HIP include, so a CPU test (tests/lzss_tile_dec_layout_test.cpp) holds it against a serial restatement.  A stream of more than
// LZSS_MID_E_MAX bytes, or one that expands to more, does not fit a workgroup's LDS, so the STREAM is cut into tiles of LZTD_TILE bytes
// for the parse and the escaped OUTPUT into tiles of LZTD_TILE bytes for the copies:
//   tiles      lztd_tiles(n) of the stream, lztd_tiles(E) of the output, the last one shorter; a token's text may reach LZTD_REACH bytes
//              into the next stream tile, and the parse of a tile looks as far back to find the bytes a token of the tile before covers;
//   scratch    Slot::GD_LZSS_TILE_DEC: LZTD_SCR_WORDS words a member, the q-th member of a group at q * LZTD_SCR_WORDS -- what a stream
//              expands to is not known before it is parsed, so every member has the scratch of the largest: eight words of its own
//              (verdict, E), per stream tile its output bytes, its malformed flag, its pointers' need and its first output byte, per
//              output tile the stream tile and the offset inside that tile's output where it begins, the escaped image (a byte a
//              position) and a descriptor a position (the earlier position it copies, LZTD_NONE: none).  LZTD_SCR_PER_STAGING times a
//              member's staging holds it, whatever the member: lzss_tile_dec.hip sizes the slot by that;
//   ownership  output tile t's bytes unescape to [off0, off1) of the result (the tiled classes' common shape).
#pragma once

#include <cstddef>
#include <cstdint>

#include "lzss_tile_layout.h"

namespace rsn {

// the class's limits: codecs.h names them LZSS_TILE_DEC_IN_MAX / LZSS_TILE_DEC_OUT_MAX
constexpr uint32_t LZTD_IN_MIN = 2048;                        // candidates are longer than the small decoder's cutoff
constexpr uint32_t LZTD_IN_MAX = LZT_E_MAX;                   // bytes of stream
constexpr uint32_t LZTD_OUT_MAX = LZT_E_MAX;                  // escaped bytes a stream may expand to
constexpr uint32_t LZTD_TILE = LZT_TILE;
constexpr uint32_t LZTD_TOKEN_TEXT = 23;                      // '<' ten digits ',' ten digits '>'
constexpr uint32_t LZTD_REACH = LZTD_TOKEN_TEXT - 1;          // bytes of a token's text behind its '<'
constexpr uint32_t LZTD_HALO = 32;                            // bytes of stream a tile's workgroup holds in front of and behind the tile
constexpr uint32_t LZTD_NONE = 0xFFFFFFFFu;
constexpr uint32_t LZTD_IN_TILES_MAX = (LZTD_IN_MAX + LZTD_TILE - 1) / LZTD_TILE, LZTD_OUT_TILES_MAX = (LZTD_OUT_MAX + LZTD_TILE - 1) / LZTD_TILE;
constexpr uint32_t LZTD_IMG_PAD = 64;
static_assert(LZTD_REACH <= LZTD_HALO && LZTD_HALO % 16 == 0 && LZTD_TILE % 16 == 0 && LZTD_OUT_MAX % 16 == 0, "whole 16-byte units");
// the sum of the tiles' output counts, each clamped to LZTD_OUT_MAX + 1, is a word
static_assert((unsigned long long)LZTD_IN_TILES_MAX * (LZTD_OUT_MAX + 1ull) < (1ull << 32), "the scan of the tiles' outputs does not overflow");

RSN_HD_FN bool lztd_candidate(size_t n) { return n > LZTD_IN_MIN && n <= LZTD_IN_MAX; }
RSN_HD_FN uint32_t lztd_tiles(uint32_t bytes) { return tile_count(bytes, LZTD_TILE); }
RSN_HD_FN uint32_t lztd_tile_len(uint32_t bytes, uint32_t t) { return tile_len(bytes, LZTD_TILE, t); }   // t < lztd_tiles(bytes)

// ---- a member's slots (group_layout.h's): the input of its stream, the output the class's largest whatever the stream
constexpr size_t lztd_in_slot(size_t n) { return lzss_in_slot(n); }
constexpr size_t lztd_out_slot() { return lzss_dec_out_slot(LZTD_OUT_MAX); }

// ---- a member's scratch, in words from the member's offset; every region begins at a multiple of four words
constexpr uint32_t lztd_round4(uint32_t w) { return (w + 3) & ~3u; }
constexpr uint32_t LZTD_META_VERDICT = 0, LZTD_META_E = 1;
constexpr uint32_t LZTD_SCR_META = 0;                                                             // eight words
constexpr uint32_t LZTD_SCR_CNT = 8;                                                              // [stream tile] its output bytes, at most LZTD_OUT_MAX + 1
constexpr uint32_t LZTD_SCR_FLAG = LZTD_SCR_CNT + lztd_round4(LZTD_IN_TILES_MAX);                 // [stream tile] non-zero: malformed
constexpr uint32_t LZTD_SCR_NEED = LZTD_SCR_FLAG + lztd_round4(LZTD_IN_TILES_MAX);                // [stream tile] the most a pointer reaches in front of the tile's first output byte
constexpr uint32_t LZTD_SCR_FIRST = LZTD_SCR_NEED + lztd_round4(LZTD_IN_TILES_MAX);               // [stream tile] its first output byte; [tiles]: E
constexpr uint32_t LZTD_SCR_OT_TILE = LZTD_SCR_FIRST + lztd_round4(LZTD_IN_TILES_MAX + 1);        // [output tile] the stream tile its first byte comes from
constexpr uint32_t LZTD_SCR_OT_OFF = LZTD_SCR_OT_TILE + lztd_round4(LZTD_OUT_TILES_MAX);          // [output tile] ... and which of that tile's output bytes it is
constexpr uint32_t LZTD_SCR_IMG = LZTD_SCR_OT_OFF + lztd_round4(LZTD_OUT_TILES_MAX);              // bytes: the escaped image
constexpr uint32_t LZTD_SCR_DESC = LZTD_SCR_IMG + (LZTD_OUT_MAX + LZTD_IMG_PAD) / 4;              // [position] the earlier position it copies
constexpr uint32_t LZTD_SCR_WORDS = LZTD_SCR_DESC + lztd_round4(LZTD_OUT_MAX);
constexpr uint32_t LZTD_SCR_PER_STAGING = 5;                  // a member's scratch is at most this many times its two slots
static_assert((unsigned long long)LZTD_SCR_WORDS * 4 <= (unsigned long long)LZTD_SCR_PER_STAGING * (lztd_in_slot(LZTD_IN_MIN + 1) + lztd_out_slot()), "the multiple that sizes the slot");
RSN_HD_FN unsigned long long lztd_scr_at(uint32_t q) { return (unsigned long long)q * LZTD_SCR_WORDS; }

// the output tile that holds the output byte `at`, and where stream tile t's output lies, from the tiles' first bytes: the plan launch
// gives output tile o the LAST stream tile whose first byte is at or before the tile's (stream tiles that put out nothing share their
// first byte with the next one that does)
RSN_HD_FN uint32_t lztd_entry_tile(const uint32_t *first, uint32_t tiles, uint32_t at) {   // first[0 .. tiles]: ascending, first[tiles] = E > at
    uint32_t lo = 0, hi = tiles;                                                 // the last t with first[t] <= at
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) / 2; if (first[mid] <= at) lo = mid; else hi = mid; }
    return lo;
}

}  // namespace rsn
