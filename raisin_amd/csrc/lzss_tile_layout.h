// lzss_tile_layout.h -- the arithmetic of the tiled class of the LZSS compress batch (lzss_tile.hip) as plain code: no HIP
// include, so a CPU test (tests/lzss_tile_layout_test.cpp) holds it against a serial restatement.  A member above LZSS_MID_IN_MAX bytes does
// not fit a workgroup's LDS, so its ESCAPED stream (EncodeOpeningSymbols, lzss.go:369-389) is cut into TILES of LZT_TILE positions, a
// workgroup each for the search and for the bytes (the tiled classes' common shape):
//   e_cap      the escaped bytes a member of n bytes may have and still be taken: at most LZT_E_MAX, and at most n + n / 2 -- a member of
//              which more than half escapes to two is handed back, so a member's scratch stays below 8 bytes a byte of input;
//   scratch    Slot::GD_LZSS_TILES: in front lzt_front_words(g) words, member m's offset into the slot; then per member lzt_scr_words(n)
//              words: eight of its own (verdict, E, length, tiles done, give-up), the tiles' first output bytes, a key a position
//              (L << 16 | distance; bit 31: the greedy chain lands here) and the escaped stream with LZT_FC_PAD zeros behind it;
//   ownership  tile t's items are the chain positions inside it; their bytes are [off[t], off[t + 1]) of the member's stream.
#pragma once

#include <cstddef>
#include <cstdint>

#include "group_layout.h"
#include "tile_layout.h"

namespace rsn {

// the class's limits: codecs.h names them LZSS_TILE_IN_MAX / LZSS_TILE_E_MAX / LZSS_TILE_POS
constexpr uint32_t LZT_IN_MIN = 65536;                        // the class begins above it: the mid class's largest member (codecs.h asserts it)
#ifndef RSN_LZSS_TILE_IN_MAX                                  // (a probe build widens the class: codecs.h)
#define RSN_LZSS_TILE_IN_MAX 262144
#endif
constexpr uint32_t LZT_IN_MAX = RSN_LZSS_TILE_IN_MAX;
constexpr uint32_t LZT_E_MAX = LZT_IN_MAX + LZT_IN_MAX / 16;
constexpr uint32_t LZT_TILE = 2048;
constexpr uint32_t LZT_W_MAX = 4096;                          // the largest window
constexpr uint32_t LZT_FC_PAD = 64;                           // zeros behind the escaped stream
constexpr uint32_t LZT_TILES_MAX = (LZT_E_MAX + LZT_TILE - 1) / LZT_TILE;
constexpr uint32_t LZT_KEY_ON = 0x80000000u;                  // a key's mark: the greedy chain lands on this position
static_assert(LZT_E_MAX % 16 == 0 && LZT_TILE % 16 == 0, "whole 16-byte units");

// what the class takes: by the length and the window alone, so one function serves the host form and the device form
RSN_HD_FN bool lzt_takes(size_t n, long long window) { return n > LZT_IN_MIN && n <= LZT_IN_MAX && window >= 1 && window <= (long long)LZT_W_MAX; }
RSN_HD_FN uint32_t lzt_tiles(uint32_t e) { return tile_count(e, LZT_TILE); }
RSN_HD_FN uint32_t lzt_tile_len(uint32_t e, uint32_t t) { return tile_len(e, LZT_TILE, t); }   // t < lzt_tiles(e)
// the escaped bytes a member of n bytes is taken with (n beyond the class counts as the class's largest: the kernels size by this)
RSN_HD_FN constexpr uint32_t lzt_e_cap(uint32_t n) {
    const uint32_t m = n < LZT_IN_MAX ? n : LZT_IN_MAX, half = m + m / 2;
    return half < LZT_E_MAX ? half : LZT_E_MAX;
}
// the first escaped position a tile's workgroup holds: the window in front of the tile, rounded down to a sub-tile of `sub` positions
// (a power of two that divides LZT_TILE), never before the member's position 0
RSN_HD_FN uint32_t lzt_window_lo(uint32_t t0, uint32_t window, uint32_t sub) { return (t0 - (t0 < window ? t0 : window)) & ~(sub - 1); }

// ---- a member's slots: the input is group_layout.h's lzss_in_slot; an item is never longer than what it stands for, so the stream has
// at most E bytes -- in whole units
constexpr size_t lzt_in_slot(size_t n) { return lzss_in_slot(n); }
RSN_HD_FN uint32_t lzt_out_slot(uint32_t n) { return ((lzt_e_cap(n) + 15) & ~15u) + 16; }

// ---- a member's scratch, in words from the member's offset
constexpr uint32_t LZT_META_VERDICT = 0, LZT_META_E = 1, LZT_META_TOTAL = 2, LZT_META_DONE = 3, LZT_META_GIVEUP = 4;
constexpr uint32_t LZT_SCR_META = 0;                                         // eight words
constexpr uint32_t LZT_SCR_OFF = 8;                                          // [tile] its first output byte; [tiles]: the stream's length
RSN_HD_FN uint32_t lzt_scr_keys(uint32_t n) { return LZT_SCR_OFF + ((lzt_tiles(lzt_e_cap(n)) + 1 + 3) & ~3u); }
RSN_HD_FN uint32_t lzt_scr_fc(uint32_t n) { return lzt_scr_keys(n) + ((lzt_e_cap(n) + 3) & ~3u); }
RSN_HD_FN uint32_t lzt_scr_words(uint32_t n) { return lzt_scr_fc(n) + ((lzt_e_cap(n) + LZT_FC_PAD + 15) & ~15u) / 4; }
// the table in front of a group's scratch: member m's offset in words (0: the member has none and is handed back)
RSN_HD_FN uint32_t lzt_front_words(uint32_t g) { return (g + 3) & ~3u; }

// ---- which tile stores which byte: tile_layout.h's rule, the image at the unit the tile's first output byte off0 lies in
using LztStore = TileStore;
RSN_HD_FN uint32_t lzt_image_first(uint32_t off0) { return tile_origin(off0); }
RSN_HD_FN LztStore lzt_tile_store(uint32_t off0, uint32_t off1, uint32_t u) { return tile_store(tile_origin(off0), off0, off1, u); }

}  // namespace rsn
