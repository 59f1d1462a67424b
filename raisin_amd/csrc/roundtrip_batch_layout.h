// roundtrip_batch_layout.h -- the arithmetic of the batch round trip (rsn.h: rsn_layers_roundtrip_batch, rsn_layers_roundtrip_batch_dev;
// DESIGN 4.12), as plain host code: no HIP include, so a CPU test (tests/roundtrip_batch_layout_test.cpp) checks it -- the tiles of a
// member cover the longer of its two buffers exactly once, the verify table and the stats block lie apart at 16-byte offsets, the counters'
// 32-bit limit, and a run need that grows with both lengths.  rsn_api.hip's suite_batch_flow is the user (the round trip is its
// one-list form), roundtrip_batch.hip's k_members_verify reads the table and writes the stats.
//
// A run of m members ends in ONE launch over a table of tiles: an entry per 64 KiB of max(original, decompressed) of every member.  The
// launch writes the run's stats block: a first-difference word per member and, when the caller asked for them, 512 counters per member.
#pragma once

#include <cstddef>
#include <cstdint>

#include "layers_batch_layout.h"

namespace rsn {

// k_members_verify's unit of work: a workgroup a tile
constexpr size_t RB_TILE = 65536;
// One entry of the verify table.  orig / dec: the member's two buffers (16-byte aligned device pointers), n_o / n_d their lengths; the
// entry is tile `tile` of member `member` (the run's numbering): the bytes [tile * RB_TILE, min((tile + 1) * RB_TILE, max(n_o, n_d))).
struct RbEntry { const uint8_t *orig, *dec; uint32_t n_o, n_d, member, tile; };
static_assert(sizeof(RbEntry) == 32, "the verify table: two 16-byte units an entry");
// what a member has in the stats block: the word (0: no differing byte below min(n_o, n_d); otherwise the COMPLEMENT of the lowest such
// offset, so that a block of zeros is the initial state and a larger word the earlier difference) ...
constexpr size_t RB_WORD = 8;
// ... and, when histograms were asked for, 256 counters of the original's bytes followed by 256 of the decompressed bytes
constexpr size_t RB_HIST_WORDS = 512, RB_HIST_BYTES = RB_HIST_WORDS * sizeof(uint32_t);

// the counters are 32 bits and the table's lengths too: a buffer of 2^32 bytes or more is not this call's
constexpr bool rb_fits(uint64_t len) { return len <= (uint64_t)UINT32_MAX; }
// the tiles of a member: none for an empty one that came back empty
constexpr size_t rb_tiles(size_t n_o, size_t n_d) { return ((n_o > n_d ? n_o : n_d) + RB_TILE - 1) / RB_TILE; }
// the bytes of tile t of a member
constexpr size_t rb_tile_lo(size_t t) { return t * RB_TILE; }
constexpr size_t rb_tile_hi(size_t n_o, size_t n_d, size_t t) {
    const size_t top = n_o > n_d ? n_o : n_d;
    return (t + 1) * RB_TILE < top ? (t + 1) * RB_TILE : top;
}

// The verify slot of a run of m members with `tiles` table entries: the table, then the stats block (words, then histograms), each at a
// 16-byte offset.  The stats block [words, bytes) is what one memset clears in front of the launch and what comes down behind it.
struct RbLayout { size_t table, words, hists, bytes; };   // offsets of the three regions, and the slot's size; hists == bytes without histograms
constexpr RbLayout rb_layout(size_t tiles, size_t m, bool hists) {
    const size_t words = lb_round16(tiles * sizeof(RbEntry)), h = words + lb_round16(m * RB_WORD);
    return RbLayout{0, words, h, h + (hists ? m * RB_HIST_BYTES : 0)};
}
constexpr size_t rb_stats_bytes(const RbLayout &l) { return l.bytes - l.words; }

// what a member holds at once in a run: its staged input (the host form; 0 when it lies in the caller's memory), a slot in each arena of
// the larger of its two passes' largest slots, its table entries and its part of the stats block
constexpr size_t rb_member_need(size_t staged_len, size_t enc_slot, size_t dec_slot, size_t n_o, size_t n_d, bool hists) {
    return lb_member_need(staged_len, enc_slot > dec_slot ? enc_slot : dec_slot) + rb_tiles(n_o, n_d) * sizeof(RbEntry) + RB_WORD + (hists ? RB_HIST_BYTES : 0);
}

}  // namespace rsn
