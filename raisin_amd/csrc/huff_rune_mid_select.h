// huff_rune_mid_select.h -- which members the mid-size rune encoder takes (codecs.h: BehindClass; huff_rune_mid.hip), and the sizes of its
// slots, as plain host code: no HIP include, so a CPU test (tests/rune_mid_select_test.cpp) holds the rules -- the lengths, the minimum,
// who stays in the pool.
#pragma once

#include "huff_rune_select.h"

namespace rsn {

constexpr uint32_t HUFF_RUNE_MID_IN_MAX = 65536;                          // (codecs.h says what these are and what was measured)
constexpr size_t HUFF_RUNE_MID_GROUP_MIN = 16;
static_assert(HUFF_RUNE_MID_IN_MAX > HUFF_RUNE_IN_MAX && HUFF_RUNE_MID_GROUP_MIN >= 16, "above the 16 KiB class; smaller calls keep their launches");

// The longest stream of a member of n bytes: at most 256 entries of 5 digits, '|' and 4 bytes, "\\\n" and the pad byte; an alphabet of at
// most 256 symbols has the flat 8-bit code as a prefix code and Huffman's is no longer, a rune is a byte at least: n bytes of payload.
// The output slot: the longest header, the payload in whole words, the image's slack, in 16-byte units.
constexpr uint32_t huff_rune_mid_stream_max(uint32_t n) { return (n < 256 ? n : 256u) * 10 + 3 + n; }
constexpr uint32_t huff_rune_mid_enc_out_slot(uint32_t n) { return (HUFF_RUNE_HDR_MAX + n + 64 + 15) & ~15u; }

// The RUNES pool as the rows left it, offered to this class BEFORE the 16 KiB class: the pool is sorted; the members of more than
// HUFF_RUNE_IN_MAX and at most HUFF_RUNE_MID_IN_MAX bytes leave it and are returned, in index order, when there are at least the minimum
// of them.  Every other member -- all of them when there are fewer -- STAYS in the pool, sorted, for rune_class_members, which sends what
// it does not keep to `rest`: where such a member went before there was this class.  len(i): member i's length.
template <class Len>
std::vector<size_t> rune_mid_class_members(std::vector<size_t> &runes, Len len) {
    std::sort(runes.begin(), runes.end());
    const auto mine = [&](size_t i) { return len(i) > HUFF_RUNE_IN_MAX && len(i) <= HUFF_RUNE_MID_IN_MAX; };
    std::vector<size_t> idx;
    if ((size_t)std::count_if(runes.begin(), runes.end(), mine) < HUFF_RUNE_MID_GROUP_MIN) return idx;
    const auto mid = std::stable_partition(runes.begin(), runes.end(), [&](size_t i) { return !mine(i); });
    idx.assign(mid, runes.end());
    runes.erase(mid, runes.end());
    return idx;
}

}  // namespace rsn
