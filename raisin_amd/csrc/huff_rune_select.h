// huff_rune_select.h -- which members the two classes behind the rows take (codecs.h: BehindClass; huff_rune.hip, huff_rune_dec.hip), as
// plain host code: no HIP include, so a CPU test (tests/rune_select_test.cpp) holds the rules -- the order, the minimums, who joins `rest`.
#pragma once

#include <algorithm>
#include <iterator>
#include <vector>

#include "group_layout.h"
#include "huff_parse_small.h"

namespace rsn {

constexpr uint32_t HUFF_RUNE_IN_MAX = 16384;                              // (codecs.h says what these are and how they were measured)
constexpr size_t HUFF_RUNE_GROUP_MIN = 16, HUFF_RUNE_DEC_GROUP_MIN = 16;

// ---- the rune encoder.  The members the Huffman byte encoders handed back as GROUP_BACK_RUNES, sorted: those the class takes move to the
// front of `runes` and their number is returned, when there are at least its minimum of them; the others -- all of them when there are
// fewer -- join `rest`, and go where they went before there was such a class.  len(i): member i's length.
template <class Len>
size_t rune_class_members(std::vector<size_t> &runes, std::vector<size_t> &rest, Len len) {
    std::sort(runes.begin(), runes.end());
    auto mid = std::stable_partition(runes.begin(), runes.end(), [&](size_t i) { return len(i) >= 2 && len(i) <= HUFF_RUNE_IN_MAX; });
    if ((size_t)(mid - runes.begin()) < HUFF_RUNE_GROUP_MIN) mid = runes.begin();
    rest.insert(rest.end(), mid, runes.end());
    return (size_t)(mid - runes.begin());
}
// ---- the rune decoder, in three steps with the planning between the first two.  The members of `rest` that may be planned at all
// (may(i): short enough, and in the device form refused by the byte decoders' plan), sorted; none when there are fewer than the minimum.
// (The minimum and the summaries' predicate are arguments for the mid-size class, huff_rune_mid_dec_select.h; the defaults are this class's.)
template <class May>
std::vector<size_t> rune_dec_candidates(const std::vector<size_t> &rest, May may, size_t group_min = HUFF_RUNE_DEC_GROUP_MIN) {
    std::vector<size_t> cand;
    for (size_t i : rest) if (may(i)) cand.push_back(i);
    if (cand.size() < group_min) cand.clear();
    std::sort(cand.begin(), cand.end());
    return cand;
}
// a summary the class takes: planned, the payload at a 4-byte boundary inside the stream, within what a workgroup holds
inline bool rune_dec_summary_ok(const HuffDevSummary &v, size_t n) {
    return v.verdict == PARSE_PLANNED && !(v.A0 & 3u) && v.A0 <= n && v.expect >= 1 && v.expect <= HUFF_RUNE_OUT_MAX && (v.span + 7) / 8 <= HUFF_RUNE_PAY_MAX;
}
// of the first k candidates those whose summary the class takes, in order: idx, and what each one's header promises
template <class Len>
void rune_dec_planned(const std::vector<size_t> &cand, size_t k, const HuffDevSummary *sums, Len len, std::vector<size_t> &idx, std::vector<uint32_t> &expect,
                      bool (*ok)(const HuffDevSummary &, size_t) = rune_dec_summary_ok) {
    for (size_t q = 0; q < k; q++) if (ok(sums[q], len(cand[q]))) { idx.push_back(cand[q]); expect.push_back(sums[q].expect); }
}
// still the minimum of them (idx sorted): they leave `rest`, which is sorted afterwards, and true; fewer: none is taken, idx is emptied
inline bool rune_dec_leave(std::vector<size_t> &rest, std::vector<size_t> &idx, size_t group_min = HUFF_RUNE_DEC_GROUP_MIN) {
    if (idx.size() < group_min) { idx.clear(); return false; }
    std::vector<size_t> others;
    std::sort(rest.begin(), rest.end());
    std::set_difference(rest.begin(), rest.end(), idx.begin(), idx.end(), std::back_inserter(others));
    rest.swap(others);
    return true;
}

}  // namespace rsn
