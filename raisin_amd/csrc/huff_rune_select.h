// huff_rune_select.h -- which members the 16 KiB rune encoder and the two rune decoders behind the rows take (codecs.h: BehindClass;
// huff_rune.hip, huff_rune_dec_body.h), as plain host code: no HIP include, so CPU tests (tests/rune_select_test.cpp,
// tests/huff_rune_mid_dec_plan_test.cpp) hold the rules -- the order, the minimums, who joins and who leaves `rest`.
#pragma once

#include <algorithm>
#include <iterator>
#include <vector>

#include "group_layout.h"
#include "huff_parse_small.h"

namespace rsn {

constexpr uint32_t HUFF_RUNE_IN_MAX = 16384;                              // (codecs.h says what these are and how they were measured)
constexpr size_t HUFF_RUNE_GROUP_MIN = 16;

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
// ---- the rune decoders, in three steps with the planning between the first two, for the class L (huff_parse_rune.h: ParseRuneSmall,
// ParseRuneMid -- its limits, its length rule, the least it may be promised, its minimum); the same functions for the host form and the
// device form of both classes.  The members of `rest` that may be planned at all (len(i): the stream's length; may(i): in the device form,
// refused by the byte decoders' plan), sorted; none when there are fewer than the minimum.
template <class L, class May, class Len>
std::vector<size_t> rune_dec_candidates(const std::vector<size_t> &rest, May may, Len len) {
    std::vector<size_t> cand;
    for (size_t i : rest) if (L::len_may(len(i)) && may(i)) cand.push_back(i);
    if (cand.size() < L::GROUP_MIN) cand.clear();
    std::sort(cand.begin(), cand.end());
    return cand;
}
// a summary (of the parse at L's limits) the class takes: planned, the payload at a 4-byte boundary inside the stream, a promise in the
// class's range and a payload within what a workgroup holds
template <class L>
bool rune_dec_summary_ok(const HuffDevSummary &v, size_t n) {
    return v.verdict == PARSE_PLANNED && !(v.A0 & 3u) && v.A0 <= n && v.expect >= L::OUT_MIN && v.expect <= L::OUT_MAX && (v.span + 7) / 8 <= L::PAY_MAX;
}
// of the first k candidates those whose summary the class takes, in order: idx, and what each one's header promises
template <class L, class Len>
void rune_dec_planned(const std::vector<size_t> &cand, size_t k, const HuffDevSummary *sums, Len len, std::vector<size_t> &idx, std::vector<uint32_t> &expect) {
    for (size_t q = 0; q < k; q++) if (rune_dec_summary_ok<L>(sums[q], len(cand[q]))) { idx.push_back(cand[q]); expect.push_back(sums[q].expect); }
}
// still the minimum of them (idx sorted): they leave `rest`, which is sorted afterwards, and true; fewer: none is taken, idx is emptied,
// `rest` is as it was
template <class L>
bool rune_dec_leave(std::vector<size_t> &rest, std::vector<size_t> &idx) {
    if (idx.size() < L::GROUP_MIN) { idx.clear(); return false; }
    std::vector<size_t> others;
    std::sort(rest.begin(), rest.end());
    std::set_difference(rest.begin(), rest.end(), idx.begin(), idx.end(), std::back_inserter(others));
    rest.swap(others);
    return true;
}

}  // namespace rsn
