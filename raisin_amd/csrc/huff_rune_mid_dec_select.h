// huff_rune_mid_dec_select.h -- the limits of the mid-size rune decoder (codecs.h: BehindClass; huff_rune_mid_dec.hip) and which members of
// `rest` it takes, as plain host code: no HIP include, so a CPU test (tests/huff_rune_mid_dec_plan_test.cpp) holds the rules -- the lengths,
// the promise's lower bound, the minimum, who leaves `rest`.  The three steps are huff_rune_select.h's (rune_dec_candidates / _planned /
// _leave) with this class's predicate and minimum, the same functions for the host form and the device form.
#pragma once

#include "huff_rune_mid_select.h"

namespace rsn {

// A stream whose header names a rune >= 0x80 and promises MORE than HUFF_RUNE_OUT_MAX bytes (up to there it is k_huff_batch_rune_dec's,
// whatever its payload) and at most HUFF_RUNE_MID_OUT_MAX, from at most 960 lanes of 576 bits of payload.  The lane width follows from
// the encoder: k_huff_mid_rune_enc bounds a member's payload by its n <= 65536 bytes, and 960 lanes of 544 bits fall short of that.
constexpr uint32_t HUFF_RUNE_MID_OUT_MAX = 65536;
constexpr uint32_t HUFF_RUNE_MID_DEC_LANES = 960, HUFF_RUNE_MID_DEC_S_MAX = 576;
constexpr uint32_t HUFF_RUNE_MID_PAY_MAX = HUFF_RUNE_MID_DEC_LANES * HUFF_RUNE_MID_DEC_S_MAX / 8;          // 69120
constexpr uint32_t HUFF_RUNE_MID_STREAM_MAX = HUFF_RUNE_HDR_MAX + 8 + HUFF_RUNE_MID_PAY_MAX;              // bytes of a stream the class takes
constexpr size_t HUFF_RUNE_MID_DEC_GROUP_MIN = 16;                         // (codecs.h says what was measured)
// A symbol takes a bit at least and a rune four bytes at most: fewer than 513 bytes of payload cannot DECODE to more than
// HUFF_RUNE_OUT_MAX bytes, whatever the header promises, and in front of the payload lie the separator and the pad byte at least.
// Shorter leftovers are no candidates: they do not count towards the minimum and cost no plan launch.  (One whose header promises more
// all the same would be an answer of fewer bytes here; it takes the single call, which gives the same bytes.)
constexpr uint32_t HUFF_RUNE_MID_DEC_PAY_MIN = HUFF_RUNE_OUT_MAX / 32 + 1;
static_assert(HUFF_RUNE_MID_OUT_MAX > HUFF_RUNE_OUT_MAX && HUFF_RUNE_MID_PAY_MAX >= HUFF_RUNE_MID_OUT_MAX &&
              (HUFF_RUNE_MID_DEC_LANES * (HUFF_RUNE_MID_DEC_S_MAX - 32)) / 8 < HUFF_RUNE_MID_OUT_MAX && HUFF_RUNE_MID_DEC_GROUP_MIN >= 16 &&
              (HUFF_RUNE_MID_DEC_PAY_MIN - 1) * 8 * 4 == HUFF_RUNE_OUT_MAX,
              "above the 16 KiB class; the lanes hold 8 bits a decoded byte and one word less a lane would not; smaller calls keep their launches");

// may this stream's length be a candidate's at all?
inline bool rune_mid_dec_len_may(size_t n) { return n >= HUFF_RUNE_MID_DEC_PAY_MIN + 3 && n <= HUFF_RUNE_MID_STREAM_MAX; }
// a summary (of the parse at the mid limits) the class takes: planned, the payload at a 4-byte boundary inside the stream, a promise above
// the 16 KiB class's and within what a workgroup holds
inline bool rune_mid_dec_summary_ok(const HuffDevSummary &v, size_t n) {
    return v.verdict == PARSE_PLANNED && !(v.A0 & 3u) && v.A0 <= n && v.expect > HUFF_RUNE_OUT_MAX && v.expect <= HUFF_RUNE_MID_OUT_MAX && (v.span + 7) / 8 <= HUFF_RUNE_MID_PAY_MAX;
}
// the members of `rest` that may be planned (may(i): in the device form, refused by the byte decoders' plan; len(i): the stream's length),
// sorted; none when there are fewer than the minimum
template <class May, class Len>
std::vector<size_t> rune_mid_dec_candidates(const std::vector<size_t> &rest, May may, Len len) {
    return rune_dec_candidates(rest, [&](size_t i) { return rune_mid_dec_len_may(len(i)) && may(i); }, HUFF_RUNE_MID_DEC_GROUP_MIN);
}
// of the first k candidates those whose summary the class takes, in order: idx, and what each one's header promises
template <class Len>
void rune_mid_dec_planned(const std::vector<size_t> &cand, size_t k, const HuffDevSummary *sums, Len len, std::vector<size_t> &idx, std::vector<uint32_t> &expect) {
    rune_dec_planned(cand, k, sums, len, idx, expect, rune_mid_dec_summary_ok);
}
// still the minimum of them: they leave `rest`, and true; fewer: none is taken, idx is emptied, `rest` is as it was
inline bool rune_mid_dec_leave(std::vector<size_t> &rest, std::vector<size_t> &idx) { return rune_dec_leave(rest, idx, HUFF_RUNE_MID_DEC_GROUP_MIN); }

}  // namespace rsn
