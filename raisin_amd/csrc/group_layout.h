// group_layout.h -- the arithmetic of a group of batch members in pinned staging, as plain host code: no HIP include, so a CPU
// test (tests/group_layout_test.cpp) checks what keeps a grouped kernel inside its buffers -- slots that do not overlap, zero padding
// behind every input, 16-byte aligned offsets.  group_run.h's run_groups and run_groups_staged (the same groups on device staging) are the users.
//
// Staging of a group of g members: a table of g entries of E bytes (E a multiple of 16), then per member its input slot (the member's
// bytes, zeros behind them), its output slot and 16 bytes of status.  Input and output slots are whole 16-byte units.
#pragma once

#include <cstddef>
#include <cstdint>

namespace rsn {

// a member's status word until its workgroup answers / the answer "not mine": the member goes back to the caller's single call.  Every
// other value is the length of the result.  GROUP_BACK_RUNES is a hand-back too, with its reason: the Huffman byte encoders answer it
// where the only obstacle was a byte >= 0x80, and the batch flows offer such members to the rune encoder (huff_rune.hip) first.
constexpr uint32_t GROUP_PENDING = 0xFFFFFFFFu, GROUP_BACK = 0xFFFFFFFEu, GROUP_BACK_RUNES = 0xFFFFFFFDu;
constexpr bool group_is_back(uint32_t v) { return v == GROUP_BACK || v == GROUP_BACK_RUNES; }
constexpr size_t GROUP_STATUS_BYTES = 16;

constexpr size_t group_round16(size_t v) { return (v + 15) & ~(size_t)15; }
// staging one member adds to its group
constexpr size_t group_need(size_t entry_bytes, size_t in_bytes, size_t out_bytes) { return entry_bytes + in_bytes + out_bytes + GROUP_STATUS_BYTES; }

// The group that starts at member lo of count: at most max_members members; the first always enters, a further one only while the group's
// bytes stay within max_bytes (a member larger than that is a group of its own).  need(k): the staging of member k.
struct GroupCut { size_t hi, bytes; };   // the group is [lo, hi)
template <class Need>
GroupCut next_group(size_t lo, size_t count, size_t max_members, size_t max_bytes, Need need) {
    size_t k = lo, bytes = 0;
    while (k < count && k - lo < max_members) {
        const size_t b = need(k);
        if (k != lo && bytes + b > max_bytes) break;
        bytes += b; k++;
    }
    return {k, bytes};
}

// Hands out the offsets of a group's members in order; end(): the group's bytes so far -- after the last member the sum of group_need.
struct MemberSlots { uint32_t in, out, status; };
class GroupLayout {
    size_t at_;
public:
    GroupLayout(size_t members, size_t entry_bytes) : at_(group_round16(members * entry_bytes)) {}
    MemberSlots member(size_t in_bytes, size_t out_bytes) {
        MemberSlots m{};
        m.in = (uint32_t)at_; at_ += in_bytes;
        m.out = (uint32_t)at_; at_ += out_bytes;
        m.status = (uint32_t)at_; at_ += GROUP_STATUS_BYTES;
        return m;
    }
    size_t end() const { return at_; }
};

// ---- the slots of the four classes.  An input slot leaves behind the member's n bytes the zeros its kernel's loads rely on: 32 bytes for
// the LZSS kernels, 16 for the Huffman encoders, 64 for the Huffman decoders.
constexpr size_t lzss_in_slot(size_t n) { return group_round16(n) + 32; }
// e_max: the escaped bytes the class's kernel holds (an input escapes to at most twice its length)
constexpr size_t lzss_enc_out_slot(size_t n, size_t e_max) { return group_round16(2 * n < e_max ? 2 * n : e_max) + 16; }
constexpr size_t lzss_dec_out_slot(size_t e_max) { return e_max + 16; }               // whatever the stream's length
constexpr size_t huff_enc_in_slot(size_t n) { return group_round16(n) + 16; }
constexpr uint32_t HUFF_HDR_MAX = 1100;         // 128 entries of at most 5 digits + '|' + 2 bytes, + "\\\n" + pad
constexpr uint32_t huff_small_enc_out_slot(uint32_t n) { return (HUFF_HDR_MAX + n + 15) & ~15u; }                    // holds header + 7n/8 + pad
constexpr uint32_t huff_mid_enc_out_slot(uint32_t n) { return (HUFF_HDR_MAX + (7 * n + 7) / 8 + 3 + 15) & ~15u; }    // header + payload in whole words
// the rune encoders (huff_rune_body.h): at most 256 entries of 5 digits + '|' + 4 bytes of UTF-8, + "\\\n" + pad -- a header maximum of its
// own, the decoders and huff_parse_small.h keep HUFF_HDR_MAX; fewer than 9 bits a rune (a Huffman code's average is below the entropy + 1,
// and 256 symbols have at most 8 bits of it) and at most a rune a byte.  huff_rune_stream_max(n): the longest stream of a member of n bytes.
constexpr uint32_t HUFF_RUNE_HDR_MAX = 256 * (5 + 1 + 4) + 3;
constexpr uint32_t huff_rune_stream_max(uint32_t n) { return (n < 256 ? n : 256u) * 10 + 3 + (9 * n + 7) / 8; }
constexpr uint32_t huff_rune_enc_out_slot(uint32_t n) { return (HUFF_RUNE_HDR_MAX + (9 * n + 7) / 8 + 64 + 15) & ~15u; }   // header + payload in whole words, and the image's slack
// the rune decoders (huff_rune_dec_body.h; their limits: huff_parse_rune.h, which states HUFF_RUNE_OUT_MAX, _PAY_MAX and _STREAM_MAX -- nine
// bits a decoded byte, what the encoder's bound above writes at most).  A member's input slot is the whole stream (the workgroup reads the
// header itself), huff_dec_in_slot of its length; its output slot huff_dec_out_slot of what the header promises.
constexpr size_t huff_dec_in_slot(size_t sn) { return group_round16(sn) + 64; }       // sn: the stream from the 4-byte boundary the kernel reads from
constexpr size_t huff_dec_out_slot(size_t expect) { return group_round16(expect) + 16; }   // expect: the bytes the header promises

// ---- a RUN of host members through a class's device form (group_run.h: run_members_staged; tests/run_layout_test.cpp) is two
// blocks.  The input block goes up in one copy: a table of g entries of T bytes (T = 0: none; the tiled decoder's plans otherwise), then
// every member's input slot.  The output block holds every member's output slot; slots are whole 16-byte units, T a multiple of 16.
// run_need: what one member adds to its run (next_group's need: runs are cut as groups are)
constexpr size_t run_need(size_t table_entry, size_t in_bytes, size_t out_bytes) { return table_entry + in_bytes + out_bytes; }
struct RunSlots { size_t in, out; };   // a member's offsets, handed out in order: into the input block (behind the table) / the output block
class RunLayout {
    size_t in_, out_ = 0;
public:
    RunLayout(size_t members, size_t table_entry) : in_(members * table_entry) {}
    RunSlots member(size_t in_bytes, size_t out_bytes) { const RunSlots m{in_, out_}; in_ += in_bytes; out_ += out_bytes; return m; }
    size_t in_total() const { return in_; }      // the table and the input slots so far: what goes up
    size_t out_total() const { return out_; }
};
// the bytes of the output block that come down, in one copy: up to the end of the last member a kernel answered (out_at[q]: its slot;
// answers[q]: a length, not a hand-back), 0 when every member was handed back
template <class Answers, class OutAt>
size_t run_down(size_t g, const Answers &answers, const OutAt &out_at) {
    size_t down = 0;
    for (size_t q = 0; q < g; q++) if (!group_is_back(answers[q])) down = out_at[q] + answers[q];
    return down;
}

}  // namespace rsn
