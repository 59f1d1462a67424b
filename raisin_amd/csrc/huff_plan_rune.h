// huff_plan_rune.h -- the Go-exact leaf order, tree, codes and header of a small RUNE alphabet, as code that compiles for the host and the
// device.  huff_rune_enc_body (huff_rune_body.h: k_huff_batch_rune_enc's and k_huff_mid_rune_enc's body) runs it per member; tests/test_huff_rune_plan_host.py compiles it with huff_host.cpp and
// checks it against build_tree / assign_codes / emit_header.  The alphabet: 2 to 256 distinct runes in no particular order (the kernel's
// come out of a hash table), every count at most 16384.
//   leaves   (count asc, rune asc) and the header's order (rune asc): plan_rune_ranks                huffman.go:64-87 (sort_leaves)
//   tree     huff_plan_small.h's plan_tree with 9 bits of node id: 256 leaves make 255 internal nodes, ids reach 510; a heap item is
//            count << 9 | id, and counts that sum to at most 16384 keep every sum far below 2^23      huffman.go:93-102 (GoHeap)
//   codes    huff_plan_small.h's plan_codes, the same way
//   header   ascending by rune, "<count>|<rune in UTF-8>", U+000A as "\n", U+FFFD as EF BF BD: plan_rune_entry
//                                                                                                   huffman.go:312-318 (emit_header)
// emit_header moves '\\' to the front when it would be the LAST entry.  That cannot happen here: a member of this class holds a rune
// >= 0x80 (an invalid byte is U+FFFD), and that rune sorts behind 0x5C.  So the rule is not implemented; the kernel hands a member
// without such a rune back, and tests/huff_rune_plan_test.cpp asserts it of every alphabet it builds.
#pragma once

#include "huff_plan_small.h"

namespace rsn {

constexpr uint32_t PLAN_RUNE_SYMS_MAX = 256;
constexpr uint32_t PLAN_RUNE_IDB = 9;                                  // bits of a node id
constexpr uint32_t PLAN_RUNE_NODES_MAX = 2 * PLAN_RUNE_SYMS_MAX - 1;
constexpr uint32_t PLAN_RUNE_COUNT_MAX = 16384;                        // a count, and the sum of all, at most
static_assert(PLAN_RUNE_NODES_MAX <= (1u << PLAN_RUNE_IDB) && ((unsigned long long)PLAN_RUNE_COUNT_MAX << PLAN_RUNE_IDB) < (1ull << 32), "a heap item is one word");
// ... but for the mid-size class (huff_rune_mid.hip), whose members' counts sum to at most PLAN_RUNE_MID_COUNT_MAX: ranks, tree and codes
// only ask that a sum of counts and a node id pack into one word, and a count of 65536 still has five digits, as the header's bound has it
// (tests/huff_rune_mid_plan_test.cpp).  The parser (huff_parse_rune.h) keeps PLAN_RUNE_COUNT_MAX at its default limits, the 16 KiB
// decoder's, and takes counts up to this one at the mid-size decoder's (ParseRuneMid; huff_rune_mid_dec.hip).
constexpr uint32_t PLAN_RUNE_MID_COUNT_MAX = 65536;
static_assert(PLAN_RUNE_MID_COUNT_MAX < (1u << 23) && ((unsigned long long)PLAN_RUNE_MID_COUNT_MAX << PLAN_RUNE_IDB) < (1ull << 32) && PLAN_RUNE_MID_COUNT_MAX < 100000,
              "every sum of counts stays below 2^23: a heap item count << 9 | id is one word; five digits a count");
constexpr uint32_t PLAN_RUNE_SLOTS =2 * PLAN_RUNE_SYMS_MAX;           // of the encoder's and the decoder's open-addressing table: twice the symbols it may hold
static_assert(PLAN_RUNE_SLOTS == 1u << 9, "plan_rune_hash gives 9 bits");

// a rune's first slot in a table of PLAN_RUNE_SLOTS slots: the ONE hash of the encoder's counts (huff_rune_body.h) and the decoder's entries
// (huff_parse_rune.h); tests/huff_rune_parse_test.cpp prints it (`slots`)
RSN_HD_FN uint32_t plan_rune_hash(uint32_t r) { return (r * 0x9E3779B1u) >> 23; }   // 9 bits

// symbol t of the a symbols (rune[], cnt[]): its position in (count asc, rune asc) order and in rune order
RSN_HD_FN void plan_rune_ranks(const uint32_t *rune, const uint32_t *cnt, uint32_t a, uint32_t t, uint32_t *leaf_rank, uint32_t *rune_rank) {
    const uint32_t r = rune[t], f = cnt[t];
    uint32_t lr = 0, rr = 0;
    for (uint32_t j = 0; j < a; j++) {
        const uint32_t g = cnt[j], q = rune[j];
        lr += (uint32_t)(g < f || (g == f && q < r));
        rr += (uint32_t)(q < r);
    }
    *leaf_rank = lr; *rune_rank = rr;
}

// bytes of string(rune) for a rune Go's decoding yields (never a surrogate, never beyond U+10FFFF)
RSN_HD_FN uint32_t plan_rune_utf8_len(uint32_t r) { return r < 0x80 ? 1u : r < 0x800 ? 2u : r < 0x10000 ? 3u : 4u; }
// one header entry: strconv.Itoa(count) '|' string(rune), newline as "\n" (huffman.go:314-316)
RSN_HD_FN uint32_t plan_rune_entry_len(uint32_t count, uint32_t r) {
    uint32_t d = 1;
    for (uint32_t v = count; v >= 10; v /= 10) d++;
    return d + 1 + (r == 10 ? 2u : plan_rune_utf8_len(r));
}
RSN_HD_FN uint32_t plan_rune_entry(uint32_t count, uint32_t r, uint8_t *out) {
    uint32_t d = 1;
    for (uint32_t v = count; v >= 10; v /= 10) d++;
    uint32_t at = d;
    for (uint32_t v = count;;) { out[--at] = (uint8_t)('0' + v % 10); v /= 10; if (!v) break; }
    at = d;
    out[at++] = '|';
    if (r == 10) { out[at++] = '\\'; out[at++] = 'n'; }
    else if (r < 0x80) out[at++] = (uint8_t)r;
    else if (r < 0x800) { out[at++] = (uint8_t)(0xC0 | r >> 6); out[at++] = (uint8_t)(0x80 | (r & 0x3F)); }
    else if (r < 0x10000) { out[at++] = (uint8_t)(0xE0 | r >> 12); out[at++] = (uint8_t)(0x80 | ((r >> 6) & 0x3F)); out[at++] = (uint8_t)(0x80 | (r & 0x3F)); }
    else { out[at++] = (uint8_t)(0xF0 | r >> 18); out[at++] = (uint8_t)(0x80 | ((r >> 12) & 0x3F)); out[at++] = (uint8_t)(0x80 | ((r >> 6) & 0x3F)); out[at++] = (uint8_t)(0x80 | (r & 0x3F)); }
    return at;
}

}  // namespace rsn
