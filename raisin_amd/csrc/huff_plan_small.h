// huff_plan_small.h -- the Go-exact tree, codes and header of a small BYTE alphabet, as code that compiles for the host and the device.
// k_huff_batch_enc (huff_small.hip) runs it in one wavefront per member; tests/test_huff_plan_host.py compiles it with huff_host.cpp and
// checks it against build_tree / assign_codes / emit_header.  The alphabet: 2 to 128 bytes below 0x80, every count below 2^16 (so that
// a count and its node id pack into one word, and every sum of counts stays below 2^24).
//   leaves   (count asc, byte asc): plan_leaf_rank                                              huffman.go:64-87 (sort_leaves)
//   tree     Go container/heap, Less = count strictly less; pop, pop, push until one is left:
//            plan_tree over a heap store and a children store                                 huffman.go:93-102 (GoHeap)
//   codes    one pass over the internal nodes in descending id order, '0' to the left: plan_codes  assign_codes(..., want_dfs = false)
//   header   ascending by byte, '\\' first when it would be last; "<count>|<byte>", newline as "\n": plan_entry / plan_header
//                                                                                                 huffman.go:312-318 (emit_header)
// The heap and the children are reached through a store (get / set of slot i): an array on the host, VGPRs read and written a lane at a
// time on the device (huff_small_body.h: LaneStore, wave_tree) -- every index is wave-uniform, so a sift level is a few scalar-indexed lane accesses instead of a
// dependent LDS round trip.
#pragma once

#include <cstdint>

#include "tile_layout.h"   // (RSN_HD_FN: the one qualifier of plain code that the kernels call too)

namespace rsn {

constexpr uint32_t PLAN_SYMS_MAX = 128;           // byte alphabet (every symbol < 0x80; runes take the general path)
constexpr uint32_t PLAN_NODES_MAX = 2 * PLAN_SYMS_MAX - 1;
constexpr uint32_t PLAN_COUNT_LIMIT = 1u << 16;   // every count below this
// ... but for the big class of the compress batch (huff_big.hip), whose members' counts sum to less than PLAN_COUNT_LIMIT_WIDE: the tree and
// the codes below only ask that a sum of counts and a node id pack into one word -- plan_item<8>, sum << 8 < 2^32.  The parsers
// (huff_parse_small.h) and the decoders keep PLAN_COUNT_LIMIT.
constexpr uint32_t PLAN_COUNT_LIMIT_WIDE = 1u << 24;
// How deep a code can be: a code of d bits needs counts that sum to at least fib(d + 2), Fibonacci counts being the worst case.  The classes
// state their depth with it, each at its own member size (huff_mid.hip, huff_big.hip, huff_rune_mid.hip).
constexpr unsigned long long plan_fib(int k) { unsigned long long a = 0, b = 1; for (int i = 0; i < k; i++) { const unsigned long long t = a + b; a = b; b = t; } return a; }

// A heap item / a node's code: one word each.
//   item   count << IDB | node id         (sums of counts < 2^23, ids < 255)
//   code   len << 24 | code (low 24 bits)  (k_small_emit's table entry; only meaningful while len <= 24)
// IDB: bits of a node id -- 8 for this alphabet; 9 for the rune alphabet of up to 256 leaves (huff_plan_rune.h: ids reach 510), which
// shares the tree and the codes below.
template <uint32_t IDB = 8> RSN_HD_FN uint32_t plan_item(uint32_t count, uint32_t id) { return count << IDB | id; }
template <uint32_t IDB = 8> RSN_HD_FN uint32_t plan_count(uint32_t item) { return item >> IDB; }

// position of byte b among the present bytes in (count asc, byte asc) order; cnt[128], cnt[b] > 0
RSN_HD_FN uint32_t plan_leaf_rank(const uint32_t *cnt, uint32_t b) {
    const uint32_t f = cnt[b];
    uint32_t r = 0;
    for (uint32_t c = 0; c < PLAN_SYMS_MAX; c++) {
        const uint32_t g = cnt[c];
        r += (uint32_t)(g != 0 && (g < f || (g == f && c < b)));
    }
    return r;
}

// The Go heap over heap slots [0, a), filled with plan_item<IDB>(count of leaf i, i) for the leaves in rank order (ascending: a heap already,
// so heap.Init moves nothing, huffman.go:93).  Internal node a + k gets kids.set(k, left | right << IDB).  Returns the root's id.
// Pop and push carry the moving item and shift the others past it: heap.go's swaps give the same final layout.
template <uint32_t IDB = 8, class Heap, class Kids>
RSN_HD_FN uint32_t plan_tree(uint32_t a, Heap &h, Kids &kids) {
    constexpr uint32_t IDM = (1u << IDB) - 1;
    uint32_t n = a, next = a;
    auto pop = [&]() -> uint32_t {                                    // heap.Pop: swap(0, n-1), down(0, n-1), take the last
        const uint32_t m = n - 1, top = h.get(0), x = h.get(m), fx = plan_count<IDB>(x);
        n = m;
        uint32_t i = 0;
        for (;;) {
            const uint32_t l = 2 * i + 1;
            if (l >= m) break;
            uint32_t j = l, hj = h.get(l);
            if (l + 1 < m) { const uint32_t hr = h.get(l + 1); if (plan_count<IDB>(hr) < plan_count<IDB>(hj)) { j = l + 1; hj = hr; } }
            if (!(plan_count<IDB>(hj) < fx)) break;
            h.set(i, hj);
            i = j;
        }
        h.set(i, x);
        return top;
    };
    while (n > 1) {                                                   // huffman.go:96-101
        const uint32_t x = pop(), y = pop();
        const uint32_t f = plan_count<IDB>(x) + plan_count<IDB>(y), it = plan_item<IDB>(f, next);
        kids.set(next - a, (x & IDM) | (y & IDM) << IDB);
        uint32_t j = n++;                                             // heap.Push: up(n)
        for (;;) {
            const uint32_t i = j ? (j - 1) / 2 : 0;
            if (i == j) break;
            const uint32_t hi = h.get(i);
            if (!(f < plan_count<IDB>(hi))) break;
            h.set(j, hi);
            j = i;
        }
        h.set(j, it);
        next++;
    }
    return next - 1;                                                  // huffman.go:102: the last node made is the one left
}

// Codes of every node [0, 2a - 1), parents before children: code.set(id, len << 24 | code).  Slots must start at 0 (the root's code).
template <uint32_t IDB = 8, class Kids, class Codes>
RSN_HD_FN void plan_codes(uint32_t a, uint32_t root, const Kids &kids, Codes &code) {
    for (uint32_t id = root + 1; id-- > a;) {
        const uint32_t p = code.get(id), l = (p >> 24) + 1, base = (p << 1) & 0xFFFFFEu;
        const uint32_t k = kids.get(id - a);
        code.set(k & ((1u << IDB) - 1), l << 24 | base);
        code.set(k >> IDB, l << 24 | base | 1u);
    }
}

// one header entry: strconv.Itoa(count) '|' byte, newline as "\n" (huffman.go:314-316)
RSN_HD_FN uint32_t plan_entry_len(uint32_t count, uint32_t b) {
    uint32_t d = 1;
    for (uint32_t v = count; v >= 10; v /= 10) d++;
    return d + 1 + (b == 10 ? 2u : 1u);
}
RSN_HD_FN uint32_t plan_entry(uint32_t count, uint32_t b, uint8_t *out) {
    const uint32_t len = plan_entry_len(count, b);
    uint32_t at = len - (b == 10 ? 3u : 2u);
    for (uint32_t v = count;;) { out[--at] = (uint8_t)('0' + v % 10); v /= 10; if (!v) break; }
    at = len - (b == 10 ? 3u : 2u);
    out[at++] = '|';
    if (b == 10) { out[at++] = '\\'; out[at] = 'n'; }
    else out[at] = (uint8_t)b;
    return len;
}
// '\\' as the LAST entry makes the reference decoder index past the header (huffman.go:210): it goes first instead
RSN_HD_FN bool plan_backslash_first(const uint32_t *cnt) {
    uint32_t hi = 0, a = 0;
    for (uint32_t b = 0; b < PLAN_SYMS_MAX; b++) if (cnt[b]) { hi = b; a++; }
    return a > 1 && hi == 0x5C;
}
// The whole header, serially: the entries, "\\\n" and the pad byte (huffman.go:245-255,312-318).  Returns its length.
RSN_HD_FN uint32_t plan_header(const uint32_t *cnt, uint32_t total_bits, uint8_t *out) {
    uint32_t at = 0;
    const bool bs = plan_backslash_first(cnt);
    if (bs) at += plan_entry(cnt[0x5C], 0x5C, out + at);
    for (uint32_t b = 0; b < PLAN_SYMS_MAX; b++) if (cnt[b] && !(bs && b == 0x5C)) at += plan_entry(cnt[b], b, out + at);
    out[at++] = '\\'; out[at++] = '\n';
    out[at++] = (uint8_t)((8 - total_bits % 8) % 8);
    return at;
}

}  // namespace rsn
