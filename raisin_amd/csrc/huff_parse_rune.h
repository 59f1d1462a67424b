// huff_parse_rune.h -- the grouped rune decoder's plan of a stream whose header names a RUNE >= 0x80, as code that compiles for the host and
// the device: huff_parse_small.h's counterpart for the alphabets k_huff_batch_rune_enc (huff_rune.hip) writes.  k_huff_batch_rune_dec
// (huff_rune_dec.hip) makes the whole plan per member, k_huff_dev_rune_plan and the host's classifier the part in front of the tree (the
// "light scan"); tests/test_huff_rune_parse_host.py compiles it with huff_host.cpp and holds it against parse_header, build_tree and
// assign_codes.
//   separator  the first 5C 0A among the first PARSE_RUNE_SCAN_MAX bytes; sep + 4 <= n                      huffman.go:261
//   header     decodeTree's scan (huffman.go:196-227; parse_header, huff_host.cpp): digits accumulate a count, every other byte that is
//              not '|' is ignored; at '|' the entry's count is what has accumulated ("" counts 0), its symbol the rune that starts at the
//              next byte by Go's decoding (huff_utf8.h's seq_len rule, restated for both sides: parse_rune_decode) -- an invalid byte, a
//              surrogate or an over-long form is U+FFFD of width 1, and the header ends at the separator: a sequence it cuts is U+FFFD
//              too.  "\n" written as '\\' 'n' is U+000A and skips two bytes, everything else skips ONE byte whatever the rune's width
//              (huffman.go:222: the rune's continuation bytes are scanned as ordinary bytes, and ignored as such); a later entry for a
//              rune replaces an earlier one, an invalid byte and a literal EF BF BD are the same rune; any order
//   table      the entries go into an open-addressing table of PARSE_RUNE_SLOTS slots, the encoder's hash (parse_rune_put): one lane
//              scans, so no atomics
//   refused    (the answer "not mine": the member takes the single call, which decodes it or words its error) a header that ends behind
//              '|' or behind "|\\"; fewer than 2 or more than PARSE_RUNE_SYMS_MAX distinct runes; no rune >= 0x80 (the byte classes'
//              stream); a count above PARSE_RUNE_COUNT_MAX; expect = the sum of count * utf8_len(rune) of 0 or above PARSE_RUNE_OUT_MAX;
//              a pad byte that leaves no code bit; more code bits than the class's lanes hold; a deepest code of 0 bits or more than 32
//   tree       leaves by plan_rune_ranks over count + 1 (a count of 0 is a leaf like any other, build_tree), plan_tree<PLAN_RUNE_IDB>,
//              plan_codes<PLAN_RUNE_IDB> for the depths; child[2 * node + bit] = 0x8000 | leaf rank, or the internal node; leaf_rune[rank]
// expect is in BYTES: what the stream decodes to once every rune is written as string(rune).  Every loop is bounded by the bytes looked
// at, by the table's slots or by the 510 nodes.
// The limits named above are the 16 KiB class's, ParseRuneSmall, the default of every function's template argument L; the mid-size
// decoder (huff_rune_mid_dec.hip) runs the same text at ParseRuneMid's (below).
#pragma once

#include "group_layout.h"
#include "huff_parse_small.h"
#include "huff_plan_rune.h"

namespace rsn {

constexpr uint32_t PARSE_RUNE_HDR_MAX = HUFF_RUNE_HDR_MAX;                 // the longest header the rune encoders write (group_layout.h)
constexpr uint32_t PARSE_RUNE_SCAN_MAX = PARSE_RUNE_HDR_MAX + 8;           // bytes of a stream the separator is looked for in
constexpr uint32_t PARSE_RUNE_OUT_MAX = 16384;                             // decoded bytes
constexpr uint32_t PARSE_RUNE_LANES = 256, PARSE_RUNE_S_MAX = 576;         // the class's lanes: subsequences, bits of one at most
constexpr uint32_t PARSE_RUNE_PAY_MAX = PARSE_RUNE_LANES * PARSE_RUNE_S_MAX / 8;   // 9 bits a byte of output
constexpr uint32_t PARSE_RUNE_STREAM_MAX = PARSE_RUNE_SCAN_MAX + PARSE_RUNE_PAY_MAX;   // bytes of a stream the class takes
constexpr uint32_t PARSE_RUNE_SYMS_MAX = PLAN_RUNE_SYMS_MAX;
constexpr uint32_t PARSE_RUNE_COUNT_MAX = PLAN_RUNE_COUNT_MAX;
constexpr uint32_t PARSE_RUNE_CHILD_MAX = 2 * (PARSE_RUNE_SYMS_MAX - 1);   // entries of child[]
constexpr uint32_t PARSE_RUNE_SLOTS = PLAN_RUNE_SLOTS, PARSE_RUNE_EMPTY = 0xFFFFFFFFu; // the table: twice the symbols it may hold; (no rune)
constexpr uint32_t PARSE_RUNE_ERROR = 0xFFFD;                              // kRuneError (huff_host.h)
static_assert(PARSE_RUNE_PAY_MAX == 9 * PARSE_RUNE_OUT_MAX / 8 && PARSE_RUNE_OUT_MAX <= PARSE_RUNE_COUNT_MAX, "nine bits a decoded byte; a sum of counts is a count");
// ---- a class's limits as a template argument: what differs between the classes that run this parse, each limit stated HERE and nowhere
// else -- every other name for one (HUFF_RUNE_*, below) is an alias.  ParseRuneSmall -- the default everywhere below -- is the constants
// above, k_huff_batch_rune_dec's (huff_rune_dec.hip); ParseRuneMid is k_huff_mid_rune_dec's (huff_rune_mid_dec.hip): 960 lanes of 576 bits
// (k_huff_mid_rune_enc bounds a member's payload by its n <= 65536 bytes, and 960 lanes of 544 bits fall short of that), a promise of at
// most 65536 bytes, counts up to PLAN_RUNE_MID_COUNT_MAX.  The header, the table, the alphabet and the tree are the same for both.
// Beside the parse's limits a class states which members of a call it takes (huff_rune_select.h: the three steps that read these):
//   len_may    may a stream of this length be a candidate at all?
//   OUT_MIN    the least a taken stream's header promises: the range [OUT_MIN, OUT_MAX] is the class's, whatever the payload
//   GROUP_MIN  a call holds that many candidates, and as many planned ones, or the class takes none (codecs.h says what was measured)
struct ParseRuneSmall {
    static constexpr uint32_t OUT_MAX = PARSE_RUNE_OUT_MAX, LANES = PARSE_RUNE_LANES, S_MAX = PARSE_RUNE_S_MAX, PAY_MAX = PARSE_RUNE_PAY_MAX;
    static constexpr uint32_t STREAM_MAX = PARSE_RUNE_STREAM_MAX, COUNT_MAX = PARSE_RUNE_COUNT_MAX;
    static constexpr uint32_t OUT_MIN = 1;
    static constexpr size_t GROUP_MIN = 16;
    static constexpr bool len_may(size_t n) { return n <= STREAM_MAX; }
};
struct ParseRuneMid {
    static constexpr uint32_t OUT_MAX = 65536, LANES = 960, S_MAX = 576, PAY_MAX = LANES * S_MAX / 8;
    static constexpr uint32_t STREAM_MAX = PARSE_RUNE_SCAN_MAX + PAY_MAX, COUNT_MAX = PLAN_RUNE_MID_COUNT_MAX;
    static constexpr uint32_t OUT_MIN = ParseRuneSmall::OUT_MAX + 1;       // (up to there a stream is k_huff_batch_rune_dec's)
    static constexpr size_t GROUP_MIN = 16;
    // A symbol takes a bit at least and a rune four bytes at most: fewer than 513 bytes of payload cannot DECODE to OUT_MIN bytes, whatever
    // the header promises, and in front of the payload lie the separator and the pad byte at least.  Shorter leftovers are no candidates:
    // they do not count towards the minimum and cost no plan launch.  (One whose header promises more all the same would be an answer of
    // fewer bytes here; it takes the single call, which gives the same bytes.)
    static constexpr uint32_t PAY_MIN = ParseRuneSmall::OUT_MAX / 32 + 1;
    static constexpr bool len_may(size_t n) { return n >= PAY_MIN + 3 && n <= STREAM_MAX; }
};
// the promise, the sum of count * utf8_len <= OUT_MAX, bounds every sum of counts: a heap item count << 9 | id stays one word; and 256
// symbols of at most COUNT_MAX + 1 counts of 4 bytes do not wrap the word the kernel accumulates them in
static_assert(ParseRuneMid::OUT_MAX <= ParseRuneMid::COUNT_MAX && ParseRuneMid::OUT_MAX < (1u << 23) && 256ull * (ParseRuneMid::COUNT_MAX + 1) * 4 < (1ull << 32) &&
              ParseRuneMid::PAY_MAX >= ParseRuneMid::OUT_MAX, "a sum of counts is a count; no wrap; a payload of 8 bits a decoded byte fits the lanes");
static_assert(ParseRuneMid::OUT_MAX > ParseRuneSmall::OUT_MAX && (ParseRuneMid::LANES * (ParseRuneMid::S_MAX - 32)) / 8 < ParseRuneMid::OUT_MAX &&
              ParseRuneSmall::GROUP_MIN >= 16 && ParseRuneMid::GROUP_MIN >= 16 && (ParseRuneMid::PAY_MIN - 1) * 8 * 4 == ParseRuneSmall::OUT_MAX,
              "above the 16 KiB class; one word less a lane would not hold 8 bits a decoded byte; smaller calls keep their launches; 512 bytes of payload decode to 16384 at most");
// the names the library, raisin_amd/huffman.py and the tests know the decoders' limits by
constexpr uint32_t HUFF_RUNE_OUT_MAX = ParseRuneSmall::OUT_MAX, HUFF_RUNE_PAY_MAX = ParseRuneSmall::PAY_MAX, HUFF_RUNE_STREAM_MAX = ParseRuneSmall::STREAM_MAX;
constexpr uint32_t HUFF_RUNE_MID_OUT_MAX = ParseRuneMid::OUT_MAX, HUFF_RUNE_MID_PAY_MAX = ParseRuneMid::PAY_MAX, HUFF_RUNE_MID_STREAM_MAX = ParseRuneMid::STREAM_MAX;
constexpr uint32_t HUFF_RUNE_MID_DEC_PAY_MIN = ParseRuneMid::PAY_MIN;
constexpr size_t HUFF_RUNE_DEC_GROUP_MIN = ParseRuneSmall::GROUP_MIN, HUFF_RUNE_MID_DEC_GROUP_MIN = ParseRuneMid::GROUP_MIN;

struct HuffRunePlan {
    HuffDevBounds b;                   // expect in bytes
    uint32_t a, pad_[3];               // leaves
    uint16_t child[PARSE_RUNE_CHILD_MAX + 2];
    uint32_t leaf_rune[PARSE_RUNE_SYMS_MAX];
};

RSN_HD_FN uint32_t parse_rune_scan_limit(uint32_t n) { return n < PARSE_RUNE_SCAN_MAX ? n : PARSE_RUNE_SCAN_MAX; }
template <class L = ParseRuneSmall>
RSN_HD_FN bool parse_rune_length_ok(unsigned long long n) { return n >= 8 && n <= L::STREAM_MAX; }

// the rune that starts at byte i of h[0, end), as Go's `range string` yields it (go_decode_rune, huff_host.cpp; seq_len, huff_utf8.h);
// only bytes below `end` are asked for
template <class Bytes>
RSN_HD_FN uint32_t parse_rune_decode(const Bytes &h, uint32_t i, uint32_t end) {
    const uint32_t b0 = h.get(i);
    if (b0 < 0x80) return b0;
    if (b0 < 0xC2 || b0 > 0xF4) return PARSE_RUNE_ERROR;
    const uint32_t need = b0 < 0xE0 ? 2u : b0 < 0xF0 ? 3u : 4u;
    if (end - i < need) return PARSE_RUNE_ERROR;
    const uint32_t lo = b0 == 0xE0 ? 0xA0u : b0 == 0xF0 ? 0x90u : 0x80u, hi = b0 == 0xED ? 0x9Fu : b0 == 0xF4 ? 0x8Fu : 0xBFu;
    const uint32_t b1 = h.get(i + 1);
    if (b1 < lo || b1 > hi) return PARSE_RUNE_ERROR;
    uint32_t r = ((need == 2 ? b0 & 0x1Fu : need == 3 ? b0 & 0x0Fu : b0 & 0x07u) << 6) | (b1 & 0x3Fu);
    for (uint32_t k = 2; k < need; k++) {
        const uint32_t b = h.get(i + k);
        if ((b & 0xC0u) != 0x80u) return PARSE_RUNE_ERROR;
        r = (r << 6) | (b & 0x3Fu);
    }
    return r;
}

// rune r's entry: cnt1 = count + 1 of its LAST entry.  key[] starts as PARSE_RUNE_EMPTY.  false: one rune more than the class takes
RSN_HD_FN bool parse_rune_put(uint32_t *key, uint32_t *cnt1, uint32_t *distinct, uint32_t r, uint32_t c1) {
    uint32_t slot = plan_rune_hash(r);
    for (uint32_t p = 0; p < PARSE_RUNE_SLOTS; p++) {
        const uint32_t k = key[slot];
        if (k == r) { cnt1[slot] = c1; return true; }
        if (k == PARSE_RUNE_EMPTY) {
            if (*distinct >= PARSE_RUNE_SYMS_MAX) return false;
            key[slot] = r; cnt1[slot] = c1; (*distinct)++;
            return true;
        }
        slot = (slot + 1) & (PARSE_RUNE_SLOTS - 1);
    }
    return false;                                                      // (at most half the slots are ever taken: not reached)
}

// The entries of h[0, sep) into the table; a count saturates at the class's COUNT_MAX + 1.  h.get(i) is asked for i < sep only.
// false: refused.
template <class L = ParseRuneSmall, class Bytes>
RSN_HD_FN bool parse_rune_scan(const Bytes &h, uint32_t sep, uint32_t *key, uint32_t *cnt1, uint32_t *distinct) {
    uint32_t acc = 0;
    for (uint32_t i = 0; i < sep; i++) {
        const uint32_t ch = h.get(i);
        if (ch != '|') {
            if (ch >= '0' && ch <= '9') { acc = acc * 10 + (ch - '0'); if (acc > L::COUNT_MAX) acc = L::COUNT_MAX + 1; }
            continue;
        }
        const uint32_t f = acc;
        acc = 0;
        if (i + 1 >= sep) return false;
        uint32_t r, skip = 1;
        if (h.get(i + 1) == '\\') {
            if (i + 2 >= sep) return false;
            if (h.get(i + 2) == 'n') { r = 10; skip = 2; }
            else r = '\\';
        } else r = parse_rune_decode(h, i + 1, sep);
        if (!parse_rune_put(key, cnt1, distinct, r, f + 1)) return false;
        i += skip;
    }
    return true;
}

// string(rune) for a rune the scan yields (never a surrogate, never beyond U+10FFFF): its bytes to out, their number returned
RSN_HD_FN uint32_t parse_rune_write(uint32_t r, uint8_t *out) {
    if (r < 0x80) { out[0] = (uint8_t)r; return 1; }
    if (r < 0x800) { out[0] = (uint8_t)(0xC0 | r >> 6); out[1] = (uint8_t)(0x80 | (r & 0x3F)); return 2; }
    if (r < 0x10000) { out[0] = (uint8_t)(0xE0 | r >> 12); out[1] = (uint8_t)(0x80 | ((r >> 6) & 0x3F)); out[2] = (uint8_t)(0x80 | (r & 0x3F)); return 3; }
    out[0] = (uint8_t)(0xF0 | r >> 18); out[1] = (uint8_t)(0x80 | ((r >> 12) & 0x3F)); out[2] = (uint8_t)(0x80 | ((r >> 6) & 0x3F)); out[3] = (uint8_t)(0x80 | (r & 0x3F));
    return 4;
}

// one symbol's part of the counts' verdict
RSN_HD_FN uint32_t parse_rune_bytes(uint32_t r, uint32_t c1) { return (c1 - 1) * plan_rune_utf8_len(r); }
// the counts' verdict: a distinct runes, one of them >= 0x80, none with a count beyond the limit, expect bytes in all
template <class L = ParseRuneSmall>
RSN_HD_FN bool parse_rune_counts_ok(uint32_t a, bool any_high, bool any_over, unsigned long long expect) {
    return a >= 2 && a <= PARSE_RUNE_SYMS_MAX && any_high && !any_over && expect != 0 && expect <= L::OUT_MAX;
}
// the stream's bounds (parse_bounds) and the class's lanes
template <class L = ParseRuneSmall>
RSN_HD_FN bool parse_rune_bounds(uint32_t n, uint32_t sep, uint32_t diff, HuffDevBounds &p, uint32_t *S, uint32_t *T) {
    return parse_bounds(n, sep, diff, p) && parse_lanes(p.end - p.p0, L::LANES, L::S_MAX, S, T);
}
// a node of plan_tree as an entry of child[]: a leaf's rank, or the internal node
RSN_HD_FN uint32_t parse_rune_child(uint32_t id, uint32_t a) { return id < a ? 0x8000u | id : id - a; }

// ---- the plan in front of the tree, serially (the "light scan"): what the host's classifier asks of a member and what
// k_huff_dev_rune_plan answers where the stream lies.  The table lives on the caller's stack; in[0, n) is all it reads.  A planned
// answer may still be handed back by the decoder: the depth of the deepest code needs the tree.
struct ParseRuneTable { uint32_t key[PARSE_RUNE_SLOTS], cnt1[PARSE_RUNE_SLOTS], distinct; };
template <class L = ParseRuneSmall>
inline bool parse_rune_light_serial(const uint8_t *in, unsigned long long n64, ParseRuneTable &t, HuffDevBounds &p, uint32_t *sep_out, uint32_t *S, uint32_t *T) {
    p = HuffDevBounds{};
    p.verdict = PARSE_NOT_MINE;
    if (!parse_rune_length_ok<L>(n64)) return false;
    const uint32_t n = (uint32_t)n64, limit = parse_rune_scan_limit(n);
    uint32_t sep = PARSE_NONE;
    for (uint32_t i = 0; i + 1 < limit; i++) if (parse_sep_at(in[i], in[i + 1])) { sep = i; break; }
    if (sep == PARSE_NONE || sep + 4 > n) return false;
    for (uint32_t s = 0; s < PARSE_RUNE_SLOTS; s++) { t.key[s] = PARSE_RUNE_EMPTY; t.cnt1[s] = 0; }
    t.distinct = 0;
    if (!parse_rune_scan<L>(ParseArrayBytes{in}, sep, t.key, t.cnt1, &t.distinct)) return false;
    bool high = false, over = false;
    unsigned long long expect = 0;
    for (uint32_t s = 0; s < PARSE_RUNE_SLOTS; s++) {
        if (t.key[s] == PARSE_RUNE_EMPTY) continue;
        high = high || t.key[s] >= 0x80;
        over = over || t.cnt1[s] - 1 > L::COUNT_MAX;
        expect += parse_rune_bytes(t.key[s], t.cnt1[s]);
    }
    if (!parse_rune_counts_ok<L>(t.distinct, high, over, expect) || !parse_rune_bounds<L>(n, sep, in[sep + 2], p, S, T)) return false;
    p.expect = (uint32_t)expect;
    *sep_out = sep;
    return true;
}
template <class L = ParseRuneSmall>
inline HuffDevSummary parse_rune_light(const uint8_t *in, unsigned long long n) {
    ParseRuneTable t;
    HuffDevBounds p;
    uint32_t sep, S, T;
    if (!parse_rune_light_serial<L>(in, n, t, p, &sep, &S, &T)) return HuffDevSummary{PARSE_NOT_MINE, 0, 0, 0};
    return HuffDevSummary{PARSE_PLANNED, p.A0, p.end - p.p0, p.expect};
}

// ---- the whole plan, serially, over array stores: what the kernel does with a workgroup (the separator by a block-wide minimum, one
// lane's scan, the ranks a thread each, the tree in one wavefront's VGPRs).  The CPU test's subject; in[0, n) is all it reads.
// info (where asked for): what the plan's fields do not say -- the distinct runes and the deepest code also of a stream that is refused for
// its depth, and the lanes; zeros where the stream is refused before they are known.
struct ParseRuneInfo { uint32_t a, deepest, S, T; };
template <class L = ParseRuneSmall>
inline void parse_rune_plan_serial(const uint8_t *in, unsigned long long n64, HuffRunePlan &plan, ParseRuneInfo *info = nullptr) {
    plan = HuffRunePlan{};
    if (info) *info = ParseRuneInfo{0, 0, 0, 0};
    HuffDevBounds &p = plan.b;
    ParseRuneTable t;
    uint32_t sep, S, T;
    if (!parse_rune_light_serial<L>(in, n64, t, p, &sep, &S, &T)) return;
    const uint32_t a = t.distinct;
    if (info) { info->a = a; info->S = S; info->T = T; }
    uint32_t rune[PARSE_RUNE_SYMS_MAX], cnt1[PARSE_RUNE_SYMS_MAX];
    for (uint32_t s = 0, at = 0; s < PARSE_RUNE_SLOTS; s++) if (t.key[s] != PARSE_RUNE_EMPTY) { rune[at] = t.key[s]; cnt1[at] = t.cnt1[s]; at++; }
    ParseArrayStore<PARSE_RUNE_SYMS_MAX> heap{}, kids{};
    ParseArrayStore<PLAN_RUNE_NODES_MAX + 1> code{};
    for (uint32_t k = 0; k < a; k++) {
        uint32_t lr, rr;
        plan_rune_ranks(rune, cnt1, a, k, &lr, &rr);
        plan.leaf_rune[lr] = rune[k];
        heap.v[lr] = plan_item<PLAN_RUNE_IDB>(cnt1[k] - 1, lr);
    }
    const uint32_t root = plan_tree<PLAN_RUNE_IDB>(a, heap, kids);
    plan_codes<PLAN_RUNE_IDB>(a, root, kids, code);
    uint32_t mn = 255, mx = 0;
    for (uint32_t r = 0; r < a; r++) { const uint32_t l = code.v[r] >> 24; mn = l < mn ? l : mn; mx = l > mx ? l : mx; }
    if (info) info->deepest = mx;
    if (!parse_depths(mn, mx, p)) return;
    for (uint32_t k = 0; k + 1 < a; k++) {
        plan.child[2 * k] = (uint16_t)parse_rune_child(kids.v[k] & ((1u << PLAN_RUNE_IDB) - 1), a);
        plan.child[2 * k + 1] = (uint16_t)parse_rune_child(kids.v[k] >> PLAN_RUNE_IDB, a);
    }
    plan.a = a;
    p.root = root - a;
    p.n_child = 2 * (a - 1);
    p.verdict = PARSE_PLANNED;
}

}  // namespace rsn
