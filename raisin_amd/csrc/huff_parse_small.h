// huff_parse_small.h -- the lane-map decoders' plan of a stream with a BYTE alphabet, as code that compiles for the host and the device:
// what small_dec_plan (huff_small.hip) does on the host through parse_header, build_tree and assign_codes, restated so that
// k_huff_dev_plan (huff_dev.hip) can run it on a stream that lies in device memory -- the header found and scanned, the Go-exact tree
// (huff_plan_small.h), its children as the decoders' child[], the deepest code and the stream's bit bounds.  tests/test_huff_parse_host.py
// compiles it with huff_host.cpp and holds it against small_dec_plan's fields.
//   separator  the first 5C 0A among the first PARSE_SCAN_MAX bytes; sep + 4 <= n                          huffman.go:261
//   header     decodeTree's scan (huffman.go:196-227; parse_header, huff_host.cpp): digits accumulate a count, every other byte that is
//              not '|' is ignored; at '|' the entry's count is what has accumulated ("" counts 0), its symbol the byte behind it --
//              "\n" written as '\\' 'n' is byte 10 and skips two bytes, anything else skips one, a digit, a '|' or a '\\' included;
//              a later entry for a byte replaces an earlier one; any order
//   refused    (the answer "not mine": the member takes the single call, which decodes it or words its error) a symbol byte >= 0x80; a
//              header that ends behind '|' or behind "|\\"; fewer than 2 distinct bytes; a count >= PLAN_COUNT_LIMIT (stricter than the
//              host's > 65536: a count and a node id pack into one word); a sum of counts of 0 or above PARSE_OUT_MAX; a pad byte that
//              leaves no code bit; a deepest code of 0 bits or of more than 32
//   tree       leaves by plan_leaf_rank over count + 1 (a count of 0 is a leaf like any other, build_tree), plan_tree, plan_codes for the depths
// The WIDE form is the same plan for the tiled decoder's class (huff_big_dec.hip; codecs.h: HUFF_BIG_OUT_MAX, HUFF_BIG_PAY_MAX): a stream
// that the limits above refuse for its SIZE alone -- longer than PARSE_STREAM_MAX, or promising more than PARSE_OUT_MAX bytes -- is planned
// under PARSE_STREAM_MAX_WIDE, PARSE_OUT_MAX_WIDE and counts below PLAN_COUNT_LIMIT_WIDE (plan_item packs them: huff_plan_small.h).  A
// stream inside the narrow sizes is judged by the narrow limits in either form, so what the other classes are handed does not change.
// The scan reads only the member's first min(n, PARSE_SCAN_MAX) bytes, every loop is bounded by that or by the 255 nodes, and the tree's
// state goes through stores (get / set), so the kernel keeps it in VGPRs as k_huff_batch_enc does.
#pragma once

#include "huff_plan_small.h"

namespace rsn {

constexpr uint32_t PARSE_HDR_MAX = 1100;                   // HUFF_HDR_MAX (group_layout.h)
constexpr uint32_t PARSE_SCAN_MAX = PARSE_HDR_MAX + 8;     // bytes of a stream the separator is looked for in
constexpr uint32_t PARSE_STREAM_MAX = 65536 + 2048;        // DEC_STREAM_MAX (huff_small_body.h)
constexpr uint32_t PARSE_OUT_MAX = 65536;                  // SMALL_MAX
constexpr uint32_t PARSE_K_MAX = 9;                        // DEC_K
constexpr uint32_t PARSE_OUT_MAX_WIDE = 262144;            // HUFF_BIG_OUT_MAX (codecs.h)
constexpr uint32_t PARSE_PAY_MAX_WIDE = 229376;            // HUFF_BIG_PAY_MAX
constexpr uint32_t PARSE_STREAM_MAX_WIDE = PARSE_HDR_MAX + 8 + PARSE_PAY_MAX_WIDE;
static_assert(PARSE_OUT_MAX_WIDE < PLAN_COUNT_LIMIT_WIDE && ((unsigned long long)PARSE_OUT_MAX_WIDE << 8) < (1ull << 32), "a sum of counts and a node id pack into one word (plan_item)");
static_assert(128ull * PLAN_COUNT_LIMIT_WIDE <= (1ull << 31), "the kernel sums 128 saturated counts in one word");
static_assert(8ull * (PARSE_STREAM_MAX_WIDE + 4) < (1ull << 32), "a bit position in the stream is one word");
constexpr uint32_t PARSE_NONE = 0xFFFFFFFFu;
constexpr uint32_t PARSE_PLANNED = 0, PARSE_NOT_MINE = 1;  // the verdicts (small_dec_plan's RSN_OK / 1)

// the pointer-free part of a SmallDecArgs (huff_small_body.h) and where the decoder's input begins: S and T follow from the class's lanes
// (parse_lanes), the pointers from the group's staging
struct HuffDevBounds {
    uint32_t verdict, A0;              // A0: the 4-byte boundary at or before the first payload byte -- what the kernel reads from
    uint32_t p0, end, pay_words;       // first code bit / the bit behind the last, counted from A0; words from A0 to the stream's end + 8
    uint32_t expect;                   // the sum of the counts: the bytes the stream decodes to
    uint32_t K, root, n_child, flat;
    uint32_t pad_[6];
};
struct HuffDevPlan {
    HuffDevBounds b;
    uint16_t child[256];
};
static_assert(sizeof(HuffDevBounds) == 64 && sizeof(HuffDevPlan) == 576, "a plan table entry is whole 16-byte units, the bounds four of them");
// what comes down to the host per candidate: the class and the slots' sizes depend on these
struct HuffDevSummary { uint32_t verdict, A0, span, expect; };   // span = end - p0: the code bits
static_assert(sizeof(HuffDevSummary) == 16, "16 bytes a member come down");

// how many of a stream's n bytes are looked at
RSN_HD_FN uint32_t parse_scan_limit(uint32_t n) { return n < PARSE_SCAN_MAX ? n : PARSE_SCAN_MAX; }
RSN_HD_FN bool parse_length_ok(unsigned long long n, bool allow_wide = false) { return n >= 8 && n <= (allow_wide ? PARSE_STREAM_MAX_WIDE : PARSE_STREAM_MAX); }
// is the stream judged by the wide limits?  n: its length; sum: the sum of its counts (saturated counts: an upper bound that errs wide, and
// wide refuses them)
RSN_HD_FN bool parse_is_wide(bool allow_wide, uint32_t n, unsigned long long sum) { return allow_wide && (n > PARSE_STREAM_MAX || sum > PARSE_OUT_MAX); }
// is position i the separator's?  (i + 1 < parse_scan_limit(n))
RSN_HD_FN bool parse_sep_at(uint32_t b0, uint32_t b1) { return b0 == 0x5Cu && b1 == 0x0Au; }

// The entries of h[0, sep): cnt1[b] = count + 1 of byte b's last entry, 0 where it has none; a count saturates at `limit` (PLAN_COUNT_LIMIT,
// or PLAN_COUNT_LIMIT_WIDE where the wide form is allowed).  h.get(i): byte i of the stream, asked for i < sep only.  false: refused.
// cnt1[128] must be zero.
template <class Bytes>
RSN_HD_FN bool parse_scan(const Bytes &h, uint32_t sep, uint32_t *cnt1, uint32_t limit = PLAN_COUNT_LIMIT) {
    uint32_t acc = 0;
    for (uint32_t i = 0; i < sep; i++) {
        const uint32_t ch = h.get(i);
        if (ch != '|') {
            if (ch >= '0' && ch <= '9') { acc = acc * 10 + (ch - '0'); if (acc > limit) acc = limit; }
            continue;
        }
        const uint32_t f = acc;
        acc = 0;
        if (i + 1 >= sep) return false;
        uint32_t sym = h.get(i + 1), skip = 1;
        if (sym == '\\') {
            if (i + 2 >= sep) return false;
            if (h.get(i + 2) == 'n') { sym = 10; skip = 2; }
        }
        if (sym >= 0x80u) return false;
        cnt1[sym] = f + 1;
        i += skip;
    }
    return true;
}

// the counts' verdict: a (distinct bytes) and the sum, from cnt1; wide: parse_is_wide's answer, any_at_limit: a count at or above that form's limit
RSN_HD_FN uint32_t parse_count_limit(bool wide) { return wide ? PLAN_COUNT_LIMIT_WIDE : PLAN_COUNT_LIMIT; }
RSN_HD_FN bool parse_counts_ok(uint32_t a, uint32_t any_at_limit, unsigned long long sum, bool wide = false) {
    return a >= 2 && a <= PLAN_SYMS_MAX && !any_at_limit && sum != 0 && sum <= (wide ? PARSE_OUT_MAX_WIDE : PARSE_OUT_MAX);
}

// the stream's bounds from the separator (small_dec_plan); diff: the pad byte, in[sep + 2].  false: it leaves no code bit
RSN_HD_FN bool parse_bounds(uint32_t n, uint32_t sep, uint32_t diff, HuffDevBounds &p) {
    const uint32_t pay = sep + 3, nbits = (n - sep - 3) * 8;
    if (diff >= nbits) return false;
    p.A0 = pay & ~3u;
    p.pay_words = (n - p.A0 + 3) / 4 + 8;
    p.p0 = 8 * (pay - p.A0) + diff;
    p.end = 8 * (pay - p.A0) + nbits;
    return true;
}

// bits per lane and lanes in use of a class of `lanes` subsequences of at most s_max bits; false: the stream is not for that class
RSN_HD_FN bool parse_lanes(uint32_t span, uint32_t lanes, uint32_t s_max, uint32_t *S, uint32_t *T) {
    uint32_t s = ((span + lanes - 1) / lanes + 31) & ~31u;
    if (s < 64) s = 64;
    *S = s; *T = (span + s - 1) / s;
    return s <= s_max;
}

// internal node k's two entries of child[]: kids = left | right << 8 as plan_tree leaves them, a leaves, leaf_byte[rank]
RSN_HD_FN uint32_t parse_child(uint32_t id, uint32_t a, const uint8_t *leaf_byte) { return id < a ? 0x8000u | leaf_byte[id] : id - a; }

// K, flat and the verdict on the code lengths; mn / mx: the shortest and the deepest leaf
RSN_HD_FN bool parse_depths(uint32_t mn, uint32_t mx, HuffDevBounds &p) {
    if (mx == 0 || mx > 32) return false;
    p.K = mx < PARSE_K_MAX ? mx : PARSE_K_MAX;
    p.flat = mn == mx ? mx : 0u;
    return true;
}

// ---- the whole plan, serially, over array stores: what the kernel does with a workgroup (the separator by a block-wide minimum, the
// ranks a thread each, the tree in one wavefront's VGPRs).  The CPU test's subject; in[0, n) is all it reads.
struct ParseArrayBytes { const uint8_t *p; RSN_HD_FN uint32_t get(uint32_t i) const { return p[i]; } };
template <int N>
struct ParseArrayStore {
    uint32_t v[N];
    RSN_HD_FN uint32_t get(uint32_t i) const { return v[i]; }
    RSN_HD_FN void set(uint32_t i, uint32_t x) { v[i] = x; }
};
inline void parse_plan_serial(const uint8_t *in, unsigned long long n64, HuffDevPlan &plan, bool allow_wide = false) {
    plan = HuffDevPlan{};
    HuffDevBounds &p = plan.b;
    p.verdict = PARSE_NOT_MINE;
    if (!parse_length_ok(n64, allow_wide)) return;
    const uint32_t n = (uint32_t)n64, limit = parse_scan_limit(n);
    uint32_t sep = PARSE_NONE;
    for (uint32_t i = 0; i + 1 < limit; i++) if (parse_sep_at(in[i], in[i + 1])) { sep = i; break; }
    if (sep == PARSE_NONE || sep + 4 > n) return;
    uint32_t cnt1[PLAN_SYMS_MAX] = {0};
    if (!parse_scan(ParseArrayBytes{in}, sep, cnt1, parse_count_limit(allow_wide))) return;
    uint32_t a = 0, most = 0;
    unsigned long long sum = 0;
    for (uint32_t b = 0; b < PLAN_SYMS_MAX; b++) if (cnt1[b]) { a++; most = cnt1[b] - 1 > most ? cnt1[b] - 1 : most; sum += cnt1[b] - 1; }
    const bool wide = parse_is_wide(allow_wide, n, sum);
    if (!parse_counts_ok(a, most >= parse_count_limit(wide), sum, wide) || !parse_bounds(n, sep, in[sep + 2], p)) return;
    p.expect = (uint32_t)sum;
    uint8_t leaf_byte[PLAN_SYMS_MAX] = {0};
    ParseArrayStore<PLAN_SYMS_MAX> heap{}, kids{};
    ParseArrayStore<PLAN_NODES_MAX + 1> code{};
    for (uint32_t b = 0; b < PLAN_SYMS_MAX; b++) if (cnt1[b]) { const uint32_t r = plan_leaf_rank(cnt1, b); leaf_byte[r] = (uint8_t)b; heap.v[r] = plan_item(cnt1[b] - 1, r); }
    const uint32_t root = plan_tree(a, heap, kids);
    plan_codes(a, root, kids, code);
    uint32_t mn = 255, mx = 0;
    for (uint32_t r = 0; r < a; r++) { const uint32_t l = code.v[r] >> 24; mn = l < mn ? l : mn; mx = l > mx ? l : mx; }
    if (!parse_depths(mn, mx, p)) return;
    for (uint32_t k = 0; k + 1 < a; k++) {
        plan.child[2 * k] = (uint16_t)parse_child(kids.v[k] & 0xFFu, a, leaf_byte);
        plan.child[2 * k + 1] = (uint16_t)parse_child(kids.v[k] >> 8, a, leaf_byte);
    }
    p.root = root - a;
    p.n_child = 2 * (a - 1);
    p.verdict = PARSE_PLANNED;
}

}  // namespace rsn
