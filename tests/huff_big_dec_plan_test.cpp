// huff_big_dec_plan_test.cpp -- the tiled class of the Huffman decompress batch (raisin_amd/csrc/huff_big_dec.hip) as far as it is plain
// code: huff_big_dec_layout.h against naive loops, the WIDE form of huff_parse_small.h against the host's parse_header + build_tree +
// assign_codes (huff_host.cpp), and a model of the three phases -- every tile's map from all 32 entries, the maps chained by bigd_chain,
// every tile emitted from its entry -- held byte for byte against the serial decoder on whole members.  Built and run by
// tests/test_huff_big_dec_host.py.  Prints "ok <layout checks> <headers> <members> periodic <taken|back>" and exits 0, or the first
// disagreement and 1.  argv[1]: a file whose bytes, repeated, are the periodic member.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "huff_big_dec_layout.h"
#include "huff_host.h"
#include "huff_parse_small.h"

using namespace rsn;

namespace {

long long g_layout = 0, g_headers = 0, g_members = 0;

#define CHECK(cond, ...) do { if (!(cond)) { printf(__VA_ARGS__); printf("\n"); return false; } } while (0)

// ---------------------------------------------------------------- the layout against naive loops
bool layout() {
    CHECK(BIGD_TILE_BITS == 61440 && BIGD_TILES_MAX == 30 && BIGD_LANES_ALL == 28800, "the shape moved");
    const uint32_t spans[] = {1, 63, 64, 65, 61439, 61440, 61441, 122880, 122881, 8 * 65537 / 2, 8 * BIGD_PAY_MAX - 7, 8 * BIGD_PAY_MAX};
    std::vector<uint32_t> all(spans, spans + sizeof spans / sizeof spans[0]);
    std::mt19937 rng(7);
    for (int i = 0; i < 2000; i++) all.push_back(1 + rng() % (8 * BIGD_PAY_MAX));
    for (uint32_t span : all) {
        uint32_t lanes = 0, tiles = 0;
        for (uint32_t bit = 0; bit < span; bit += BIGD_S) lanes++;
        for (uint32_t l = 0; l < lanes; l += BIGD_LANES) tiles++;
        CHECK(bigd_lanes(span) == lanes && bigd_tiles(span) == tiles && tiles <= BIGD_TILES_MAX, "span %u: %u lanes, %u tiles", span, bigd_lanes(span), bigd_tiles(span));
        CHECK((tiles - 1) * BIGD_TILE_BITS < span && span <= tiles * BIGD_TILE_BITS, "span %u: the tiles do not cover it", span);
        uint32_t S = 0, T = 0;
        CHECK(parse_lanes(span, BIGD_LANES_ALL, BIGD_S, &S, &T) && S == BIGD_S && T == lanes, "span %u: parse_lanes answers S = %u, T = %u", span, S, T);
        g_layout++;
    }
    uint32_t S = 0, T = 0;
    CHECK(!parse_lanes(8 * BIGD_PAY_MAX + 8 * 1024 + 1, BIGD_LANES_ALL, BIGD_S, &S, &T), "a span beyond the tiles is taken");
    // the scratch: the three parts do not overlap and end at BIGD_SCR_WORDS
    std::vector<int> owner(BIGD_SCR_WORDS, 0);
    for (uint32_t t = 0; t < BIGD_TILES_MAX; t++) for (uint32_t c = 0; c < 32; c++) owner[BIGD_SCR_MAP + t * 32 + c]++;
    for (uint32_t t = 0; t < BIGD_TILES_MAX; t++) for (uint32_t k = 0; k < 4; k++) owner[BIGD_SCR_TILE + t * 4 + k]++;
    for (uint32_t k = 0; k < 4; k++) owner[BIGD_SCR_META + k]++;
    for (uint32_t w = 0; w < BIGD_SCR_WORDS; w++) CHECK(owner[w] == 1, "scratch word %u has %d owners", w, owner[w]);
    CHECK(BIGD_SCR_WORDS == 30 * 32 + 30 * 4 + 4 && BIGD_SCR_WORDS % 4 == 0, "scratch of %u words", BIGD_SCR_WORDS);
    CHECK(BIGD_META_VERDICT < 4 && BIGD_META_TOTAL < 4 && BIGD_META_DONE < 4 && BIGD_TILE_COUNT < 4, "a member's words");
    // the chain's refusals on hand-made maps
    std::vector<uint32_t> maps(BIGD_TILES_MAX * 32, (uint32_t)BIGD_OFF_BAD << 24), rec(BIGD_TILES_MAX * 4);
    uint32_t total = 0;
    maps[0] = 5u << 24 | 100; maps[32 + 5] = 0u << 24 | 50;
    CHECK(bigd_chain(maps.data(), 2, 150, rec.data(), &total) && total == 150 && rec[4 + BIGD_TILE_ENTRY] == 5 && rec[4 + BIGD_TILE_BASE] == 100 && rec[4 + BIGD_TILE_COUNT] == 50, "two tiles");
    CHECK(!bigd_chain(maps.data(), 2, 149, rec.data(), &total), "more symbols than the header promises");
    CHECK(!bigd_chain(maps.data(), 1, 150, rec.data(), &total), "a stream that ends inside a codeword");
    CHECK(!bigd_chain(maps.data(), 3, 1000, rec.data(), &total), "a lost tile");
    CHECK(!bigd_chain(maps.data(), 0, 150, rec.data(), &total) && !bigd_chain(maps.data(), BIGD_TILES_MAX + 1, 150, rec.data(), &total), "no tiles, too many");
    maps[0] = 0u << 24 | (BIGD_OUT_CAP - 16);
    CHECK(bigd_chain(maps.data(), 1, BIGD_OUT_MAX, rec.data(), &total) && total == BIGD_OUT_CAP - 16, "a tile at the image's cap");
    maps[0] = 0u << 24 | (BIGD_OUT_CAP - 15);
    CHECK(!bigd_chain(maps.data(), 1, BIGD_OUT_MAX, rec.data(), &total), "a tile beyond the image's cap");
    g_layout += 9;
    return true;
}

// ---------------------------------------------------------------- the wide parse against the host
std::string entry(unsigned long long count, uint32_t b) {
    std::string e = std::to_string(count) + "|";
    if (b == 10) e += "\\n"; else e.push_back((char)b);
    return e;
}
std::vector<uint8_t> stream_of(const std::string &hdr, size_t pay_bytes, unsigned pad) {
    std::vector<uint8_t> out(hdr.begin(), hdr.end());
    out.push_back(0x5C); out.push_back(0x0A); out.push_back((uint8_t)pad);
    for (size_t i = 0; i < pay_bytes; i++) out.push_back((uint8_t)(i * 131 + 7));
    return out;
}
// small_dec_plan's wide form (huff_small.hip) from the host's pieces: 0 planned, 1 refused
struct Ref { int verdict = 1; uint16_t child[256] = {0}; uint32_t root = 0, n_child = 0, K = 0, flat = 0, A0 = 0, p0 = 0, end = 0; unsigned long long expect = 0; };
void ref_plan(const uint8_t *in, size_t n, Ref &r) {
    r = Ref();
    if (n < 8 || n > PARSE_STREAM_MAX_WIDE) return;
    size_t sep = (size_t)-1;
    for (size_t i = 0; i + 1 < std::min<size_t>(n, PARSE_SCAN_MAX); i++) if (in[i] == 0x5C && in[i + 1] == 0x0A) { sep = i; break; }
    if (sep == (size_t)-1 || sep + 4 > n) return;
    std::vector<HuffSym> syms; std::string msg;
    if (!parse_header(in, sep, syms, msg) || syms.size() < 2 || syms.size() > 128) return;
    unsigned long long expect = 0;
    for (const HuffSym &sy : syms) { if (sy.rune >= 0x80 || sy.freq >= PLAN_COUNT_LIMIT_WIDE) return; expect += sy.freq; }
    if (expect == 0 || expect > PARSE_OUT_MAX_WIDE) return;
    const size_t pay = sep + 3;
    const unsigned long long nbits = (unsigned long long)(n - pay) * 8;
    if (in[sep + 2] >= nbits) return;
    HuffTree tree; HuffCodes codes;
    if (!build_tree(syms, tree, msg) || !assign_codes(tree, codes, msg, false) || codes.max_len > 32 || codes.max_len == 0) return;
    const uint32_t A = tree.n_leaves;
    for (size_t i = 0; i < tree.freq.size() - A; i++) {
        const int32_t kids[2] = {tree.left[A + i], tree.right[A + i]};
        for (int b = 0; b < 2; b++) r.child[2 * i + b] = tree.is_leaf(kids[b]) ? (uint16_t)(0x8000u | tree.rune[kids[b]]) : (uint16_t)(kids[b] - (int32_t)A);
    }
    r.root = (uint32_t)(tree.root - (int32_t)A); r.n_child = (uint32_t)(2 * (tree.freq.size() - A));
    r.A0 = (uint32_t)(pay & ~(size_t)3);
    r.p0 = (uint32_t)(8 * (pay - r.A0) + in[sep + 2]); r.end = (uint32_t)(8 * (pay - r.A0) + nbits);
    r.K = std::min<unsigned>(codes.max_len, PARSE_K_MAX); r.flat = codes.min_len == codes.max_len ? codes.max_len : 0u;
    r.expect = expect; r.verdict = 0;
}
// want_wide / want_narrow: the verdicts expected of the two forms (0 planned, 1 refused)
bool header_case(const char *what, const std::string &hdr, size_t pay_bytes, int want_wide, int want_narrow) {
    const std::vector<uint8_t> s = stream_of(hdr, pay_bytes, 3);
    uint8_t *exact = (uint8_t *)malloc(s.size());                          // (an allocation of exactly n bytes: a read behind it is the sanitizer's to see)
    memcpy(exact, s.data(), s.size());
    HuffDevPlan wide, narrow;
    parse_plan_serial(exact, s.size(), wide, true);
    parse_plan_serial(exact, s.size(), narrow);
    Ref r;
    ref_plan(exact, s.size(), r);
    free(exact);
    g_headers++;
    CHECK((int)wide.b.verdict == want_wide, "%s: the wide form answers %u, expected %d", what, wide.b.verdict, want_wide);
    CHECK((int)narrow.b.verdict == want_narrow, "%s: the narrow form answers %u, expected %d", what, narrow.b.verdict, want_narrow);
    if (want_wide != 0) return true;
    CHECK(r.verdict == 0, "%s: the host refuses what the wide form plans", what);
    CHECK(r.root == wide.b.root && r.n_child == wide.b.n_child && r.K == wide.b.K && r.flat == wide.b.flat, "%s: root / n_child / K / flat differ", what);
    CHECK(r.A0 == wide.b.A0 && r.p0 == wide.b.p0 && r.end == wide.b.end && r.expect == wide.b.expect, "%s: the bounds differ (expect %llu, plan %u)", what, r.expect, wide.b.expect);
    CHECK(memcmp(r.child, wide.child, sizeof r.child) == 0, "%s: child[] differs", what);
    if (want_narrow == 0) CHECK(memcmp(&narrow, &wide, sizeof wide) == 0, "%s: the two forms plan a narrow stream differently", what);
    return true;
}
bool headers() {
    // (a payload of 9000 bytes is inside the narrow stream length: the counts alone decide)
    if (!header_case("a count of 65535 and one", entry(65535, 'a') + entry(1, 'b'), 9000, 0, 0)) return false;
    if (!header_case("a count of 65535 and two", entry(65535, 'a') + entry(2, 'b'), 9000, 0, 1)) return false;          // the sum is 65537: wide
    if (!header_case("a count of 65536 alone", entry(65536, 'a') + entry(0, 'b'), 9000, 1, 1)) return false;            // the sum is narrow: the narrow count limit judges
    if (!header_case("a count of 65536 and one", entry(65536, 'a') + entry(1, 'b'), 9000, 0, 1)) return false;
    if (!header_case("a count of 262143 and one", entry(262143, 'a') + entry(1, 'b'), 40000, 0, 1)) return false;
    if (!header_case("a sum of 262144 over three", entry(200000, 'a') + entry(62143, 'b') + entry(1, 'c'), 40000, 0, 1)) return false;
    if (!header_case("a sum of 262145", entry(262143, 'a') + entry(2, 'b'), 40000, 1, 1)) return false;
    if (!header_case("a count of 2^24", entry(1u << 24, 'a') + entry(1, 'b'), 40000, 1, 1)) return false;
    if (!header_case("a count of 20 digits", "12345678901234567890|a" + entry(3, 'b'), 9000, 1, 1)) return false;
    if (!header_case("a large count that a later entry replaces", entry(70000, 'a') + entry(2, 'b') + entry(5, 'a'), 9000, 0, 0)) return false;
    if (!header_case("a rune", entry(100000, 'a') + "5|\xC3\xA9", 40000, 1, 1)) return false;
    if (!header_case("one distinct byte", entry(100000, 'a'), 40000, 1, 1)) return false;
    // the stream's length: narrow counts in a long stream are the wide form's; the wide length limit
    if (!header_case("a long stream of narrow counts", entry(30000, 'a') + entry(30000, 'b'), PARSE_STREAM_MAX, 0, 1)) return false;
    {
        const std::string h = entry(131072, 'a') + entry(131072, 'b');
        if (!header_case("the longest stream", h, PARSE_STREAM_MAX_WIDE - h.size() - 3, 0, 1)) return false;
        if (!header_case("one byte longer", h, PARSE_STREAM_MAX_WIDE - h.size() - 2, 1, 1)) return false;
    }
    // 128 counts that sum to the limit, and Fibonacci counts (the deepest codes)
    {
        std::string h; for (uint32_t b = 0; b < 128; b++) h += entry(2048, b);
        if (!header_case("128 counts of 2048", h, 40000, 0, 1)) return false;
        std::string f; unsigned long long f0 = 1, f1 = 1;
        for (uint32_t k = 0; k < 25; k++) { f += entry(f0, 33 + k); const unsigned long long t = f0 + f1; f0 = f1; f1 = t; }
        if (!header_case("F1..F25", f, 40000, 0, 1)) return false;
    }
    return true;
}

// ---------------------------------------------------------------- the three phases as a model
// the library's own stream of `data` (a byte alphabet, two distinct bytes at least), from the host's tree and codes
std::vector<uint8_t> encode(const std::vector<uint8_t> &data) {
    std::vector<uint64_t> cnt(128, 0);
    for (uint8_t b : data) cnt[b]++;
    std::vector<HuffSym> syms;
    for (uint32_t b = 0; b < 128; b++) if (cnt[b]) syms.push_back({b, cnt[b]});
    std::string hdr, msg;
    emit_header(syms, hdr);
    HuffTree tree; HuffCodes codes;
    std::vector<HuffSym> work = syms;
    if (!build_tree(work, tree, msg) || !assign_codes(tree, codes, msg, false)) abort();
    uint64_t code_of[128] = {0}; uint32_t len_of[128] = {0};
    for (uint32_t i = 0; i < tree.n_leaves; i++) { code_of[tree.rune[i]] = codes.code[i]; len_of[tree.rune[i]] = codes.len[i]; }
    const unsigned pad = (unsigned)((8 - codes.total_bits % 8) % 8);
    std::vector<uint8_t> out(hdr.begin(), hdr.end());
    out.push_back(0x5C); out.push_back(0x0A); out.push_back((uint8_t)pad);
    const size_t pay = out.size();
    out.resize(pay + (size_t)((codes.total_bits + pad) / 8), 0);
    uint64_t at = pad;
    for (uint8_t b : data)
        for (uint32_t k = len_of[b]; k-- > 0; at++) if ((code_of[b] >> k) & 1) out[pay + at / 8] |= (uint8_t)(0x80 >> (at % 8));
    return out;
}
struct Bits {                                                              // the stream from A0 on, as the kernels count its bits
    const uint8_t *p; const HuffDevPlan *plan;
    uint32_t bit(uint32_t i) const { return (p[i >> 3] >> (7 - (i & 7))) & 1; }
    // the codeword at `pos`: its byte; pos moves behind it.  false: it runs off the payload
    bool next(uint32_t &pos, uint8_t &sym) const {
        uint32_t node = plan->b.root;
        for (;;) {
            if (pos >= plan->b.end) return false;
            node = plan->child[2 * node + bit(pos++)];
            if (node & 0x8000) { sym = (uint8_t)node; return true; }
        }
    }
};
// what lane_dec_body's map says of a tile entered at bit c: the codewords that START in [lo + c, hi)
uint32_t tile_map(const Bits &s, uint32_t lo, uint32_t hi, uint32_t c) {
    uint32_t pos = lo + c, n = 0;
    uint8_t sym;
    if (pos > s.plan->b.end) return (uint32_t)BIGD_OFF_BAD << 24;
    while (pos < hi) { if (!s.next(pos, sym)) return (uint32_t)BIGD_OFF_BAD << 24; n++; }
    return (pos - hi) << 24 | n;
}
bool member(const char *what, const std::vector<uint8_t> &data, bool *taken_out = nullptr) {
    const std::vector<uint8_t> stream = encode(data);
    HuffDevPlan plan;
    parse_plan_serial(stream.data(), stream.size(), plan, true);
    CHECK(plan.b.verdict == PARSE_PLANNED && plan.b.expect == data.size(), "%s: not planned (%zu bytes)", what, data.size());
    const Bits s{stream.data() + plan.b.A0, &plan};
    const uint32_t p0 = plan.b.p0, end = plan.b.end, span = end - p0, tiles = bigd_tiles(span);
    // the serial decoder, and from its codeword starts the naive answer: every tile's first output byte and symbols
    std::vector<uint8_t> serial;
    std::vector<uint32_t> naive_base(tiles + 1, 0);
    {
        uint32_t pos = p0; uint8_t sym;
        while (pos < end) {
            const uint32_t t = (pos - p0) / BIGD_TILE_BITS;
            if (!s.next(pos, sym)) break;
            serial.push_back(sym);
            for (uint32_t u = t + 1; u <= tiles; u++) naive_base[u]++;
        }
        CHECK(pos == end && serial == data, "%s: the serial decoder does not give the member back", what);
    }
    bool fits = true;
    for (uint32_t t = 0; t < tiles; t++) fits = fits && naive_base[t + 1] - naive_base[t] + 16 <= BIGD_OUT_CAP;
    // phase 1: every tile's map from all 32 entries (tile 0 is entered at its first bit alone)
    std::vector<uint32_t> maps(tiles * 32, (uint32_t)BIGD_OFF_BAD << 24);
    for (uint32_t t = 0; t < tiles; t++) {
        const uint32_t lo = p0 + t * BIGD_TILE_BITS, hi = std::min(end, lo + BIGD_TILE_BITS);
        for (uint32_t c = 0; c < (t ? 32u : 1u); c++) maps[t * 32 + c] = tile_map(s, lo, hi, c);
    }
    // phase 2: the chain
    std::vector<uint32_t> rec(tiles * 4);
    uint32_t total = 0;
    const bool taken = bigd_chain(maps.data(), tiles, plan.b.expect, rec.data(), &total);
    if (taken_out) *taken_out = taken;
    CHECK(taken == fits, "%s: the chain %s a member whose tiles %s the image", what, taken ? "takes" : "hands back", fits ? "fit" : "do not fit");
    g_members++;
    if (!taken) return true;
    CHECK(total == data.size(), "%s: the chain counts %u symbols of %zu", what, total, data.size());
    // phase 3: every tile from its entry, its bytes to [base, base + count): every byte once
    std::vector<uint8_t> out(data.size(), 0);
    std::vector<uint8_t> stored(data.size(), 0);
    for (uint32_t t = 0; t < tiles; t++) {
        const uint32_t entry_bit = rec[4 * t + BIGD_TILE_ENTRY], base = rec[4 * t + BIGD_TILE_BASE], count = rec[4 * t + BIGD_TILE_COUNT];
        CHECK(base == naive_base[t] && count == naive_base[t + 1] - naive_base[t], "%s: tile %u at byte %u with %u symbols, naive %u with %u", what, t, base, count, naive_base[t], naive_base[t + 1] - naive_base[t]);
        uint32_t pos = p0 + t * BIGD_TILE_BITS + entry_bit;
        for (uint32_t i = 0; i < count; i++) { uint8_t sym; CHECK(s.next(pos, sym), "%s: tile %u runs off the payload", what, t); out[base + i] = sym; stored[base + i]++; }
    }
    for (size_t i = 0; i < data.size(); i++) CHECK(stored[i] == 1, "%s: byte %zu stored %u times", what, i, stored[i]);
    CHECK(out == data, "%s: the tiles' bytes differ from the serial decoder's", what);
    return true;
}

std::vector<uint8_t> draw(uint32_t seed, size_t n, const std::vector<uint8_t> &alphabet, const std::vector<double> &weights) {
    std::mt19937 rng(seed);
    std::discrete_distribution<int> d(weights.begin(), weights.end());
    std::vector<uint8_t> out(n);
    for (auto &b : out) b = alphabet[d(rng)];
    return out;
}

}  // namespace

int main(int argc, char **argv) {
    if (!layout() || !headers()) return 1;
    // text: letters, spaces and newlines at text's frequencies (4 to 5 bits a symbol)
    {
        const char *letters = " etaoinshrdlucmfwypvbgkqjxz\n,.";
        std::vector<uint8_t> a(letters, letters + strlen(letters));
        std::vector<double> w;
        for (size_t i = 0; i < a.size(); i++) w.push_back(1.0 / (1 + i));
        for (size_t n : {(size_t)65537, (size_t)100000, (size_t)200000, (size_t)262144})
            if (!member("text", draw(11 + (uint32_t)n, n, a, w))) return 1;
    }
    {   // two symbols: a payload tile decodes to far more than it holds, and to more than the image's cap
        bool taken = true;
        if (!member("two symbols", draw(12, 262144, {'a', 'b'}, {1, 1}), &taken)) return 1;
        if (taken) { printf("two symbols of a bit each fit an image of %u bytes\n", BIGD_OUT_CAP); return 1; }
    }
    {   // 128 symbols near 7 bits, and the flat code: the largest payload
        std::vector<uint8_t> a(128); std::vector<double> w(128);
        for (uint32_t b = 0; b < 128; b++) { a[b] = (uint8_t)b; w[b] = 1.0 + (b % 5) * 0.05; }
        if (!member("128 symbols", draw(13, 250000, a, w))) return 1;
        std::vector<uint8_t> flat(262144);
        for (size_t i = 0; i < flat.size(); i++) flat[i] = (uint8_t)((i * 37 + i / 128) % 128);
        if (!member("the flat code", flat)) return 1;
    }
    {   // Fibonacci counts F1..F25: 196417 bytes, a deepest code of 24 bits, codewords that straddle tiles
        std::vector<uint8_t> fib;
        unsigned long long f0 = 1, f1 = 1;
        for (uint32_t k = 0; k < 25; k++) { fib.insert(fib.end(), (size_t)f0, (uint8_t)(33 + k)); const unsigned long long t = f0 + f1; f0 = f1; f1 = t; }
        std::mt19937 rng(14);
        std::shuffle(fib.begin(), fib.end(), rng);
        bool taken = false;
        if (fib.size() != 196417 || !member("fibonacci", fib, &taken)) return 1;
        if (!taken) { printf("the Fibonacci member is handed back\n"); return 1; }
    }
    bool periodic_taken = false;
    if (argc > 1) {   // periodic data: the model has no phases to lose, so it is taken here; the lanes' model (tests/lane_maps.py) takes it too
        FILE *f = fopen(argv[1], "rb");
        if (!f) { printf("cannot open %s\n", argv[1]); return 1; }
        std::vector<uint8_t> one(1 << 16);
        one.resize(fread(one.data(), 1, one.size(), f));
        fclose(f);
        std::vector<uint8_t> per;
        while (per.size() < 150000) per.insert(per.end(), one.begin(), one.end());
        per.resize(150000);
        if (*std::max_element(per.begin(), per.end()) >= 0x80 || !member("periodic", per, &periodic_taken)) return 1;
    }
    printf("ok %lld %lld %lld periodic %s\n", g_layout, g_headers, g_members, periodic_taken ? "taken" : "back");
    return 0;
}
