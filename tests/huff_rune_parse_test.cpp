// huff_rune_parse_test.cpp -- the grouped rune decoder's plan of a stream (raisin_amd/csrc/huff_parse_rune.h: what k_huff_batch_rune_dec
// runs per member) against the host's parse_header + build_tree + assign_codes (huff_host.cpp), field by field: verdict, A0, p0, end,
// expect, K, root, flat, every child[] entry and every leaf's rune.  Built and run by tests/test_huff_rune_parse_host.py.
// Prints "ok <streams> planned <k> deepest <bits>" and exits 0, or the first disagreement and 1.
// Two more modes for tests/test_rune_limits_host.py: `slots <rune>...` prints plan_rune_hash of each rune, `plan <file>` the plan's verdict,
// distinct runes, deepest code and lanes of every stream in a file of length-prefixed records.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "huff_host.h"
#include "huff_parse_rune.h"

using namespace rsn;

namespace {
constexpr uint32_t SCAN_MAX = PARSE_RUNE_SCAN_MAX, STREAM_MAX = PARSE_RUNE_STREAM_MAX, OUT_MAX = PARSE_RUNE_OUT_MAX, K_MAX = PARSE_K_MAX;

struct Ref {
    int verdict = 1;
    uint16_t child[512] = {0};
    uint32_t leaf_rune[256] = {0};
    uint32_t a = 0, root = 0, n_child = 0, K = 0, flat = 0, A0 = 0, p0 = 0, end = 0, pay_words = 0, max_len = 0;
    unsigned long long expect = 0;
};

// the plan as the host's own functions give it
void ref_plan(const uint8_t *in, size_t n, Ref &r) {
    r = Ref();
    if (n < 8 || n > STREAM_MAX) return;
    size_t sep = (size_t)-1;
    for (size_t i = 0; i + 1 < std::min<size_t>(n, SCAN_MAX); i++) if (in[i] == 0x5C && in[i + 1] == 0x0A) { sep = i; break; }
    if (sep == (size_t)-1 || sep + 4 > n) return;
    std::vector<HuffSym> syms; std::string msg;
    if (!parse_header(in, sep, syms, msg) || syms.size() < 2 || syms.size() > 256) return;
    unsigned long long expect = 0;
    bool high = false;
    for (const HuffSym &sy : syms) { if (sy.freq > 16384) return; high = high || sy.rune >= 0x80; expect += sy.freq * (unsigned)utf8_len(sy.rune); }
    if (!high || expect == 0 || expect > OUT_MAX) return;
    const size_t pay = sep + 3, sn = n - sep - 2;
    const unsigned diff = in[sep + 2];
    const unsigned long long nbits = (unsigned long long)(sn - 1) * 8;
    if (diff >= nbits) return;
    const uint32_t span = (uint32_t)(nbits - diff);
    if (std::max<uint32_t>(64, ((span + 255) / 256 + 31) / 32 * 32) > 576) return;     // 256 lanes of at most 576 bits
    HuffTree tree; HuffCodes codes;
    if (!build_tree(syms, tree, msg) || !assign_codes(tree, codes, msg, false)) return;
    if (codes.max_len > 32 || codes.max_len == 0) return;
    const uint32_t A = tree.n_leaves;
    const size_t n_int = tree.freq.size() - A;
    for (size_t i = 0; i < n_int; i++) {
        const int32_t kids[2] = {tree.left[A + i], tree.right[A + i]};
        for (int b = 0; b < 2; b++) r.child[2 * i + b] = tree.is_leaf(kids[b]) ? (uint16_t)(0x8000u | (uint32_t)kids[b]) : (uint16_t)(kids[b] - (int32_t)A);
    }
    for (uint32_t l = 0; l < A; l++) r.leaf_rune[l] = tree.rune[l];
    r.a = A;
    r.root = (uint32_t)(tree.root - (int32_t)A);
    r.A0 = (uint32_t)(pay & ~(size_t)3);
    r.pay_words = (uint32_t)((n - r.A0 + 3) / 4) + 8;
    r.p0 = (uint32_t)(8 * (pay - r.A0) + diff);
    r.end = (uint32_t)(8 * (pay - r.A0) + nbits);
    r.K = std::min<unsigned>(codes.max_len, K_MAX); r.n_child = (uint32_t)(2 * n_int);
    r.flat = codes.min_len == codes.max_len ? codes.max_len : 0u;
    r.max_len = codes.max_len;
    r.expect = expect;
    r.verdict = 0;
}

long long g_streams = 0, g_planned = 0;
uint32_t g_deepest = 0;

// in[0, n) is the stream; the subject gets a copy of n bytes in an allocation of exactly n bytes, so that the sanitizer sees a read at or
// behind n
bool check(const std::vector<uint8_t> &buf, size_t n, const char *what, int want_verdict = -1) {
    g_streams++;
    Ref r;
    ref_plan(buf.data(), n, r);
    uint8_t *exact = (uint8_t *)malloc(n ? n : 1);
    memcpy(exact, buf.data(), n);
    HuffRunePlan plan;
    parse_rune_plan_serial(exact, n, plan);
    const HuffDevSummary light = parse_rune_light(exact, n);
    free(exact);
    const HuffDevBounds &p = plan.b;
    auto fail = [&](const char *part, unsigned long long a, unsigned long long b) { printf("%s (n = %zu): %s differs: host %llu, plan %llu\n", what, n, part, a, b); return false; };
    if (want_verdict >= 0 && r.verdict != want_verdict) return fail("the host's verdict from the expected one", (unsigned long long)r.verdict, (unsigned long long)want_verdict);
    if ((uint32_t)r.verdict != p.verdict) return fail("verdict", (unsigned long long)r.verdict, p.verdict);
    if (r.verdict != 0) return true;                                    // (the light scan may still say planned: the depths need the tree)
    g_planned++;
    g_deepest = std::max(g_deepest, r.max_len);
    if (light.verdict != PARSE_PLANNED || light.A0 != r.A0 || light.span != r.end - r.p0 || light.expect != r.expect) return fail("the light scan", r.expect, light.expect);
    if (r.a != plan.a) return fail("leaves", r.a, plan.a);
    if (r.root != p.root) return fail("root", r.root, p.root);
    if (r.n_child != p.n_child) return fail("n_child", r.n_child, p.n_child);
    for (uint32_t i = 0; i < 512; i++) if (r.child[i] != plan.child[i]) return fail("child", r.child[i], plan.child[i]);
    for (uint32_t i = 0; i < 256; i++) if (r.leaf_rune[i] != plan.leaf_rune[i]) return fail("leaf rune", r.leaf_rune[i], plan.leaf_rune[i]);
    if (r.K != p.K) return fail("K", r.K, p.K);
    if (r.flat != p.flat) return fail("flat", r.flat, p.flat);
    if (r.A0 != p.A0) return fail("A0", r.A0, p.A0);
    if (r.p0 != p.p0) return fail("p0", r.p0, p.p0);
    if (r.end != p.end) return fail("end", r.end, p.end);
    if (r.pay_words != p.pay_words) return fail("pay_words", r.pay_words, p.pay_words);
    if (r.expect != p.expect) return fail("expect", r.expect, p.expect);
    return true;
}

// a stream with this header: "\\\n", the pad byte and a payload of as many bytes as the header's codes need (or pay_bytes, with the pad byte diff)
std::vector<uint8_t> stream_of(const std::string &hdr, std::mt19937_64 &rng, int diff = -1, long pay_bytes = -1) {
    std::vector<HuffSym> syms; std::string msg;
    unsigned long long bits = 8;
    if (parse_header((const uint8_t *)hdr.data(), hdr.size(), syms, msg) && syms.size() >= 2) {
        HuffTree tree; HuffCodes codes;
        std::vector<HuffSym> work = syms;
        bool small = true;
        for (const HuffSym &s : syms) small = small && s.freq <= 65536;
        if (small && build_tree(work, tree, msg) && assign_codes(tree, codes, msg, false)) bits = std::max<unsigned long long>(codes.total_bits, 1);
    }
    std::vector<uint8_t> out(hdr.begin(), hdr.end());
    out.push_back(0x5C); out.push_back(0x0A);
    out.push_back((uint8_t)(diff >= 0 ? diff : (int)((8 - bits % 8) % 8)));
    const size_t pay = pay_bytes >= 0 ? (size_t)pay_bytes : (size_t)std::min<unsigned long long>((bits + 7) / 8, 20000);
    for (size_t i = 0; i < pay; i++) out.push_back((uint8_t)rng());
    return out;
}

std::string own_header(const std::vector<uint32_t> &runes, const std::vector<uint32_t> &counts) {
    std::vector<HuffSym> syms;
    for (size_t k = 0; k < runes.size(); k++) syms.push_back({runes[k], counts[k]});
    std::sort(syms.begin(), syms.end(), [](const HuffSym &x, const HuffSym &y) { return x.rune < y.rune; });
    std::string hdr;
    emit_header(syms, hdr);
    return hdr;
}

std::string entry(const std::string &count, uint32_t r) {
    std::string e = count + "|";
    if (r == 10) return e + "\\n";
    uint8_t b[4];
    const int k = go_encode_rune(r, b);
    e.append((const char *)b, (size_t)k);
    return e;
}

uint32_t rune_of_width(std::mt19937_64 &rng, int width) {
    for (;;) {
        const uint32_t r = width == 1 ? (uint32_t)(rng() % 0x80) : width == 2 ? 0x80 + (uint32_t)(rng() % (0x800 - 0x80))
                         : width == 3 ? 0x800 + (uint32_t)(rng() % (0x10000 - 0x800)) : 0x10000 + (uint32_t)(rng() % (0x110000 - 0x10000));
        if ((r >= 0xD800 && r < 0xE000) || r == 0x5C) continue;            // ('\\' is placed on purpose: last, the header moves it)
        return r;
    }
}
// a runes of all four widths, one >= 0x80 among them
std::vector<uint32_t> distinct_runes(std::mt19937_64 &rng, uint32_t a) {
    std::set<uint32_t> seen;
    std::vector<uint32_t> out;
    for (int w = 4; w >= 1 && out.size() < a; w--) { const uint32_t r = rune_of_width(rng, a == 2 && w == 4 ? 2 : w); if (seen.insert(r).second) out.push_back(r); }
    while (out.size() < a) { const uint32_t r = rune_of_width(rng, 1 + (int)(rng() % 4)); if (seen.insert(r).second) out.push_back(r); }
    return out;
}

// `slots <rune>...`: the first slot of each rune (decimal, 0x... or 0...) in the encoder's and the decoder's table, one a line
int slots_mode(int argc, char **argv) {
    for (int k = 2; k < argc; k++) printf("%u\n", plan_rune_hash((uint32_t)strtoul(argv[k], nullptr, 0)));
    return 0;
}

// `plan <file>`: the file holds streams as records of a 4-byte little-endian length and that many bytes.  One line a stream: the verdict
// of parse_rune_plan_serial, the distinct runes, the deepest code, and the lanes (zeros where the stream is refused before they are known)
int plan_mode(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { printf("cannot open %s\n", path); return 1; }
    for (;;) {
        uint8_t len[4];
        const size_t got = fread(len, 1, 4, f);
        if (got == 0) break;
        const size_t n = (size_t)len[0] | (size_t)len[1] << 8 | (size_t)len[2] << 16 | (size_t)len[3] << 24;
        if (got != 4 || n > (1u << 24)) { printf("a record's length is cut or beyond 16 MiB\n"); fclose(f); return 1; }
        uint8_t *exact = (uint8_t *)malloc(n ? n : 1);                  // (exactly n bytes: the sanitizer sees a read at or behind n)
        if (fread(exact, 1, n, f) != n) { printf("a record of %zu bytes is cut\n", n); free(exact); fclose(f); return 1; }
        HuffRunePlan plan;
        ParseRuneInfo info;
        parse_rune_plan_serial(exact, n, plan, &info);
        free(exact);
        printf("%s a %u deepest %u S %u T %u\n", plan.b.verdict == PARSE_PLANNED ? "taken" : "refused", info.a, info.deepest, info.S, info.T);
    }
    fclose(f);
    return 0;
}
}  // namespace

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "slots")) return slots_mode(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "plan")) {
        if (argc != 3) { printf("usage: plan <file>\n"); return 2; }
        return plan_mode(argv[2]);
    }
    const long long n_random = argc > 1 ? atoll(argv[1]) : 3000;
    std::mt19937_64 rng(20261019);
    auto run = [&](const std::string &hdr, const char *what, int want = -1) { const std::vector<uint8_t> s = stream_of(hdr, rng); return check(s, s.size(), what, want); };
    // ---- the library's own headers: 2, 3, 255, 256 and 257 runes of widths 1 to 4
    for (uint32_t a : {2u, 3u, 255u, 256u, 257u}) {
        const int want = a <= 256 ? 0 : 1;
        const std::vector<uint32_t> r = distinct_runes(rng, a);
        std::vector<uint32_t> c(a);
        for (uint32_t v : {1u, 2u, 7u, 13u}) { if (v * a * 4 > OUT_MAX) continue; for (auto &x : c) x = v; if (!run(own_header(r, c), "equal counts", want)) return 1; }
        for (auto &x : c) x = 1 + (uint32_t)(rng() % 3);
        if (!run(own_header(r, c), "three counts", want)) return 1;
        for (int t = 0; t < 20; t++) {
            const uint32_t range = t % 2 ? 4 : std::max(1u, OUT_MAX / 4 / a);
            for (auto &x : c) x = 1 + (uint32_t)(rng() % range);
            if (!run(own_header(r, c), "random counts", want)) return 1;
        }
    }
    {   // counts 1..256 over one-byte and two-byte runes promise more than the class holds; counts 1..100 fit
        std::vector<uint32_t> r, c;
        for (uint32_t k = 0; k < 256; k++) { r.push_back(k < 100 ? 0x100 + k : 0x4E00 + k); c.push_back(k + 1); }
        if (!run(own_header(r, c), "256 counts 1..256", 1)) return 1;
        r.resize(100); c.resize(100);
        if (!run(own_header(r, c), "100 counts 1..100", 0)) return 1;
    }
    for (uint32_t a = 2; a <= 21; a++) {                                // Fibonacci counts: the deepest codes 16 KiB of output allow
        std::vector<uint32_t> c;
        unsigned long long f0 = 1, f1 = 1, sum = 0;
        while (c.size() < a) { c.push_back((uint32_t)f0); sum += f0; const unsigned long long t = f0 + f1; f0 = f1; f1 = t; }
        std::vector<uint32_t> r;
        for (uint32_t k = 0; k < a; k++) r.push_back(k == 0 ? 0xE9 : 'a' + k);
        if (!run(own_header(r, c), "fibonacci", sum + 1 <= OUT_MAX ? 0 : 1)) return 1;
    }
    const uint32_t deepest_own = g_deepest;
    // ---- foreign headers
    {
        const std::vector<uint32_t> runes = distinct_runes(rng, 24);
        std::vector<std::string> es;
        for (uint32_t k = 0; k < 24; k++) es.push_back(entry(std::to_string(1 + k * k), runes[k]));
        auto join = [](const std::vector<std::string> &v, const char *between = "") { std::string s; for (const auto &e : v) { s += e; s += between; } return s; };
        std::vector<std::string> desc(es.rbegin(), es.rend());
        if (!run(join(desc), "descending order", 0)) return 1;
        for (int t = 0; t < 20; t++) { std::vector<std::string> sh = es; std::shuffle(sh.begin(), sh.end(), rng); if (!run(join(sh), "shuffled order", 0)) return 1; }
        { std::vector<std::string> sh = es; sh.insert(sh.begin() + 3, entry("777", runes[9])); sh.push_back(entry("5", runes[12])); if (!run(join(sh), "a duplicate entry", 0)) return 1; }
        if (!run(join(es, "xyz \t"), "letters between the entries", 0)) return 1;
        if (!run(entry("12", 'a') + entry("0", 0xE9) + entry("4", 0x4E2D), "a zero count", 0)) return 1;
        if (!run("|a" + entry("3", 0xE9) + entry("4", 'c'), "an empty count", 0)) return 1;
        if (!run(entry("0", 'a') + entry("0", 0xE9) + entry("0", 0x1F600) + entry("9", 'd'), "zero counts that tie", 0)) return 1;
        if (!run(entry("0", 'a') + entry("0", 0xE9), "only zero counts", 1)) return 1;
        if (!run("3|\\n4||15|\\6|77|9" + entry("2", 0xE9), "newline, |, backslash and digits as symbols", 0)) return 1;
        if (!run(entry("2", 0xE9) + "3|\\x4|a", "a backslash that is the symbol", 0)) return 1;
        // an invalid byte and a literal EF BF BD are the same rune: the later entry counts
        if (!run("3|a5|\xFF" "7|\xEF\xBF\xBD", "an invalid byte, then U+FFFD", 0)) return 1;
        if (!run("3|a7|\xEF\xBF\xBD" "5|\x80", "U+FFFD, then a lone continuation byte", 0)) return 1;
        if (!run("3|a5|\xED\xA0\x80", "a surrogate's bytes", 0)) return 1;
        if (!run("3|a5|\xC0\xAF", "an over-long form", 0)) return 1;
        if (!run("3|a5|\xF4\x90\x80\x80", "beyond U+10FFFF", 0)) return 1;
        if (!run("3|a5|\xE4\xB8", "a rune the separator cuts", 0)) return 1;
        if (!run("3|a5|\xF0\x9F\x98", "a four-byte rune the separator cuts", 0)) return 1;
        if (!run("5|\xC3\xA9" "3|a", "the rune first", 0)) return 1;
        if (!run(entry("16384", 'a') + entry("0", 0xE9), "a count of 16384", 0)) return 1;
        if (!run(entry("16385", 'a') + entry("0", 0xE9), "a count of 16385", 1)) return 1;
        if (!run(entry("12345678901234567890", 'a') + entry("3", 0xE9), "a count of 20 digits", 1)) return 1;
        if (!run(entry("99999", 0xE9) + entry("2", 'b') + entry("5", 0xE9), "a large count that a later entry replaces", 0)) return 1;
        if (!run(entry("8192", 0xE9) + entry("0", 'b'), "expect 16384", 0)) return 1;
        if (!run(entry("8192", 0xE9) + entry("1", 'b'), "expect 16385", 1)) return 1;
        if (!run(entry("4096", 0x1F600) + entry("0", 0x1F601), "4096 runes of width 4 and a zero", 0)) return 1;
        if (!run(entry("2048", 0x1F600) + entry("2048", 0x1F601), "two runes of width 4, 16384 bytes from 512", 0)) return 1;
    }
    // ---- refused
    {
        if (!run("3|a4|", "a header that ends behind |", 1)) return 1;
        if (!run("3|\xC3\xA9" "4|", "a header that ends behind |, a rune before", 1)) return 1;
        if (!run("3|\xC3\xA9" "4|\\", "a header that ends behind |\\", 1)) return 1;
        if (!run("3|a4|b12|c", "a pure byte alphabet", 1)) return 1;
        if (!run("3|\xC3\xA9", "one distinct rune", 1)) return 1;
        if (!run("3|\xC3\xA9" "4|\xC3\xA9", "one distinct rune twice", 1)) return 1;
        if (!run("", "no entries", 1)) return 1;
        { std::vector<uint8_t> s = stream_of("3|a4|\xC3\xA9", rng); s[8] = 'x'; if (!check(s, s.size(), "no separator", 1)) return 1; }
        { std::vector<uint8_t> d = stream_of("3|a4|\xC3\xA9", rng, 16, 2); if (!check(d, d.size(), "a pad byte that leaves no code bit", 1)) return 1; }
        { std::vector<uint8_t> d = stream_of("3|a4|\xC3\xA9", rng, 15, 2); if (!check(d, d.size(), "a pad byte that leaves one", 0)) return 1; }
        { std::vector<uint8_t> d = stream_of("3|a4|\xC3\xA9", rng, 0, 0); if (!check(d, d.size(), "no payload byte", 1)) return 1; }
        { std::vector<uint8_t> d = stream_of("|a|\xC3\xA9", rng, 0, 3); if (!check(d, 7, "n = 7", 1) || !check(d, 8, "n = 8: sep + 4 > n", 1) || !check(d, 9, "n = 9: counts of 0", 1)) return 1; }
        { std::vector<uint8_t> d = stream_of("9|a1|\xC3\xA9", rng, 0, PARSE_RUNE_PAY_MAX); if (!check(d, d.size(), "a payload of the lanes' bits", 0)) return 1; }
        { std::vector<uint8_t> d = stream_of("9|a1|\xC3\xA9", rng, 0, PARSE_RUNE_PAY_MAX + 1); if (!check(d, d.size(), "more code bits than the lanes hold", 1)) return 1; }
        { std::vector<uint8_t> d = stream_of("9|a1|\xC3\xA9", rng, 0, STREAM_MAX); if (!check(d, STREAM_MAX + 1, "n above the class's stream", 1)) return 1; }
    }
    // ---- the separator at the last scanned position, one before it and one behind it
    for (int at = -1; at <= 1; at++) {
        std::string h;
        for (int k = 0; h.size() + 32 < SCAN_MAX; k++) h += entry("1", 0x4E00 + (uint32_t)(k % 200)) + "      ";
        h.resize((size_t)((long)SCAN_MAX - 2 + at), ' ');
        if (!run(h, at < 0 ? "the separator before the last scanned position" : at == 0 ? "the separator at the last scanned position" : "the separator one behind it", at <= 0 ? 0 : 1)) return 1;
    }
    // ---- what lies behind n must not be seen: the bytes that would complete a cut rune, a separator, digits, a whole valid tail
    {
        const std::vector<uint8_t> good = stream_of("3|a4|\xE4\xB8\xAD" "12|c", rng);
        const std::vector<uint8_t> tail = stream_of("9|x8|\xC3\xA9", rng);
        for (size_t cut = 8; cut <= good.size(); cut++) {
            std::vector<uint8_t> b(good.begin(), good.begin() + (long)cut);
            b.insert(b.end(), tail.begin(), tail.end());
            Ref alone;
            ref_plan(good.data(), cut, alone);
            if (!check(b, cut, "a stream with a tail behind n", alone.verdict)) return 1;
        }
    }
    // ---- random alphabets: entries in any order, duplicates, zero counts, invalid bytes
    for (long long t = 0; t < n_random; t++) {
        const uint32_t shape = (uint32_t)(rng() % 5);
        const uint32_t a = shape == 0 ? 2 + (uint32_t)(rng() % 4) : shape == 1 ? 256 : 2 + (uint32_t)(rng() % 255);
        const std::vector<uint32_t> r = distinct_runes(rng, a);
        std::vector<std::string> es;
        const uint32_t range = shape == 2 ? 4 : shape == 3 ? 24 : std::max(1u, OUT_MAX / 3 / a);
        for (uint32_t k = 0; k < a; k++) es.push_back(entry(std::to_string(rng() % 16 == 0 ? 0 : 1 + (uint32_t)(rng() % range)), r[k]));
        if (rng() % 3 == 0) es.push_back(entry(std::to_string(1 + rng() % 9), r[rng() % a]));
        if (rng() % 4 == 0) es.push_back(std::string("2|") + (char)(0x80 + rng() % 0x80));
        if (rng() % 4 == 0) es.push_back("3|\\");
        std::shuffle(es.begin(), es.end(), rng);
        std::string h;
        for (const auto &e : es) h += e;
        if (!h.empty() && h.back() == '\\') h += "1|z";                  // (a header must not end behind "|\\")
        if (!run(h, "random alphabet")) return 1;
    }
    const char alphabet[] = "0123456789|\\n\nab \x80\xC3\xA9\xE4\xB8\xAD\xF0\x9F\x98\x80\xEF\xBF\xBD\xED";
    for (long long t = 0; t < n_random; t++) {
        std::string h;
        const size_t len = 1 + rng() % 40;
        for (size_t i = 0; i < len; i++) h.push_back(alphabet[rng() % (sizeof alphabet - 1)]);
        std::vector<uint8_t> s = stream_of(h, rng, (int)(rng() % 12), (long)(rng() % 40));
        const size_t n = rng() % 4 ? s.size() : rng() % (s.size() + 1);
        if (!check(s, n, "random header")) return 1;
    }
    if (g_planned < n_random / 2) { printf("only %lld of %lld streams were planned\n", g_planned, g_streams); return 1; }
    printf("ok %lld planned %lld deepest %u\n", g_streams, g_planned, deepest_own);
    return 0;
}
