// huff_parse_test.cpp -- the device-side plan of a Huffman stream (raisin_amd/csrc/huff_parse_small.h: what k_huff_dev_plan runs) against
// the host's parse_header + build_tree + assign_codes (huff_host.cpp), restated as small_dec_plan's fields (huff_small.hip).  Built and
// run by tests/test_huff_parse_host.py.  Prints "ok <streams> stricter <k> deepest <bits>" and exits 0, or the first disagreement and 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "huff_host.h"
#include "huff_parse_small.h"

using namespace rsn;

namespace {
constexpr uint32_t HDR_MAX = PARSE_HDR_MAX, DEC_STREAM_MAX = PARSE_STREAM_MAX, SMALL_MAX = PARSE_OUT_MAX, DEC_K = PARSE_K_MAX;
// the two lane shapes (huff_small_body.h: DL, HB_S_MAX; huff_mid.hip: HM_DL, HM_S_MAX)
constexpr uint32_t LANES[2] = {256, 960}, S_MAX[2] = {512, 480};

struct Ref {
    int verdict = 1;
    uint16_t child[256] = {0};
    uint32_t root = 0, n_child = 0, K = 0, flat = 0, A0 = 0, p0 = 0, end = 0, pay_words = 0, max_len = 0;
    unsigned long long expect = 0;
    bool count_at_limit = false;       // the host accepted a count of exactly 65536: the one case the device is stricter in
};

// small_dec_plan (huff_small.hip), without S and T
void ref_plan(const uint8_t *in, size_t n, Ref &r) {
    r = Ref();
    if (n < 8 || n > DEC_STREAM_MAX) return;
    size_t sep = (size_t)-1;
    for (size_t i = 0; i + 1 < std::min<size_t>(n, HDR_MAX + 8); i++) if (in[i] == 0x5C && in[i + 1] == 0x0A) { sep = i; break; }
    if (sep == (size_t)-1 || sep + 4 > n) return;
    std::vector<HuffSym> syms; std::string msg;
    if (!parse_header(in, sep, syms, msg) || syms.size() < 2 || syms.size() > 128) return;
    unsigned long long expect = 0;
    for (const HuffSym &sy : syms) { if (sy.rune >= 0x80 || sy.freq > SMALL_MAX) return; expect += sy.freq; if (sy.freq == SMALL_MAX) r.count_at_limit = true; }
    if (expect == 0 || expect > SMALL_MAX) return;
    const size_t pay = sep + 3, sn = n - sep - 2;
    const unsigned diff = in[sep + 2];
    const unsigned long long nbits = (unsigned long long)(sn - 1) * 8;
    if (diff >= nbits) return;
    HuffTree tree; HuffCodes codes;
    if (!build_tree(syms, tree, msg) || !assign_codes(tree, codes, msg, false)) return;
    if (codes.max_len > 32 || codes.max_len == 0) return;
    const uint32_t A = tree.n_leaves;
    const size_t n_int = tree.freq.size() - A;
    for (size_t i = 0; i < n_int; i++) {
        const int32_t kids[2] = {tree.left[A + i], tree.right[A + i]};
        for (int b = 0; b < 2; b++) r.child[2 * i + b] = tree.is_leaf(kids[b]) ? (uint16_t)(0x8000u | tree.rune[kids[b]]) : (uint16_t)(kids[b] - (int32_t)A);
    }
    r.root = (uint32_t)(tree.root - (int32_t)A);
    r.A0 = (uint32_t)(pay & ~(size_t)3);
    r.pay_words = (uint32_t)((n - r.A0 + 3) / 4) + 8;
    r.p0 = (uint32_t)(8 * (pay - r.A0) + diff);
    r.end = (uint32_t)(8 * (pay - r.A0) + nbits);
    r.K = std::min<unsigned>(codes.max_len, DEC_K); r.n_child = (uint32_t)(2 * n_int);
    r.flat = codes.min_len == codes.max_len ? codes.max_len : 0u;
    r.max_len = codes.max_len;
    r.expect = expect;
    r.verdict = 0;
}

long long g_streams = 0, g_stricter = 0, g_planned = 0;
uint32_t g_deepest = 0;
bool g_sep_mod[4] = {false, false, false, false};

// in[0, n) is the stream; the buffer may hold more behind it (cap bytes), which neither side may look at -- the subject gets a copy of n
// bytes in an allocation of exactly n bytes, so that the sanitizer sees a read behind it
bool check(const std::vector<uint8_t> &buf, size_t n, const char *what, int want_verdict = -1) {
    g_streams++;
    Ref r;
    ref_plan(buf.data(), n, r);
    uint8_t *exact = (uint8_t *)malloc(n ? n : 1);
    memcpy(exact, buf.data(), n);
    HuffDevPlan plan;
    parse_plan_serial(exact, n, plan);
    const HuffDevBounds &p = plan.b;
    free(exact);
    auto fail = [&](const char *part, unsigned long long a, unsigned long long b) { printf("%s (n = %zu): %s differs: host %llu, plan %llu\n", what, n, part, a, b); return false; };
    if (want_verdict >= 0 && r.verdict != want_verdict) return fail("the host's verdict from the expected one", (unsigned long long)r.verdict, (unsigned long long)want_verdict);
    if (r.verdict == 0 && r.count_at_limit) {                          // the device is stricter here, and only here
        if (p.verdict != PARSE_NOT_MINE) return fail("verdict on a count of 65536", 1, p.verdict);
        g_stricter++;
        return true;
    }
    if ((uint32_t)r.verdict != p.verdict) return fail("verdict", (unsigned long long)r.verdict, p.verdict);
    if (r.verdict != 0) return true;
    g_planned++;
    g_deepest = std::max(g_deepest, r.max_len);
    g_sep_mod[(r.p0 >> 3) & 3] = true;                                    // (the payload's first byte from A0, while the pad byte is below 8)
    if (r.root != p.root) return fail("root", r.root, p.root);
    if (r.n_child != p.n_child) return fail("n_child", r.n_child, p.n_child);
    for (uint32_t i = 0; i < 256; i++) if (r.child[i] != plan.child[i]) return fail("child", r.child[i], plan.child[i]);
    if (r.K != p.K) return fail("K", r.K, p.K);
    if (r.flat != p.flat) return fail("flat", r.flat, p.flat);
    if (r.A0 != p.A0) return fail("A0", r.A0, p.A0);
    if (r.p0 != p.p0) return fail("p0", r.p0, p.p0);
    if (r.end != p.end) return fail("end", r.end, p.end);
    if (r.pay_words != p.pay_words) return fail("pay_words", r.pay_words, p.pay_words);
    if (r.expect != p.expect) return fail("expect", r.expect, p.expect);
    for (int k = 0; k < 2; k++) {                                      // S and T as small_dec_plan computes them, both lane shapes
        const uint32_t span = r.end - r.p0;
        const uint32_t S = std::max<uint32_t>(64, (uint32_t)(((span + LANES[k] - 1) / LANES[k] + 31) / 32 * 32));
        const uint32_t T = (span + S - 1) / S;
        uint32_t s2 = 0, t2 = 0;
        const bool ok = parse_lanes(p.end - p.p0, LANES[k], S_MAX[k], &s2, &t2);
        if (ok != (S <= S_MAX[k])) return fail("the lanes' verdict", S <= S_MAX[k], ok);
        if (S != s2) return fail("S", S, s2);
        if (T != t2) return fail("T", T, t2);
    }
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
    const size_t pay = pay_bytes >= 0 ? (size_t)pay_bytes : (size_t)std::min<unsigned long long>((bits + 7) / 8, 60000);
    for (size_t i = 0; i < pay; i++) out.push_back((uint8_t)rng());
    return out;
}

std::string own_header(const std::vector<uint32_t> &bytes, const std::vector<uint32_t> &counts) {
    std::vector<HuffSym> syms;
    for (size_t k = 0; k < bytes.size(); k++) syms.push_back({bytes[k], counts[k]});
    std::sort(syms.begin(), syms.end(), [](const HuffSym &x, const HuffSym &y) { return x.rune < y.rune; });
    std::string hdr;
    emit_header(syms, hdr);
    return hdr;
}

std::string entry(const std::string &count, uint32_t b) {
    std::string e = count + "|";
    if (b == 10) e += "\\n"; else e.push_back((char)b);
    return e;
}
}  // namespace

int main(int argc, char **argv) {
    const long long n_random = argc > 1 ? atoll(argv[1]) : 20000;
    std::mt19937_64 rng(20261018);
    auto pick_bytes = [&](uint32_t a, int kind) {                      // kind 1: '\\' the highest; 2: the header's own syntax among the symbols
        std::vector<uint32_t> all;
        for (uint32_t b = 0; b < (kind == 1 ? 0x5Cu : 128u); b++) all.push_back(b);
        std::shuffle(all.begin(), all.end(), rng);
        std::vector<uint32_t> out;
        if (kind == 1) out.push_back(0x5C);
        if (kind == 2) for (uint32_t b : {10u, (uint32_t)'|', 0x5Cu, (uint32_t)'0', (uint32_t)'7', (uint32_t)'9'}) if (out.size() < a) out.push_back(b);
        for (uint32_t b : all) if (out.size() < a && std::find(out.begin(), out.end(), b) == out.end()) out.push_back(b);
        return out;
    };
    auto run = [&](const std::string &hdr, const char *what, int want = -1) { const std::vector<uint8_t> s = stream_of(hdr, rng); return check(s, s.size(), what, want); };
    const uint32_t sizes[] = {2, 3, 64, 127, 128};
    // ---- the library's own headers
    for (uint32_t a : sizes) {
        for (int kind = 0; kind < 3; kind++) {
            if (kind == 1 && a > 0x5D) continue;
            const std::vector<uint32_t> bytes = pick_bytes(a, kind);
            std::vector<uint32_t> c(a);
            for (uint32_t v : {1u, 2u, 7u, 100u, 512u}) { if (v * a > SMALL_MAX) continue; for (auto &x : c) x = v; if (!run(own_header(bytes, c), "equal counts", 0)) return 1; }
            for (uint32_t k = 0; k < a; k++) c[k] = 1 + (uint32_t)(rng() % 3);
            if (!run(own_header(bytes, c), "three counts", 0)) return 1;
            for (uint32_t k = 0; k < a; k++) c[k] = (k % 2) ? 5 : 2 + (k % 3);
            if (!run(own_header(bytes, c), "duplicate counts", 0)) return 1;
            for (uint32_t k = 0; k < a; k++) c[k] = 1u << (k % 9);
            if (!run(own_header(bytes, c), "powers of two", 0)) return 1;
            for (int t = 0; t < 40; t++) {
                const uint32_t range = t % 2 ? 4 : SMALL_MAX / a;
                for (auto &x : c) x = 1 + (uint32_t)(rng() % range);
                if (!run(own_header(bytes, c), "random", 0)) return 1;
            }
        }
    }
    // Fibonacci counts: the deepest codes 64 KiB of output allow (1, 1, 1, 2, 3, 5, ... forces a chain; so does 1, 1, 2, 3, ...)
    for (int lead = 0; lead < 2; lead++) {
        for (uint32_t a = 2; a <= 26; a++) {
            std::vector<uint32_t> c;
            if (lead) c.push_back(1);
            unsigned long long f0 = 1, f1 = 1, sum = lead;
            while (c.size() < a) { c.push_back((uint32_t)f0); sum += f0; const unsigned long long t = f0 + f1; f0 = f1; f1 = t; }
            if (sum > SMALL_MAX) break;
            if (!run(own_header(pick_bytes(a, 0), c), "fibonacci", 0)) return 1;
        }
    }
    const uint32_t deepest_own = g_deepest;
    // ---- every separator position mod 4: the counts' digits move the header's length
    for (uint32_t a = 2; a <= 9; a++) {
        std::vector<uint32_t> c(a, 3);
        for (uint32_t k = 0; k < 4; k++) { c[0] = k == 0 ? 3 : k == 1 ? 30 : k == 2 ? 300 : 3000; if (!run(own_header(pick_bytes(a, 0), c), "separator residues", 0)) return 1; }
    }
    for (int k = 0; k < 4; k++) if (!g_sep_mod[k]) { printf("no planned stream with a payload at residue %d mod 4\n", k); return 1; }
    // ---- foreign headers
    {
        const std::vector<uint32_t> bytes = pick_bytes(20, 2);
        std::vector<std::string> es;
        for (uint32_t k = 0; k < 20; k++) es.push_back(entry(std::to_string(1 + k * k), bytes[k]));
        auto join = [](const std::vector<std::string> &v, const char *between = "") { std::string s; for (const auto &e : v) { s += e; s += between; } return s; };
        std::vector<std::string> desc(es.rbegin(), es.rend());
        // ('\\' must not come last: the reference reads behind the header there, and so refuses the host -- see the malformed ones)
        auto bs_not_last = [&](std::vector<std::string> v) { const std::string bs = entry(std::to_string(1 + 2 * 2), 0x5C); auto it = std::find(v.begin(), v.end(), bs); if (it != v.end() && it + 1 == v.end()) std::swap(*it, v.front()); return v; };
        if (!run(join(bs_not_last(desc)), "descending order", 0)) return 1;
        for (int t = 0; t < 20; t++) { std::vector<std::string> sh = es; std::shuffle(sh.begin(), sh.end(), rng); if (!run(join(bs_not_last(sh)), "shuffled order", 0)) return 1; }
        { std::vector<std::string> sh = es; sh.insert(sh.begin() + 3, entry("777", bytes[9])); sh.push_back(entry("5", bytes[12])); if (!run(join(sh), "a repeated entry", 0)) return 1; }
        if (!run(entry("0007", 'a') + entry("00", 'b') + entry("010", 'c'), "leading zeros", 0)) return 1;
        if (!run(join(es, "xyz \t"), "letters between the entries", 0)) return 1;
        if (!run(entry("12", 'a') + entry("0", 'b') + entry("4", 'c'), "a zero count", 0)) return 1;
        if (!run("|a" + entry("3", 'b') + entry("4", 'c'), "an empty count", 0)) return 1;
        if (!run(entry("0", 'a') + entry("0", 'b') + entry("0", 'c') + entry("9", 'd'), "zero counts that tie", 0)) return 1;
        if (!run(entry("12345678901234567890", 'a') + entry("3", 'b'), "a count of 20 digits", 1)) return 1;
        if (!run(entry("65536", 'a') + entry("3", 'b'), "a count of 65536 and another", 1)) return 1;
        const long long before = g_stricter;
        if (!run(entry("65536", 'a') + entry("0", 'b'), "a count of 65536 alone", 0)) return 1;
        if (!run(entry("0", 'z') + entry("65536", 'q') + entry("0", 'b'), "a count of 65536 between zeros", 0)) return 1;
        if (g_stricter - before != 2) { printf("the two constructed counts of 65536 are not where the device is stricter: %lld\n", g_stricter - before); return 1; }
        if (!run(entry("65535", 'a') + entry("1", 'b'), "a count of 65535", 0)) return 1;
        if (!run(entry("70000", 'a') + entry("2", 'b') + entry("5", 'a'), "a large count that a later entry replaces", 0)) return 1;
        // a '|' and a digit as the symbols behind a '|', a "\\" that is not "\\n"
        if (!run("3||4|15|\\6|7", "syntax bytes as symbols", 0)) return 1;
        if (!run("3|\\x4|a", "a backslash that is the symbol", 0)) return 1;
    }
    // ---- malformed
    {
        std::vector<uint8_t> s = stream_of("3|a4|b", rng);
        std::vector<uint8_t> nosep = s; nosep[6] = 'x';
        if (!check(nosep, nosep.size(), "no separator", 1)) return 1;
        std::string longh;                                                // 1200 bytes of entries: the separator lies behind HDR_MAX + 8
        for (int k = 0; longh.size() < PARSE_SCAN_MAX; k++) longh += entry("1", 'a' + k % 20) + "      ";
        if (!run(longh, "the separator behind the scanned bytes", 1)) return 1;
        std::string at_edge;                                              // ... and exactly at the last position that is looked at
        for (int k = 0; at_edge.size() + 16 < PARSE_SCAN_MAX; k++) at_edge += entry("1", 'a' + k % 20) + "      ";
        at_edge.resize(PARSE_SCAN_MAX - 2, ' ');
        if (!run(at_edge, "the separator at the last scanned position", 0)) return 1;
        if (!run(at_edge + " ", "the separator one behind it", 1)) return 1;
        if (!run("3|a4|", "a header that ends in |", 1)) return 1;
        if (!run("3|a4|\\", "a header that ends in |\\", 1)) return 1;
        if (!run("3|a4|\xC3\xA9", "a symbol >= 0x80", 1)) return 1;
        if (!run("3|a4|\x80", "a lone continuation byte", 1)) return 1;
        if (!run("3|a", "one distinct symbol", 1)) return 1;
        if (!run("3|a4|a", "one distinct symbol twice", 1)) return 1;
        if (!run("", "no entries", 1)) return 1;
        { std::string h; for (uint32_t b = 0; b < 128; b++) h += entry("1", b); h += entry("1", 200); if (!run(h, "129 symbols", 1)) return 1; }
        { std::vector<uint8_t> d = stream_of("3|a4|b", rng, 16, 2); if (!check(d, d.size(), "diff >= nbits", 1)) return 1; }
        { std::vector<uint8_t> d = stream_of("3|a4|b", rng, 15, 2); if (!check(d, d.size(), "diff = nbits - 1", 0)) return 1; }
        { std::vector<uint8_t> d = stream_of("3|a4|b", rng, 0, 0); if (!check(d, d.size(), "no payload byte", 1)) return 1; }
        { std::vector<uint8_t> d = stream_of("1|a1|b", rng, 0, 0); if (d.size() != 9) return 1; if (!check(d, 7, "n = 7", 1) || !check(d, 8, "n = 8: sep + 4 > n", 1)) return 1; }
        { std::vector<uint8_t> d = stream_of("|a|b", rng, 0, 1); if (d.size() != 8) return 1; if (!check(d, 8, "n = 8 with a payload byte, counts of 0", 1)) return 1; }
        { std::vector<uint8_t> d = stream_of("|a1|b", rng, 0, 1); d.resize(8); d[4] = 0x5C; d[5] = 0x0A; d[6] = 0; if (!check(d, 8, "n = 8, one count", 1)) return 1; }
        { std::vector<uint8_t> d = {'1', '|', 'a', '|', 'b', 0x5C, 0x0A, 0, 0x55}; if (!check(d, 8, "n = 8: the payload byte is behind n", 1) || !check(d, 9, "n = 9", 0)) return 1; }
        { std::vector<uint8_t> d = stream_of("30000|a30000|b", rng, 0, DEC_STREAM_MAX); if (!check(d, DEC_STREAM_MAX, "n = DEC_STREAM_MAX", 0) || !check(d, DEC_STREAM_MAX + 1, "n above DEC_STREAM_MAX", 1)) return 1; }
    }
    // ---- what lies behind n must not be seen: a separator, digits, a whole valid tail
    {
        const std::vector<uint8_t> good = stream_of("3|a4|b12|c", rng);
        const std::vector<uint8_t> tail = stream_of("9|x8|y", rng);
        for (size_t cut = 8; cut <= good.size(); cut++) {
            std::vector<uint8_t> b(good.begin(), good.begin() + (long)cut);
            b.insert(b.end(), tail.begin(), tail.end());
            Ref alone;
            ref_plan(good.data(), cut, alone);
            if (!check(b, cut, "a stream with a separator and digits behind n", alone.verdict)) return 1;
        }
        std::vector<uint8_t> b = {'3', '|', 'a', '4', '|', 'b', '1', '2', 0x5C, 0x0A, 0, 0xFF, 0xFF};   // n = 8 ends in digits; behind it a separator
        if (!check(b, 8, "digits at the end, a separator behind n", 1) || !check(b, 9, "the separator cut in two", 1)) return 1;
    }
    // ---- random headers in the scan's own alphabet, and mutations of good streams
    const char alphabet[] = "0123456789|\\n\nab \x80";
    for (long long t = 0; t < n_random; t++) {
        std::string h;
        const size_t len = 1 + rng() % 40;
        for (size_t i = 0; i < len; i++) h.push_back(alphabet[rng() % (sizeof alphabet - 1)]);
        std::vector<uint8_t> s = stream_of(h, rng, (int)(rng() % 12), (long)(rng() % 40));
        const size_t n = rng() % 4 ? s.size() : rng() % (s.size() + 1);
        if (!check(s, n, "random header")) return 1;
    }
    if (g_stricter != 2) { printf("the device was stricter on %lld streams, 2 were constructed\n", g_stricter); return 1; }
    printf("ok %lld planned %lld stricter %lld deepest %u\n", g_streams, g_planned, g_stricter, deepest_own);
    return 0;
}
