// huff_rune_mid_plan_test.cpp -- the rune planner (raisin_amd/csrc/huff_plan_rune.h) at the counts of the mid-size rune class
// (k_huff_mid_rune_enc, huff_rune_mid.hip): a count up to 65535, a sum up to PLAN_RUNE_MID_COUNT_MAX = 65536, where tests/huff_rune_plan_test.cpp
// stays within 16384.  Leaf order, tree, codes and header against the host's build_tree / assign_codes / emit_header (huff_host.cpp), the
// planner driven as the kernel drives it: symbols in no particular order, a rank per symbol, the entries at a scan of their lengths.
// Built and run by tests/test_huff_rune_mid_host.py.  Prints "ok <alphabets>" and exits 0, or prints the first disagreement and exits 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "huff_host.h"
#include "huff_plan_rune.h"

using namespace rsn;

namespace {
struct Arr {
    uint32_t v[512];
    Arr() { memset(v, 0, sizeof v); }
    uint32_t get(uint32_t i) const { return v[i]; }
    void set(uint32_t i, uint32_t x) { v[i] = x; }
};

long long g_alphabets = 0;

// runes[k] occurs counts[k] times; the last rune by value is >= 0x80 (a member of the class holds one).  want_depth: the longest code, 0: any
bool check(const std::vector<uint32_t> &runes, const std::vector<uint32_t> &counts, const char *what, std::mt19937_64 &rng, uint32_t want_depth = 0) {
    g_alphabets++;
    std::vector<HuffSym> syms;
    for (size_t k = 0; k < runes.size(); k++) syms.push_back({runes[k], counts[k]});
    std::shuffle(syms.begin(), syms.end(), rng);                          // the kernel's symbols come in hash-slot order
    const uint32_t a = (uint32_t)syms.size();
    auto fail = [&](const char *part, uint32_t at) { printf("%s: %s differs (a = %u, at %u)\n", what, part, a, at); return false; };
    unsigned long long sum = 0;
    for (const HuffSym &s : syms) { sum += s.freq; if (s.freq < 1 || s.freq > 65535) return fail("the test's own count", (uint32_t)s.freq); }
    if (a < 2 || a > PLAN_RUNE_SYMS_MAX || sum > PLAN_RUNE_MID_COUNT_MAX) return fail("the test's own alphabet", a);
    // ---- the host (the single call's sequence)
    std::vector<HuffSym> by_rune = syms;
    std::sort(by_rune.begin(), by_rune.end(), [](const HuffSym &x, const HuffSym &y) { return x.rune < y.rune; });
    for (uint32_t i = 0; i + 1 < a; i++) if (by_rune[i].rune == by_rune[i + 1].rune) return fail("the test's own runes (distinct)", i);
    if (by_rune.back().rune < 0x80) return fail("the test's own alphabet (a rune >= 0x80)", a);
    std::string hdr, msg;
    emit_header(by_rune, hdr);
    HuffTree tree; HuffCodes codes;
    std::vector<HuffSym> work = by_rune;
    if (!build_tree(work, tree, msg) || !assign_codes(tree, codes, msg, false)) { printf("%s: host failed: %s\n", what, msg.c_str()); return false; }
    // ---- the planner, as the kernel runs it
    uint32_t rune[256], cnt[256], lf[256], lsym[256], ord[256];
    for (uint32_t t = 0; t < a; t++) { rune[t] = syms[t].rune; cnt[t] = (uint32_t)syms[t].freq; }
    for (uint32_t t = 0; t < a; t++) {
        uint32_t lr, rr;
        plan_rune_ranks(rune, cnt, a, t, &lr, &rr);
        if (lr >= a || rr >= a) return fail("rank range", t);
        lf[lr] = cnt[t]; lsym[lr] = t; ord[rr] = t;
    }
    Arr heap, kids, code;
    for (uint32_t i = 0; i < a; i++) heap.set(i, plan_item<PLAN_RUNE_IDB>(lf[i], i));
    const uint32_t root = plan_tree<PLAN_RUNE_IDB>(a, heap, kids);
    plan_codes<PLAN_RUNE_IDB>(a, root, kids, code);
    uint32_t max_len = 0, total_bits = 0;
    for (uint32_t i = 0; i < a; i++) { const uint32_t l = code.get(i) >> 24; max_len = l > max_len ? l : max_len; total_bits += lf[i] * l; }
    uint8_t ph[4096];
    uint32_t at = 0;
    for (uint32_t q = 0; q < a; q++) {
        const uint32_t t = ord[q], len = plan_rune_entry_len(cnt[t], rune[t]);
        if (plan_rune_entry(cnt[t], rune[t], ph + at) != len) return fail("entry length against the entry", q);
        at += len;
    }
    ph[at++] = '\\'; ph[at++] = '\n'; ph[at++] = (uint8_t)((8 - total_bits % 8) % 8);
    const uint32_t H = at;
    // ---- compare
    for (uint32_t i = 0; i < a; i++) if (tree.rune[i] != rune[lsym[i]] || tree.freq[i] != lf[i]) return fail("leaf order", i);
    if ((uint32_t)tree.root != root) return fail("root", root);
    for (uint32_t id = a; id <= root; id++) {
        const uint32_t k = kids.get(id - a);
        if ((uint32_t)tree.left[id] != (k & 0x1FF) || (uint32_t)tree.right[id] != (k >> 9)) return fail("tree", id);
    }
    for (uint32_t i = 0; i < a; i++) {
        const uint32_t c = code.get(i);
        if ((c >> 24) != codes.len[i] || (c & 0xFFFFFFu) != (uint32_t)(codes.code[i] & 0xFFFFFFu)) return fail("code", i);
    }
    if (max_len != codes.max_len) return fail("max length", max_len);
    if (max_len > 22) return fail("a code beyond 22 bits within 65536", max_len);
    if (want_depth && max_len != want_depth) return fail("the depth the table was built for", max_len);
    if (total_bits != codes.total_bits) return fail("total bits", total_bits);
    if (total_bits > 8 * sum) return fail("payload beyond a byte a rune", total_bits);   // (huff_rune_mid_select.h: the image's bound)
    std::string want = hdr;
    want += "\\\n";
    want.push_back((char)((8 - codes.total_bits % 8) % 8));
    if (H != want.size()) return fail("header length", H);
    for (uint32_t i = 0; i < H; i++) if (ph[i] != (uint8_t)want[i]) return fail("header byte", i);
    if (H > 256 * 10 + 3) return fail("header beyond its maximum", H);
    return true;
}

// `a` distinct runes of 1, 2, 3 and 4 bytes in turn (never a surrogate), from a base that varies
std::vector<uint32_t> runes_of_all_widths(uint32_t a, uint32_t seed) {
    static const uint32_t base[4] = {0x21, 0xC0, 0x1000, 0x10400};
    std::vector<uint32_t> out;
    for (uint32_t i = 0; i < a; i++) out.push_back(base[i % 4] + (i / 4) + (i % 4 ? 3 * seed : 0));   // (64 ASCII runes at most: 0x21 .. 0x60)
    return out;
}
}  // namespace

int main() {
    std::mt19937_64 rng(20261020);
    // ---- one count of 65534 beside a count of 1 and of 2: the largest sums, and the largest count the class can meet (two runes at least)
    if (!check({'a', 0xE9}, {65534, 1}, "65534, 1", rng, 1)) return 1;
    if (!check({0xE9, 'a'}, {65534, 2}, "65534, 2", rng, 1)) return 1;
    if (!check({' ', 0xE9, 0x20AC}, {65533, 1, 2}, "65533, 1, 2", rng, 2)) return 1;
    if (!check({0x1D11E, 0xE9}, {65535, 1}, "65535, 1", rng, 1)) return 1;
    // ---- the counts next to the 16 KiB class's limit and the digit boundaries
    if (!check({'e', 0xE9, 0x20AC, 0x1D11E}, {16384, 16385, 9999, 10000}, "16384, 16385, 9999, 10000", rng)) return 1;
    if (!check({'\n', '|', '\\', 0xFFFD, '9'}, {9999, 10000, 16385, 16384, 99}, "digit boundaries at the special entries", rng)) return 1;
    if (!check({'0', 0x80, 0x7FF}, {10000, 9999, 45537}, "three counts that fill 65536", rng)) return 1;
    // ---- 256 equal counts of 256: the sum is 65536, ties are broken by rune, the code is the flat 8 bits
    for (uint32_t seed = 0; seed < 3; seed++)
        if (!check(runes_of_all_widths(256, seed), std::vector<uint32_t>(256, 256), "256 equal counts of 256", rng, 8)) return 1;
    // ---- Fibonacci counts over runes >= 0x80: F1..F22 (no ties: a chain, 21 bits, sum 46367), and the table of 23 leaves whose ties the
    // reference's heap breaks towards the chain (1 1 1 3 4 7 11 ...: sum 64074, the deepest code 22 bits -- the deepest within 65536)
    {
        std::vector<uint32_t> r, c;
        uint32_t f0 = 1, f1 = 1;
        for (uint32_t k = 0; k < 22; k++) { r.push_back(0x100 + 7 * k); c.push_back(f0); const uint32_t t = f0 + f1; f0 = f1; f1 = t; }
        if (!check(r, c, "fibonacci 22", rng, 21)) return 1;
        const std::vector<uint32_t> deep = {1, 1, 1, 3, 4, 7, 11, 18, 29, 47, 76, 123, 199, 322, 521, 843, 1364, 2207, 3571, 5778, 9348, 15126, 24474};
        r.push_back(0x100 + 7 * 22);
        if (!check(r, deep, "23 leaves, 22 bits", rng, 22)) return 1;
        std::vector<uint32_t> wide;                                      // the same counts over 2-, 3- and 4-byte runes
        for (uint32_t k = 0; k < 23; k++) wide.push_back(k % 3 == 0 ? 0x100 + k : k % 3 == 1 ? 0x1000 + k : 0x10400 + k);
        std::sort(wide.begin(), wide.end());
        if (!check(wide, deep, "23 leaves, 22 bits, all widths", rng, 22)) return 1;
    }
    // ---- ties in count broken by rune across 1-, 2-, 3- and 4-byte runes: groups of equal counts, each group of every width
    for (uint32_t seed = 0; seed < 8; seed++) {
        const uint32_t a = 8 + 31 * seed;                                    // 8 .. 225
        std::vector<uint32_t> c(a);
        for (uint32_t i = 0; i < a; i++) c[i] = 1 + (i / 8) * (65536 / (a * (a / 8 + 1)));   // eight runes share a count; the sum stays within 65536
        if (!check(runes_of_all_widths(a, seed), c, "ties across the widths", rng)) return 1;
    }
    if (!check({0x7F, 0x80, 0x7FF, 0x800, 0xFFFF, 0x10000, 0x10FFFF, 'A'}, {8192, 8192, 8192, 8192, 8192, 8192, 8192, 8192}, "eight equal counts at the width edges", rng, 3)) return 1;
    // ---- random alphabets whose counts sum to 16385 .. 65536
    for (int t = 0; t < 400; t++) {
        const uint32_t a = t % 4 == 0 ? 256 : 2 + (uint32_t)(rng() % 255), total = 16385 + (uint32_t)(rng() % (65536 - 16385 + 1));
        std::vector<uint32_t> c(a, 1);
        uint32_t left = total - a;
        for (uint32_t i = 0; i + 1 < a && left; i++) { const uint32_t add = std::min<uint32_t>((uint32_t)(rng() % (left + 1)) >> (rng() % 8), 65534); c[i] += add; left -= add; }
        c[a - 1] += std::min<uint32_t>(left, 65534);
        std::shuffle(c.begin(), c.end(), rng);
        if (!check(runes_of_all_widths(a, (uint32_t)t % 5), c, "random", rng)) return 1;
    }
    printf("ok %lld\n", g_alphabets);
    return 0;
}
