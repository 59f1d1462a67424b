// huff_rune_plan_test.cpp -- the grouped rune encoder's planner (raisin_amd/csrc/huff_plan_rune.h, with huff_plan_small.h's tree and codes
// at 9 bits of node id) against the host's Go-exact leaf order, tree, codes and header (huff_host.cpp).  The planner is driven the way
// k_huff_batch_rune_enc drives it: symbols in no particular order, a rank per symbol, the entries at a scan of their lengths.
// Built and run by tests/test_huff_rune_plan_host.py.  Prints "ok <alphabets>" and exits 0, or prints the first disagreement and exits 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
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
constexpr uint32_t TOTAL_MAX = 16384;

// a rune Go's decoding can yield, of the given UTF-8 width
uint32_t rune_of_width(std::mt19937_64 &rng, int width) {
    for (;;) {
        const uint32_t r = width == 1 ? (uint32_t)(rng() % 0x80) : width == 2 ? 0x80 + (uint32_t)(rng() % (0x800 - 0x80))
                         : width == 3 ? 0x800 + (uint32_t)(rng() % (0x10000 - 0x800)) : 0x10000 + (uint32_t)(rng() % (0x110000 - 0x10000));
        if (r >= 0xD800 && r < 0xE000) continue;
        return r;
    }
}

// syms: 2 to 256 distinct runes in any order, counts >= 1 (a member's sum to at most 16384; the planner's words hold sums below 2^22)
bool check(std::vector<HuffSym> syms, const char *what) {
    g_alphabets++;
    const uint32_t a = (uint32_t)syms.size();
    auto fail = [&](const char *part, uint32_t at) { printf("%s: %s differs (a = %u, at %u)\n", what, part, a, at); return false; };
    unsigned long long sum = 0;
    for (const HuffSym &s : syms) sum += s.freq;
    if (a < 2 || a > PLAN_RUNE_SYMS_MAX || sum >= (1u << 23) >> 1) return fail("the test's own alphabet", a);
    // ---- the host (the single call's sequence)
    std::vector<HuffSym> by_rune = syms;
    std::sort(by_rune.begin(), by_rune.end(), [](const HuffSym &x, const HuffSym &y) { return x.rune < y.rune; });
    std::string hdr, msg;
    emit_header(by_rune, hdr);
    HuffTree tree; HuffCodes codes;
    std::vector<HuffSym> work = by_rune;
    if (!build_tree(work, tree, msg) || !assign_codes(tree, codes, msg, false)) { printf("%s: host failed: %s\n", what, msg.c_str()); return false; }
    // the rule the planner leaves out: '\\' is moved only when it would be last, and with a rune >= 0x80 present it never is
    const bool has_high = by_rune.back().rune >= 0x80;
    if (has_high && by_rune.back().rune == 0x5C) return fail("backslash last with a rune >= 0x80 present", 0);
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
    if (sum <= TOTAL_MAX && max_len > 24) return fail("a code beyond 24 bits below 16 KiB", max_len);
    if (total_bits != codes.total_bits) return fail("total bits", total_bits);
    if (has_high) {                                                      // (the planner's header is the host's only where the rule cannot fire)
        std::string want = hdr;
        want += "\\\n";
        want.push_back((char)((8 - codes.total_bits % 8) % 8));
        if (H != want.size()) return fail("header length", H);
        for (uint32_t i = 0; i < H; i++) if (ph[i] != (uint8_t)want[i]) return fail("header byte", i);
    }
    if (H > 256 * 10 + 3) return fail("header beyond its maximum", H);
    return true;
}

bool table_of(const std::vector<uint32_t> &runes, const std::vector<uint32_t> &counts, const char *what, std::mt19937_64 &rng) {
    std::vector<HuffSym> syms;
    for (size_t k = 0; k < runes.size(); k++) syms.push_back({runes[k], counts[k]});
    std::shuffle(syms.begin(), syms.end(), rng);                         // the kernel's symbols come in hash-slot order
    return check(syms, what);
}

std::vector<uint32_t> distinct_runes(std::mt19937_64 &rng, uint32_t a, bool all_widths) {
    std::set<uint32_t> seen;
    std::vector<uint32_t> out;
    if (all_widths) for (int w = 4; w >= 1 && out.size() < a; w--) { const uint32_t r = rune_of_width(rng, w); if (seen.insert(r).second) out.push_back(r); }
    while (out.size() < a) { const uint32_t r = rune_of_width(rng, 1 + (int)(rng() % 4)); if (seen.insert(r).second) out.push_back(r); }
    return out;
}
}  // namespace

int main(int argc, char **argv) {
    const long long n_random = argc > 1 ? atoll(argv[1]) : 2000;
    std::mt19937_64 rng(20261019);
    // ---- two symbols
    if (!table_of({'a', 0xE9}, {1, 1}, "a, e-acute", rng)) return 1;
    if (!table_of({'a', 0xE9}, {3, 16381}, "a, e-acute, full", rng)) return 1;
    // ---- exactly 256 symbols, all counts equal: ties are broken by rune, and the heap is the whole story
    for (uint32_t v : {1u, 2u, 7u, 64u}) {
        const std::vector<uint32_t> r = distinct_runes(rng, 256, true);
        if (!table_of(r, std::vector<uint32_t>(256, v), "256 equal counts", rng)) return 1;
    }
    for (uint32_t a = 2; a <= 256; a++) {                                // every alphabet size, equal counts and three counts
        const std::vector<uint32_t> r = distinct_runes(rng, a, a >= 4);
        if (!table_of(r, std::vector<uint32_t>(a, 1 + a % 5), "equal counts", rng)) return 1;
        std::vector<uint32_t> c(a);
        for (auto &x : c) x = 1 + (uint32_t)(rng() % 3);
        if (!table_of(r, c, "three counts", rng)) return 1;
    }
    // ---- 256 symbols with counts 1..256 (their sum, 32896, is more than a member holds: the planner's words take it), and two that a member can hold
    {
        const std::vector<uint32_t> r = distinct_runes(rng, 256, true);
        std::vector<uint32_t> c(256);
        for (uint32_t k = 0; k < 256; k++) c[k] = k + 1;
        if (!table_of(r, c, "256 counts 1..256", rng)) return 1;
        for (uint32_t k = 0; k < 256; k++) c[k] = k / 2 + 1;
        if (!table_of(r, c, "256 counts 1,1,2,2..128,128", rng)) return 1;
        const std::vector<uint32_t> r2 = distinct_runes(rng, 180, true);  // 1 + 2 + .. + 180 = 16290
        std::vector<uint32_t> c2(180);
        for (uint32_t k = 0; k < 180; k++) c2[k] = k + 1;
        if (!table_of(r2, c2, "180 counts 1..180", rng)) return 1;
    }
    // ---- Fibonacci counts over 20 runes, sum 17710 > 16384: over 19 (sum 10945) and over 20 with the last cut to fit -- the longest codes
    {
        std::vector<uint32_t> c;
        uint32_t f0 = 1, f1 = 1, sum = 0;
        for (int k = 0; k < 19; k++) { c.push_back(f0); sum += f0; const uint32_t t = f0 + f1; f0 = f1; f1 = t; }
        if (!table_of(distinct_runes(rng, 19, true), c, "fibonacci 19", rng)) return 1;
        c.push_back(TOTAL_MAX - sum);
        if (!table_of(distinct_runes(rng, 20, true), c, "fibonacci 20", rng)) return 1;
    }
    // ---- the bytes the header treats specially, with U+FFFD and a 4-byte rune
    if (!table_of({'\n', '|', '0', '7', '9', '\\', 0xFFFD, 0x1D11E}, {3, 10, 100, 1000, 12, 5, 7, 1}, "special entries", rng)) return 1;
    if (!table_of({'\\', 0xFFFD}, {9, 10}, "backslash, U+FFFD", rng)) return 1;
    if (!table_of({'\n', '\\', 0x80}, {16000, 1, 383}, "newline, backslash, U+0080", rng)) return 1;
    if (!table_of({0x7F, 0x80, 0x7FF, 0x800, 0xFFFF, 0x10000, 0x10FFFF}, {1, 2, 3, 4, 5, 6, 7}, "width edges", rng)) return 1;
    // ---- random alphabets of 2 to 256 runes drawn from all four widths, random counts, total <= 16384
    for (long long t = 0; t < n_random; t++) {
        const uint32_t shape = (uint32_t)(rng() % 5);
        const uint32_t a = shape == 0 ? 2 + (uint32_t)(rng() % 4) : shape == 1 ? 256 : 2 + (uint32_t)(rng() % 255);
        std::vector<uint32_t> r = distinct_runes(rng, a, a >= 4);
        if (rng() % 4 == 0) { bool has = false; for (uint32_t x : r) has = has || x == 0x5C; if (!has) r[0] = 0x5C; }
        bool high = false;
        for (uint32_t x : r) high = high || x >= 0x80;
        if (!high) r[a - 1] = 0xFFFD;                                       // (a member of the class holds a rune >= 0x80)
        std::vector<uint32_t> c(a);
        const uint32_t range = shape == 2 ? 4 : shape == 3 ? 64 : TOTAL_MAX / a;
        for (auto &x : c) x = 1 + (uint32_t)(rng() % (range ? range : 1));
        if (shape == 4) { uint32_t left = TOTAL_MAX - a; for (auto &x : c) { const uint32_t add = left ? (uint32_t)(rng() % (left + 1)) >> (rng() % 8) : 0; x = 1 + add; left -= add; } }
        if (!table_of(r, c, "random", rng)) return 1;
    }
    printf("ok %lld\n", g_alphabets);
    return 0;
}
