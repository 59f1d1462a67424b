// huff_plan_test.cpp -- the grouped Huffman encoder's planner (raisin_amd/csrc/huff_plan_small.h) against the host's Go-exact tree,
// codes and header (huff_host.cpp), on tie-heavy tables and on random ones.  Built and run by tests/test_huff_plan_host.py.
// Prints "ok <tables>" and exits 0, or prints the first disagreement and exits 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "huff_host.h"
#include "huff_plan_small.h"

using namespace rsn;

namespace {
struct Arr {
    uint32_t v[256];
    Arr() { memset(v, 0, sizeof v); }
    uint32_t get(uint32_t i) const { return v[i]; }
    void set(uint32_t i, uint32_t x) { v[i] = x; }
};

long long g_tables = 0;

// cnt[128]: at least two non-zero counts, each below PLAN_COUNT_LIMIT
bool check(const uint32_t *cnt, const char *what) {
    g_tables++;
    // ---- the host (huff_small_compress's sequence)
    std::vector<HuffSym> syms;
    for (uint32_t b = 0; b < 128; b++) if (cnt[b]) syms.push_back({b, cnt[b]});
    std::string hdr, msg;
    emit_header(syms, hdr);
    HuffTree tree; HuffCodes codes;
    std::vector<HuffSym> work = syms;
    if (!build_tree(work, tree, msg) || !assign_codes(tree, codes, msg, false)) { printf("%s: host failed: %s\n", what, msg.c_str()); return false; }
    const uint32_t a = (uint32_t)syms.size();
    // ---- the planner
    uint32_t leaf[128], lf[128];
    for (uint32_t b = 0; b < 128; b++) if (cnt[b]) { const uint32_t r = plan_leaf_rank(cnt, b); leaf[r] = b; lf[r] = cnt[b]; }
    Arr heap, kids, code;
    for (uint32_t i = 0; i < a; i++) heap.set(i, plan_item(lf[i], i));
    const uint32_t root = plan_tree(a, heap, kids);
    plan_codes(a, root, kids, code);
    uint32_t max_len = 0, total_bits = 0;
    for (uint32_t i = 0; i < a; i++) { const uint32_t l = code.get(i) >> 24; max_len = l > max_len ? l : max_len; total_bits += lf[i] * l; }
    uint8_t ph[2048];
    const uint32_t H = plan_header(cnt, total_bits, ph);
    // ---- compare
    auto fail = [&](const char *part, uint32_t at) { printf("%s: %s differs (a = %u, at %u)\n", what, part, a, at); return false; };
    for (uint32_t i = 0; i < a; i++) if (tree.rune[i] != leaf[i] || tree.freq[i] != lf[i]) return fail("leaf order", i);
    if ((uint32_t)tree.root != root) return fail("root", root);
    for (uint32_t id = a; id <= root; id++) {
        const uint32_t k = kids.get(id - a);
        if ((uint32_t)tree.left[id] != (k & 0xFF) || (uint32_t)tree.right[id] != (k >> 8)) return fail("tree", id);
    }
    for (uint32_t i = 0; i < a; i++) {
        const uint32_t c = code.get(i);
        if ((c >> 24) != codes.len[i] || (c & 0xFFFFFFu) != (uint32_t)(codes.code[i] & 0xFFFFFFu)) return fail("code", i);
    }
    if (max_len != codes.max_len) return fail("max length", max_len);
    if (total_bits != codes.total_bits) return fail("total bits", total_bits);
    std::string want = hdr;
    want += "\\\n";
    want.push_back((char)((8 - codes.total_bits % 8) % 8));
    if (H != want.size()) return fail("header length", H);
    for (uint32_t i = 0; i < H; i++) if (ph[i] != (uint8_t)want[i]) return fail("header byte", i);
    // the kernel's pieces of the header: the entries' lengths, '\\' first
    uint32_t sum = 0;
    for (uint32_t b = 0; b < 128; b++) if (cnt[b]) sum += plan_entry_len(cnt[b], b);
    if (sum + 3 != H) return fail("entry lengths", sum);
    return true;
}

bool table_of(const std::vector<uint32_t> &bytes, const std::vector<uint32_t> &counts, const char *what) {
    uint32_t cnt[128] = {0};
    for (size_t k = 0; k < bytes.size(); k++) cnt[bytes[k]] = counts[k];
    return check(cnt, what);
}
}  // namespace

int main(int argc, char **argv) {
    const long long n_random = argc > 1 ? atoll(argv[1]) : 100000;
    std::mt19937_64 rng(20261016);
    auto pick_bytes = [&](uint32_t a, bool want_bs_last) {
        std::vector<uint32_t> all(128);
        for (uint32_t b = 0; b < 128; b++) all[b] = b;
        if (want_bs_last) all.resize(0x5C);                             // every byte below '\\', then '\\' itself
        std::shuffle(all.begin(), all.end(), rng);
        all.resize(want_bs_last ? a - 1 : a);
        if (want_bs_last) all.push_back(0x5C);
        return all;
    };
    // ---- tie-heavy tables, every alphabet size
    for (uint32_t a = 2; a <= 128; a++) {
        for (int bs = 0; bs < (a <= 0x5D ? 2 : 1); bs++) {
            const std::vector<uint32_t> bytes = pick_bytes(a, bs);
            std::vector<uint32_t> c(a);
            const uint32_t equal_at[] = {1, 2, 7, 100, 255, 16384, 65535};
            for (uint32_t v : equal_at) { for (auto &x : c) x = v; if (!table_of(bytes, c, "equal counts")) return 1; }
            for (uint32_t k = 0; k < a; k++) c[k] = 1u << (k % 16);
            if (!table_of(bytes, c, "powers of two")) return 1;
            for (uint32_t k = 0; k < a; k++) c[k] = 1u << (15 - k % 16);
            if (!table_of(bytes, c, "powers of two, descending")) return 1;
            uint32_t f0 = 1, f1 = 1;                                      // Fibonacci counts: the deepest codes (repeating past 2^16)
            for (uint32_t k = 0; k < a; k++) { c[k] = f0; const uint32_t t = f0 + f1; f0 = f1; f1 = t; if (f1 >= PLAN_COUNT_LIMIT) { f0 = 1; f1 = 1; } }
            if (!table_of(bytes, c, "fibonacci")) return 1;
            for (uint32_t k = 0; k < a; k++) c[k] = 1 + (uint32_t)(rng() % 3);
            if (!table_of(bytes, c, "three counts")) return 1;
            for (uint32_t k = 0; k < a; k++) c[k] = (k % 2) ? 5 : 2 + (k % 3);
            if (!table_of(bytes, c, "duplicate counts")) return 1;
            for (uint32_t k = 0; k < a; k++) c[k] = 16384 - (uint32_t)(rng() % 4);
            if (!table_of(bytes, c, "counts near 16 KiB")) return 1;
        }
    }
    {   // newline and '\\' together, the single-digit to five-digit counts
        if (!table_of({10, 0x5C}, {9, 10}, "newline, backslash")) return 1;
        if (!table_of({0, 10, 0x5C}, {65535, 1, 34463}, "edge bytes")) return 1;
        if (!table_of({0, 127}, {1, 65535}, "two symbols")) return 1;
    }
    // ---- random tables
    for (long long t = 0; t < n_random; t++) {
        const uint32_t shape = (uint32_t)(rng() % 6);
        const uint32_t a = shape == 0 ? 2 + (uint32_t)(rng() % 4) : shape == 1 ? 128 : 2 + (uint32_t)(rng() % 127);
        const bool bs = a <= 0x5D && rng() % 8 == 0;
        const std::vector<uint32_t> bytes = pick_bytes(a, bs);
        std::vector<uint32_t> c(a);
        const uint32_t range = shape == 2 ? 4 : shape == 3 ? 64 : shape == 4 ? 16384 : PLAN_COUNT_LIMIT - 1;
        for (auto &x : c) x = 1 + (uint32_t)(rng() % range);
        if (shape == 5) for (auto &x : c) x = 1u << (rng() % 16);
        if (!table_of(bytes, c, "random")) return 1;
    }
    printf("ok %lld\n", g_tables);
    return 0;
}
