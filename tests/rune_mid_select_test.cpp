// Which members the mid-size rune encoder takes out of the RUNES pool (raisin_amd/csrc/huff_rune_mid_select.h; codecs.h: BehindClass), and
// what the 16 KiB class (huff_rune_select.h: rune_class_members) then makes of the pool it is left -- the two offers in the order
// batch_classes lists them -- against a brute-force statement of the rules: a member is the mid class's when its length is in
// (HUFF_RUNE_IN_MAX, HUFF_RUNE_MID_IN_MAX] and the pool holds at least HUFF_RUNE_MID_GROUP_MIN such members; it is the 16 KiB class's when
// its length is in [2, HUFF_RUNE_IN_MAX] and the pool holds at least HUFF_RUNE_GROUP_MIN such; every other member reaches `rest`, once,
// in index order, behind what `rest` held.  Prints the number of checks it made.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

#include "huff_rune_mid_select.h"

using namespace rsn;
using Idx = std::vector<size_t>;

static unsigned long long checks = 0;
#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        checks++;                                                                                    \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

static const size_t MID = HUFF_RUNE_MID_GROUP_MIN, SMALL = HUFF_RUNE_GROUP_MIN;

// the rules, member by member
struct Want { Idx mid, small, rest; };
static Want brute(const Idx &pool, const std::map<size_t, size_t> &lens, const Idx &rest0) {
    auto is_mid = [&](size_t i) { const size_t n = lens.at(i); return n >= 16385 && n <= 65536; };
    auto is_small = [&](size_t i) { const size_t n = lens.at(i); return n >= 2 && n <= 16384; };
    size_t n_mid = 0, n_small = 0;
    for (size_t i : pool) { n_mid += is_mid(i); n_small += is_small(i); }
    Idx sorted = pool;
    std::sort(sorted.begin(), sorted.end());
    Want w;
    w.rest = rest0;
    for (size_t i : sorted) {
        if (is_mid(i) && n_mid >= MID) w.mid.push_back(i);
        else if (is_small(i) && n_small >= SMALL) w.small.push_back(i);
    }
    // rest: what the 16 KiB class does not keep, those it could take first when there are too few of them (rune_class_members' own order:
    // tests/rune_select_test.cpp; the flows sort `rest` afterwards), so as a SET and sorted
    for (size_t i : sorted) if (!std::binary_search(w.mid.begin(), w.mid.end(), i) && !std::binary_search(w.small.begin(), w.small.end(), i)) w.rest.push_back(i);
    return w;
}

// both offers over one pool, as batch_front and layer_batch_run make them
static void both(Idx pool, const std::map<size_t, size_t> &lens, const Idx &rest0 = {}) {
    const Want w = brute(pool, lens, rest0);
    auto len = [&](size_t i) { return lens.at(i); };
    const size_t before = pool.size();
    Idx rest = rest0;
    const Idx mid = rune_mid_class_members(pool, len);
    CHECK(mid == w.mid);                                                  // in index order
    CHECK(pool.size() + mid.size() == before && std::is_sorted(pool.begin(), pool.end()));   // the others stay, sorted
    for (size_t i : mid) CHECK(!std::binary_search(pool.begin(), pool.end(), i));
    CHECK(rest == rest0);                                                 // (nothing of this class's reaches rest by selection)
    const size_t kept = rune_class_members(pool, rest, len);
    pool.resize(kept);
    CHECK(pool == w.small);
    CHECK(Idx(rest.begin(), rest.begin() + rest0.size()) == rest0);
    Idx tail(rest.begin() + rest0.size(), rest.end()), want_tail(w.rest.begin() + rest0.size(), w.rest.end());
    std::sort(tail.begin(), tail.end());
    CHECK(tail == want_tail);                                             // the remainder reaches rest once (equal sizes, equal sorted contents)
    CHECK(mid.size() + kept + tail.size() == before);
}

int main() {
    std::map<size_t, size_t> lens;
    // ---- the lengths at the class's edges, the minimum of each: 16384 is not taken, 16385 and 65536 are, 65537 is not
    for (size_t n : {(size_t)16384, (size_t)16385, (size_t)65536, (size_t)65537}) {
        Idx pool;
        lens.clear();
        for (size_t k = 0; k < MID; k++) { pool.push_back(3 * k + 1); lens[3 * k + 1] = n; }
        Idx p = pool;
        const Idx got = rune_mid_class_members(p, [&](size_t i) { return lens.at(i); });
        const bool taken = n == 16385 || n == 65536;
        CHECK(got == (taken ? pool : Idx{}));
        CHECK(p == (taken ? Idx{} : pool));
        both(pool, lens, {900, 7});
    }
    // ---- exactly the minimum and one fewer, at mixed lengths of the class
    for (size_t count : {MID, MID - 1}) {
        Idx pool;
        lens.clear();
        for (size_t k = 0; k < count; k++) { pool.push_back(100 - 3 * k); lens[100 - 3 * k] = k % 3 == 0 ? 16385 : k % 3 == 1 ? 65536 : 40000; }
        Idx p = pool, sorted = pool;
        std::sort(sorted.begin(), sorted.end());
        const Idx got = rune_mid_class_members(p, [&](size_t i) { return lens.at(i); });
        CHECK(got == (count == MID ? sorted : Idx{}));
        CHECK(p == (count == MID ? Idx{} : sorted));                      // fewer: none is taken, all stay
        both(pool, lens, {5});
    }
    // ---- members outside the class never count towards its minimum
    {
        Idx pool;
        lens.clear();
        for (size_t k = 0; k + 1 < MID; k++) { pool.push_back(2 * k); lens[2 * k] = 20000; }
        for (size_t k = 0; k < 2 * MID; k++) { pool.push_back(2 * k + 1); lens[2 * k + 1] = k % 2 ? 16384 : 65537; }
        Idx p = pool;
        CHECK(rune_mid_class_members(p, [&](size_t i) { return lens.at(i); }).empty() && p.size() == pool.size());
        both(pool, lens);
    }
    // ---- a pool of both classes on both sides of both minimums, with members neither takes (1 byte, 65537, 70000), unsorted
    std::mt19937_64 rng(20261020);
    for (size_t n_mid : {MID - 1, MID, MID + 3})
        for (size_t n_small : {SMALL - 1, SMALL, SMALL + 5}) {
            Idx pool;
            lens.clear();
            size_t next = 0;
            auto add = [&](size_t count, std::vector<size_t> sizes) { for (size_t k = 0; k < count; k++) { next += 1 + rng() % 4; pool.push_back(next); lens[next] = sizes[k % sizes.size()]; } };
            add(n_mid, {16385, 65536, 32768, 49153});
            add(n_small, {2, 16384, 25, 1000});
            add(4, {1, 65537, 70000, 262144});
            std::shuffle(pool.begin(), pool.end(), rng);
            both(pool, lens, {100000, 3});
        }
    // ---- random unsorted pools around the edges
    for (int t = 0; t < 300; t++) {
        Idx pool;
        lens.clear();
        const size_t count = rng() % 60;
        for (size_t k = 0; k < count; k++) {
            const size_t i = 2 * k + 1;
            static const size_t sizes[] = {1, 2, 300, 16383, 16384, 16385, 16386, 30000, 65535, 65536, 65537, 100000};
            pool.push_back(i); lens[i] = sizes[rng() % (t % 3 == 0 ? 12 : t % 3 == 1 ? 6 : 9)];
        }
        std::shuffle(pool.begin(), pool.end(), rng);
        both(pool, lens, {1000});
    }
    { Idx pool; CHECK(rune_mid_class_members(pool, [](size_t) { return (size_t)20000; }).empty() && pool.empty()); }
    // ---- the slot holds the longest stream, in whole words
    for (uint32_t n : {2u, 255u, 256u, 16385u, 65535u, 65536u}) CHECK(huff_rune_mid_stream_max(n) + 3 <= huff_rune_mid_enc_out_slot(n) && huff_rune_mid_enc_out_slot(n) % 16 == 0);
    std::printf("rune mid select: %llu checks\n", checks);
    return 0;
}
