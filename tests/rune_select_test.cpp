// Which members the two classes behind the rows take (raisin_amd/csrc/huff_rune_select.h; codecs.h: BehindClass) as plain host code: the
// rune encoder's rune_class_members and the rune decoder's candidates / planned / leave -- one below the minimum takes none and all join
// `rest`, exactly the minimum is taken in sorted order, the remainder keeps its order, and members over the size limit never count
// towards the minimum.  Prints the number of checks it made.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "huff_rune_select.h"

using namespace rsn;
using Idx = std::vector<size_t>;

static unsigned long long checks = 0;
#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        checks++;                                                                                    \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

static void test_encoder() {
    const size_t MIN = HUFF_RUNE_GROUP_MIN;
    std::map<size_t, size_t> lens;
    auto len = [&](size_t i) { return lens[i]; };
    // one below the minimum: none is taken, all join rest behind what it held, sorted
    {
        Idx runes, rest = {900, 7};
        for (size_t k = 0; k + 1 < MIN; k++) { runes.push_back(100 - 3 * k); lens[100 - 3 * k] = 25; }
        Idx want = runes;
        std::sort(want.begin(), want.end());
        CHECK(rune_class_members(runes, rest, len) == 0);
        CHECK(rest.size() == 2 + want.size() && rest[0] == 900 && rest[1] == 7 && Idx(rest.begin() + 2, rest.end()) == want);
    }
    // exactly the minimum: taken in sorted order, rest untouched
    {
        Idx runes, rest = {900, 7};
        for (size_t k = 0; k < MIN; k++) { runes.push_back(100 - 3 * k); lens[100 - 3 * k] = k % 2 ? 2 : HUFF_RUNE_IN_MAX; }
        Idx want = runes;
        std::sort(want.begin(), want.end());
        CHECK(rune_class_members(runes, rest, len) == MIN);
        CHECK(runes == want && (rest == Idx{900, 7}));
    }
    // the minimum of them and members over the limit between them: the taken at the front in sorted order, the remainder to rest in its (sorted) order
    {
        Idx runes, rest = {900};
        for (size_t k = 0; k < MIN; k++) { runes.push_back(200 - 2 * k); lens[200 - 2 * k] = 300; }
        for (size_t i : {201, 175, 1, 189}) { runes.push_back(i); lens[i] = i == 1 ? 1 : HUFF_RUNE_IN_MAX + 1; }
        CHECK(rune_class_members(runes, rest, len) == MIN);
        for (size_t k = 0; k < MIN; k++) CHECK(runes[k] == 200 - 2 * (MIN - 1 - k));
        CHECK((rest == Idx{900, 1, 175, 189, 201}));
    }
    // members over the limit never count towards the minimum: MIN - 1 that fit and many that do not -- none is taken
    {
        Idx runes, rest;
        for (size_t k = 0; k + 1 < MIN; k++) { runes.push_back(2 * k); lens[2 * k] = 16384; }
        for (size_t k = 0; k < 2 * MIN; k++) { runes.push_back(2 * k + 1); lens[2 * k + 1] = 16385; }
        const Idx want = runes;                                                             // (those that fit in order, then the others in order: the flows sort rest)
        CHECK(rune_class_members(runes, rest, len) == 0);
        CHECK(rest == want);
    }
    { Idx runes, rest = {3}; CHECK(rune_class_members(runes, rest, len) == 0 && (rest == Idx{3})); }
}

static HuffDevSummary planned(uint32_t expect, uint32_t A0 = 12, uint32_t span = 64) { return HuffDevSummary{PARSE_PLANNED, A0, span, expect}; }

static void test_decoder() {
    const size_t MIN = HUFF_RUNE_DEC_GROUP_MIN;
    auto len = [](size_t) { return (size_t)100; };
    // a summary the class takes: planned, A0 a multiple of 4 inside the stream, 1 to HUFF_RUNE_OUT_MAX bytes from at most HUFF_RUNE_PAY_MAX of payload
    CHECK(rune_dec_summary_ok(planned(1), 100) && rune_dec_summary_ok(planned(HUFF_RUNE_OUT_MAX, 100, 8 * HUFF_RUNE_PAY_MAX), 100));
    CHECK(!rune_dec_summary_ok(planned(0), 100) && !rune_dec_summary_ok(planned(HUFF_RUNE_OUT_MAX + 1), 100));
    CHECK(!rune_dec_summary_ok(planned(5, 10), 100) && !rune_dec_summary_ok(planned(5, 104), 100) && !rune_dec_summary_ok(planned(5, 12, 8 * HUFF_RUNE_PAY_MAX + 1), 100));
    CHECK(!rune_dec_summary_ok(HuffDevSummary{PARSE_NOT_MINE, 12, 64, 5}, 100));
    // the candidates: one below the minimum -- none; the minimum -- sorted, whatever rest's order; those that may not be planned never count
    Idx rest;
    for (size_t k = 0; k < MIN + 4; k++) rest.push_back(3 * ((7 * k) % (MIN + 4)));            // a permutation of 0, 3, 6, ...
    auto small = [&](size_t lim) { return [lim](size_t i) { return i < lim; }; };
    CHECK(rune_dec_candidates(rest, small(3 * (MIN - 1))).empty());
    Idx cand = rune_dec_candidates(rest, small(3 * MIN));
    CHECK(cand.size() == MIN);
    for (size_t k = 0; k < MIN; k++) CHECK(cand[k] == 3 * k);
    CHECK(rune_dec_candidates(Idx(rest.begin(), rest.begin() + MIN - 1), small(1000)).empty());
    // planned, among the first k candidates only, in order, with what each promises
    cand = rune_dec_candidates(rest, small(1000));
    CHECK(cand.size() == MIN + 4);
    std::vector<HuffDevSummary> sums;
    for (size_t q = 0; q < cand.size(); q++) sums.push_back(q == 2 || q == 9 ? HuffDevSummary{PARSE_NOT_MINE, 0, 0, 0} : planned(10 + (uint32_t)q));
    Idx idx; std::vector<uint32_t> expect;
    rune_dec_planned(cand, 5, sums.data(), len, idx, expect);
    CHECK((idx == Idx{0, 3, 9, 12}) && (expect == std::vector<uint32_t>{10, 11, 13, 14}));
    idx.clear(); expect.clear();
    rune_dec_planned(cand, cand.size(), sums.data(), len, idx, expect);
    CHECK(idx.size() == MIN + 2 && expect.size() == idx.size() && std::is_sorted(idx.begin(), idx.end()));
    // still the minimum: they leave rest, which is sorted afterwards and keeps the others
    Idx left = rest;
    CHECK(rune_dec_leave(left, idx) && idx.size() == MIN + 2);
    CHECK((left == Idx{6, 27}));
    // exactly the minimum leaves too; one fewer: none is taken, idx is emptied, rest stays as it came
    Idx exact(idx.begin(), idx.begin() + MIN), below(idx.begin(), idx.begin() + MIN - 1);
    left = rest;
    CHECK(rune_dec_leave(left, exact) && exact.size() == MIN && left.size() == 4 && std::is_sorted(left.begin(), left.end()));
    left = rest;
    CHECK(!rune_dec_leave(left, below) && below.empty() && left == rest);
}

int main() {
    test_encoder();
    test_decoder();
    std::printf("rune select: %llu checks\n", checks);
    return 0;
}
