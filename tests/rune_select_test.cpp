// Which members the two classes behind the rows take (raisin_amd/csrc/huff_rune_select.h; codecs.h: BehindClass) as plain host code: the
// rune encoder's rune_class_members and the rune decoders' candidates / planned / leave, the one selection at the rules of both classes
// (huff_parse_rune.h: ParseRuneSmall, ParseRuneMid) -- one below the minimum takes none and all join
// `rest`, exactly the minimum is taken in sorted order, the remainder keeps its order, and members over the size limit never count
// towards the minimum.  Prints the number of checks it made.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "huff_parse_rune.h"
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

// the classes' rules as numbers: what the one selection reads out of each
static_assert(ParseRuneSmall::OUT_MIN == 1 && ParseRuneSmall::OUT_MAX == 16384 && ParseRuneSmall::PAY_MAX == 18432 && ParseRuneSmall::GROUP_MIN == 16 &&
              ParseRuneSmall::len_may(0) && ParseRuneSmall::len_may(21003) && !ParseRuneSmall::len_may(21004), "the 16 KiB class");
static_assert(ParseRuneMid::OUT_MIN == 16385 && ParseRuneMid::OUT_MAX == 65536 && ParseRuneMid::PAY_MAX == 69120 && ParseRuneMid::GROUP_MIN == 16 &&
              !ParseRuneMid::len_may(515) && ParseRuneMid::len_may(516) && ParseRuneMid::len_may(71691) && !ParseRuneMid::len_may(71692), "the mid-size class");
static_assert(HUFF_RUNE_OUT_MAX == 16384 && HUFF_RUNE_PAY_MAX == 18432 && HUFF_RUNE_DEC_GROUP_MIN == 16 && HUFF_RUNE_STREAM_MAX == 21003, "the names the library knows them by");

// the three steps at the class L's rules
template <class L>
static void test_decoder() {
    const size_t MIN = L::GROUP_MIN;
    constexpr size_t N = 1000;                                                                 // a length both classes take
    CHECK(L::len_may(N));
    auto len = [](size_t) { return N; };
    auto ok = [](const HuffDevSummary &v, size_t n) { return rune_dec_summary_ok<L>(v, n); };
    // a summary the class takes: planned, A0 a multiple of 4 inside the stream, L::OUT_MIN to L::OUT_MAX bytes from at most L::PAY_MAX of payload
    CHECK(ok(planned(L::OUT_MIN), N) && ok(planned(L::OUT_MAX, N, 8 * L::PAY_MAX), N));
    CHECK(!ok(planned(L::OUT_MIN - 1), N) && !ok(planned(L::OUT_MAX + 1), N));
    CHECK(!ok(planned(L::OUT_MIN, 10), N) && !ok(planned(L::OUT_MIN, N + 4), N) && !ok(planned(L::OUT_MIN, 12, 8 * L::PAY_MAX + 1), N));
    CHECK(!ok(HuffDevSummary{PARSE_NOT_MINE, 12, 64, L::OUT_MIN}, N));
    // the candidates: one below the minimum -- none; the minimum -- sorted, whatever rest's order; those that may not be planned never count
    Idx rest;
    for (size_t k = 0; k < MIN + 4; k++) rest.push_back(3 * ((7 * k) % (MIN + 4)));            // a permutation of 0, 3, 6, ...
    auto small = [&](size_t lim) { return [lim](size_t i) { return i < lim; }; };
    CHECK(rune_dec_candidates<L>(rest, small(3 * (MIN - 1)), len).empty());
    Idx cand = rune_dec_candidates<L>(rest, small(3 * MIN), len);
    CHECK(cand.size() == MIN);
    for (size_t k = 0; k < MIN; k++) CHECK(cand[k] == 3 * k);
    CHECK(rune_dec_candidates<L>(Idx(rest.begin(), rest.begin() + MIN - 1), small(1000), len).empty());
    // ... and neither do those whose length the class does not take, whatever may() says
    auto long_from = [&](size_t lim) { return [lim](size_t i) { return i < lim ? N : (size_t)L::STREAM_MAX + 1; }; };
    CHECK(rune_dec_candidates<L>(rest, small(1000), long_from(3 * (MIN - 1))).empty());
    CHECK(rune_dec_candidates<L>(rest, small(1000), long_from(3 * MIN)) == cand);
    // planned, among the first k candidates only, in order, with what each promises
    cand = rune_dec_candidates<L>(rest, small(1000), len);
    CHECK(cand.size() == MIN + 4);
    const uint32_t P = L::OUT_MIN + 9;
    std::vector<HuffDevSummary> sums;
    for (size_t q = 0; q < cand.size(); q++) sums.push_back(q == 2 || q == 9 ? HuffDevSummary{PARSE_NOT_MINE, 0, 0, 0} : planned(P + (uint32_t)q));
    Idx idx; std::vector<uint32_t> expect;
    rune_dec_planned<L>(cand, 5, sums.data(), len, idx, expect);
    CHECK((idx == Idx{0, 3, 9, 12}) && (expect == std::vector<uint32_t>{P, P + 1, P + 3, P + 4}));
    idx.clear(); expect.clear();
    rune_dec_planned<L>(cand, cand.size(), sums.data(), len, idx, expect);
    CHECK(idx.size() == MIN + 2 && expect.size() == idx.size() && std::is_sorted(idx.begin(), idx.end()));
    // still the minimum: they leave rest, which is sorted afterwards and keeps the others
    Idx left = rest;
    CHECK(rune_dec_leave<L>(left, idx) && idx.size() == MIN + 2);
    CHECK((left == Idx{6, 27}));
    // exactly the minimum leaves too; one fewer: none is taken, idx is emptied, rest stays as it came
    Idx exact(idx.begin(), idx.begin() + MIN), below(idx.begin(), idx.begin() + MIN - 1);
    left = rest;
    CHECK(rune_dec_leave<L>(left, exact) && exact.size() == MIN && left.size() == 4 && std::is_sorted(left.begin(), left.end()));
    left = rest;
    CHECK(!rune_dec_leave<L>(left, below) && below.empty() && left == rest);
}

int main() {
    test_encoder();
    test_decoder<ParseRuneSmall>();
    test_decoder<ParseRuneMid>();
    std::printf("rune select: %llu checks\n", checks);
    return 0;
}
