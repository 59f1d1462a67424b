// The arithmetic of the layered batch calls (raisin_amd/csrc/layers_batch_layout.h) as plain host code, held against a brute-force
// statement of what it promises: offsets on 16-byte boundaries, slots that are disjoint, inside their arena and followed by their slack,
// runs that are consecutive, cover every member, hold as many members as fit and stay within the budget unless they hold one member.
// Prints the number of checks it made.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "layers_batch_layout.h"

using namespace rsn;

static unsigned long long checks = 0;
#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        checks++;                                                                                    \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

static bool meet(size_t a, size_t na, size_t b, size_t nb) { return na && nb && a < b + nb && b < a + na; }

static void test_arena(const std::vector<size_t> &caps) {
    std::vector<size_t> offs(3, 12345);                                    // (resized by the call)
    const size_t total = lb_arena(caps.data(), caps.size(), offs);
    CHECK(offs.size() == caps.size());
    size_t sum = 0;
    for (size_t i = 0; i < caps.size(); i++) {
        const size_t slot = lb_slot_bytes(caps[i]);
        CHECK(offs[i] % 16 == 0 && slot % 16 == 0);
        CHECK(slot >= caps[i] + LB_SLACK && slot < caps[i] + LB_SLACK + 16);   // the capacity, then the slack the single calls read into
        CHECK(offs[i] + slot <= total);
        for (size_t j = 0; j < i; j++) CHECK(!meet(offs[i], slot, offs[j], lb_slot_bytes(caps[j])));
        sum += slot;
    }
    CHECK(total == sum);                                                   // (no gaps: the budget counts what is allocated)
}

static void test_packed(const std::vector<size_t> &lens) {
    std::vector<size_t> offs;
    const size_t total = lb_packed(lens.data(), lens.size(), offs);
    CHECK(offs.size() == lens.size());
    size_t sum = 0;
    for (size_t i = 0; i < lens.size(); i++) {
        CHECK(offs[i] % 16 == 0 && offs[i] + lens[i] <= total);
        for (size_t j = 0; j < i; j++) CHECK(!meet(offs[i], lens[i], offs[j], lens[j]));
        if (i) CHECK(offs[i] >= offs[i - 1] + lens[i - 1] && offs[i] - (offs[i - 1] + lens[i - 1]) < 16);   // back to back: what crosses is the lengths rounded up
        sum += (lens[i] + 15) / 16 * 16;
    }
    CHECK(total == sum && total % 16 == 0);
}

static void test_runs(const std::vector<size_t> &needs, size_t budget) {
    const std::vector<LbRun> runs = lb_runs(needs.size(), budget, [&](size_t i) { return needs[i]; });
    if (needs.empty()) { CHECK(runs.empty()); return; }
    CHECK(!runs.empty() && runs.front().lo == 0 && runs.back().hi == needs.size());
    for (size_t r = 0; r < runs.size(); r++) {
        const LbRun &run = runs[r];
        CHECK(run.lo < run.hi);
        if (r) CHECK(run.lo == runs[r - 1].hi);
        unsigned __int128 sum = 0;
        for (size_t i = run.lo; i < run.hi; i++) sum += needs[i];
        CHECK(sum > (size_t)-1 ? run.bytes == (size_t)-1 : run.bytes == (size_t)sum);
        CHECK(sum <= budget || run.hi - run.lo == 1);                      // within the budget unless it holds one member
        if (run.hi < needs.size()) CHECK(sum + needs[run.hi] > budget);    // ... and the next member did not fit
    }
}

static void test_tiles(size_t len) {
    size_t count = 0, covered = 0;
    for (size_t at = 0; at < len; at += LB_TILE) { const size_t t = len - at < LB_TILE ? len - at : LB_TILE; CHECK(t > 0 && at % 16 == 0); covered += t; count++; }
    CHECK(covered == len && lb_tiles(len) == count);
}

int main(int argc, char **argv) {
    const int lists = argc > 1 ? std::atoi(argv[1]) : 4000;
    // named cases
    test_arena({}); test_arena({0}); test_arena({0, 0, 1, 15, 16, 17}); test_packed({}); test_packed({0, 0, 5, 0, 16, 17, 0});
    test_runs({}, 100); test_runs({5}, 0); test_runs({200}, 100); test_runs({50, 50, 1}, 100); test_runs({100, 100, 100}, 100);
    test_runs({1, 200, 1}, 100); test_runs({0, 0, 0}, 0); test_runs({1, 1, 1}, 0);
    test_runs({(size_t)-1, (size_t)-1, 7}, (size_t)-1);                    // sums that do not fit a size_t
    test_runs({(size_t)-16, 32, 5}, (size_t)-1);
    for (size_t len : {(size_t)0, (size_t)1, (size_t)16, LB_TILE - 1, LB_TILE, LB_TILE + 1, 5 * LB_TILE, 5 * LB_TILE + 17}) test_tiles(len);
    CHECK(lb_member_need(0, 0) == 2 * LB_SLACK && lb_member_need(17, 100) == 32 + 2 * (112 + LB_SLACK));
    std::mt19937_64 rng(0x1A7E25);
    int single_runs = 0, full_runs = 0;
    for (int it = 0; it < lists; it++) {
        const size_t count = rng() % (it % 16 == 0 ? 60 : 9);
        std::vector<size_t> v(count);
        const size_t scale = it % 3 == 0 ? 40 : it % 3 == 1 ? 5000 : 300000;
        for (size_t &x : v) x = rng() % 5 == 0 ? 0 : rng() % scale;
        test_arena(v);
        test_packed(v);
        const size_t budget = rng() % (4 * scale) + (it % 7 == 0 ? 0 : 1);
        std::vector<size_t> needs(count);
        for (size_t i = 0; i < count; i++) needs[i] = lb_member_need(it % 2 ? v[i] : 0, v[i]);
        test_runs(needs, budget * 3);
        test_runs(v, budget);
        for (const LbRun &r : lb_runs(count, budget, [&](size_t i) { return v[i]; })) { single_runs += r.hi - r.lo == 1 && r.bytes > budget; full_runs += r.hi - r.lo > 1; }
        test_tiles(rng() % (8 * LB_TILE));
    }
    CHECK(single_runs > lists / 50 && full_runs > lists / 50);            // (the generator reaches both kinds of run)
    std::printf("layers batch layout: %d runs above the budget alone, %d of several members; %llu checks\n", single_runs, full_runs, checks);
    return 0;
}
