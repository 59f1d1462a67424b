// The layout of a run of host members through a class's device form (raisin_amd/csrc/group_layout.h: RunLayout; group_run.h: run_members_staged) as plain
// host code: runs cut where next_group says, 16-aligned disjoint slots, the plan table in front of the inputs when one is asked for, and how
// much of the output block comes down.  Production runs are 256 MiB, so the cut is covered here, with a run limit of 4 KiB.
// Prints the number of checks it made.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "group_layout.h"

using namespace rsn;

static unsigned long long checks = 0;
#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        checks++;                                                                                    \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

constexpr size_t RUN_BYTES = 4096, RUN_MEMBERS = 4096, PLAN = 576;         // a tiny run limit; sizeof(HuffDevPlan)
struct Span { size_t lo, hi; };

// the members as the two tiled classes size them: the input slot the bytes rounded up to 16, the output slot a rounded size and 16 more
static size_t in_slot(size_t n) { return group_round16(n); }
static size_t out_slot(size_t n) { return group_round16(n) + 16; }

// every run of `sizes` under a table entry of `table` bytes; returns the runs' first members
static std::vector<size_t> walk(const std::vector<size_t> &sizes, size_t table) {
    auto need = [&](size_t k) { return run_need(table, in_slot(sizes[k]), out_slot(sizes[k])); };
    std::vector<size_t> firsts;
    for (size_t j = 0; j < sizes.size();) {
        const GroupCut cut = next_group(j, sizes.size(), RUN_MEMBERS, RUN_BYTES, need);
        const size_t g = cut.hi - j;
        firsts.push_back(j);
        CHECK(cut.hi > j && cut.hi <= sizes.size());
        CHECK(g == 1 || cut.bytes <= RUN_BYTES);                                            // only a member larger than the limit passes it, alone
        CHECK(cut.hi == sizes.size() || cut.bytes + need(cut.hi) > RUN_BYTES);              // (not cut a member early)
        RunLayout lay(g, table);
        CHECK(lay.in_total() == g * table && lay.out_total() == 0);
        std::vector<Span> ins{{0, g * table}}, outs;                                        // the table of g entries precedes the inputs
        for (size_t k = j; k < cut.hi; k++) {
            const RunSlots o = lay.member(in_slot(sizes[k]), out_slot(sizes[k]));
            CHECK(o.in % 16 == 0 && o.out % 16 == 0);
            CHECK(o.in >= g * table && in_slot(sizes[k]) >= sizes[k]);
            ins.push_back({o.in, o.in + in_slot(sizes[k])});
            outs.push_back({o.out, o.out + out_slot(sizes[k])});
        }
        // handed out in rising order, so disjoint iff no span starts before its predecessor ends; and tight: the totals are the ends
        for (size_t q = 1; q < ins.size(); q++) CHECK(ins[q].lo == ins[q - 1].hi && ins[q].hi > ins[q].lo);
        for (size_t q = 1; q < outs.size(); q++) CHECK(outs[q].lo == outs[q - 1].hi);
        CHECK(outs[0].lo == 0 && ins.back().hi == lay.in_total() && outs.back().hi == lay.out_total());
        CHECK(lay.in_total() + lay.out_total() == cut.bytes);                               // what the admission and the buffers are sized by
        j = cut.hi;
    }
    return firsts;
}

static void test_runs() {
    const std::vector<size_t> sizes = {1, 15, 16, 17, 4000, 1, 15, 16, 17, 4000, 4000, 17, 16, 15, 1, 1, 1, 1, 1};
    // no table: 1 + 15 + 16 + 17 are 16+32, 16+32, 16+32, 32+48 = 224 bytes, 4000 (4000 + 4016) is a run of its own
    std::vector<size_t> firsts = walk(sizes, 0);
    CHECK((firsts == std::vector<size_t>{0, 4, 5, 9, 10, 11}));
    // a plan entry a member: 576 more each -- the last eight members, one run of 416 bytes without it, are 5024 with it and cut after six (3776)
    firsts = walk(sizes, PLAN);
    CHECK((firsts == std::vector<size_t>{0, 4, 5, 9, 10, 11, 17}));
    for (size_t n = 1; n <= 64; n++) walk(std::vector<size_t>(n, 17 * n), 0), walk(std::vector<size_t>(n, 17 * n), PLAN);
}

static void test_down() {
    const size_t sizes[5] = {1, 15, 16, 17, 4000};
    RunLayout lay(5, PLAN);
    size_t out_at[5];
    for (size_t q = 0; q < 5; q++) out_at[q] = lay.member(in_slot(sizes[q]), out_slot(sizes[q])).out;
    const uint32_t all[5] = {1, 15, 16, 17, 4000};
    CHECK(run_down(5, all, out_at) == out_at[4] + 4000);                                    // every member answered: the end of the last result, not of its slot
    const uint32_t end_back[5] = {1, 15, 16, 17, GROUP_BACK};
    CHECK(run_down(5, end_back, out_at) == out_at[3] + 17);                                 // handed back at the end: down stops at the member before
    const uint32_t end_runes[5] = {1, 15, 16, GROUP_BACK_RUNES, GROUP_BACK};
    CHECK(run_down(5, end_runes, out_at) == out_at[2] + 16);
    const uint32_t mid_back[5] = {1, GROUP_BACK, GROUP_BACK_RUNES, 17, 9};
    CHECK(run_down(5, mid_back, out_at) == out_at[4] + 9);                                  // in the middle: the slots in between come down unread
    const uint32_t none[5] = {GROUP_BACK, GROUP_BACK, GROUP_BACK_RUNES, GROUP_BACK, GROUP_BACK};
    CHECK(run_down(5, none, out_at) == 0);                                                  // everywhere: nothing comes down
    const uint32_t first_only[5] = {1, GROUP_BACK, GROUP_BACK, GROUP_BACK, GROUP_BACK};
    CHECK(run_down(5, first_only, out_at) == 1);
    CHECK(run_down(0, all, out_at) == 0);
    for (size_t q = 0; q < 5; q++) CHECK(out_at[q] + all[q] <= lay.out_total());            // down never passes the output block
}

int main() {
    test_runs();
    test_down();
    std::printf("run layout: %llu checks\n", checks);
    return 0;
}
