// The plan of the batch suite (raisin_amd/csrc/suite_layout.h) as plain host code, held against a brute-force statement of what it
// promises: the prefix tree holds every distinct prefix of the lists exactly once, a list ends at the node of its own layers, a node is
// kept exactly where more than one user reads it -- the tree branches, or a list ends while another goes on --, the kept bytes are the
// kept nodes' slots of the bounds applied in turn, a member's run need is monotone in its length and at least the need of every list run
// alone -- and exactly the round trip's need when there is one list, whose tree keeps nothing --, the decompress-only stats block lies
// apart at 16-byte offsets, and best is the first smallest among the lists that succeeded.
// Prints the number of checks it made.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "suite_layout.h"

using namespace rsn;

static unsigned long long checks = 0;
#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        checks++;                                                                                    \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

typedef std::vector<std::vector<int>> Lists;

static SuiteTree tree_of(const Lists &lists) {
    std::vector<const int *> p;
    std::vector<size_t> k;
    for (const std::vector<int> &l : lists) { p.push_back(l.data()); k.push_back(l.size()); }
    return suite_tree(p.data(), k.data(), lists.size());
}

// the layers from the root to node v
static std::vector<int> path_of(const SuiteTree &t, size_t v) {
    std::vector<int> path;
    for (; v != SUITE_ROOT; v = t.nodes[v].parent) path.push_back(t.nodes[v].layer);
    std::reverse(path.begin(), path.end());
    return path;
}

// two stand-ins for the codecs' compress bounds: both grow with n, as the library's do
static size_t bound(int id, size_t n) { return id == 1 ? n + n / 8 + 16 : n + n / 2 + 1040; }
// the largest slot of the compress pass of one list, as rsn_api.hip's layers_batch_slot takes it
static size_t enc_slot(const std::vector<int> &l, size_t n) {
    size_t most = 0;
    for (int id : l) { n = bound(id, n); most = std::max(most, n); }
    return most;
}
// a stand-in for the decompress pass's estimate: grows with n
static size_t dec_slot(const std::vector<int> &l, size_t n) { return l.empty() ? 0 : 2 * n + 4096 + 8 * l.size(); }

static void test_tree(const Lists &lists) {
    const SuiteTree t = tree_of(lists);
    // brute force: the distinct prefixes of the lists, the empty one included
    std::set<std::vector<int>> prefixes;
    prefixes.insert(std::vector<int>());
    for (const std::vector<int> &l : lists)
        for (size_t k = 1; k <= l.size(); k++) prefixes.insert(std::vector<int>(l.begin(), l.begin() + (long)k));
    CHECK(t.nodes.size() == prefixes.size());                              // every shared prefix is found once ...
    std::set<std::vector<int>> seen;
    for (size_t v = 0; v < t.nodes.size(); v++) {
        const std::vector<int> path = path_of(t, v);
        CHECK(prefixes.count(path) == 1 && seen.insert(path).second);      // ... and every node is a prefix of its own
        CHECK(path.size() == t.nodes[v].depth);
        if (v != SUITE_ROOT) {
            CHECK(t.nodes[v].parent < v);                                  // a child lies behind its parent: one pass in index order visits parents first
            const std::vector<size_t> &sib = t.nodes[t.nodes[v].parent].kids;
            CHECK(std::count(sib.begin(), sib.end(), v) == 1);
        }
        for (size_t kid : t.nodes[v].kids) CHECK(t.nodes[kid].parent == v && t.nodes[kid].depth == t.nodes[v].depth + 1);
    }
    CHECK(t.nodes[SUITE_ROOT].depth == 0 && t.nodes[SUITE_ROOT].parent == SUITE_ROOT);
    // a list ends at the node of its layers, and the lists that end at a node are the equal ones, ascending
    CHECK(t.end.size() == lists.size());
    size_t ended = 0;
    for (size_t l = 0; l < lists.size(); l++) CHECK(path_of(t, t.end[l]) == lists[l]);
    for (size_t v = 0; v < t.nodes.size(); v++) {
        const std::vector<size_t> &e = t.nodes[v].ends;
        ended += e.size();
        CHECK(std::is_sorted(e.begin(), e.end()));
        for (size_t l : e) CHECK(t.end[l] == v && lists[l] == lists[e[0]]);
    }
    CHECK(ended == lists.size());
    // kept exactly where a list ends while another goes on, or the tree branches: brute force over the lists
    for (size_t v = 0; v < t.nodes.size(); v++) {
        const std::vector<int> path = path_of(t, v);
        std::set<int> next;
        bool ends = false;
        for (const std::vector<int> &l : lists) {
            if (l.size() < path.size() || !std::equal(path.begin(), path.end(), l.begin())) continue;
            if (l.size() == path.size()) ends = true; else next.insert(l[path.size()]);
        }
        const size_t users = next.size() + (ends ? 1 : 0);
        CHECK(suite_users(t.nodes[v]) == users && (users >= 1 || lists.empty()));   // (no node without a user, but the root of no lists)
        CHECK(t.nodes[v].kept == (v != SUITE_ROOT && users > 1));
    }
}

static void test_need(const Lists &lists, size_t len, bool staged, bool hists) {
    const SuiteTree t = tree_of(lists);
    auto need_of = [&](size_t n) {
        size_t enc = 0, dec = 0;
        for (const std::vector<int> &l : lists) { enc = std::max(enc, enc_slot(l, n)); dec = std::max(dec, dec_slot(l, n)); }
        return suite_member_need(staged ? n : 0, enc, dec, suite_keep_bytes(t, n, bound), n, n, hists);
    };
    const size_t need = need_of(len);
    // the kept bytes: a slot for every kept node, of the bounds applied in turn along its path
    std::vector<size_t> caps;
    const size_t keep = suite_keep_bytes(t, len, bound, &caps);
    size_t want = 0;
    CHECK(caps.size() == t.nodes.size() && caps[SUITE_ROOT] == len);
    for (size_t v = 1; v < t.nodes.size(); v++) {
        size_t n = len;
        for (int id : path_of(t, v)) n = bound(id, n);
        CHECK(caps[v] == n);
        if (t.nodes[v].kept) want += lb_slot_bytes(n);
    }
    CHECK(keep == want && keep % 16 == 0);
    // at least what every list holds run alone, and more by what is kept
    for (const std::vector<int> &l : lists) CHECK(need >= rb_member_need(staged ? len : 0, enc_slot(l, len), dec_slot(l, len), len, len, hists));
    bool any_kept = false;
    for (const SuiteNode &v : t.nodes) any_kept = any_kept || v.kept;
    CHECK((keep > 0) == any_kept);
    // monotone in the member length
    for (size_t more : {(size_t)1, (size_t)15, (size_t)16, RB_TILE, 3 * RB_TILE + 1}) CHECK(need_of(len + more) >= need);
}

// What lets the batch round trip run as the suite of its one list: the tree of one list is a chain with no kept node, so no kept bytes,
// and the member's run need is the round trip's own, whatever its two slot figures are
static void test_one_list(size_t layers) {
    std::vector<int> list(layers);
    for (size_t k = 0; k < layers; k++) list[k] = 1 + (int)(k % 2);
    const SuiteTree t = tree_of({list});
    CHECK(t.nodes.size() == layers + 1 && t.end[0] == layers);
    for (size_t v = 0; v < t.nodes.size(); v++) {
        CHECK(!t.nodes[v].kept && suite_users(t.nodes[v]) == 1);
        CHECK(t.nodes[v].depth == v && t.nodes[v].kids.size() == (v < layers ? 1u : 0u) && t.nodes[v].ends.size() == (v == layers ? 1u : 0u));
    }
    for (size_t len : {(size_t)0, (size_t)1, (size_t)65535, (size_t)65536, (size_t)65537, (size_t)UINT32_MAX})
        for (bool hists : {false, true})
            for (bool staged : {false, true}) {
                const size_t keep = suite_keep_bytes(t, len, bound), enc = enc_slot(list, len), dec = dec_slot(list, len);
                CHECK(keep == 0);
                CHECK(suite_member_need(staged ? len : 0, enc, dec, keep, len, len, hists) == rb_member_need(staged ? len : 0, enc, dec, len, len, hists));
            }
}

static void test_dec_layout(size_t tiles, size_t m, bool hists) {
    const RbLayout l = suite_dec_layout(tiles, m, hists), full = rb_layout(tiles, m, hists);
    const size_t table = tiles * sizeof(RbEntry), words = m * RB_WORD, counts = hists ? m * SUITE_HIST_BYTES : 0;
    CHECK(l.table % 16 == 0 && l.words % 16 == 0 && l.hists % 16 == 0);
    CHECK(l.table + table <= l.words && l.words + words <= l.hists && l.hists + counts == l.bytes);
    CHECK(l.words - (l.table + table) < 16 && l.hists - (l.words + words) < 16);
    CHECK(l.table == full.table && l.words == full.words && l.hists == full.hists);   // the same block but for the rows' width
    CHECK(full.bytes - l.bytes == counts);                                 // half the counters of the round trip's block
    CHECK(rb_stats_bytes(l) == l.bytes - l.words);
}

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 2000;
    static_assert(SUITE_LISTS_MAX == 16 && SUITE_HIST_BYTES == 1024, "the figures the documents state");
    // named cases
    {   // {[1],[1,2],[2]}: root -> 1 -> 2, root -> 2; [1] is kept (a list ends there and another goes on), nothing else
        const SuiteTree t = tree_of({{1}, {1, 2}, {2}});
        CHECK(t.nodes.size() == 4);
        CHECK(t.end[0] == 1 && t.end[1] == 2 && t.end[2] == 3);
        CHECK(t.nodes[1].kept && !t.nodes[2].kept && !t.nodes[3].kept && !t.nodes[0].kept);
        CHECK(t.nodes[0].kids == (std::vector<size_t>{1, 3}) && t.nodes[1].kids == (std::vector<size_t>{2}));
    }
    {   // {[1,2],[1,2]}: one chain, both lists end at its tip, nothing kept: equal lists are one user
        const SuiteTree t = tree_of({{1, 2}, {1, 2}});
        CHECK(t.nodes.size() == 3 && t.end[0] == 2 && t.end[1] == 2);
        CHECK(t.nodes[2].ends == (std::vector<size_t>{0, 1}));
        for (const SuiteNode &v : t.nodes) CHECK(!v.kept);
    }
    {   // {[],[1]}: the empty list ends at the root, which is the member itself and never kept
        const SuiteTree t = tree_of({{}, {1}});
        CHECK(t.nodes.size() == 2 && t.end[0] == SUITE_ROOT && t.end[1] == 1);
        CHECK(!t.nodes[0].kept && !t.nodes[1].kept && suite_users(t.nodes[0]) == 2);
    }
    {   // eight layers deep, alone and beside its own prefixes and a branch at the bottom
        const std::vector<int> deep = {1, 2, 1, 2, 1, 2, 1, 2};
        const SuiteTree t = tree_of({deep});
        CHECK(t.nodes.size() == 9 && t.end[0] == 8 && t.nodes[8].depth == 8);
        for (const SuiteNode &v : t.nodes) CHECK(!v.kept);
        const SuiteTree u = tree_of({deep, {1, 2, 1, 2}, {1, 2, 1, 2, 1, 2, 1, 1}});
        CHECK(u.nodes.size() == 10 && u.end[1] == 4 && u.nodes[4].kept && u.nodes[7].kept);
        for (size_t v = 0; v < u.nodes.size(); v++) if (v != 4 && v != 7) CHECK(!u.nodes[v].kept);
    }
    {   // {[1],[2]}: a branch at the root keeps nothing
        const SuiteTree t = tree_of({{1}, {2}});
        for (const SuiteNode &v : t.nodes) CHECK(!v.kept);
    }
    {   // the standard suite: huffman, lzss, [lzss, huffman] -- the LZSS output is the one kept node
        const SuiteTree t = tree_of({{2}, {1}, {1, 2}});
        CHECK(t.nodes.size() == 4 && t.nodes[t.end[1]].kept && t.nodes[t.end[2]].parent == t.end[1]);
        CHECK(suite_keep_bytes(t, 1000, bound) == lb_slot_bytes(bound(1, 1000)));
    }
    for (const Lists &lists : {Lists{{1}, {1, 2}, {2}}, Lists{{1, 2}, {1, 2}}, Lists{{}, {1}}, Lists{{1, 2, 1, 2, 1, 2, 1, 2}}, Lists{}, Lists{{}}, Lists{{}, {}},
                               Lists{{2}, {1}, {1, 2}, {2, 1}, {1, 1}, {}, {1}}}) {
        test_tree(lists);
        for (size_t len : {(size_t)0, (size_t)1, (size_t)25, (size_t)1024, RB_TILE, RB_TILE + 1}) { test_need(lists, len, true, true); test_need(lists, len, false, false); }
    }
    for (size_t layers : {(size_t)0, (size_t)1, (size_t)3, (size_t)8}) test_one_list(layers);
    // best: the first smallest among the lists that succeeded
    {
        const uint64_t sizes[4] = {7, 5, 5, 9};
        auto size = [&](size_t l) { return sizes[l]; };
        CHECK(suite_best(4, [](size_t) { return true; }, size) == 1);
        CHECK(suite_best(4, [](size_t l) { return l != 1; }, size) == 2);
        CHECK(suite_best(4, [](size_t l) { return l == 0 || l == 3; }, size) == 0);
        CHECK(suite_best(4, [](size_t) { return false; }, size) == UINT32_MAX);
        CHECK(suite_best(0, [](size_t) { return true; }, size) == UINT32_MAX);
    }
    for (size_t tiles : {(size_t)0, (size_t)1, (size_t)3, (size_t)4097})
        for (size_t m : {(size_t)0, (size_t)1, (size_t)3, (size_t)4097}) { test_dec_layout(tiles, m, false); test_dec_layout(tiles, m, true); }
    std::mt19937_64 rng(0x5017E);
    for (int it = 0; it < rounds; it++) {
        Lists lists(1 + rng() % SUITE_LISTS_MAX);
        for (std::vector<int> &l : lists) { l.resize(rng() % 9); for (int &id : l) id = 1 + (int)(rng() % 2); }
        test_tree(lists);
        test_need(lists, it % 3 == 0 ? rng() % 40 : rng() % (3 * RB_TILE), it % 2 == 0, it % 4 < 2);
        test_dec_layout(rng() % 5000, rng() % 5000, it % 2 == 0);
    }
    std::printf("suite layout: %llu checks\n", checks);
    return 0;
}
