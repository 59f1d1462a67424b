// suite_layout.h -- the plan of the batch suite (rsn.h: rsn_layers_suite_batch, rsn_layers_suite_batch_dev), as plain host
// code: no HIP include, so a CPU test (tests/suite_layout_test.cpp) checks it -- the prefix tree of the layer lists holds every distinct
// prefix once, a node's output is kept exactly where more than one user reads it, the decompress-only stats block lies apart at 16-byte
// offsets, and a member's run need counts the kept bytes and is at least the need of every list run alone.  rsn_api.hip's
// suite_batch_flow is the user -- for the batch round trip too, whose one list is a chain with nothing kept --, roundtrip_batch.hip's
// second instance of k_members_verify writes the decompress-only stats.
//
// The lists of a call form a prefix tree over their layers in compress order: node 0 is the empty prefix (the member as it came), every
// other node one more compress layer behind its parent.  A run compresses every node once, walking the tree depth first; a list's
// decompress pass starts from the node its last layer ends at.  A node that only one user reads -- a single child, or a single list that
// ends there -- hands its output over in the arenas of the layered batch calls, as a call of that list alone would.  A node with more
// users is KEPT: its step writes into a slot of its own (Slot::LB_KEEP), sub-allocated per node and member, which no later step reuses.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "roundtrip_batch_layout.h"

namespace rsn {

constexpr size_t SUITE_LISTS_MAX = 16;   // RSN_SUITE_LISTS_MAX
constexpr size_t SUITE_ROOT = 0;

// parent: the node one layer shorter (the root: itself); layer: the compress layer that leads here from the parent (the root: 0); depth:
// the layers from the root; kids: in the order the lists first name them; ends: the lists that end here, ascending -- the first is the
// one that is run, the others are copies of it
struct SuiteNode {
    size_t parent = SUITE_ROOT, depth = 0;
    int layer = 0;
    std::vector<size_t> kids, ends;
    bool kept = false;
};
// nodes[0] is the root; a child always lies behind its parent.  end[l]: the node list l ends at
struct SuiteTree { std::vector<SuiteNode> nodes; std::vector<size_t> end; };

// who reads a node's output: every child's compress step, and ONE decompress pass when lists end here (equal lists run once)
inline size_t suite_users(const SuiteNode &v) { return v.kids.size() + (v.ends.empty() ? 0 : 1); }

// the tree of n_lists lists: list l is layers[l][0 .. n_layers[l])
inline SuiteTree suite_tree(const int *const *layers, const size_t *n_layers, size_t n_lists) {
    SuiteTree t;
    t.nodes.emplace_back();
    t.end.resize(n_lists);
    for (size_t l = 0; l < n_lists; l++) {
        size_t at = SUITE_ROOT;
        for (size_t k = 0; k < n_layers[l]; k++) {
            size_t next = 0;
            for (size_t kid : t.nodes[at].kids) if (t.nodes[kid].layer == layers[l][k]) { next = kid; break; }
            if (!next) {
                next = t.nodes.size();
                SuiteNode v;
                v.parent = at; v.depth = k + 1; v.layer = layers[l][k];
                t.nodes.push_back(v);
                t.nodes[at].kids.push_back(next);
            }
            at = next;
        }
        t.nodes[at].ends.push_back(l);
        t.end[l] = at;
    }
    // the root is the member itself, which nothing overwrites: never kept
    for (size_t v = 1; v < t.nodes.size(); v++) t.nodes[v].kept = suite_users(t.nodes[v]) > 1;
    return t;
}

// The kept bytes of a member of `len` bytes: a slot (its slack included) for every kept node, of the compress bounds applied in turn
// from the root -- an upper bound of what the node's step is given, as bound(layer, n) grows with n.  caps: per node, the bound chain's
// figure (the root: len), for the caller that carves the slot -- and the vector a caller with many members hands in again, so that a
// member costs no allocation.
template <class Bound>
size_t suite_keep_bytes(const SuiteTree &t, size_t len, Bound bound, std::vector<size_t> *caps = nullptr) {
    std::vector<size_t> own;
    std::vector<size_t> &cap = caps ? *caps : own;
    cap.resize(t.nodes.size());
    cap[SUITE_ROOT] = len;
    size_t bytes = 0;
    for (size_t v = 1; v < t.nodes.size(); v++) {
        cap[v] = bound(t.nodes[v].layer, cap[t.nodes[v].parent]);
        if (t.nodes[v].kept) bytes += lb_slot_bytes(cap[v]);
    }
    return bytes;
}

// what a member holds at once in a run of the suite: what the most demanding of its lists holds run alone (enc_slot / dec_slot: the
// largest over the lists of rb_member_need's two figures), and the kept bytes
constexpr size_t suite_member_need(size_t staged_len, size_t enc_slot, size_t dec_slot, size_t keep_bytes, size_t n_o, size_t n_d, bool hists) {
    return rb_member_need(staged_len, enc_slot, dec_slot, n_o, n_d, hists) + keep_bytes;
}

// The verify slot of a run's second and further lists: the table, then the stats block of the decompress-only instance -- a word per
// member and, when histograms were asked for, 256 counters per member (the decompressed bytes alone).  As RbLayout in everything else.
constexpr size_t SUITE_HIST_WORDS = 256, SUITE_HIST_BYTES = SUITE_HIST_WORDS * sizeof(uint32_t);
constexpr RbLayout suite_dec_layout(size_t tiles, size_t m, bool hists) {
    const size_t words = lb_round16(tiles * sizeof(RbEntry)), h = words + lb_round16(m * RB_WORD);
    return RbLayout{0, words, h, h + (hists ? m * SUITE_HIST_BYTES : 0)};
}
static_assert(SUITE_HIST_BYTES * 2 == RB_HIST_BYTES, "the decompress-only row is the second half of the round trip's");
// the verify slot of either instance of k_members_verify: both sides counted (a run's first list), or the decompressed side alone
constexpr RbLayout verify_layout(bool both, size_t tiles, size_t m, bool hists) { return both ? rb_layout(tiles, m, hists) : suite_dec_layout(tiles, m, hists); }

// best[i] of a call: the list with the smallest compressed size among those that succeeded, the lowest index among equals; UINT32_MAX
// when none did.  ok(l): list l succeeded; size(l): the member's compressed size under list l
template <class Ok, class Size>
uint32_t suite_best(size_t n_lists, Ok ok, Size size) {
    uint32_t best = UINT32_MAX;
    for (size_t l = 0; l < n_lists; l++)
        if (ok(l) && (best == UINT32_MAX || size(l) < size(best))) best = (uint32_t)l;
    return best;
}

}  // namespace rsn
