// dev_ranges.h -- the overlap check of the batch calls on device buffers (rsn.h; rsn_api.hip), as plain host code: no HIP include, so a
// CPU test (tests/dev_ranges_test.cpp) holds it against the quadratic comparison it replaces.  The rule: no member's output range may
// overlap ANY member's input range, and the output ranges are pairwise disjoint; input ranges may overlap each other (one buffer may be
// handed in twice), and an empty range overlaps nothing.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rsn {

struct DevRange { uintptr_t lo, hi; size_t member; };                     // [lo, hi), never empty: add_dev_range keeps the empty ones out
inline void add_dev_range(std::vector<DevRange> &v, const void *p, size_t n, size_t member) {
    if (p && n) v.push_back({(uintptr_t)p, (uintptr_t)p + n, member});
}

// 0: none.  1: the outputs of members *a and *b overlap.  2: member *a's output overlaps member *b's input.  Sorts both lists: the outputs
// by their start -- disjoint iff none starts before its predecessor ends -- then one sweep over the inputs in the order of their starts,
// during which an output that ends at or before an input's start is done with for every later input, too.
inline int dev_ranges_clash(std::vector<DevRange> &ins, std::vector<DevRange> &outs, size_t *a, size_t *b) {
    auto by_lo = [](const DevRange &x, const DevRange &y) { return x.lo < y.lo; };
    std::sort(outs.begin(), outs.end(), by_lo);
    for (size_t k = 1; k < outs.size(); k++)
        if (outs[k].lo < outs[k - 1].hi) { *a = std::min(outs[k - 1].member, outs[k].member); *b = std::max(outs[k - 1].member, outs[k].member); return 1; }
    std::sort(ins.begin(), ins.end(), by_lo);
    size_t o = 0;
    for (const DevRange &in : ins) {
        while (o < outs.size() && outs[o].hi <= in.lo) o++;
        if (o == outs.size()) break;
        if (outs[o].lo < in.hi) { *a = outs[o].member; *b = in.member; return 2; }   // (the outputs behind it start later still)
    }
    return 0;
}

}  // namespace rsn
