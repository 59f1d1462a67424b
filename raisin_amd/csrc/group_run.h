// group_run.h -- the one packer of the grouped batch kernels (lzss_small.hip, lzss_mid.hip, huff_small.hip, huff_mid.hip).
#pragma once

#include "codecs.h"
#include "group_layout.h"

namespace rsn {

// what run_groups asks of member k of a class: its index in the call, the bytes its kernel reads, and its slots' sizes (group_layout.h)
struct GroupItem { size_t i; const uint8_t *in; size_t n, in_bytes, out_bytes; };

// `count` members in groups of at most SMALL_GROUP_MAX members and SMALL_GROUP_BYTES of the thread's pinned staging, ONE launch a group.
// Per group: the table of Entry, then per member its input (zeros behind it), its output slot and its status word, set to GROUP_PENDING;
//   fill(entry, k, base, slots)   writes member k's table entry (base + slots.in / .out / .status are the member's);
//   launch(s, g, tab, base)       queues the group's kernel, g workgroups; non-zero: the call's code;
//   answer(status)                once every status word has changed: GROUP_BACK, GROUP_BACK_RUNES, or the length of the result in the output slot.
// take() receives the results, `back` the members handed back, in the members' order (back_runes, when given, those of them that were
// handed back as GROUP_BACK_RUNES).  *failed: the group's first member when staging,
// launch or wait fail, the member itself when take() does.
template <class Entry, class Member, class Fill, class Launch, class Answer>
int run_groups(Ctx &c, const char *what, size_t count, Member member, Fill fill, Launch launch, Answer answer,
               const SmallTake &take, std::vector<size_t> &back, size_t *failed, std::vector<size_t> *back_runes = nullptr) {
    static_assert(sizeof(Entry) % 16 == 0, "the members' slots start behind the table, 16-aligned");
    if (count == 0) return RSN_OK;
    int rc = ctx_init(c); if (rc) { *failed = member(0).i; return rc; }
    hipStream_t s = c.own_stream;
    auto need = [&](size_t k) { const GroupItem m = member(k); return group_need(sizeof(Entry), m.in_bytes, m.out_bytes); };
    std::vector<uint32_t> st, out;
    for (size_t j = 0; j < count;) {
        const GroupCut cut = next_group(j, count, SMALL_GROUP_MAX, SMALL_GROUP_BYTES, need);
        const size_t g = cut.hi - j, first = member(j).i;
        void *pp; rc = pinned_buf(c, cut.bytes + 64, &pp); if (rc) { *failed = first; return rc; }
        uint8_t *base = (uint8_t *)pp;
        Entry *tab = (Entry *)base;
        GroupLayout lay(g, sizeof(Entry));
        st.assign(g, 0); out.assign(g, 0);
        for (size_t q = 0; q < g; q++) {
            const GroupItem m = member(j + q);
            const MemberSlots o = lay.member(m.in_bytes, m.out_bytes);
            memcpy(base + o.in, m.in, m.n); memset(base + o.in + m.n, 0, m.in_bytes - m.n);
            *(uint32_t *)(base + o.status) = GROUP_PENDING;
            st[q] = o.status; out[q] = o.out;
            fill(tab[q], j + q, base, o);
        }
        rc = launch(s, (uint32_t)g, (const Entry *)tab, base);
        if (rc == RSN_OK) rc = group_wait(c, s, base, st, GROUP_PENDING, what);
        if (rc) { *failed = first; return rc; }
        for (size_t q = 0; q < g; q++) {
            const size_t i = member(j + q).i;
            const uint32_t v = answer((const uint32_t *)(base + st[q]));
            if (group_is_back(v)) { (v == GROUP_BACK_RUNES && back_runes ? *back_runes : back).push_back(i); continue; }
            rc = take(i, base + out[q], v); if (rc) { *failed = i; return rc; }
        }
        j = cut.hi;
    }
    return RSN_OK;
}

// The classes whose table entry is a SmallMember (both LZSS classes, the Huffman encoders): member k is idx[k] as it came, the status word
// is the answer.  out_bytes(n): the output slot of a member of n bytes.
template <class InBytes, class OutBytes, class Launch>
int run_member_groups(Ctx &c, const char *what, const std::vector<size_t> &idx, const uint8_t *const *ins, const size_t *lens,
                      InBytes in_bytes, OutBytes out_bytes, Launch launch, const SmallTake &take, std::vector<size_t> &back, size_t *failed,
                      std::vector<size_t> *back_runes) {
    return run_groups<SmallMember>(c, what, idx.size(),
        [&](size_t k) { const size_t i = idx[k], n = lens[i]; return GroupItem{i, ins[i], n, (size_t)in_bytes(n), (size_t)out_bytes(n)}; },
        [&](SmallMember &m, size_t k, uint8_t *, const MemberSlots &o) { m = SmallMember{o.in, (uint32_t)lens[idx[k]], o.out, o.status}; },
        launch, [](const uint32_t *w) { return w[0]; }, take, back, failed, back_runes);
}

// The same classes on device buffers (the batch calls on device buffers, rsn.h; group_dev.hip): the members idx[k] of `mem`
// in the same groups (next_group, GroupLayout), the staging in device scratch (Slot::GD_STAGE) -- per group one small copy up, the member
// table and a gather table from a pinned region of the group's own, then k_group_gather (the members into their input slots, zeros behind
// them, the status words GROUP_PENDING), the class's kernel through `launch` as above, and k_group_scatter (what fits the member's buffer
// out of the output slot, the status into a word per member).  No host wait between the groups -- the stream orders the staging's reuse --
// and one at the end, when the words come down: answers[k] is GROUP_BACK, GROUP_BACK_RUNES or the length of member idx[k]'s result, which is complete in
// mem[idx[k]].d_out when it is at most its out_cap.
using GroupLaunch = std::function<int(hipStream_t s, uint32_t g, const SmallMember *tab, uint8_t *base)>;
int run_groups_dev(Ctx &c, hipStream_t s, const char *what, const std::vector<size_t> &idx, const rsn_dev_member *mem,
                   size_t (*in_bytes)(size_t n), size_t (*out_bytes)(size_t n), const GroupLaunch &launch, std::vector<uint32_t> &answers);
// ... with slots that depend on more than the member's length (the rune decoder's output slot is what its header promises): in_bytes(k) /
// out_bytes(k) of member idx[k]
using GroupSlotBytes = std::function<size_t(size_t k)>;
int run_groups_dev_sized(Ctx &c, hipStream_t s, const char *what, const std::vector<size_t> &idx, const rsn_dev_member *mem,
                         const GroupSlotBytes &in_bytes, const GroupSlotBytes &out_bytes, const GroupLaunch &launch, std::vector<uint32_t> &answers,
                         size_t group_bytes = SMALL_GROUP_BYTES);   // (a class whose members are large states a larger group of its own: huff_big.hip)

// A class of SmallMember entries is stated ONCE, as a type K -- K::what (the name in messages), K::in_bytes(n) / K::out_bytes(n) (the slots of
// a member of n bytes, group_layout.h) and K::launch(c, s, g, tab, base, window) (the group's kernel) -- and both of its runners, the
// host-buffer form and the device-buffer form (BatchClass::run / run_dev, codecs.h), are these two.
template <class K>
int class_run(Ctx &c, const std::vector<size_t> &idx, const uint8_t *const *ins, const size_t *lens, int64_t window,
              const SmallTake &take, std::vector<size_t> &back, size_t *failed, std::vector<size_t> *back_runes) {
    return run_member_groups(c, K::what, idx, ins, lens, K::in_bytes, K::out_bytes,
        [&](hipStream_t s, uint32_t g, const SmallMember *tab, uint8_t *base) { return K::launch(c, s, g, tab, base, window); }, take, back, failed, back_runes);
}
template <class K>
int class_run_dev(Ctx &c, hipStream_t s, const std::vector<size_t> &idx, const rsn_dev_member *mem, int64_t window, const DevPlans *, std::vector<uint32_t> &answers) {
    return run_groups_dev(c, s, K::what, idx, mem, K::in_bytes, K::out_bytes,
        [&](hipStream_t s2, uint32_t g, const SmallMember *tab, uint8_t *base) { return K::launch(c, s2, g, tab, base, window); }, answers);
}

}  // namespace rsn
