// group_run.h -- the host code the grouped batch classes share: ONE packer of host members into pinned staging (run_groups),
// ONE driver of groups on device staging (run_groups_staged), ONE run of host members through a device form (run_members_staged).
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

// The classes whose table entry is a SmallMember (both LZSS classes, the Huffman encoders, the rune decoder): member k is idx[k] as it
// came, the status word is the answer.  in_bytes(k) / out_bytes(k): the slots of member idx[k].
template <class InBytes, class OutBytes, class Launch>
int run_member_groups(Ctx &c, const char *what, const std::vector<size_t> &idx, const uint8_t *const *ins, const size_t *lens,
                      InBytes in_bytes, OutBytes out_bytes, Launch launch, const SmallTake &take, std::vector<size_t> &back, size_t *failed,
                      std::vector<size_t> *back_runes) {
    return run_groups<SmallMember>(c, what, idx.size(),
        [&](size_t k) { const size_t i = idx[k]; return GroupItem{i, ins[i], lens[i], (size_t)in_bytes(k), (size_t)out_bytes(k)}; },
        [&](SmallMember &m, size_t k, uint8_t *, const MemberSlots &o) { m = SmallMember{o.in, (uint32_t)lens[idx[k]], o.out, o.status}; },
        launch, [](const uint32_t *w) { return w[0]; }, take, back, failed, back_runes);
}

// The grouped kernels on members that lie in device memory (the batch calls on device buffers, rsn.h): ONE driver for every
// family of classes.  The same groups (next_group, GroupLayout), the staging in device scratch (Slot::GD_STAGE); per group one small copy
// up, the group's tables from a pinned region of its own, then the family's launches -- gather, the class's kernel, scatter.  No host wait
// between the groups (the stream orders the staging's reuse) and one at the end, when the answers come down: answers[k] is GROUP_BACK,
// GROUP_BACK_RUNES or the length of member k's result, complete in its d_out when at most its out_cap.  A family states what differs:
// ENTRY, a member's table entry in its group's layout; UP, the bytes of table it sends up; in_bytes(k) / out_bytes(k), its slots; fill(tab,
// g, q, k, o, ib, ob), member k as the q-th of its group of g into the group's pinned tables (o: its slots); up_at(g), where in the staging
// those g * UP bytes go (d_tab); launch(g, base, d_tab, d_ans), which queues the three steps.
template <size_t ENTRY, size_t UP, class InBytes, class OutBytes, class Fill, class UpAt, class Launch>
int run_groups_staged(Ctx &c, hipStream_t s, const char *what, size_t count, size_t group_bytes, const InBytes &in_bytes, const OutBytes &out_bytes, const Fill &fill,
                      const UpAt &up_at, const Launch &launch, std::vector<uint32_t> &answers) {
    answers.assign(count, GROUP_PENDING);
    if (count == 0) return RSN_OK;
    auto need = [&](size_t k) { return group_need(ENTRY, in_bytes(k), out_bytes(k)); };
    // the groups first: the largest one sizes the staging, and every group's tables have a pinned region of their own -- no group waits
    // for the copy of the one before it
    std::vector<GroupCut> cuts;
    size_t stage = 0;
    for (size_t j = 0; j < count;) { const GroupCut cut = next_group(j, count, SMALL_GROUP_MAX, group_bytes, need); stage = std::max(stage, cut.bytes); cuts.push_back(cut); j = cut.hi; }
    const size_t tables = count * UP, down = round_up(count * sizeof(uint32_t), 16);
    Admission gate(c, slotset::GROUP_DEV); gate.admit(stage + down, ADMIT_FROM);
    void *pp, *d_stage, *d_ans;
    int rc = pinned_buf(c, tables + down, &pp); if (rc) return rc;
    rc = dev_buf(c, Slot::GD_STAGE, stage + 64, &d_stage); if (rc) return rc;
    rc = dev_buf(c, Slot::GD_LENS, down, &d_ans); if (rc) return rc;
    uint8_t *pin = (uint8_t *)pp, *base = (uint8_t *)d_stage;
    size_t j = 0;
    for (const GroupCut &cut : cuts) {
        const size_t g = cut.hi - j;
        uint8_t *tab = pin + j * UP, *d_tab = base + up_at(g);
        GroupLayout lay(g, ENTRY);
        for (size_t q = 0; q < g; q++) { const size_t ib = in_bytes(j + q), ob = out_bytes(j + q); fill(tab, g, q, j + q, lay.member(ib, ob), ib, ob); }
        if (lay.end() != cut.bytes || lay.end() > 0xFFFFFFFFull) return c.fail(RSN_ERR_DEVICE, "%s: internal error: a group of %zu members lays out to %zu bytes, cut at %zu", what, g, lay.end(), cut.bytes);
        RSN_HIP(copy_async(d_tab, tab, g * UP, hipMemcpyHostToDevice, s));
        rc = launch((uint32_t)g, base, d_tab, (uint32_t *)d_ans + j); if (rc) return rc;
        j = cut.hi;
    }
    uint32_t *h_ans = (uint32_t *)(pin + tables);
    RSN_HIP(copy_async(h_ans, d_ans, count * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    RSN_HIP(hipStreamSynchronize(s));
    for (size_t k = 0; k < count; k++) {
        if (h_ans[k] == GROUP_PENDING) return c.fail(RSN_ERR_DEVICE, "%s: the grouped kernel finished without an answer for one of its members", what);
        answers[k] = h_ans[k];
    }
    return RSN_OK;
}
// The family of SmallMember entries (group_dev.hip: k_group_gather, the class's kernel as `launch` queues it in the host form,
// k_group_scatter) over the members idx[k] of `mem`.  group_bytes: a class of large members states a larger group of its own (huff_big.hip).
using GroupLaunch = std::function<int(hipStream_t s, uint32_t g, const SmallMember *tab, uint8_t *base)>;
using GroupSlotBytes = std::function<size_t(size_t k)>;
int run_groups_dev(Ctx &c, hipStream_t s, const char *what, const std::vector<size_t> &idx, const rsn_dev_member *mem, const GroupSlotBytes &in_bytes,
                   const GroupSlotBytes &out_bytes, const GroupLaunch &launch, std::vector<uint32_t> &answers, size_t group_bytes = SMALL_GROUP_BYTES);

// A plan launch over members where they lie (huff_dev_plan; the rune decoder's offer): a table of {src, n} goes up in one copy, launch(d_tab,
// d_front, d_sums) queues the plan kernel, a workgroup per candidate, the summaries come down in one copy, and the host waits once.  The
// scratch slot: `front` bytes of the kernel's own (*d_front), the entries, the summaries; *sums: in pinned memory, until its next user.
struct PlanEntry { const uint8_t *src; unsigned long long n; };
static_assert(sizeof(PlanEntry) == 16 && sizeof(HuffDevSummary) == 16, "16 bytes a candidate go up and 16 come down");
template <class Launch>
int plan_where_they_lie(Ctx &c, hipStream_t s, Slot slot, size_t front, const std::vector<size_t> &cand, const rsn_dev_member *mem, Launch launch,
                        void **d_front, const HuffDevSummary **sums) {
    const size_t k = cand.size(), up = k * sizeof(PlanEntry), down = k * sizeof(HuffDevSummary);
    void *pp, *dp;
    int rc = pinned_buf(c, up + down, &pp); if (rc) return rc;
    rc = dev_buf(c, slot, front + up + down, &dp); if (rc) return rc;
    PlanEntry *h_tab = (PlanEntry *)pp, *d_tab = (PlanEntry *)((uint8_t *)dp + front);
    HuffDevSummary *h_sum = (HuffDevSummary *)(h_tab + k), *d_sum = (HuffDevSummary *)(d_tab + k);
    for (size_t q = 0; q < k; q++) h_tab[q] = PlanEntry{(const uint8_t *)mem[cand[q]].d_in, (unsigned long long)mem[cand[q]].n};
    RSN_HIP(copy_async(d_tab, h_tab, up, hipMemcpyHostToDevice, s));
    rc = launch((const PlanEntry *)d_tab, dp, d_sum); if (rc) return rc;
    RSN_HIP(copy_async(h_sum, d_sum, down, hipMemcpyDeviceToHost, s));
    RSN_HIP(hipStreamSynchronize(s));
    *d_front = dp; *sums = h_sum;
    return RSN_OK;
}

// Host members through a class's DEVICE form, for the classes whose kernels never run on pinned host memory (huff_big.hip, huff_big_dec.hip):
// a RUN of members -- up to STAGED_RUN_BYTES of table, inputs and output slots (group_layout.h) -- is packed into the pinned staging and goes
// up in ONE copy (Slot::STAGE_IN), the class's run_dev runs it into Slot::STAGE_OUT, and the output slots come down in one copy.  The pinned
// staging is the device form's too (its tables and answers): the copy up is waited for before it, the buffer taken again behind it.
// Results, hand-backs and *failed as run_groups gives them.  The class states its members as RunItems (the index in the call, the slots,
// what of the output slot the device form may fill), TABLE, an entry of the table in front of the inputs (0: none), slot_error, the internal
// error's format (what, bytes, slot), and two functions: pack(k, r, g, d_table, tab, in) packs member k as the r-th of its run of g -- its
// table entry (the table at d_table on the device) at `tab`, its input at `in` -- and returns the input's bytes; run_dev(s, all, mem,
// answers) is the device form over the run's member table.
struct RunItem { size_t i, in_bytes, out_bytes, out_cap; };
constexpr size_t STAGED_RUN_BYTES = 4 * HUFF_BIG_GROUP_BYTES;
template <size_t TABLE, class Pack, class RunDev>
int run_members_staged(Ctx &c, const char *what, const char *slot_error, const std::vector<RunItem> &items, Pack pack, RunDev run_dev,
                       const SmallTake &take, std::vector<size_t> &back, size_t *failed, std::vector<size_t> *back_runes) {
    static_assert(TABLE % 16 == 0, "the input slots start behind the table, 16-aligned");
    const size_t count = items.size();
    if (count == 0) return RSN_OK;
    int rc = ctx_init(c); if (rc) { *failed = items[0].i; return rc; }
    hipStream_t s = c.own_stream;
    auto need = [&](size_t k) { return run_need(TABLE, items[k].in_bytes, items[k].out_bytes); };
    std::vector<rsn_dev_member> mem;
    std::vector<size_t> all, out_at;
    std::vector<uint32_t> answers;
    for (size_t j = 0; j < count;) {
        const GroupCut cut = next_group(j, count, SMALL_GROUP_MAX, STAGED_RUN_BYTES, need);
        const size_t g = cut.hi - j;
        *failed = items[j].i;
        RunLayout whole(g, TABLE);
        for (size_t q = 0; q < g; q++) whole.member(items[j + q].in_bytes, items[j + q].out_bytes);
        const size_t in_total = whole.in_total(), out_total = whole.out_total();
        Admission gate(c, slotset::STAGING | slotset::GROUP_DEV); gate.admit(2 * (in_total + out_total), ADMIT_FROM);
        void *pp, *d_in, *d_out;
        rc = pinned_buf(c, std::max(in_total, out_total) + 64, &pp); if (rc) return rc;
        rc = dev_buf(c, Slot::STAGE_IN, in_total + 64, &d_in); if (rc) return rc;
        rc = dev_buf(c, Slot::STAGE_OUT, out_total + 64, &d_out); if (rc) return rc;
        uint8_t *pin = (uint8_t *)pp;
        mem.assign(g, rsn_dev_member{}); all.resize(g); out_at.resize(g);
        RunLayout lay(g, TABLE);
        for (size_t q = 0; q < g; q++) {
            const RunItem &m = items[j + q];
            const RunSlots o = lay.member(m.in_bytes, m.out_bytes);
            mem[q].n = pack(j + q, q, g, (const void *)d_in, pin + q * TABLE, pin + o.in);
            mem[q].d_in = (uint8_t *)d_in + o.in; mem[q].d_out = (uint8_t *)d_out + o.out; mem[q].out_cap = m.out_cap;
            all[q] = q; out_at[q] = o.out;
        }
        RSN_HIP(copy_async(d_in, pin, in_total, hipMemcpyHostToDevice, s));
        RSN_HIP(hipStreamSynchronize(s));                                 // (the staging is the device form's from here on)
        rc = run_dev(s, all, mem.data(), answers); if (rc) return rc;
        if (const size_t down = run_down(g, answers, out_at)) {
            rc = pinned_buf(c, std::max(in_total, out_total) + 64, &pp); if (rc) return rc;
            pin = (uint8_t *)pp;
            RSN_HIP(copy_async(pin, d_out, down, hipMemcpyDeviceToHost, s));
            RSN_HIP(hipStreamSynchronize(s));
        }
        for (size_t q = 0; q < g; q++) {
            const size_t i = items[j + q].i;
            const uint32_t v = answers[q];
            if (group_is_back(v)) { (v == GROUP_BACK_RUNES && back_runes ? *back_runes : back).push_back(i); continue; }
            if (v > mem[q].out_cap) { *failed = i; return c.fail(RSN_ERR_DEVICE, slot_error, what, v, (size_t)mem[q].out_cap); }
            rc = take(i, pin + out_at[q], v); if (rc) { *failed = i; return rc; }
        }
        j = cut.hi;
    }
    return RSN_OK;
}

// The same for a class whose input goes up as it is (huff_big.hip, lzss_tile.hip, lzss_tile_dec.hip): no table, an input slot the member's
// bytes rounded up to 16, an output slot of out_bytes(n).  noun: what the internal error calls a result beyond its slot.
template <class OutBytes, class RunDev>
int run_members_copied(Ctx &c, const char *what, const char *noun, const std::vector<size_t> &idx, const uint8_t *const *ins, const size_t *lens, OutBytes out_bytes,
                       RunDev run_dev, const SmallTake &take, std::vector<size_t> &back, size_t *failed, std::vector<size_t> *back_runes) {
    std::vector<RunItem> items;
    for (size_t i : idx) items.push_back(RunItem{i, group_round16(lens[i]), out_bytes(lens[i]), out_bytes(lens[i])});
    const std::string slot_error = std::string("%s: internal error: ") + noun + " of %u bytes in a slot of %zu";
    return run_members_staged<0>(c, what, slot_error.c_str(), items,
        [&](size_t k, size_t, size_t, const void *, uint8_t *, uint8_t *in) { memcpy(in, ins[idx[k]], lens[idx[k]]); return lens[idx[k]]; },
        run_dev, take, back, failed, back_runes);
}
// the x of a tiled class's grid: tiles(n) of the largest of the members idx of `mem`, n at most n_cap, one at least
template <class Tiles>
uint32_t grid_tiles_of_largest(const std::vector<size_t> &idx, const rsn_dev_member *mem, size_t n_cap, Tiles tiles) {
    size_t n_max = 0;
    for (size_t i : idx) n_max = std::max(n_max, (size_t)mem[i].n);
    return std::max(1u, (uint32_t)tiles((uint32_t)std::min(n_max, n_cap)));
}

// A class of SmallMember entries is stated ONCE, as a type K -- K::what (the name in messages), K::in_bytes(n) / K::out_bytes(n) (the slots of
// a member of n bytes, group_layout.h) and K::launch(c, s, g, tab, base, window) (the group's kernel) -- and both of its runners, the
// host-buffer form and the device-buffer form (BatchClass::run / run_dev, codecs.h), are these two.
template <class K>
int class_run(Ctx &c, const std::vector<size_t> &idx, const uint8_t *const *ins, const size_t *lens, int64_t window,
              const SmallTake &take, std::vector<size_t> &back, size_t *failed, std::vector<size_t> *back_runes) {
    return run_member_groups(c, K::what, idx, ins, lens, [&](size_t k) { return K::in_bytes(lens[idx[k]]); }, [&](size_t k) { return K::out_bytes(lens[idx[k]]); },
        [&](hipStream_t s, uint32_t g, const SmallMember *tab, uint8_t *base) { return K::launch(c, s, g, tab, base, window); }, take, back, failed, back_runes);
}
template <class K>
int class_run_dev(Ctx &c, hipStream_t s, const std::vector<size_t> &idx, const rsn_dev_member *mem, int64_t window, const DevPlans *, std::vector<uint32_t> &answers) {
    return run_groups_dev(c, s, K::what, idx, mem, [&](size_t k) { return K::in_bytes(mem[idx[k]].n); }, [&](size_t k) { return K::out_bytes(mem[idx[k]].n); },
        [&](hipStream_t s2, uint32_t g, const SmallMember *tab, uint8_t *base) { return K::launch(c, s2, g, tab, base, window); }, answers);
}

}  // namespace rsn
