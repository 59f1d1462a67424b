// layers_batch_layout.h -- the arithmetic of the layered batch calls (rsn.h: rsn_layers_*_batch, rsn_layers_*_batch_dev), as
// plain host code: no HIP include, so a CPU test (tests/layers_batch_layout_test.cpp) checks what keeps a step inside its arena -- slots at
// 16-byte offsets that do not overlap, the slack behind every slot, runs that are consecutive, cover the call and stay within the budget.
// rsn_api.hip's layers_batch is the user.
//
// A call's members are cut into RUNS; a run's members go through the layers together.  Step k of a run reads its members where step k - 1
// left them and writes each into a slot of the other of two arenas; a host-form run's inputs lie packed in a staging block in front of the
// first step, and its results are packed into one behind the last.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace rsn {

// what a run may hold at once unless the call says otherwise (RSN_LAYERS_BATCH_BUDGET, bytes, read at every call): DESIGN 7
constexpr size_t LB_BUDGET = (size_t)1 << 30;
// behind a slot's capacity: the single calls load whole 16-byte units, and up to 64 bytes from the last boundary at or before the end of
// their input (stage_buf, rsn_api.hip); run_chain gives the same 80
constexpr size_t LB_SLACK = 80;
// k_members_move's unit of work: a workgroup a tile
constexpr size_t LB_TILE = 65536;

constexpr size_t lb_round16(size_t v) { return (v + 15) & ~(size_t)15; }
constexpr size_t lb_slot_bytes(size_t cap) { return lb_round16(cap) + LB_SLACK; }
constexpr size_t lb_tiles(size_t len) { return (len + LB_TILE - 1) / LB_TILE; }
static_assert(LB_SLACK % 16 == 0 && LB_TILE % 16 == 0, "slots and tiles begin at 16-byte offsets");

// An arena of `count` slots: slot i holds caps[i] bytes and its slack and begins at offs[i].  Returns the arena's bytes.
inline size_t lb_arena(const size_t *caps, size_t count, std::vector<size_t> &offs) {
    offs.resize(count);
    size_t at = 0;
    for (size_t i = 0; i < count; i++) { offs[i] = at; at += lb_slot_bytes(caps[i]); }
    return at;
}

// `count` members back to back at 16-byte offsets -- a run's inputs on the way up, its results on the way down: member i's lens[i] bytes
// at offs[i].  Returns the bytes that cross (the sum of the lengths rounded up to 16); the device block behind it holds LB_SLACK more.
inline size_t lb_packed(const size_t *lens, size_t count, std::vector<size_t> &offs) {
    offs.resize(count);
    size_t at = 0;
    for (size_t i = 0; i < count; i++) { offs[i] = at; at += lb_round16(lens[i]); }
    return at;
}

// The runs of n members under `budget`: consecutive members, the first of a run always enters, a further one only while the run's bytes
// stay within the budget -- a member that exceeds it alone is a run of its own.  need(i): what member i holds at once.
struct LbRun { size_t lo, hi, bytes; };   // the run is [lo, hi)
template <class Need>
std::vector<LbRun> lb_runs(size_t n, size_t budget, Need need) {
    std::vector<LbRun> runs;
    for (size_t lo = 0; lo < n;) {
        size_t k = lo, bytes = 0;
        while (k < n) {
            const size_t b = need(k);
            if (k != lo && (b > budget || bytes > budget - b)) break;
            bytes = bytes > (size_t)-1 - b ? (size_t)-1 : bytes + b;
            k++;
        }
        runs.push_back({lo, k, bytes});
        lo = k;
    }
    return runs;
}

// what a member holds at once: its staged input (the host form; 0 when it lies in the caller's memory) and a slot in each arena
constexpr size_t lb_member_need(size_t staged_len, size_t slot_cap) { return lb_round16(staged_len) + 2 * lb_slot_bytes(slot_cap); }

}  // namespace rsn
