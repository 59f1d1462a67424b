// group_dev.hip -- the grouped batch kernels on members that lie in device memory (the batch calls on device buffers, rsn.h).
// The host form (group_run.h: run_groups) packs a group's members into pinned staging with memcpy and reads the results out of it; here the
// staging is device scratch and two kernels stand where the host's copies stood: k_group_gather in front of the class's kernel,
// k_group_scatter behind it.  The class's kernel is the host form's, launched unchanged with the device staging as `base`.  The loop over
// the groups is run_groups_staged (group_run.h), the one driver of every family; this unit is the family of SmallMember entries.  What
// crosses PCIe per group is its tables (64 bytes a member, one copy up) and per class its answers (4 bytes a member, one copy down).
// Here too: the two waits for words in pinned memory (codecs.h: flags_wait, group_wait) that every grouped class and single small call
// of every codec ends with.
#include <atomic>
#include <chrono>
#include <thread>

#include "group_run.h"

namespace rsn {

namespace {

constexpr int GD_THREADS = 256;

// a member of a group: where it comes from, where its result goes, and its slots in the staging (the SmallMember beside it says the same to
// the class's kernel)
struct GatherEntry {
    const uint8_t *src; uint8_t *dst;
    unsigned long long cap;                       // bytes of dst (0: a size query, dst may be null)
    uint32_t n, in_off, in_bytes, out_off, out_bytes, status_off;
};
static_assert(sizeof(GatherEntry) == 48 && (sizeof(SmallMember) + sizeof(GatherEntry)) % 16 == 0, "a group's two tables are whole 16-byte units");
constexpr size_t GD_ENTRY = sizeof(SmallMember) + sizeof(GatherEntry);

// A workgroup per member: the member's n bytes into its input slot, 16 at a time, zeros from byte n to the slot's end -- the class kernels
// rely on those zeros, so what lies behind the member in the caller's memory never takes their place: the one unit that reaches beyond
// src + n is masked, and nothing is loaded at or behind src + n rounded up to 16.  Then the status word: GROUP_PENDING.
__global__ __launch_bounds__(GD_THREADS) void k_group_gather(const GatherEntry *__restrict__ tab, uint8_t *__restrict__ base) {
    const GatherEntry e = tab[blockIdx.x];
    const uint4 *src = reinterpret_cast<const uint4 *>(e.src);
    uint4 *dst = reinterpret_cast<uint4 *>(base + e.in_off);
    const uint32_t units = e.in_bytes / 16, full = e.n / 16, rest = e.n & 15;
    for (uint32_t u = threadIdx.x; u < units; u += GD_THREADS) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (u < full) v = src[u];
        else if (u == full && rest) {
            v = src[u];
            uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                const uint32_t keep = rest > 4 * k ? min(rest - 4 * k, 4u) : 0u;   // bytes of word k that are the member's
                w[k] = keep == 4 ? w[k] : keep == 0 ? 0u : w[k] & ((1u << (8 * keep)) - 1);
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        dst[u] = v;
    }
    if (threadIdx.x == 0) *reinterpret_cast<uint32_t *>(base + e.status_off) = GROUP_PENDING;
}

// A workgroup per member, behind the class's kernel on the stream: the status word into the class's compact array -- GROUP_BACK, GROUP_BACK_RUNES, or the
// length of the result -- and, when the result fits the member's buffer, the output slot into it: whole 16-byte units, then the tail byte
// by byte, never a byte at or behind dst + len.  A word no kernel of the class can have written (still GROUP_PENDING, or a length beyond
// the output slot) goes down as GROUP_PENDING: the host words it as the device failure it is, and nothing is copied.
__global__ __launch_bounds__(GD_THREADS) void k_group_scatter(const GatherEntry *__restrict__ tab, const uint8_t *__restrict__ base, uint32_t *__restrict__ answers) {
    const GatherEntry e = tab[blockIdx.x];
    uint32_t v = *reinterpret_cast<const uint32_t *>(base + e.status_off);
    if (!group_is_back(v) && v > e.out_bytes) v = GROUP_PENDING;
    if (threadIdx.x == 0) answers[blockIdx.x] = v;
    if (v >= GROUP_BACK_RUNES || v > e.cap) return;                          // (a hand-back of either kind, or no answer)
    const uint4 *src = reinterpret_cast<const uint4 *>(base + e.out_off);
    uint4 *dst = reinterpret_cast<uint4 *>(e.dst);
    const uint32_t full = v / 16;
    for (uint32_t u = threadIdx.x; u < full; u += GD_THREADS) dst[u] = src[u];
    const uint32_t i = full * 16 + threadIdx.x;
    if (threadIdx.x < 16 && i < v) e.dst[i] = base[e.out_off + i];
}

}  // namespace

int flags_wait(Ctx &c, hipStream_t s, const uint32_t *flags, uint32_t n, const char *what) {
    const volatile uint32_t *vf = flags;
    auto pending = [&] { uint32_t p = 0; for (uint32_t i = 0; i < n; i++) p |= vf[i] == GROUP_PENDING; return p != 0; };
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 1;; spins++) {
        if (!pending()) { std::atomic_thread_fence(std::memory_order_acquire); return RSN_OK; }
        if ((spins & 1023) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(5)) {
            RSN_HIP(hipStreamSynchronize(s));
            if (pending()) return c.fail(RSN_ERR_DEVICE, "%s: a small-input kernel finished without its answer", what);
            return RSN_OK;
        }
        __builtin_ia32_pause();
    }
}

int group_wait(Ctx &c, hipStream_t s, const uint8_t *base, const std::vector<uint32_t> &off, uint32_t pending, const char *what) {
    auto at = [&](size_t k) { return *reinterpret_cast<const volatile uint32_t *>(base + off[k]); };
    const auto t0 = std::chrono::steady_clock::now();
    size_t k = 0;                                                                  // every member before k has answered
    for (uint32_t spins = 1;; spins++) {
        while (k < off.size() && at(k) != pending) k++;
        if (k == off.size()) { std::atomic_thread_fence(std::memory_order_acquire); return RSN_OK; }
        if ((spins & 1023) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(5)) break;
        __builtin_ia32_pause();
    }
    for (;;) {                                                                     // (a large group, or a busy device: the stream, with a limit)
        const hipError_t e = hipStreamQuery(s);
        if (e == hipSuccess) break;
        if (e != hipErrorNotReady) return c.fail(RSN_ERR_DEVICE, "%s: hipStreamQuery: %s", what, hipGetErrorString(e));
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(20)) return c.fail(RSN_ERR_DEVICE, "%s: the grouped kernel did not finish within 20 s", what);
        std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
    for (; k < off.size(); k++) if (at(k) == pending) return c.fail(RSN_ERR_DEVICE, "%s: the grouped kernel finished without an answer for one of its members", what);
    std::atomic_thread_fence(std::memory_order_acquire);
    return RSN_OK;
}

int run_groups_dev(Ctx &c, hipStream_t s, const char *what, const std::vector<size_t> &idx, const rsn_dev_member *mem, const GroupSlotBytes &in_bytes,
                   const GroupSlotBytes &out_bytes, const GroupLaunch &launch, std::vector<uint32_t> &answers, size_t group_bytes) {
    return run_groups_staged<GD_ENTRY, GD_ENTRY>(c, s, what, idx.size(), group_bytes, in_bytes, out_bytes,
        [&](uint8_t *tab, size_t g, size_t q, size_t k, const MemberSlots &o, size_t ib, size_t ob) {
            const rsn_dev_member &m = mem[idx[k]];
            ((SmallMember *)tab)[q] = SmallMember{o.in, (uint32_t)m.n, o.out, o.status};
            ((GatherEntry *)((SmallMember *)tab + g))[q] = GatherEntry{(const uint8_t *)m.d_in, (uint8_t *)m.d_out, m.d_out ? (unsigned long long)m.out_cap : 0ull,
                                                                      (uint32_t)m.n, o.in, (uint32_t)ib, o.out, (uint32_t)ob, o.status};
        }, [](size_t) { return (size_t)0; },
        [&](uint32_t g, uint8_t *base, uint8_t *, uint32_t *d_ans) {
            const GatherEntry *d_gat = (const GatherEntry *)(base + g * sizeof(SmallMember));
            RSN_LAUNCH("group_gather", k_group_gather, dim3(g), dim3(GD_THREADS), 0, s, d_gat, base);
            const int rc = launch(s, g, (const SmallMember *)base, base); if (rc) return rc;
            RSN_LAUNCH("group_scatter", k_group_scatter, dim3(g), dim3(GD_THREADS), 0, s, d_gat, (const uint8_t *)base, d_ans);
            return RSN_OK;
        }, answers);
}

}  // namespace rsn
