// rsn_common.h -- per-thread context, scratch arena, error plumbing and
// kernel-launch profiling shared by the codec translation units.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rsn.h"

namespace rsn {

struct ProfSlot {
    std::string name;
    uint64_t launches = 0;
    double total_ms = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

// The scratch slots of a thread's arena (Ctx::bufs, dev_buf): one row per slot -- who allocates it, what it holds, and in [..] the
// codec gates that give its block back (E: the LZSS encoder's, D: the LZSS decoder's; X*: released by X's gate though X never allocates
// it; the masks are below the table).  The gates of the host-buffer calls release what E releases plus the staging pair; the layered
// calls' gate releases those and its own four slots; the layered batch calls' gate what E releases and its own five; the batch round
// trip's gate those and its verify slot; the batch suite's gate those and its keep slot.
// A slot with two users is shared by convention: every codec call synchronises its stream before it returns, and the calls of one
// thread -- the layers of a layered call included -- run one after the other, so the two users are never live together.
// The numbers are fixed: DESIGN 4.8 and comments cite them, and a parked arena is adopted by index.
enum class Slot : int {
    HE_TILE_HIST = 0,   // Huffman encoder: per-tile histograms
    HE_BYTE_HIST = 1,   // Huffman encoder: the 256 byte counts
    HE_RUNE_HIST = 2,   // Huffman encoder, rune path: a count per rune
    HE_CODES = 3,       // Huffman encoder: the code table in the form its emit kernel wants (flat / rune list / Tab)
    HE_TILE_BITS = 4,   // Huffman encoder: the tiles' bit counts and offsets
    HD_TABLES = 5,      // Huffman decoder: first-level table, tree children, second level
    H_RUNES_SUBSEQ = 6, // SHARED -- Huffman encoder, rune path: rune flags, offsets and (rune, count) pairs; Huffman decoder: the subsequences' exit / entry / byte records
    HD_BLOCKS = 7,      // Huffman decoder: the blocks' byte counts and offsets
    LE_ESC_BLOCKS = 8,  // LZSS encoder: the escape pass's per-block counts, offsets and flags (a sectioned call: its flag word) [E]
    LE_ESCAPED = 9,     // LZSS encoder: the escaped stream [E]
    LE_KEYS = 10,       // LZSS encoder: the positions' hash keys (4 bytes each; lzss_big: 8) [E]
    LE_LISTS_EXITS = 11,// LZSS encoder: the chain walk's compact lists, later the general parse's exits (2 bytes a position), lzss_big's two next-arrays
                        //   -- grow-only: the lists' larger block stays when the exits ask for less [E]
    LE_TILES = 12,      // LZSS encoder: the parse tiles' bytes, offsets, entry bits and chains (lzss_big: its blocks' and the on-bits) [E]
    LD_BLOCKS = 13,     // LZSS decoder: the count pass's per-block lengths, offsets and flags [D, E*]
    LD_DESC = 14,       // LZSS decoder: the tiles' descriptors (tile path) or a source index per escaped byte [D, E*]
    LD_ESCAPED = 15,    // LZSS decoder: the escaped stream [D, E*]
    LD_UNESCAPE = 16,   // LZSS decoder: the unescape blocks' lengths, offsets, summaries (lzss_unescape's layout) [D, E*]
    LE_SUPER = 17,      // LZSS encoder: the general parse's super-tiles and group entries [E]
    LE_STRIPS = 18,     // LZSS encoder: the strips' heavy / redo / dense marks [E]
    LZ_DUMP_TILES = 19, // SHARED -- LZSS encoder: the chain walk's dump; LZSS decoder: the tile list [E, D]
    STAGE_IN = 20,      // host-buffer calls: the uploaded input (stage_input, rsn_api.hip)
    STAGE_OUT = 21,     // host-buffer calls: the codec's output before it goes down
    LD_MAPS = 22,       // LZSS decoder, tile path: the groups' two map arrays and tails [D, E*]
    LD_RUNS = 23,       // LZSS decoder, tile path: the tiles' runs and their counts [D, E*]
    SCAN_PARTIALS = 24, // SHARED by all four directions -- scan_u64's block partials (huff_encode.hip): both Huffman directions, the LZSS encoder (lzss_big too) and
                        //   the LZSS decoder call it, each scan finished before the next begins [E; not D, though the decoder allocates it too]
    LE_PREV = 25,       // LZSS encoder: the chain walk's n_prev partials [E, D*]
    RUNES_REDO = 26,    // SHARED -- Huffman encoder, rune path: the rune start map; LZSS encoder: the chain walk's redo list [E]
    LZ_COUNTS = 27,     // SHARED -- LZSS encoder: the compact lists' counts; LZSS decoder: the count pass's needs and spans [E, D]
    RING_IN0 = 28, RING_IN1 = 29, RING_IN2 = 30,        // the batch pipeline's ring (ring_in / ring_out below): the chunks' inputs ...
    RING_OUT0 = 31, RING_OUT1 = 32, RING_OUT2 = 33,     // ... and their segments; freed by the batch itself above RSN_BATCH_KEEP_MIB
    HD_TILE_WORDS = 34, // Huffman decoder, one-pass path: the tile words and block map
    LE_SAME = 35,       // LZSS encoder: k_esc_try's block flags [E]
    LZ_SECTION = 36,    // SHARED -- a section's stream.  LZSS encoder: the aligned copy; LZSS decoder: the escaped bytes in front + the section's tokens [E, D]
    HS_INPUT = 37,      // small-input Huffman path: the device copy
    HS_DEC_MAPS = 38,   // small-input Huffman decoder: the blocks' maps and flags (keyed on Buf::gen)
    L_IN = 39,          // layered calls: the uploaded input (the round trip keeps it to the end) [layered]
    L_A = 40,           // layered calls: the stream between the layers ... [layered]
    L_B = 41,           // ... the two taking turns [layered]
    L_STAT = 42,        // layered round trip: the two histograms and the first-difference word [layered]
    AR_STATE = 43,      // arithmetic codec: the members' state records (table, coder state, cursors), their summaries, sizes and offsets [arith]
    AR_RAW = 44,        // arithmetic codec: the encoder's raw bits before the front pad (a device-buffer call: its descriptor in front);
                        //   the decoder's descriptors (the batch call on device buffers: both directions' descriptors in front) [arith]
    GD_STAGE = 45,      // batch calls on device buffers (group_dev.hip): a group's staging -- the member and gather tables, then the members' slots [group_dev]
    GD_LENS = 46,       // batch calls on device buffers: a class's answers, a word per member [group_dev]
    GD_PLANS = 47,      // Huffman decompress batch on device buffers (huff_dev.hip): the candidates' plans (a HuffDevPlan each), then their table entries
                        //   and their summaries -- written by k_huff_dev_plan, read by every class's groups until the call ends [huff_dev]
    LB_STAGE = 48,      // layered batch calls (rsn_api.hip: layers_batch): a run's inputs packed on the way up (the host form); behind the last
                        //   step the move table and, in the host form, the results packed on the way down [layers_batch]
    LB_A = 49,          // layered batch calls: the members' slots between the steps ... [layers_batch]
    LB_B = 50,          // ... the two arenas taking turns [layers_batch]
    LB_XA = 51,         // layered batch calls: the slots of the members that outgrew their first slot in LB_A and were run again alone ... [layers_batch]
    LB_XB = 52,         // ... and of those that outgrew theirs in LB_B [layers_batch]
    LB_VERIFY = 53,     // batch round trip (rsn_api.hip: suite_batch_flow over one list): a run's verify table, behind it the stats block -- the members'
                        //   first-difference words and histograms (roundtrip_batch_layout.h) [roundtrip_batch]
    GD_RUNE_PLANS = 54, // Huffman decompress batch on device buffers (huff_rune_dec.hip): the rune candidates' table entries and their summaries -- written by
                        //   k_huff_dev_rune_plan, read by the host once; the call's gate gives it back with the plan table [huff_dev]
    LB_KEEP = 55,       // batch suite (rsn_api.hip: suite_batch_flow): a run's kept node outputs -- a slot per kept node of the lists' prefix
                        //   tree and member (suite_layout.h), written by the node's compress step and read by every user of the node [suite_batch]
    GD_BIG_TILES = 56,  // Huffman compress batch, big class (huff_big.hip; huff_big_layout.h): per member of a group its tiles' counts and flags, its code
                        //   table, its tiles' first bits and its verdict -- written by the count and plan launches, read by the emit launch [group_dev]
    GD_BIG_DEC = 57,    // Huffman decompress batch, tiled class (huff_big_dec.hip; huff_big_dec_layout.h): per member of a group its tiles' 32-entry maps,
                        //   their true entries, first output bytes and symbol counts, and its verdict -- written by the map and chain launches, read by the emit launch [group_dev]
    GD_LZSS_TILES = 58, // LZSS compress batch, tiled class (lzss_tile.hip; lzss_tile_layout.h): a table of the members' offsets, then per member of a group its
                        //   verdict and lengths, its tiles' first output bytes, a key a position and its escaped stream -- written by the esc, search and chain
                        //   launches, read by the emit launch [group_dev]
    GD_LZSS_TILE_DEC = 59, // LZSS decompress batch, tiled class (lzss_tile_dec.hip; lzss_tile_dec_layout.h): per member of a group its verdict and E, its stream
                        //   tiles' outputs, flags, needs and first output bytes, its output tiles' entries, its escaped image and a descriptor a position --
                        //   written by the parse, plan and resolve launches, read by the finish launch [group_dev]
    GD_RUNE_MID_PLANS = 60, // Huffman decompress batch on device buffers (huff_rune_mid_dec.hip): the mid-size rune candidates' table entries and their
                        //   summaries -- written by k_huff_dev_rune_mid_plan, read by the host once; the call's gate gives it back with the plan table [huff_dev]
};
constexpr int RING = 3;                                                  // the batch pipeline's depth: RING inputs, RING segments
constexpr Slot ring_in(int r) { return (Slot)((int)Slot::RING_IN0 + r); }
constexpr Slot ring_out(int r) { return (Slot)((int)Slot::RING_OUT0 + r); }
template <class... S> constexpr unsigned long long slot_mask(S... s) { return ((1ull << (int)s) | ... | 0ull); }

namespace slotset {   // bit k = slot k (scratch_release)
using S = Slot;
// what each codec allocates (the structural checks below; the rows above say what for)
constexpr unsigned long long HUFF_OWN = slot_mask(S::HE_TILE_HIST, S::HE_BYTE_HIST, S::HE_RUNE_HIST, S::HE_CODES, S::HE_TILE_BITS, S::HD_TABLES, S::H_RUNES_SUBSEQ, S::HD_BLOCKS, S::SCAN_PARTIALS, S::RUNES_REDO, S::HD_TILE_WORDS, S::HS_INPUT, S::HS_DEC_MAPS);
constexpr unsigned long long LZSS_ENC_OWN = slot_mask(S::LE_ESC_BLOCKS, S::LE_ESCAPED, S::LE_KEYS, S::LE_LISTS_EXITS, S::LE_TILES, S::LE_SUPER, S::LE_STRIPS, S::LZ_DUMP_TILES, S::SCAN_PARTIALS, S::LE_PREV, S::RUNES_REDO, S::LZ_COUNTS, S::LE_SAME, S::LZ_SECTION);
constexpr unsigned long long LZSS_DEC_OWN = slot_mask(S::LD_BLOCKS, S::LD_DESC, S::LD_ESCAPED, S::LD_UNESCAPE, S::LZ_DUMP_TILES, S::LD_MAPS, S::LD_RUNS, S::SCAN_PARTIALS, S::LZ_COUNTS, S::LZ_SECTION);
// what the gates give back: kept bit for bit as they have been (whether the oddities are meant is a question of behaviour, not of naming).
// The encoder's set is its own slots plus six that only the decoder allocates; the decoder's is its own WITHOUT the scan's partials,
// which it allocates but has never released, plus one slot of the encoder's
constexpr unsigned long long LZSS_ENC = LZSS_ENC_OWN | slot_mask(S::LD_BLOCKS, S::LD_DESC, S::LD_ESCAPED, S::LD_UNESCAPE, S::LD_MAPS, S::LD_RUNS);
constexpr unsigned long long LZSS_DEC = (LZSS_DEC_OWN & ~slot_mask(S::SCAN_PARTIALS)) | slot_mask(S::LE_PREV);
constexpr unsigned long long STAGING = slot_mask(S::STAGE_IN, S::STAGE_OUT);
constexpr unsigned long long LAYERED = slot_mask(S::L_IN, S::L_A, S::L_B, S::L_STAT);
constexpr unsigned long long RINGS = slot_mask(ring_in(0), ring_in(1), ring_in(2), ring_out(0), ring_out(1), ring_out(2));
constexpr unsigned long long HOST_CALL = STAGING | LZSS_ENC;              // (the decoder's set lies inside the encoder's)
constexpr unsigned long long LAYERED_CALL = HOST_CALL | LAYERED;
constexpr unsigned long long ARITH = slot_mask(S::AR_STATE, S::AR_RAW);   // the arithmetic codec's own: what its device-buffer calls' gate gives back
constexpr unsigned long long ARITH_HOST = STAGING | ARITH;                // ... and its host-buffer calls', which stage through the staging pair
constexpr unsigned long long GROUP_DEV = slot_mask(S::GD_STAGE, S::GD_LENS, S::GD_BIG_TILES, S::GD_BIG_DEC, S::GD_LZSS_TILES, S::GD_LZSS_TILE_DEC);   // the grouped kernels' staging on the device: what a class's run of the batch calls on device buffers gives back
constexpr unsigned long long HUFF_DEV_PLANS = slot_mask(S::GD_PLANS, S::GD_RUNE_PLANS, S::GD_RUNE_MID_PLANS);          // the plan table outlives the classes' runs: the call's own gate gives it back, never a class's
constexpr unsigned long long LAYERS_BATCH = slot_mask(S::LB_STAGE, S::LB_A, S::LB_B, S::LB_XA, S::LB_XB);   // the layered batch calls' own
constexpr unsigned long long LAYERS_BATCH_CALL = LZSS_ENC | LAYERS_BATCH;      // ... and what their gate gives back: the single calls that run inside a step leave the LZSS codecs' scratch
constexpr unsigned long long ROUNDTRIP_BATCH = slot_mask(S::LB_VERIFY);        // the batch round trip's own: the verify table and the stats block
constexpr unsigned long long ROUNDTRIP_BATCH_CALL = LAYERS_BATCH_CALL | ROUNDTRIP_BATCH;   // ... and what its gate gives back: both passes are the layered batch calls' steps
constexpr unsigned long long SUITE_BATCH = slot_mask(S::LB_KEEP);              // the batch suite's own: the kept node outputs
constexpr unsigned long long SUITE_BATCH_CALL = ROUNDTRIP_BATCH_CALL | SUITE_BATCH;   // ... and what its gate gives back: its passes are the batch round trip's
// (RING is written out three times: the enumerators, RINGS and this check change together)
static_assert(ring_in(RING) == Slot::RING_OUT0 && ring_out(RING - 1) == Slot::RING_OUT2, "the ring's slots are RING inputs, then RING segments");
static_assert(((STAGING | RINGS | LAYERED) & (LZSS_ENC | LZSS_DEC)) == 0, "a codec's gate releases no staging, ring or layered slot: their callers still use them");
static_assert(((STAGING | LAYERED) & (HUFF_OWN | LZSS_ENC_OWN | LZSS_DEC_OWN)) == 0, "no codec allocates a staging or a layered slot");
static_assert((LZSS_DEC & ~LZSS_ENC) == 0, "HOST_CALL covers both LZSS directions");
static_assert((GROUP_DEV & (HUFF_OWN | LZSS_ENC | LZSS_DEC | STAGING | RINGS | LAYERED | ARITH)) == 0, "the device staging is released by its own gate only: the single calls that follow a class never hold it");
static_assert((HUFF_DEV_PLANS & (GROUP_DEV | HUFF_OWN | LZSS_ENC | LZSS_DEC | STAGING | RINGS | LAYERED | ARITH)) == 0, "no class run and no single call gives the plan table back while the call still reads it");
static_assert((LAYERS_BATCH & (GROUP_DEV | HUFF_DEV_PLANS | HUFF_OWN | LZSS_ENC | LZSS_DEC | STAGING | RINGS | LAYERED | ARITH)) == 0, "no step of a layered batch call gives an arena back: the next step reads it");
static_assert((ROUNDTRIP_BATCH & (LAYERS_BATCH | GROUP_DEV | HUFF_DEV_PLANS | HUFF_OWN | LZSS_ENC | LZSS_DEC | STAGING | RINGS | LAYERED | ARITH)) == 0, "no step of either pass gives the verify slot back, and the verify pass regrows no arena it reads");
static_assert((SUITE_BATCH & (ROUNDTRIP_BATCH | LAYERS_BATCH | GROUP_DEV | HUFF_DEV_PLANS | HUFF_OWN | LZSS_ENC | LZSS_DEC | STAGING | RINGS | LAYERED | ARITH)) == 0, "no step, no verify pass and no other call's gate gives the kept outputs back: a later list of the run still reads them");
static_assert((int)S::GD_RUNE_MID_PLANS < 64, "a slot is a bit of a 64-bit mask");
static_assert((ARITH & (HUFF_OWN | LZSS_ENC | LZSS_DEC | STAGING | RINGS | LAYERED)) == 0, "the arithmetic codec shares no slot of its own with another codec or a caller");
}  // namespace slotset

// One per host thread (thread_local): device, stream, reusable device scratch
// buffers and pinned staging.  Nothing here is shared between threads.
struct Ctx {
    int device = 0;
    bool device_chosen = false;     // by rsn_device_set(); otherwise the first call picks RSN_DEVICE's (rsn_api.hip)
    bool inited = false;
    hipStream_t own_stream = nullptr;
    std::string err;
    bool prof = false;
    std::vector<ProfSlot> slots;
    std::vector<hipEvent_t> free_events;

    struct Buf { void *p = nullptr; size_t cap = 0; unsigned long long gen = 0; };   // gen: process-unique number of this allocation (dev_buf) -- an address can come back with other contents
    enum { N_BUFS = (int)Slot::GD_RUNE_MID_PLANS + 1 };   // (the table above)
    Buf bufs[N_BUFS];
    Buf &buf(Slot k) { return bufs[(int)k]; }
    void *pinned = nullptr; size_t pinned_cap = 0;
    bool lz_runs = false;           // the LZSS input in hand holds runs of a byte (k_esc_try's flag): lzss_encode_stream walks it with k_match_chain<RUNS>
    size_t gate_held = 0;           // scratch this thread's call in progress has been admitted with (rsn_api.hip: a nested admission is covered by it)

    ~Ctx();     // parks the device resources for the next thread (rsn_api.hip); makes no HIP call

    int fail(int code, const char *fmt, ...) {
        char tmp[512];
        va_list ap; va_start(ap, fmt); vsnprintf(tmp, sizeof tmp, fmt, ap); va_end(ap);
        err = tmp;
        return code;
    }
};

Ctx &ctx();
int ctx_init(Ctx &c);                       // lazy: picks device, creates stream
int dev_buf(Ctx &c, Slot slot, size_t bytes, void **out);  // grow-only scratch
int pinned_buf(Ctx &c, size_t bytes, void **out);
// admission of calls with gigabytes of scratch (rsn_api.hip): waits while the device's calls in flight need more than it holds
size_t scratch_admit(Ctx &c, size_t need);                                   // returns what to hand to scratch_release: `need`, or 0 inside a call that has been admitted already
void scratch_release(Ctx &c, size_t held, unsigned long long slots);         // ... and gives those slots' large buffers back when others wait (bit k = slot k); held == 0: nothing to do
// A call's place behind that gate: admitted at most once, released -- with the large buffers of `slots` when others wait -- on every way
// out.  from: needs below it pass without asking (ADMIT_FROM: the calls whose small sizes are not worth the lock).  The sites' four rules:
// admit(need) always asks (piped_call); the same with a need that may be 0 asks only when it is not, because scratch_admit(0) admits
// nothing (lzss_encode_dev); admit(need, ADMIT_FROM) asks from 64 MiB (host_call, the layered calls); the decoder calls admit late, once
// the escaped size is known.  Not copyable: a copy would release one admission twice.
constexpr size_t ADMIT_FROM = (size_t)64 << 20;
struct Admission {
    Ctx &c; unsigned long long slots; size_t held = 0; bool asked = false;
    Admission(Ctx &c_, unsigned long long slots_) : c(c_), slots(slots_) {}
    Admission(const Admission &) = delete; Admission &operator=(const Admission &) = delete;
    void admit(size_t need, size_t from = 0) { if (!asked && need >= from) { asked = true; held = scratch_admit(c, need); } }
    ~Admission() { scratch_release(c, held, slots); }
};
void scratch_forget(Ctx &c, size_t bytes);
unsigned long long scratch_queued(int device);                               // calls that have had to wait so far (tests)
void prof_collect(Ctx &c);
// hipFuncAttributeMaxDynamicSharedMemorySize belongs to the FUNCTION on a device, not to the calling thread: raised only, under a lock (r06:
// every thread kept its own "largest so far" and set the attribute whenever its own grew -- a thread with a small need lowered what another's
// next launch relied on)
int func_dyn_lds(Ctx &c, const void *fn, size_t bytes);

#define RSN_HIP(call)                                                                              \
    do {                                                                                           \
        hipError_t e__ = (call);                                                                   \
        if (e__ != hipSuccess)                                                                     \
            return c.fail(RSN_ERR_DEVICE, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__),  \
                          __FILE__, __LINE__);                                                     \
    } while (0)

// The grid of a persistent kernel (`fn` at `block` threads, no dynamic LDS) over `work` items: the blocks that are resident at once on
// c.device -- the occupancy query times the CUs -- and never more than `work`.  A constant grid above the resident count runs its
// surplus blocks as a second wave after the first has done all of its own work: a quarter of a 1 GiB flat encode at 2 blocks a CU
// (DESIGN 4.5).  Cached per (function, device, block) under one lock: the library is called from many threads at once.
inline int persistent_grid(Ctx &c, const void *fn, int block, size_t work, dim3 *grid) {
    struct Entry { const void *fn; int device, block; uint32_t blocks; };
    static std::mutex mu;
    static std::vector<Entry> *seen = new std::vector<Entry>();   // never destroyed: callers may still launch while the process exits
    uint32_t blocks = 0;
    {
        std::lock_guard<std::mutex> lk(mu);
        for (const Entry &e : *seen)
            if (e.fn == fn && e.device == c.device && e.block == block) { blocks = e.blocks; break; }
        if (!blocks) {
            int per_cu = 0, cus = 0;
            RSN_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, block, 0));
            RSN_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c.device));
            if (per_cu < 1 || cus < 1) return c.fail(RSN_ERR_DEVICE, "occupancy query: %d blocks of %d threads a CU on %d CUs", per_cu, block, cus);
            blocks = (uint32_t)per_cu * (uint32_t)cus;
            seen->push_back({fn, c.device, block, blocks});
        }
    }
    *grid = dim3((uint32_t)std::min<size_t>(work, blocks));
    return RSN_OK;
}

// Every copy command between host and device goes through here: rsn_prof_copied's process-wide byte counts (rsn.h), kept while
// profiling is on.  Device-to-device copies are not counted.
struct CopyCount { std::atomic<int> on{0}; std::atomic<unsigned long long> h2d{0}, d2h{0}; };
inline CopyCount g_copy_count;
inline hipError_t copy_async(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    if (g_copy_count.on.load(std::memory_order_relaxed)) {
        if (kind == hipMemcpyHostToDevice) g_copy_count.h2d.fetch_add(bytes, std::memory_order_relaxed);
        else if (kind == hipMemcpyDeviceToHost) g_copy_count.d2h.fetch_add(bytes, std::memory_order_relaxed);
    }
    return hipMemcpyAsync(dst, src, bytes, kind, s);
}

// Brackets a kernel launch with events when profiling is on.
struct ProfScope {
    Ctx &c; hipStream_t s; int slot = -1; hipEvent_t a = nullptr, b = nullptr;
    ProfScope(Ctx &c_, hipStream_t s_, const char *name) : c(c_), s(s_) {
        if (!c.prof) return;
        for (size_t i = 0; i < c.slots.size(); i++) if (c.slots[i].name == name) slot = (int)i;
        if (slot < 0) { c.slots.emplace_back(); c.slots.back().name = name; slot = (int)c.slots.size() - 1; }
        auto get = [&]() { hipEvent_t e = nullptr; if (!c.free_events.empty()) { e = c.free_events.back(); c.free_events.pop_back(); } else (void)hipEventCreate(&e); return e; };
        a = get(); b = get();
        (void)hipEventRecord(a, s);
    }
    ~ProfScope() {
        if (slot < 0) return;
        (void)hipEventRecord(b, s);
        c.slots[slot].pending.emplace_back(a, b);
    }
};

#define RSN_LAUNCH(name, kernel, grid, block, shmem, stream, ...)                                  \
    do {                                                                                           \
        {                                                                                          \
            rsn::ProfScope ps__(c, stream, name);                                                  \
            hipLaunchKernelGGL(kernel, grid, block, shmem, stream, __VA_ARGS__);                   \
        }                                                                                          \
        RSN_HIP(hipGetLastError());                                                                \
    } while (0)

// Streaming (touched-once) global accesses as `nt` loads / stores.  Which of the headline kernels' streams use them is a
// build-time A/B mask (Makefile: EXTRA=-DRSN_NT_MASK=<bits>, scripts/ab_nt.sh):
//   1 k_byte_hist loads   2 k_emit_flat loads   4 k_emit_flat stores   8 k_dec_flat loads   16 k_dec_flat stores
//   32 k_lzd_resolve's descriptor stores   64 k_lzd_emit's descriptor loads
// Measured (r03, 1 GiB, step = encode + decode in a loop; gpurun_out/ab_nt*.txt): only bit 1 pays -- k_byte_hist
// 0.231 -> 0.185 ms (5.8 TB/s) and the step 1.175 -> 1.137 ms.  The three kernels trade the write-back of the previous kernel's
// dirty lines among themselves (nt stores in k_dec_flat: that kernel +0.05 ms, the histogram after it -0.035; nt loads in the
// histogram: k_emit_flat +0.015 because the decoder's dirty lines are then still in the cache when it starts), so every other
// bit moves time between kernels and loses a little in total; walking k_emit_flat's chunks from the end (to meet what the
// histogram read last in the Infinity Cache) changed nothing.
#ifndef RSN_NT_MASK
#define RSN_NT_MASK 1
#endif
#ifdef __HIPCC__
typedef uint32_t rsn_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t rsn_u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
template <bool NT> __device__ __forceinline__ uint4 ld16(const uint4 *p) {
    if constexpr (NT) { const rsn_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const rsn_u32x4 *>(p)); return make_uint4(v.x, v.y, v.z, v.w); }
    else return *p;
}
template <bool NT> __device__ __forceinline__ uint32_t ld4(const uint32_t *p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}
template <bool NT> __device__ __forceinline__ void st16(uint4 *p, const uint4 &v) {
    if constexpr (NT) { rsn_u32x4 x = {v.x, v.y, v.z, v.w}; __builtin_nontemporal_store(x, reinterpret_cast<rsn_u32x4 *>(p)); }
    else *p = v;
}
// four dwords to an address that is only dword-aligned (global stores accept that)
template <bool NT> __device__ __forceinline__ void st16_a4(uint32_t *p, uint32_t a, uint32_t b, uint32_t c_, uint32_t d) {
    rsn_u32x4_a4 x = {a, b, c_, d};
    if constexpr (NT) __builtin_nontemporal_store(x, reinterpret_cast<rsn_u32x4_a4 *>(p));
    else *reinterpret_cast<rsn_u32x4_a4 *>(p) = x;
}
#endif

static inline size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }
static inline size_t round_up(size_t a, size_t b) { return ceil_div(a, b) * b; }

}  // namespace rsn
