// huff_big_dec.hip -- the Huffman decoder for the big members of a decompress batch: streams of a byte alphabet that promise more than
// HUFF_MID_OUT_MAX bytes, where the output no longer fits one workgroup's LDS (huff_mid.hip), up to HUFF_BIG_OUT_MAX bytes from at most
// HUFF_BIG_PAY_MAX bytes of payload (codecs.h) -- every stream huff_big.hip's encoder writes.
//
// Inside a batch such a stream used to be the single call: the general decoder's launches, copy commands and a host wait, a member after
// the other.  The stream is one bit string without an index, so it is cut into TILES of its payload -- BIGD_LANES lanes of BIGD_S code bits,
// 7680 bytes (huff_big_dec_layout.h) -- and a group of members is three launches, queued one behind the other with nothing on the host
// between them.  They are the two halves of lane_dec_body's multi-block form (huff_small_body.h) with its wait taken out: there a block
// publishes its map and spins until the blocks before it have published theirs, which needs them co-resident; a group of hundreds of
// members cannot promise that, so the launch boundary is the wait.
//   map    k_huff_big_dec_map, a workgroup per tile: the tile's payload words and the look-ahead a codeword reaches into, the lookup table
//          from the member's child[], the lanes' maps of up to four starts settled in at most DEC_ROUNDS rounds (the flat code's shortcut
//          included) -- lane_dec_body<TILE_MAP>, which stops at the publication: the tile's 32-entry map "entered at bit c -> left at bit
//          c', n symbols" goes to the member's scratch.  No output image.
//   chain  k_huff_big_dec_chain, a wavefront per member: the tiles' maps composed in order from the first code bit (bigd_chain) into every
//          tile's true entry, first output byte and symbol count.  The verdict is complete here: a lost tile, an exit that is none, a
//          stream that ends inside a codeword, more symbols than the header promises, a tile beyond the emit image.  A member that is
//          handed back gets its status word here, and the emit launch stores no byte of it.
//   emit   k_huff_big_dec_emit, a workgroup per tile of a taken member: lane_dec_body<TILE_EMIT> -- the same lanes from the tile's known
//          entry, the symbols into an LDS image shifted so that 16-byte units of the output line up, whole units out as 16-byte stores, the
//          first and the last unit byte by byte.  A tile stores exactly the bytes [base, base + count): no byte is stored twice, nothing
//          is ORed into the output, and what the slot held before does not matter.
// The emit launch settles a subset of what the map launch settled -- its first lane is entered at one bit instead of 32, every other lane
// starts from the same first guess -- so every (lane, start) it meets the map launch met no later: it needs no more starts a lane and no
// more rounds, and it arrives at the count the chain computed.  Were that ever not so, the tile stores no length and the member's word
// stays GROUP_PENDING, which the host reports as an error: never wrong bytes.
// The member's two status words by the last of its tiles and the grid are the tiled classes' common shape (tile_dev.h); the
// done-counter is zeroed by the chain, and k_huff_dev_scatter reads the words.  No workgroup waits for another; every loop is bounded by
// the tile's bits, DEC_ROUNDS, the tiles of a member or a constant.
#include "huff_small_body.h"
#include "huff_big_dec_layout.h"
#include "tile_dev.h"

namespace rsn {
namespace {

constexpr int BD_T = 1024;                        // threads of a tile's workgroup
constexpr int BD_DL = BD_T - 64;                  // ... 15 wavefronts of lanes and the sixteenth for the first lane's 32 entries
constexpr int BD_CT = 64;                         // threads of a member's chain: one wavefront
static_assert((uint32_t)BD_DL == BIGD_LANES, "a thread a lane, and the sixteenth wavefront");
static_assert(BIGD_OFF_BAD == OFF_BAD && BIGD_S >= 64 && BIGD_S <= DEC_S_MAX, "the lanes are lane_dec_body's: an exit is a byte, a lane 64 bits at least");
static_assert(HUFF_BIG_OUT_MAX < (1u << 24), "a tile's symbols and a member's are the low 24 bits of a map entry");
constexpr uint32_t BD_PAY_WORDS = BIGD_LANES * BIGD_S / 32 + 8;   // the tile's words, the six behind it a 32-bit codeword and the reader's look-ahead reach, two of zeros
// a tile's symbols are at most its bits (a code has a bit at least); the image holds BIGD_OUT_CAP - 16 of them: fewer than 1.875 bits a
// symbol over a WHOLE tile is handed back (two symbols; one symbol at 0.9), text (4 to 5 bits) and 128 symbols (7 bits) never are
static_assert(BIGD_OUT_CAP % 16 == 0 && BIGD_OUT_CAP - 16 >= BIGD_TILE_BITS / 2, "every tile of at least two bits a symbol is taken");
// static LDS of the emit kernel: the entry, the words, the image, lane_dec_body's own (the 2 KiB table, the tree, 960 lanes' maps)
static_assert(sizeof(SmallDecArgs) + BD_PAY_WORDS * 4 + BIGD_OUT_CAP + 32 + 16 * 1024 <= 64 * 1024, "LDS of k_huff_big_dec_emit: two workgroups to a CU");

// the member's entry into LDS; its tiles, 0 where the entry is not one of this class's (the host never sends one)
__device__ __forceinline__ uint32_t bd_entry(const SmallDecArgs *__restrict__ tab, uint32_t member, SmallDecArgs &s_a, int threads) {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(tab + member);
    for (uint32_t i = threadIdx.x; i < sizeof(SmallDecArgs) / 4; i += threads) reinterpret_cast<uint32_t *>(&s_a)[i] = src[i];
    __syncthreads();
    const uint32_t tiles = (s_a.T + BIGD_LANES - 1) / BIGD_LANES;
    return s_a.S == BIGD_S && tiles <= BIGD_TILES_MAX ? tiles : 0u;
}

__global__ __launch_bounds__(BD_T) void k_huff_big_dec_map(const SmallDecArgs *__restrict__ tab, uint32_t *__restrict__ scr) {
    __shared__ SmallDecArgs s_a;
    __shared__ uint32_t s_pay[BD_PAY_WORDS];
    const uint32_t tiles = bd_entry(tab, blockIdx.y, s_a, BD_T);
    if (blockIdx.x >= tiles) return;                                      // (uniform: the whole workgroup)
    if (threadIdx.x == 0) s_a.g_maps = scr + (size_t)blockIdx.y * BIGD_SCR_WORDS + BIGD_SCR_MAP;
    __syncthreads();
    (void)lane_dec_body<BD_PAY_WORDS, BIGD_OUT_CAP, true, BD_DL, 256, false, TILE_MAP>(s_a, s_a.child, s_pay, nullptr);
}

__global__ __launch_bounds__(BD_CT) void k_huff_big_dec_chain(const SmallDecArgs *__restrict__ tab, uint32_t *__restrict__ scr) {
    __shared__ SmallDecArgs s_a;
    __shared__ uint32_t s_map[BIGD_TILES_MAX * 32], s_rec[BIGD_TILES_MAX * 4];
    __shared__ uint32_t s_ok;
    const uint32_t tiles = bd_entry(tab, blockIdx.x, s_a, BD_CT), tid = threadIdx.x;
    uint32_t *my = scr + (size_t)blockIdx.x * BIGD_SCR_WORDS;
    for (uint32_t i = tid; i < tiles * 32; i += BD_CT) s_map[i] = my[BIGD_SCR_MAP + i];
    __syncthreads();
    if (tid == 0) {
        uint32_t total = 0;
        const bool ok = bigd_chain(s_map, tiles, s_a.out_max, s_rec, &total);   // (no tiles: not of the class)
        s_ok = ok ? 1u : 0u;
        my[BIGD_SCR_META + BIGD_META_VERDICT] = ok ? 0u : 1u; my[BIGD_SCR_META + BIGD_META_TOTAL] = total; my[BIGD_SCR_META + BIGD_META_DONE] = 0;
        if (!ok) s_a.status[0] = 1;                                       // handed back: no byte of the member will be written, so its word is stored here
    }
    __syncthreads();
    if (s_ok) for (uint32_t i = tid; i < tiles * 4; i += BD_CT) my[BIGD_SCR_TILE + i] = s_rec[i];
}

__global__ __launch_bounds__(BD_T) void k_huff_big_dec_emit(const SmallDecArgs *__restrict__ tab, uint32_t *__restrict__ scr) {
    __shared__ SmallDecArgs s_a;
    __shared__ uint32_t s_pay[BD_PAY_WORDS];
    __shared__ __attribute__((aligned(16))) uint8_t s_out[BIGD_OUT_CAP + 32];
    const uint32_t tiles = bd_entry(tab, blockIdx.y, s_a, BD_T), t = blockIdx.x;
    if (t >= tiles) return;                                               // (uniform: the whole workgroup)
    uint32_t *my = scr + (size_t)blockIdx.y * BIGD_SCR_WORDS;
    if (my[BIGD_SCR_META + BIGD_META_VERDICT] != 0) return;               // handed back by the chain, which has stored its word
    const uint32_t *rec = my + BIGD_SCR_TILE + 4 * t;
    const uint32_t entry = rec[BIGD_TILE_ENTRY], base = rec[BIGD_TILE_BASE], count = rec[BIGD_TILE_COUNT], total = my[BIGD_SCR_META + BIGD_META_TOTAL];
    const uint32_t n = lane_dec_body<BD_PAY_WORDS, BIGD_OUT_CAP, true, BD_DL, 256, true, TILE_EMIT>(s_a, s_a.child, s_pay, s_out, entry, base);
    if (n != count) return;                                               // (cannot be, see above: the member stays without an answer)
    // ---- the member's words, by the last of its tiles to get here: every byte of the output is then in place
    if (tile_finish(&my[BIGD_SCR_META + BIGD_META_DONE], tiles)) {
        __hip_atomic_store(&s_a.status[1], total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&s_a.status[0], 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the three launches of a group of g members; gx: tiles of the largest member the call holds
int bigd_launch(Ctx &c, hipStream_t s, uint32_t g, uint32_t gx, const SmallDecArgs *tab) {
    void *p;
    const int rc = dev_buf(c, Slot::GD_BIG_DEC, (size_t)g * BIGD_SCR_WORDS * 4, &p); if (rc) return rc;
    uint32_t *scr = (uint32_t *)p;
    RSN_LAUNCH("huff_batch_big_dec_map", k_huff_big_dec_map, dim3(gx, g), dim3(BD_T), 0, s, tab, scr);
    RSN_LAUNCH("huff_batch_big_dec_chain", k_huff_big_dec_chain, dim3(g), dim3(BD_CT), 0, s, tab, scr);
    RSN_LAUNCH("huff_batch_big_dec_emit", k_huff_big_dec_emit, dim3(gx, g), dim3(BD_T), 0, s, tab, scr);
    return RSN_OK;
}

constexpr const char *BIGD_WHAT = "huffman batch decompress";
// all the tiles' lanes of BIGD_S bits: parse_lanes answers S = BIGD_S for every span the class takes (huff_big_dec_layout.h asserts it)
constexpr HuffDecShape BIG_DEC_SHAPE = {BIGD_LANES_ALL, BIGD_S, HUFF_BIG_PAY_MAX, HUFF_BIG_OUT_MAX};
// the class's cutoffs, stated once for both forms of takes: above what the mid class's workgroup holds, within the tiles
bool big_dec_wants(size_t pay, unsigned long long expect) { return pay <= HUFF_BIG_PAY_MAX && expect > HUFF_MID_OUT_MAX && expect <= HUFF_BIG_OUT_MAX; }
// The header alone decides, as for the mid class (huff_dec_promise: its scan of the counts).  A symbol takes a bit at least, so a stream
// that is no longer than HUFF_MID_OUT_MAX bits cannot promise more.
bool big_dec_takes(const uint8_t *in, size_t n, int64_t) {
    if (n < 8 || n > HDR_MAX + 8 + HUFF_BIG_PAY_MAX || 8 * n <= HUFF_MID_OUT_MAX) return false;
    size_t pay = 0; unsigned long long expect = 0;
    return huff_dec_promise(in, n, &pay, &expect) && big_dec_wants(pay, expect);
}
bool big_dec_takes_plan(size_t n, const HuffDevSummary &sum) {
    return n >= 8 && n <= HDR_MAX + 8 + HUFF_BIG_PAY_MAX && big_dec_wants((sum.span + 7) / 8, sum.expect) && huff_dec_shape_takes(BIG_DEC_SHAPE, sum);
}

// The device form: huff_dec_run_dev's groups -- k_huff_dev_gather, the three launches, k_huff_dev_scatter -- of up to HUFF_BIG_GROUP_BYTES of staging.
int big_dec_run_dev(Ctx &c, hipStream_t s, const std::vector<size_t> &idx, const rsn_dev_member *mem, int64_t, const DevPlans *plans, std::vector<uint32_t> &answers) {
    uint32_t gx = 1;
    for (size_t i : idx) if (const HuffDevSummary *v = plans->of(i)) gx = std::max(gx, bigd_tiles(v->span));
    gx = std::min(gx, BIGD_TILES_MAX);
    return huff_dec_run_dev(c, s, BIG_DEC_SHAPE, [gx](Ctx &c2, hipStream_t s2, uint32_t g, const SmallDecArgs *tab) { return bigd_launch(c2, s2, g, gx, tab); },
                            idx, mem, *plans, answers, HUFF_BIG_GROUP_BYTES);
}

// The host form.  The kernels read the payload twice and store the output in pieces, so they never run on pinned host memory: the host
// plans every stream (small_dec_plan's wide form; what it refuses goes back untouched) and the planned ones go through the device form in
// runs (group_run.h: run_members_staged) -- the table a run's plans (member r is entry r), an input slot the stream from its 4-byte boundary.
int big_dec_run(Ctx &c, const std::vector<size_t> &idx, const uint8_t *const *ins, const size_t *lens, int64_t window,
                const SmallTake &take, std::vector<size_t> &back, size_t *failed, std::vector<size_t> *) {
    struct Plan { size_t A0; unsigned long long expect; SmallDecArgs a; };
    std::vector<Plan> planned;
    std::vector<RunItem> items;
    planned.reserve(idx.size());
    for (size_t i : idx) {
        Plan p;
        if (small_dec_plan(ins[i], lens[i], BIG_DEC_SHAPE.lanes, BIG_DEC_SHAPE.s_max, p.a, &p.A0, &p.expect, true) != RSN_OK ||
            !big_dec_wants((p.a.end - p.a.p0 + 7) / 8, p.expect)) { back.push_back(i); continue; }
        planned.push_back(p);
        items.push_back(RunItem{i, group_round16(lens[i] - p.A0), huff_dec_out_slot(p.expect), group_round16(p.expect)});
    }
    if (planned.empty()) return RSN_OK;
    DevPlans plans;
    const int rc = run_members_staged<sizeof(HuffDevPlan)>(c, BIGD_WHAT, "%s: internal error: %u decoded bytes in a slot of %zu", items,
        [&](size_t k, size_t r, size_t g, const void *d_table, uint8_t *tab, uint8_t *in) {
            const Plan &p = planned[k];
            const size_t i = items[k].i, sn = lens[i] - p.A0;
            HuffDevPlan hp{};                                             // (the stream is staged from A0 on: the member's own A0 is 0)
            hp.b.verdict = PARSE_PLANNED; hp.b.p0 = p.a.p0; hp.b.end = p.a.end; hp.b.pay_words = p.a.pay_words; hp.b.expect = (uint32_t)p.expect;
            hp.b.K = p.a.K; hp.b.root = p.a.root; hp.b.n_child = p.a.n_child; hp.b.flat = p.a.flat;
            memcpy(hp.child, p.a.child, sizeof hp.child);
            memcpy(tab, &hp, sizeof hp);
            memcpy(in, ins[i] + p.A0, sn); memset(in + sn, 0, items[k].in_bytes - sn);
            if (r == 0) { plans.at.resize(g); plans.sum.resize(g); plans.d_table = (const HuffDevPlan *)d_table; }
            plans.at[r] = (uint32_t)r; plans.sum[r] = HuffDevSummary{PARSE_PLANNED, 0, p.a.end - p.a.p0, (uint32_t)p.expect};
            return sn;
        },
        [&](hipStream_t s, const std::vector<size_t> &all, const rsn_dev_member *mem, std::vector<uint32_t> &answers) { return big_dec_run_dev(c, s, all, mem, window, &plans, answers); },
        take, back, failed, nullptr);
    if (rc) return rc;
    std::sort(back.begin(), back.end());
    return RSN_OK;
}

}  // namespace
const BatchClass &huff_big_dec_class() {
    static const BatchClass dec = {"huffman big decompress", HUFF_BIG_DEC_GROUP_MIN, big_dec_takes, big_dec_run, big_dec_run_dev, big_dec_takes_plan};
    return dec;
}

}  // namespace rsn
