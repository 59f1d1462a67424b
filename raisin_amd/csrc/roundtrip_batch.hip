// roundtrip_batch.hip -- k_members_verify, the one kernel of the batch round trip (rsn.h: rsn_layers_roundtrip_batch,
// rsn_layers_roundtrip_batch_dev).  Behind the two passes of such a call every member has an original and a decompressed
// buffer on the device; this kernel compares them and counts their bytes -- engine.BenchmarkFile's reflect.DeepEqual and its two
// histograms (engine.go:367-370, :412-415, :424) -- for all members in ONE launch.  The flow itself is rsn_api.hip's suite_batch_flow,
// which the round trip runs over its one list.
#include "codecs.h"
#include "roundtrip_batch_layout.h"
#include "suite_layout.h"

namespace rsn {

namespace {

constexpr int VF_THREADS = 256;
constexpr int VF_UNITS = (int)(RB_TILE / 16 / VF_THREADS);   // 16-byte units a thread in a whole tile
constexpr uint32_t VF_NONE = 0xFFFFFFFFu;
// copies of every bin in LDS (copy = lane % copies).  Measured (LEDGER.md): 4 beat 8 and 16 wherever a block has less than a
// tile to count -- clearing and folding the copies is most of such a block's work -- and lose a tenth to them on whole tiles
constexpr int VF_COPIES = 4;
static_assert(RB_TILE % (16 * VF_THREADS) == 0 && VF_UNITS % 4 == 0, "a whole tile is whole batches of four loads a thread");

// A workgroup per table entry (a tile of at most RB_TILE bytes of one member).  Both buffers are read in 16-byte units, a unit only when
// it begins in front of its buffer's length -- so nothing at or behind base + round16(len) -- and of a unit that straddles the length only
// the bytes in front of it are counted or compared: what lies behind a member is another member's, or garbage.
// Histograms: bin-major in LDS, COPIES counters a bin, a thread a bin at the end.  First difference: per lane from the XOR's lowest set
// bit, the minimum over the wavefront by shuffles, over the block through one LDS word.
// Output: words[member] and hists[512 * member ..) were zeroed by ONE memset in front of the launch.  The block of a member of one tile owns
// the member's row and stores it; the blocks of a larger member add their non-zero bins and raise the word -- the COMPLEMENT of the
// offset, so the lowest offset wins and zero stays "nothing differs".
// ORIG = false is the batch suite's second instance (rsn_layers_suite_batch): a run's first list has counted the originals, so
// every further list compares as above and counts the decompressed side alone -- no LDS counters and no atomics for the original, and
// hists[256 * member ..) holds the one histogram (suite_layout.h: suite_dec_layout).  ORIG = true is the instance as it has been.
template <int COPIES, bool ORIG = true>
__global__ __launch_bounds__(VF_THREADS) void k_members_verify(const RbEntry *__restrict__ tab, unsigned long long *__restrict__ words, uint32_t *__restrict__ hists) {
    static_assert(COPIES >= 1 && COPIES <= 16 && (COPIES & (COPIES - 1)) == 0, "copy = lane % COPIES; both histograms within the 64 KiB a block may hold");
    constexpr int SIDES = ORIG ? 2 : 1, DEC = SIDES - 1;                 // the histograms in LDS, and which of them is the decompressed side's
    __shared__ uint32_t h[SIDES][256 * COPIES];
    __shared__ uint32_t s_min;
    const RbEntry e = tab[blockIdx.x];
    const int tid = threadIdx.x;
    const uint32_t copy = tid & (COPIES - 1);
    const bool counting = hists != nullptr;                              // (the same for every thread of the launch)
    if (counting) for (int i = tid; i < SIDES * 256 * COPIES; i += VF_THREADS) (&h[0][0])[i] = 0;
    if (tid == 0) s_min = VF_NONE;
    __syncthreads();

    const uint32_t top = e.n_o > e.n_d ? e.n_o : e.n_d, both = e.n_o < e.n_d ? e.n_o : e.n_d;
    const uint32_t lo = e.tile * (uint32_t)RB_TILE;                      // (below top, which a 32-bit word holds)
    const uint32_t span = top - lo < (uint32_t)RB_TILE ? top - lo : (uint32_t)RB_TILE;
    const uint4 *__restrict__ po = reinterpret_cast<const uint4 *>(e.orig + lo);
    const uint4 *__restrict__ pd = reinterpret_cast<const uint4 *>(e.dec + lo);

    auto add16 = [&](uint32_t *hh, const uint4 &v) {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            atomicAdd(&hh[(w[j] & 0xFF) * COPIES + copy], 1u);
            atomicAdd(&hh[((w[j] >> 8) & 0xFF) * COPIES + copy], 1u);
            atomicAdd(&hh[((w[j] >> 16) & 0xFF) * COPIES + copy], 1u);
            atomicAdd(&hh[(w[j] >> 24) * COPIES + copy], 1u);
        }
    };
    auto byte_of = [](const uint4 &v, uint32_t j) -> uint32_t {          // byte j of the 16
        const uint32_t w = (j >> 2) == 0 ? v.x : (j >> 2) == 1 ? v.y : (j >> 2) == 2 ? v.z : v.w;
        return (w >> (8 * (j & 3))) & 0xFF;
    };
    auto diff16 = [](const uint4 &x, const uint4 &y) -> uint32_t {       // index of the first differing byte of the 16, or 16
        const uint32_t d[4] = {x.x ^ y.x, x.y ^ y.y, x.z ^ y.z, x.w ^ y.w};
        uint32_t at = 16;
#pragma unroll
        for (int j = 3; j >= 0; j--) if (d[j]) at = 4 * j + ((uint32_t)__ffs((int)d[j]) - 1) / 8;
        return at;
    };

    uint32_t mine = VF_NONE;                                             // the lowest differing offset this lane has seen, counted from lo
    if (both >= lo && both - lo >= (uint32_t)RB_TILE) {                  // the tile lies inside both buffers: whole units only
#pragma unroll 1                                                         // (unrolled, the loads of all four batches are hoisted: 135 VGPRs, 3 waves a SIMD, and slower; LEDGER.md)
        for (int k0 = 0; k0 < VF_UNITS; k0 += 4) {
            uint4 a[4], b[4];
#pragma unroll
            for (int k = 0; k < 4; k++) { a[k] = po[(k0 + k) * VF_THREADS + tid]; b[k] = pd[(k0 + k) * VF_THREADS + tid]; }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (counting) { if constexpr (ORIG) add16(h[0], a[k]); add16(h[DEC], b[k]); }
                const uint32_t at = diff16(a[k], b[k]);
                if (at < 16 && mine == VF_NONE) mine = (uint32_t)((k0 + k) * VF_THREADS + tid) * 16 + at;
            }
        }
    } else {
        const uint32_t units = (span + 15) / 16;
        for (uint32_t u = tid; u < units; u += VF_THREADS) {
            const uint32_t pos = lo + 16 * u;                            // (below top)
            const uint32_t vo = pos < e.n_o ? (e.n_o - pos < 16 ? e.n_o - pos : 16) : 0;   // this unit's bytes in front of the original's length ...
            const uint32_t vd = pos < e.n_d ? (e.n_d - pos < 16 ? e.n_d - pos : 16) : 0;   // ... and of the decompressed buffer's
            uint4 a = make_uint4(0, 0, 0, 0), b = make_uint4(0, 0, 0, 0);
            if (vo) a = po[u];
            if (vd) b = pd[u];
            if (counting) {
                if constexpr (ORIG) { if (vo == 16) add16(h[0], a); else for (uint32_t j = 0; j < vo; j++) atomicAdd(&h[0][byte_of(a, j) * COPIES + copy], 1u); }
                if (vd == 16) add16(h[DEC], b); else for (uint32_t j = 0; j < vd; j++) atomicAdd(&h[DEC][byte_of(b, j) * COPIES + copy], 1u);
            }
            const uint32_t at = diff16(a, b), vc = vo < vd ? vo : vd;
            if (at < vc && mine == VF_NONE) mine = 16 * u + at;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = __shfl_xor(mine, d); mine = o < mine ? o : mine; }
    if ((tid & 63) == 0 && mine != VF_NONE) atomicMin(&s_min, mine);
    __syncthreads();

    const bool alone = top <= (uint32_t)RB_TILE;                         // the member's only tile: its row is this block's
    if (tid == 0) {
        const uint32_t found = s_min;
        const unsigned long long word = found == VF_NONE ? 0ull : ~((unsigned long long)lo + found);
        if (alone) words[e.member] = word;
        else if (word) atomicMax(&words[e.member], word);
    }
    if (counting) {
        uint32_t so = 0, sd = 0;
#pragma unroll
        for (int r = 0; r < COPIES; r++) {                               // rotated: the lanes of a group begin at different copies
            const int at = tid * COPIES + ((r + tid) & (COPIES - 1));
            if constexpr (ORIG) so += h[0][at];
            sd += h[DEC][at];
        }
        if constexpr (ORIG) {
            uint32_t *row = hists + (size_t)e.member * RB_HIST_WORDS;
            if (alone) { row[tid] = so; row[256 + tid] = sd; }
            else { if (so) atomicAdd(&row[tid], so); if (sd) atomicAdd(&row[256 + tid], sd); }
        } else {
            uint32_t *row = hists + (size_t)e.member * SUITE_HIST_WORDS;
            if (alone) row[tid] = sd;
            else if (sd) atomicAdd(&row[tid], sd);
        }
    }
}

}  // namespace

// the table checked and sent up, the stats block cleared: what both instances have in front of their launch
static int verify_prepare(Ctx &c, hipStream_t s, const RbEntry *h_tab, size_t tiles, size_t m, const RbLayout &lay, void *d_slot) {
    if (tiles > 0x7FFFFFFFull || m > 0xFFFFFFFFull) return c.fail(RSN_ERR_LIMIT, "layers: %zu tiles of %zu members to verify in one launch", tiles, m);
    for (size_t t = 0; t < tiles; t++) {
        const RbEntry &e = h_tab[t];
        if (e.member >= m || e.tile >= rb_tiles(e.n_o, e.n_d) || (((uintptr_t)e.orig | (uintptr_t)e.dec) & 15) || (!e.orig && e.n_o) || (!e.dec && e.n_d))
            return c.fail(RSN_ERR_DEVICE, "layers: internal error: entry %zu of the verify table (member %u, tile %u) is not one", t, e.member, e.tile);
    }
    uint8_t *d = (uint8_t *)d_slot;
    if (tiles) RSN_HIP(copy_async(d + lay.table, h_tab, tiles * sizeof(RbEntry), hipMemcpyHostToDevice, s));
    RSN_HIP(hipMemsetAsync(d + lay.words, 0, rb_stats_bytes(lay), s));
    return RSN_OK;
}

int members_verify(Ctx &c, hipStream_t s, bool both, const RbEntry *h_tab, size_t tiles, size_t m, bool hists, void *d_slot) {
    const RbLayout lay = verify_layout(both, tiles, m, hists);
    const int rc = verify_prepare(c, s, h_tab, tiles, m, lay, d_slot); if (rc) return rc;
    uint8_t *d = (uint8_t *)d_slot;
    if (tiles == 0) return RSN_OK;
    const RbEntry *tab = (const RbEntry *)(d + lay.table);
    unsigned long long *words = (unsigned long long *)(d + lay.words);
    uint32_t *counts = hists ? (uint32_t *)(d + lay.hists) : (uint32_t *)nullptr;
    if (both) RSN_LAUNCH("members_verify", (k_members_verify<VF_COPIES>), dim3((uint32_t)tiles), dim3(VF_THREADS), 0, s, tab, words, counts);
    else RSN_LAUNCH("members_verify_dec", (k_members_verify<VF_COPIES, false>), dim3((uint32_t)tiles), dim3(VF_THREADS), 0, s, tab, words, counts);
    return RSN_OK;
}

}  // namespace rsn
