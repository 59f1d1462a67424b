// lzss_tile.hip -- the LZSS encoder for the members of a compress batch above the mid class: more than LZSS_MID_IN_MAX and at most
// LZSS_TILE_IN_MAX bytes, a window of 1 to 4096 (codecs.h).
//
// Inside a batch such a member used to be the single call -- a dozen launches and three host round trips, a member after the other.  A
// bigger one-workgroup kernel is no answer: the mid class's workgroup already takes 6.7 ms for 64 KiB while the rest of the device idles.
// But a position's best match depends only on the W <= 4096 escaped bytes in front of it and the bytes behind it, so the search can be
// cut into TILES of LZSS_TILE_POS escaped positions and spread over every CU.  A group of members is four launches, queued one behind the
// other with nothing on the host between them (lzss_tile_layout.h: the tiles, a member's scratch, which tile stores which byte):
//   esc      k_lzss_tile_esc, a workgroup per member: the member's place in the group's scratch (the sum of the scratch of the members
//            in front of it, stored in the table at the scratch's front); EncodeOpeningSymbols (lzss.go:369-389) of the member into its
//            escaped stream in scratch, 16 KiB a round by a block scan; E.  A member that escapes to more than lzt_e_cap(n) bytes gets
//            its status word here: GROUP_BACK.
//   search   k_lzss_tile_search, a workgroup per escaped tile: fc[t0 - W', t0 + TILE + 4096 + 64) into LDS (W': the window rounded down
//            to a sub-tile; a match may be as long as its distance, hence the look-ahead), the window's positions linked into the hash
//            chains without searching them, then the tile's positions linked and searched sub-tile by sub-tile by chain_best
//            (lzss_enc_body.h) -- the walk k_lzss_mid_enc calls, so the keys are the same keys.  L << 16 | distance of every position goes
//            to scratch.  A tile that exceeds the step cap sets the member's give-up word.
//   chain    k_lzss_tile_chain, a workgroup per member: a member of which a tile gave up is answered GROUP_BACK.  Otherwise the greedy
//            chain r -> r + max(1, L) (lzss.go:134-151) tile by tile with the mid kernel's pointer doubling, the entry into a tile where
//            the tile before it left, a tile the chain steps over skipped; the chain's positions marked in their keys (bit 31), every
//            item sized (a token iff 3 + digits(d) + digits(L) < L, lzss.go:143), and the tiles' first output bytes and the stream's
//            length as the running sum.
//   emit     k_lzss_tile_emit, a workgroup per tile: the tile's items into an LDS image that begins at the 16-byte unit its first byte
//            lies in, and the tile's own bytes out of it.
// Ownership, the member's status word by the last of its tiles, the grid and the host form are the tiled classes' common shape (DESIGN
// 4.7; tile_dev.h); the done-counter is zeroed by esc.  No workgroup waits for another; every loop is bounded by the tile, the ring,
// the step cap or the tiles of a member.  Nothing a launch reads from scratch is left from an earlier group: esc writes the table, the
// member's words and the stream, search every key below E, chain every offset.
#include "group_run.h"
#include "lzss_enc_body.h"
#include "lzss_tile_layout.h"
#include "tile_dev.h"

namespace rsn {
namespace {

constexpr int TT = 1024;                          // threads of every workgroup here
constexpr uint32_t TILE = LZSS_TILE_POS;          // positions of a tile (two per thread)
constexpr uint32_t T_RING = 8192;                 // links kept: the window, rounded down to a sub-tile, and the tile
constexpr uint32_t T_HEADS = 4096;                // chains (chain_hash's 12 bits)
constexpr uint32_t T_STEP_CAP = 4096;             // eight-byte extension steps a thread spends on its two positions of a tile: k_lzss_mid_enc's MID_STEP_CAP
constexpr uint32_t T_FC_BYTES = LZT_W_MAX + TILE + LZT_W_MAX + 64;   // the window, the tile, the look-ahead of the longest match, the loads' reach behind it
constexpr uint32_t T_ESC_ROUND = 16 * TT;         // input bytes of a round of the escape pass
constexpr uint32_t T_IMG = TILE + 64;             // the emit image: up to 15 bytes in front of the tile's first, its items, slack
static_assert(TILE == 2 * TT, "two positions a thread");
static_assert(T_RING >= LZT_W_MAX + TILE + TT && (T_RING & (T_RING - 1)) == 0, "a link is never overwritten while a walk may still read it");
static_assert(T_FC_BYTES % 16 == 0 && T_FC_BYTES + T_RING * 4 + T_HEADS * 4 + 64 <= 80 * 1024, "static LDS of k_lzss_tile_search; two workgroups to a CU");
// an item is a token or at most 11 bytes (3 + 4 + 4 digits >= L), and never longer than what it stands for: the items that begin in a
// tile put out at most TILE - 1 + 11 bytes
static_assert(15 + TILE + 11 <= T_IMG && T_IMG % 16 == 0, "the image holds the longest tile");

struct TileScr { uint32_t *my; bool ok; };
// a member's scratch, from the table esc wrote; not ok: the member was handed back (esc has stored its word)
__device__ __forceinline__ TileScr tile_scr(uint32_t *scr, uint32_t member) {
    const uint32_t off = scr[member];
    TileScr r;
    r.my = scr + off;
    r.ok = off != 0 && r.my[LZT_SCR_META + LZT_META_VERDICT] == 0;
    return r;
}

// ---------------------------------------------------------------- esc: a workgroup per member
__global__ __launch_bounds__(TT) void k_lzss_tile_esc(const SmallMember *__restrict__ tab, uint8_t *__restrict__ base, uint32_t *__restrict__ scr, uint32_t g,
                                                       unsigned long long scr_words, uint32_t W) {
    __shared__ uint32_t s_wave[TT / 64 + 4];
    const SmallMember m = tab[blockIdx.x];
    uint32_t *status = reinterpret_cast<uint32_t *>(base + m.status_off);
    const uint32_t tid = threadIdx.x, n = m.n;
    // ---- the member's place: behind the table and the scratch of the members in front of it
    uint32_t mine = 0, before;
    for (uint32_t q = tid; q < blockIdx.x; q += TT) mine += lzt_scr_words(tab[q].n);
    block_scan<TT>(mine, s_wave, &before);
    const unsigned long long off = (unsigned long long)lzt_front_words(g) + before;
    const bool fits = off + lzt_scr_words(n) <= scr_words;
    if (n == 0 || n > LZSS_TILE_IN_MAX || W == 0 || W > LZT_W_MAX || !fits) {     // (the host does not send these)
        if (tid == 0) { if (fits) scr[off + LZT_SCR_META + LZT_META_VERDICT] = GROUP_BACK; scr[blockIdx.x] = fits ? (uint32_t)off : 0u; *status = GROUP_BACK; }
        return;
    }
    uint32_t *my = scr + off;
    uint8_t *fc = reinterpret_cast<uint8_t *>(my + lzt_scr_fc(n));
    const uint32_t ecap = lzt_e_cap(n);
    // ---- EncodeOpeningSymbols: 3C -> FF; FF -> 5C FF; 5C -> 5C 5C.  A round is 16 bytes a thread.
    const uint4 *in = reinterpret_cast<const uint4 *>(base + m.in_off);
    uint32_t E = 0;
    bool over = false;
    for (uint32_t r0 = 0; r0 < n; r0 += T_ESC_ROUND) {
        const uint32_t i = r0 + 16 * tid, valid = i < n ? min(16u, n - i) : 0u;
        const uint4 v = valid ? in[i >> 4] : make_uint4(0, 0, 0, 0);            // (the input slot holds whole units)
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t cnt = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) if ((uint32_t)k < valid) cnt += lzss_esc_len((w[k >> 2] >> (8 * (k & 3))) & 0xFF);
        uint32_t tot;
        uint32_t at = E + block_scan<TT>(cnt, s_wave, &tot);
        if (tot > ecap - E) { over = true; break; }                             // (uniform)
#pragma unroll
        for (int k = 0; k < 16; k++) if ((uint32_t)k < valid) at = lzss_esc_put(fc, at, (w[k >> 2] >> (8 * (k & 3))) & 0xFF);
        E += tot;
    }
    if (!over && tid < LZT_FC_PAD) fc[E + tid] = 0;                              // (E <= ecap: the pad lies inside the member's scratch)
    if (tid == 0) {
        scr[blockIdx.x] = (uint32_t)off;
        my[LZT_SCR_META + LZT_META_VERDICT] = over ? GROUP_BACK : 0u;
        my[LZT_SCR_META + LZT_META_E] = over ? 0u : E;
        my[LZT_SCR_META + LZT_META_TOTAL] = 0; my[LZT_SCR_META + LZT_META_DONE] = 0; my[LZT_SCR_META + LZT_META_GIVEUP] = 0;
        if (over) *status = GROUP_BACK;
    }
}

// ---------------------------------------------------------------- search: a workgroup per escaped tile
__global__ __launch_bounds__(TT) void k_lzss_tile_search(const SmallMember *__restrict__ tab, uint32_t *__restrict__ scr, uint32_t W) {
    __shared__ __attribute__((aligned(16))) uint32_t s_fcw[T_FC_BYTES / 4];
    __shared__ uint32_t s_ring[T_RING], s_head[T_HEADS];
    const uint32_t n = tab[blockIdx.y].n, tid = threadIdx.x, t0 = blockIdx.x * TILE;
    const TileScr ts = tile_scr(scr, blockIdx.y);
    if (!ts.ok) return;                                                          // (uniform: the whole workgroup)
    uint32_t *my = ts.my;
    const uint32_t E = my[LZT_SCR_META + LZT_META_E];
    if (t0 >= E) return;
    uint32_t *keys = my + lzt_scr_keys(n);
    const uint32_t *fcw = my + lzt_scr_fc(n);
    const uint32_t lo = lzt_window_lo(t0, W, TT);                                // (a multiple of TT: word loads are aligned)
    // ---- the stream from lo on, zeros from E on whatever the scratch holds there
    for (uint32_t w = tid; w < T_FC_BYTES / 4; w += TT) {
        const uint32_t p = lo + 4 * w;
        uint32_t x = 0;
        if (p < E) { x = fcw[p >> 2]; if (E - p < 4) x &= (1u << (8 * (E - p))) - 1; }
        s_fcw[w] = x;
    }
    for (uint32_t i = tid; i < T_HEADS; i += TT) s_head[i] = CHAIN_NONE;
    __syncthreads();
    const uint8_t *s_fc = reinterpret_cast<const uint8_t *>(s_fcw);
    // ---- the window's positions join their chains, a sub-tile at a time: between sub-tiles a chain is in descending order
    for (uint32_t p0 = lo; p0 < t0; p0 += TT) {
        const uint32_t i = p0 + tid;                                             // (below t0 < E)
        s_ring[i & (T_RING - 1)] = atomicExch(&s_head[chain_hash(s_fc[i - lo], s_fc[i + 1 - lo])], i);
        __syncthreads();
    }
    // ---- the tile's positions join and search, as k_lzss_mid_enc's do
    uint32_t steps = 0;
    for (uint32_t sub = 0; sub < TILE; sub += TT) {
        const uint32_t i = t0 + sub + tid;
        const uint32_t h = i < E ? chain_hash(s_fc[i - lo], s_fc[i + 1 - lo]) : 0u;
        if (i < E) s_ring[i & (T_RING - 1)] = atomicExch(&s_head[h], i);
        __syncthreads();
        if (i < E) keys[i] = chain_best<T_RING, TT, T_STEP_CAP>(s_fc, s_ring, s_head[h], i, E, W, lo, steps);
        __syncthreads();                                                         // (the next sub-tile's links are written behind this)
    }
    if (__syncthreads_or(steps > T_STEP_CAP) && tid == 0) atomicOr(&my[LZT_SCR_META + LZT_META_GIVEUP], 1u);
}

// ---------------------------------------------------------------- chain: a workgroup per member
__global__ __launch_bounds__(TT) void k_lzss_tile_chain(const SmallMember *__restrict__ tab, uint8_t *__restrict__ base, uint32_t *__restrict__ scr) {
    __shared__ uint32_t s_key[TILE];
    __shared__ uint16_t s_jmp[2][TILE + 8];
    __shared__ uint8_t s_on[TILE + 16];
    __shared__ uint32_t s_wave[TT / 64 + 4];
    __shared__ uint32_t s_misc[4];                                               // [0]: where the chain enters the next tile
    const SmallMember m = tab[blockIdx.x];
    const uint32_t n = m.n, tid = threadIdx.x;
    const TileScr ts = tile_scr(scr, blockIdx.x);
    if (!ts.ok) return;
    uint32_t *my = ts.my;
    if (my[LZT_SCR_META + LZT_META_GIVEUP] != 0) {                               // (uniform) runs and short periods: the single call's
        if (tid == 0) { my[LZT_SCR_META + LZT_META_VERDICT] = GROUP_BACK; *reinterpret_cast<uint32_t *>(base + m.status_off) = GROUP_BACK; }
        return;
    }
    const uint32_t E = my[LZT_SCR_META + LZT_META_E], T = lzt_tiles(E);
    uint32_t *keys = my + lzt_scr_keys(n);
    uint32_t entry = 0, out_at = 0;                                              // the chain's first position in the tile, from the tile's start; bytes of the stream so far
    for (uint32_t t = 0; t < T; t++) {
        const uint32_t t0 = t * TILE;
        if (tid == 0) my[LZT_SCR_OFF + t] = out_at;
        if (entry >= TILE) { entry -= TILE; continue; }                          // (a match steps over the whole tile: the search left its keys unmarked)
        const uint32_t R = lzt_tile_len(E, t);
        for (uint32_t r = tid; r < TILE; r += TT) s_key[r] = r < R ? keys[t0 + r] : 0u;
        __syncthreads();
        // ---- the greedy chain inside the tile: r -> r + max(1, L) (lzss.go:139-142), TILE: beyond the tile
        // (the kernel's own copy of lzss_greedy_chain, as k_lzss_mid_enc's: through the helper 16 x 128 KiB sat above the parent's spread in five runs of seven; LEDGER)
        for (uint32_t r = tid; r <= TILE; r += TT) {
            s_jmp[0][r] = (uint16_t)(r < R ? min(TILE, r + max(1u, s_key[r] >> 16)) : TILE);
            s_on[r] = r == entry;
        }
        __syncthreads();
        int cur = 0;
        for (uint32_t reach = 1; reach < TILE + 1; reach <<= 1) {                // after the round: everything within 2 * reach - 1 steps of the entry
            const uint16_t *ja = s_jmp[cur];
            uint16_t *jb = s_jmp[cur ^ 1];
            for (uint32_t r = tid; r < TILE; r += TT) if (s_on[r]) s_on[ja[r]] = 1;
            for (uint32_t r = tid; r <= TILE; r += TT) jb[r] = ja[ja[r]];
            cur ^= 1;
            __syncthreads();
        }
        // ---- what every chain position puts out: a token iff it is shorter than what it stands for (lzss.go:143), else the bytes
        uint32_t sz = 0, total;
        for (uint32_t r = 2 * tid; r < 2 * tid + 2; r++) {
            if (r < R && s_on[r]) {
                const uint32_t key = s_key[r];                                   // (as the search stored it: LZT_KEY_ON is not set)
                const LzssItem it = lzss_item(key >> 16, key & 0xFFFFu);
                sz += it.sz;
                keys[t0 + r] = key | LZT_KEY_ON;
                if (r + max(1u, it.L) >= TILE) s_misc[0] = r + max(1u, it.L) - TILE;   // (one position of the tile: the chain's last in it)
            }
        }
        block_scan<TT>(sz, s_wave, &total);
        out_at += total;
        entry = s_misc[0];
        __syncthreads();
    }
    if (tid == 0) { my[LZT_SCR_OFF + T] = out_at; my[LZT_SCR_META + LZT_META_TOTAL] = out_at; }
}

// ---------------------------------------------------------------- emit: a workgroup per tile
__global__ __launch_bounds__(TT) void k_lzss_tile_emit(const SmallMember *__restrict__ tab, uint8_t *__restrict__ base, uint32_t *__restrict__ scr) {
    __shared__ __attribute__((aligned(16))) uint8_t s_out[T_IMG];
    __shared__ uint32_t s_wave[TT / 64 + 4];
    const SmallMember m = tab[blockIdx.y];
    const uint32_t n = m.n, tid = threadIdx.x, t = blockIdx.x, t0 = t * TILE;
    const TileScr ts = tile_scr(scr, blockIdx.y);
    if (!ts.ok) return;                                                          // handed back by esc or by chain, which have stored the word
    uint32_t *my = ts.my;
    const uint32_t E = my[LZT_SCR_META + LZT_META_E], T = lzt_tiles(E);
    if (t >= T) return;
    const uint32_t *keys = my + lzt_scr_keys(n);
    const uint8_t *fc = reinterpret_cast<const uint8_t *>(my + lzt_scr_fc(n));
    const uint32_t off0 = my[LZT_SCR_OFF + t], off1 = my[LZT_SCR_OFF + t + 1], total = my[LZT_SCR_META + LZT_META_TOTAL];
    const uint32_t u0 = lzt_image_first(off0), R = lzt_tile_len(E, t);
    LzssItem it[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};                                // (sz 0: not on the chain)
    for (int k = 0; k < 2; k++) {
        const uint32_t r = 2 * tid + k, key = r < R ? keys[t0 + r] : 0u;
        if (key & LZT_KEY_ON) it[k] = lzss_item((key & ~LZT_KEY_ON) >> 16, key & 0xFFFFu);
    }
    uint32_t sum;
    uint32_t at = off0 - u0 + block_scan<TT>(it[0].sz + it[1].sz, s_wave, &sum);
    for (int k = 0; k < 2; k++) {
        if (!it[k].sz || at + it[k].sz > T_IMG) continue;                        // (the image holds every tile: the assert above)
        lzss_item_put(s_out, at, it[k], fc + t0 + 2 * tid + k);
        at += it[k].sz;
    }
    __syncthreads();
    // ---- the tile's own bytes out (sum == off1 - off0: chain sized the same items)
    if (sum == off1 - off0 && off1 <= lzt_out_slot(n)) tile_store_out<TT>(base + m.out_off, s_out, u0, off0, off1);
    // ---- the member's word, by the last of its tiles to get here: every byte of the stream is then in place
    if (tile_finish(&my[LZT_SCR_META + LZT_META_DONE], T))
        __hip_atomic_store(reinterpret_cast<uint32_t *>(base + m.status_off), total, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

// the launches of a group of g members; gx: tiles of the largest member the call holds; scr_words: what the slot must hold
int tile_launch(Ctx &c, hipStream_t s, uint32_t g, uint32_t gx, size_t scr_words, const SmallMember *tab, uint8_t *base, int64_t window) {
    void *p;
    const int rc = dev_buf(c, Slot::GD_LZSS_TILES, scr_words * 4, &p); if (rc) return rc;
    uint32_t *scr = (uint32_t *)p;
    const uint32_t W = (uint32_t)window;
    RSN_LAUNCH("lzss_batch_tile_esc", k_lzss_tile_esc, dim3(g), dim3(TT), 0, s, tab, base, scr, g, (unsigned long long)scr_words, W);
    RSN_LAUNCH("lzss_batch_tile_search", k_lzss_tile_search, dim3(gx, g), dim3(TT), 0, s, tab, scr, W);
    RSN_LAUNCH("lzss_batch_tile_chain", k_lzss_tile_chain, dim3(g), dim3(TT), 0, s, tab, base, scr);
    RSN_LAUNCH("lzss_batch_tile_emit", k_lzss_tile_emit, dim3(gx, g), dim3(TT), 0, s, tab, base, scr);
    return RSN_OK;
}

constexpr const char *TILE_WHAT = "lzss batch compress";
bool tile_enc_takes(const uint8_t *, size_t n, int64_t window) {                  // (the length and the window alone: both forms)
    return lzt_takes(n, window);
}
size_t tile_out_bytes(size_t n) { return lzt_out_slot((uint32_t)std::min<size_t>(n, LZSS_TILE_IN_MAX)); }

// The device form: run_groups_dev's groups -- k_group_gather, the launches, k_group_scatter -- of up to LZSS_TILE_GROUP_BYTES of staging.
// A member's scratch is less than four times its staging (its two slots hold 2 n bytes at least, lzss_tile_layout.h), so the slot that
// holds the call's whole scratch, or four times a group's staging when that is less, holds every group's.
int tile_enc_run_dev(Ctx &c, hipStream_t s, const std::vector<size_t> &idx, const rsn_dev_member *mem, int64_t window, const DevPlans *, std::vector<uint32_t> &answers) {
    size_t words = 0;
    for (size_t i : idx) words += lzt_scr_words((uint32_t)std::min<size_t>(mem[i].n, LZSS_TILE_IN_MAX));
    const uint32_t gx = grid_tiles_of_largest(idx, mem, LZSS_TILE_IN_MAX, [](uint32_t n) { return lzt_tiles(lzt_e_cap(n)); });
    const size_t scr_words = lzt_front_words((uint32_t)std::min(idx.size(), SMALL_GROUP_MAX)) + std::min(words, LZSS_TILE_GROUP_BYTES + lzt_scr_words(LZSS_TILE_IN_MAX));
    return run_groups_dev(c, s, TILE_WHAT, idx, mem, [&](size_t k) { return lzt_in_slot(mem[idx[k]].n); }, [&](size_t k) { return tile_out_bytes(mem[idx[k]].n); },
        [&](hipStream_t s2, uint32_t g, const SmallMember *tab, uint8_t *base) { return tile_launch(c, s2, g, gx, scr_words, tab, base, window); }, answers, LZSS_TILE_GROUP_BYTES);
}

// The host form: the members through the device form above (the kernels read a member's stream from scratch: never out of pinned host memory).
int tile_enc_run(Ctx &c, const std::vector<size_t> &idx, const uint8_t *const *ins, const size_t *lens, int64_t window,
                 const SmallTake &take, std::vector<size_t> &back, size_t *failed, std::vector<size_t> *back_runes) {
    return run_members_copied(c, TILE_WHAT, "a stream", idx, ins, lens, tile_out_bytes,
        [&](hipStream_t s, const std::vector<size_t> &all, const rsn_dev_member *mem, std::vector<uint32_t> &answers) { return tile_enc_run_dev(c, s, all, mem, window, nullptr, answers); },
        take, back, failed, back_runes);
}

}  // namespace
const BatchClass &lzss_tile_class() {
    static const BatchClass enc = {"lzss tile compress", LZSS_TILE_GROUP_MIN, tile_enc_takes, tile_enc_run, tile_enc_run_dev};
    return enc;
}

}  // namespace rsn
