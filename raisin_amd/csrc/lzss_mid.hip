// lzss_mid.hip -- the LZSS codec for the mid-size members of a batch: above lzss_small.hip's cutoffs, up to LZSS_MID_IN_MAX bytes to
// compress and LZSS_MID_E_MAX bytes of stream to decompress.
//
// A directory of source files, configs, JSON documents or log slices is mostly 1 to 64 KiB a file.  The single call's general path was
// built for gigabytes -- a dozen launches and three host round trips, 0.23 ms however few the bytes -- and the brute-force search of
// lzss_small.hip looks at every distance for every position.  Here a member is ONE workgroup of a launch that holds many members, the
// whole escaped stream of the member lies in LDS, and the search walks hash chains keyed on a position's first two bytes.
//
//   compress    EncodeOpeningSymbols (lzss.go:369-389) by a block-wide scan into LDS.  Then tile by tile (MID_TILE positions): the tile's
//               positions join the chains of their two-byte keys (a ring of links that covers the window and the tile); every position
//               walks its chain over the window -- the longest match that lies entirely inside the window, at its largest distance
//               (lzss.go:166-184,418-421); the greedy chain (lzss.go:134-151) enters the tile where the tile before it left, and is marked by
//               pointer doubling inside the tile; item sizes, a scan, the bytes (lzss.go:143,318-320), flushed in 16-byte units.
//               A match of length 1 and no match give the same bytes and the same step, so a position without a two-byte candidate is a
//               literal.  Runs and short periods (every candidate matches as far as it may) exceed MID_STEP_CAP and are handed back.
//   decompress  the stream in chunks of MID_TILE bytes: every '<' parses its token (lzss.go:323-364), a scan gives the output offsets; the
//               chunk's output in tiles of MID_TILE bytes in output order -- a source in an earlier tile is final, chains inside the tile
//               are settled by pointer jumping; DecodeOpeningSymbols (lzss.go:391-406) as lzss_small.hip does it.
// What the kernels do not take is handed back (GROUP_BACK) and goes through the single call, which also words the errors.
// No loop waits for another workgroup, and every loop is bounded: the chain walk by the ring's size, the extensions by MID_STEP_CAP.
#include "group_run.h"
#include "lzss_dec_body.h"
#include "lzss_enc_body.h"

namespace rsn {
namespace {

constexpr int MT = 1024;                          // threads of a workgroup
constexpr uint32_t MID_TILE = 2048;               // positions of a tile (two per thread)
constexpr uint32_t MID_W_MAX = 4096;              // the largest window (what the pipelined host call takes, too)
constexpr uint32_t MID_RING = 8192;               // links kept: the window, rounded down to a sub-tile, and the tile in hand
constexpr uint32_t MID_HEADS = 4096;              // chains (a 12-bit hash of the two-byte key)
constexpr uint32_t MID_NONE = CHAIN_NONE;
constexpr uint32_t MID_STEP_CAP = 4096;           // eight-byte extension steps a thread spends on a tile (its two positions) before the member is handed back -- lzss_small.hip's SL_STEP_CAP, for the same two positions
constexpr uint32_t E_PAD = 64;                    // zeros behind the escaped stream (an eight-byte load may start at its last byte)
constexpr uint32_t E_MAX = LZSS_MID_E_MAX;

// ---- LDS of the encoder (dynamic; offsets in bytes)
constexpr uint32_t EL_FC = 0;                                   // the escaped stream
constexpr uint32_t EL_RING = EL_FC + E_MAX + E_PAD;             // uint32[MID_RING]: the position that was the chain's head when this one joined
constexpr uint32_t EL_HEAD = EL_RING + MID_RING * 4;            // uint32[MID_HEADS]
constexpr uint32_t EL_KEY = EL_HEAD + MID_HEADS * 4;            // uint32[MID_TILE]: L << 16 | distance
constexpr uint32_t EL_JMP = EL_KEY + MID_TILE * 4;              // uint16[2][MID_TILE + 8]
constexpr uint32_t EL_ON = EL_JMP + 2 * (MID_TILE + 8) * 2;     // uint8[MID_TILE + 16]
constexpr uint32_t EL_OUT = EL_ON + MID_TILE + 16;              // uint8[MID_TILE + 64]: at most 15 bytes carried over, the tile's items
constexpr uint32_t EL_WAVE = EL_OUT + MID_TILE + 64;            // uint32[MT / 64 + 1 (+ 3)]
constexpr uint32_t EL_MISC = EL_WAVE + (MT / 64 + 4) * 4;       // uint32[4]
constexpr uint32_t EL_BYTES = EL_MISC + 16;
constexpr uint32_t EL_IN = EL_RING;                             // the member as it came, until it is escaped: over the tile's arrays
static_assert(EL_IN + LZSS_MID_IN_MAX + 16 <= EL_WAVE, "the raw member lies over the tile arrays, not over the scan's words");
static_assert(EL_BYTES <= 160 * 1024 && EL_RING % 16 == 0 && EL_OUT % 16 == 0 && EL_WAVE % 4 == 0, "LDS of k_lzss_mid_enc");
static_assert(MID_RING >= MID_W_MAX + MID_TILE + MT, "a link is never overwritten while a walk may still read it");

// ---- LDS of the decoder
constexpr uint32_t DL_IN = 0;                                   // the stream; in the end the result
constexpr uint32_t DL_VAL = DL_IN + E_MAX + E_PAD;              // the escaped bytes
constexpr uint32_t DL_SRC = DL_VAL + E_MAX + E_PAD;             // uint32[2][MID_TILE]: where a byte of the tile comes from
constexpr uint32_t DL_COV = DL_SRC + 2 * MID_TILE * 4;          // uint8[MID_TILE + 64]: the byte of the chunk belongs to a token's text
constexpr uint32_t DL_WAVE = DL_COV + MID_TILE + 64;
constexpr uint32_t DL_BYTES = DL_WAVE + (MT / 64 + 4) * 4;
static_assert(DL_BYTES <= 160 * 1024 && DL_VAL % 16 == 0 && DL_SRC % 16 == 0 && DL_WAVE % 4 == 0, "LDS of k_lzss_mid_dec");
constexpr uint32_t MID_TOKEN_TEXT = 23;                         // '<' ten digits ',' ten digits '>'
static_assert(MID_TOKEN_TEXT <= 32, "a token's text spills at most 32 bytes into the next chunk");

// ---------------------------------------------------------------- compress
__global__ __launch_bounds__(MT) void k_lzss_mid_enc(const SmallMember *__restrict__ tab, uint8_t *__restrict__ base, uint32_t W) {
    extern __shared__ uint4 mid_lds[];
    uint8_t *sm = reinterpret_cast<uint8_t *>(mid_lds);
    uint8_t *s_fc = sm + EL_FC;
    uint32_t *s_ring = reinterpret_cast<uint32_t *>(sm + EL_RING);
    uint32_t *s_head = reinterpret_cast<uint32_t *>(sm + EL_HEAD);
    uint32_t *s_key = reinterpret_cast<uint32_t *>(sm + EL_KEY);
    uint16_t *s_jmp = reinterpret_cast<uint16_t *>(sm + EL_JMP);                  // [2][MID_TILE + 8]
    uint8_t *s_on = sm + EL_ON;
    uint8_t *s_out = sm + EL_OUT;
    uint32_t *s_wave = reinterpret_cast<uint32_t *>(sm + EL_WAVE);
    uint32_t *s_misc = reinterpret_cast<uint32_t *>(sm + EL_MISC);                // [0]: where the chain enters the next tile
    const uint8_t *s_in = sm + EL_IN;
    const SmallMember m = tab[blockIdx.x];
    const uint8_t *hin = base + m.in_off;
    uint8_t *hout = base + m.out_off;
    uint32_t *flag = reinterpret_cast<uint32_t *>(base + m.status_off);
    const uint32_t tid = threadIdx.x, n = m.n;
    if (n > LZSS_MID_IN_MAX || W == 0 || W > MID_W_MAX) { block_done(flag, GROUP_BACK); return; }   // (the host does not send these)
    for (uint32_t u = tid; u * 16 < n; u += MT) reinterpret_cast<uint4 *>(sm + EL_IN)[u] = reinterpret_cast<const uint4 *>(hin)[u];   // (pinned host memory, zero behind n)
    for (uint32_t i = tid; i < (E_MAX + E_PAD) / 4; i += MT) reinterpret_cast<uint32_t *>(s_fc)[i] = 0;
    __syncthreads();
    // ---- EncodeOpeningSymbols: 3C -> FF; FF -> 5C FF; 5C -> 5C 5C.  A run of ceil(n / MT) input bytes per thread.
    uint32_t E;
    {
        const uint32_t per = (n + MT - 1) / MT, i0 = min(n, tid * per), i1 = min(n, i0 + per);
        uint32_t cnt = 0;
        for (uint32_t i = i0; i < i1; i++) cnt += lzss_esc_len(s_in[i]);
        uint32_t at = block_scan<MT>(cnt, s_wave, &E);
        if (E > E_MAX) { block_done(flag, GROUP_BACK); return; }                  // (uniform)
        for (uint32_t i = i0; i < i1; i++) at = lzss_esc_put(s_fc, at, s_in[i]);
    }
    __syncthreads();                                                              // (the raw member is no longer read: its LDS is the tile's now)
    for (uint32_t i = tid; i < MID_HEADS; i += MT) s_head[i] = MID_NONE;
    __syncthreads();
    uint32_t entry = 0;                                                           // the greedy chain's first position in the tile, from the tile's start
    uint32_t flushed = 0, carry = 0;                                              // bytes of the result in hout; bytes waiting at the front of s_out (< 16)
    for (uint32_t t0 = 0; t0 < E; t0 += MID_TILE) {
        const bool live = entry < MID_TILE;                                       // (a match may step over a whole tile: nothing to search or emit in it)
        uint32_t steps = 0;
        for (uint32_t sub = 0; sub < MID_TILE; sub += MT) {
            // ---- the sub-tile's positions join their chains.  Between sub-tiles a chain is in descending order; inside one, in any order.
            const uint32_t i = t0 + sub + tid;
            const uint32_t h = i < E ? chain_hash(s_fc[i], s_fc[i + 1]) : 0u;
            if (i < E) s_ring[i & (MID_RING - 1)] = atomicExch(&s_head[h], i);
            __syncthreads();
            // ---- the longest L >= 2 with fc[i, i + L) inside the window (L <= distance, L <= E - i), at its largest distance
            if (live && i < E) {
                const uint32_t best = chain_best<MID_RING, MT, MID_STEP_CAP>(s_fc, s_ring, s_head[h], i, E, W, 0u, steps);
                s_key[sub + tid] = best;
            }
            __syncthreads();                                                      // (the next sub-tile's links are written behind this)
        }
        if (!live) { entry -= MID_TILE; continue; }
        if (__syncthreads_or(steps > MID_STEP_CAP)) { block_done(flag, GROUP_BACK); return; }
        // ---- the greedy chain inside the tile: r -> r + max(1, L) (lzss.go:139-142), MID_TILE: beyond the tile
        // (the kernel's own copy of lzss_greedy_chain: through the helper 256 x 64 KiB measured 1 % slower, above the parent's spread; LEDGER)
        const uint32_t R = min(MID_TILE, E - t0);
        for (uint32_t r = tid; r <= MID_TILE; r += MT) {
            s_jmp[r] = (uint16_t)(r < R ? min(MID_TILE, r + max(1u, s_key[r] >> 16)) : MID_TILE);
            s_on[r] = r == entry;
        }
        __syncthreads();
        int cur = 0;
        for (uint32_t reach = 1; reach < MID_TILE + 1; reach <<= 1) {              // after the round: everything within 2 * reach - 1 steps of the entry
            const uint16_t *ja = s_jmp + cur * (MID_TILE + 8);
            uint16_t *jb = s_jmp + (cur ^ 1) * (MID_TILE + 8);
            for (uint32_t r = tid; r < MID_TILE; r += MT) if (s_on[r]) s_on[ja[r]] = 1;
            for (uint32_t r = tid; r <= MID_TILE; r += MT) jb[r] = ja[ja[r]];
            cur ^= 1;
            __syncthreads();
        }
        // ---- what every chain position puts out: a token iff it is shorter than what it stands for (lzss.go:143), else the bytes
        uint32_t total = 0;
        {
            const uint32_t r0 = 2 * tid;
            LzssItem it[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};                        // (sz 0: not on the chain)
            for (int k = 0; k < 2; k++) {
                const uint32_t r = r0 + k;
                if (r < R && s_on[r]) {
                    it[k] = lzss_item(s_key[r] >> 16, s_key[r] & 0xFFFFu);
                    if (r + max(1u, it[k].L) >= MID_TILE) s_misc[0] = r + max(1u, it[k].L) - MID_TILE;   // (one position of the tile: the chain's last in it)
                }
            }
            uint32_t at = carry + block_scan<MT>(it[0].sz + it[1].sz, s_wave, &total);
            for (int k = 0; k < 2; k++) {
                if (!it[k].sz) continue;
                lzss_item_put(s_out, at, it[k], s_fc + t0 + r0 + k);
                at += it[k].sz;
            }
        }
        __syncthreads();
        // ---- whole 16-byte units go out; what is left waits at the front for the next tile's
        const uint32_t avail = carry + total, units = avail >> 4, rem = avail & 15u;
        if (tid < units) reinterpret_cast<uint4 *>(hout + flushed)[tid] = reinterpret_cast<const uint4 *>(s_out)[tid];
        const uint32_t keep = tid < rem ? s_out[units * 16 + tid] : 0u;
        entry = s_misc[0];
        __syncthreads();
        if (tid < rem) s_out[tid] = (uint8_t)keep;
        flushed += units * 16; carry = rem;
        __syncthreads();
    }
    if (tid == 0 && carry) reinterpret_cast<uint4 *>(hout + flushed)[0] = reinterpret_cast<const uint4 *>(s_out)[0];   // (the slot ends on a whole unit)
    block_done(flag, flushed + carry);
}

// ---------------------------------------------------------------- decompress
__global__ __launch_bounds__(MT) void k_lzss_mid_dec(const SmallMember *__restrict__ tab, uint8_t *__restrict__ base) {
    extern __shared__ uint4 mid_lds[];
    uint8_t *sm = reinterpret_cast<uint8_t *>(mid_lds);
    uint8_t *s_in = sm + DL_IN;
    uint8_t *s_val = sm + DL_VAL;
    uint32_t *s_src = reinterpret_cast<uint32_t *>(sm + DL_SRC);                   // [2][MID_TILE]
    uint8_t *s_cov = sm + DL_COV;
    uint32_t *s_wave = reinterpret_cast<uint32_t *>(sm + DL_WAVE);
    const SmallMember m = tab[blockIdx.x];
    const uint8_t *hin = base + m.in_off;
    uint8_t *hout = base + m.out_off;
    uint32_t *flag = reinterpret_cast<uint32_t *>(base + m.status_off);
    const uint32_t tid = threadIdx.x, n = m.n;
    if (n > E_MAX) { block_done(flag, GROUP_BACK); return; }                       // (the host does not send these)
    for (uint32_t u = tid; u * 16 < n + 32; u += MT) reinterpret_cast<uint4 *>(s_in)[u] = u * 16 < n ? reinterpret_cast<const uint4 *>(hin)[u] : make_uint4(0, 0, 0, 0);
    for (uint32_t i = tid; i < MID_TILE + 64; i += MT) s_cov[i] = 0;
    __syncthreads();
    uint32_t E = 0;                                                                // escaped bytes so far
    for (uint32_t c0 = 0; c0 < n; c0 += MID_TILE) {
        if (c0) {                                                                  // a token's text that began in the chunk before covers this one's first bytes
            const uint32_t spill = tid < 32 ? s_cov[MID_TILE + tid] : 0u;
            __syncthreads();
            for (uint32_t i = tid; i < MID_TILE + 64; i += MT) s_cov[i] = i < 32 ? (uint8_t)spill : (uint8_t)0;
            __syncthreads();
        }
        // ---- the chunk's items, two bytes of it per thread
        TileItems it;
        lzd_items(s_in, 0u, c0, n, E_MAX, s_cov, it);
        uint32_t tot;
        const uint32_t at0 = E + block_scan<MT>(it.outl[0] + it.outl[1], s_wave, &tot);
        if (tot > E_MAX - E) { block_done(flag, GROUP_BACK); return; }             // expands beyond the limit (uniform; every outl <= E_MAX, 2048 of them: no overflow)
        // malformed (the single call words the error), or the slice starts before the data (lzss.go:349): one answer for both, GROUP_BACK
        const bool bad = it.bad || (it.ttl[0] && it.tptr[0] > at0) || (it.ttl[1] && it.tptr[1] > at0 + it.outl[0]);
        if (__syncthreads_or(bad)) { block_done(flag, GROUP_BACK); return; }
        // ---- the chunk's output, a tile at a time in output order
        for (uint32_t s0 = E; s0 < E + tot; s0 += MID_TILE) {
            const uint32_t s1 = min(s0 + MID_TILE, E + tot);
            uint32_t a = at0;
            for (int k = 0; k < 2; k++) {
                if (!it.outl[k]) continue;
                const uint32_t lo = max(a, s0), hi = min(a + it.outl[k], s1);
                if (it.ttl[k]) for (uint32_t q = lo; q < hi; q++) s_src[q - s0] = q - it.tptr[k];
                else if (lo < hi) { s_src[a - s0] = a; s_val[a] = s_in[c0 + 2 * tid + k]; }
                a += it.outl[k];
            }
            __syncthreads();
            // every byte's source: src <- src[src] while it lies in the tile and is not a literal (a copied byte lies before the byte that copies it)
            const int cur = lzd_jump<MT, MID_TILE>(s_src, s0, s1 - s0, 13);
            for (uint32_t r = tid; r < s1 - s0; r += MT) { const uint32_t x = s_src[cur * MID_TILE + r]; if (x != s0 + r) s_val[s0 + r] = s_val[x]; }   // (x: a literal of the tile, or final in an earlier one)
            __syncthreads();
        }
        E += tot;
    }
    if (E == 0) { block_done(flag, GROUP_BACK); return; }                          // (an empty result is the single call's to word)
    // ---- DecodeOpeningSymbols (lzss.go:391-406): a byte is escaped iff the run of 5C right in front of it has odd length, counted from the
    //      last byte that is not 5C (as lzss_small.hip).  A run of ceil(E / MT) bytes per thread.
    const uint32_t per = (E + MT - 1) / MT, q0 = min(E, tid * per), q1 = min(E, q0 + per);
    const uint32_t before = lzd_plain_before<MT>(lzd_last_plain(s_val, 0u, q0, q1), s_wave);   // 1 + the last position in front of q0 whose byte is not 5C; 0: none
    uint32_t total;
    const uint32_t o = block_scan<MT>(lzd_unesc_count(s_val, 0u, q0, q1, before), s_wave, &total);
    uint8_t *s_res = s_in;                                                         // (the stream is parsed: its LDS takes the result)
    lzd_unesc_write(s_val, 0u, q0, q1, before, s_res, o);
    __syncthreads();
    for (uint32_t u = tid; u * 16 < total; u += MT) reinterpret_cast<uint4 *>(hout)[u] = reinterpret_cast<const uint4 *>(s_res)[u];
    block_done(flag, total);
}

}  // namespace

// ---------------------------------------------------------------- the host side: groups in pinned staging (group_run.h)
namespace {
bool mid_enc_takes(const uint8_t *, size_t n, int64_t window) { return n != 0 && n <= LZSS_MID_IN_MAX && window >= 1 && window <= (int64_t)MID_W_MAX; }
bool mid_dec_takes(const uint8_t *, size_t n, int64_t) { return n != 0 && n <= LZSS_MID_E_MAX; }
struct MidEncClass {
    static constexpr const char *what = "lzss batch compress";
    static size_t in_bytes(size_t n) { return lzss_in_slot(n); }
    static size_t out_bytes(size_t n) { return lzss_enc_out_slot(n, LZSS_MID_E_MAX); }
    static int launch(Ctx &c, hipStream_t s, uint32_t g, const SmallMember *tab, uint8_t *base, int64_t window) {
        const int rc = func_dyn_lds(c, reinterpret_cast<const void *>(k_lzss_mid_enc), EL_BYTES); if (rc) return rc;
        RSN_LAUNCH("lzss_batch_mid_enc", k_lzss_mid_enc, dim3(g), dim3(MT), EL_BYTES, s, tab, base, (uint32_t)window);
        return RSN_OK;
    }
};
struct MidDecClass {
    static constexpr const char *what = "lzss batch decompress";
    static size_t in_bytes(size_t n) { return lzss_in_slot(n); }
    static size_t out_bytes(size_t) { return lzss_dec_out_slot(LZSS_MID_E_MAX); }
    static int launch(Ctx &c, hipStream_t s, uint32_t g, const SmallMember *tab, uint8_t *base, int64_t) {
        const int rc = func_dyn_lds(c, reinterpret_cast<const void *>(k_lzss_mid_dec), DL_BYTES); if (rc) return rc;
        RSN_LAUNCH("lzss_batch_mid_dec", k_lzss_mid_dec, dim3(g), dim3(MT), DL_BYTES, s, tab, base);
        return RSN_OK;
    }
};
}  // namespace
const BatchClass &lzss_mid_class(bool compress) {
    static const BatchClass enc = {"lzss mid compress", LZSS_MID_GROUP_MIN, mid_enc_takes, class_run<MidEncClass>, class_run_dev<MidEncClass>},
                            dec = {"lzss mid decompress", LZSS_MID_GROUP_MIN, mid_dec_takes, class_run<MidDecClass>, class_run_dev<MidDecClass>};
    return compress ? enc : dec;
}

}  // namespace rsn
