// lzss_tile_dec.hip -- the LZSS decoder for the streams of a decompress batch that no workgroup holds: longer than LZSS_MID_E_MAX, or
// expanding to more than that, up to LZSS_TILE_DEC_IN_MAX bytes of stream and LZSS_TILE_DEC_OUT_MAX escaped bytes (codecs.h).
//
// Inside a batch such a stream used to be the single call -- a dozen launches and host round trips, a stream after the other -- and it is
// the ordinary case for what lzss_tile.hip writes.  Nothing about a stream is known before it is parsed, so the class stands BEHIND the
// rows (codecs.h: BehindClass, pool REST) and a group of members is four launches, queued one behind the other with nothing on the host
// between them (lzss_tile_dec_layout.h: the tiles, a member's scratch, which tile stores which byte):
//   parse    k_lzss_tile_dec_parse, a workgroup per tile of LZSS_TILE_POS STREAM bytes: every '<' parses its token (an escaped stream
//            holds no '<' of its own, so every '<' begins a token and no token holds one), reading up to 22 bytes past the tile's end; the
//            tile's leading bytes that belong to a token begun in the tile before are found by looking back the same 22 bytes.  Per tile:
//            its output bytes, a malformed flag, and the most a pointer reaches in front of the tile's first output byte.  The rules are
//            k_lzss_mid_dec's (lzss_dec_body.h: lzd_token).
//   plan     k_lzss_tile_dec_plan, a workgroup per member: a scan of the tiles' outputs gives every stream tile's first escaped byte and
//            E; GROUP_BACK for a malformed stream, a pointer that starts before the data, E = 0 and E > LZSS_TILE_DEC_OUT_MAX; per OUTPUT
//            tile the stream tile its first byte comes from.
//   resolve  k_lzss_tile_dec_resolve, a workgroup per tile of LZSS_TILE_POS OUTPUT bytes of a taken member: the items of the stream tiles
//            that reach into it are parsed again (a tile may span any number of stream tiles, zero-length tokens give nothing: the loop is
//            bounded by the member's tiles), every byte gets its source, the chains inside the tile are settled by pointer jumping in LDS
//            (lzd_jump).  A byte whose chain ends at a literal of the tile goes into the member's escaped image in scratch; a byte whose
//            chain leaves the tile keeps a descriptor: the position in an EARLIER tile it copies.
//   finish   k_lzss_tile_dec_finish, a workgroup per member, its output tiles in order: every descriptor's byte is read from the image --
//            its tile is one this workgroup has finished, so pointers of any reach are allowed -- and written back; the tile is unescaped
//            (DecodeOpeningSymbols, lzss.go:391-406) with the 5C run's parity carried from tile to tile; the result goes to the output slot
//            at the running offset, whole 16-byte units where it can (tile_dev.h: tile_store_out).  Between tiles: a barrier between a release and an
//            acquire fence of workgroup scope -- the image is read again by this workgroup alone, whose waves share one CU's cache.  The
//            image is read with ordinary loads through a pointer that promises nothing.  The member's length goes into its status word
//            last, as an agent-scope release.
// Nothing polls the status word: k_group_scatter reads it, on the same stream.  No workgroup waits for another; every loop is bounded by
// the tile, the token's text, the doublings or the tiles of a member.  Nothing a launch reads from scratch is left from an earlier group:
// parse writes every stream tile's three words, plan the verdict, E and both tile tables, resolve the image or the descriptor of every
// position below E.
#include "group_run.h"
#include "lzss_dec_body.h"
#include "lzss_tile_dec_layout.h"
#include "tile_dev.h"

namespace rsn {
namespace {

constexpr int TT = 1024;                          // threads of parse, resolve and finish
constexpr int PT = 256;                           // threads of plan: one per stream tile
constexpr uint32_t TILE = LZSS_TILE_POS;          // bytes of a tile (two per thread)
constexpr uint32_t D_IN_BYTES = LZTD_HALO + TILE + LZTD_HALO;   // the stream a tile's workgroup holds
constexpr uint32_t D_COV_BYTES = TILE + 64;       // cover marks: the tile and a token's reach behind it
constexpr uint32_t D_IMG = TILE + 64;             // the finish image: up to 15 bytes in front of the tile's first, its bytes, slack
constexpr int D_ROUNDS = 13;                      // doublings of the pointer jumping: 2048 positions need 12 (k_lzss_mid_dec's count)
static_assert(TILE == 2 * TT && LZTD_IN_TILES_MAX <= PT && D_IN_BYTES % 16 == 0 && LZTD_REACH + 1 <= 64, "two bytes a thread; a plan thread a stream tile");
static_assert(15 + TILE <= D_IMG && D_IMG % 16 == 0, "the image holds the longest tile: unescaping never adds a byte");

// the q-th member's scratch; null: the slot does not hold it (the host sizes the slot for every group: lzss_tile_dec_layout.h)
__device__ __forceinline__ uint32_t *dec_scr(uint32_t *scr, unsigned long long scr_words, uint32_t q) {
    return lztd_scr_at(q + 1) <= scr_words ? scr + lztd_scr_at(q) : nullptr;
}

// The items of the stream tile that begins at c0 (a multiple of TILE, below n), as k_lzss_mid_dec parses a chunk (lzss_dec_body.h:
// lzd_items).  s_in: uint8[D_IN_BYTES], the stream from c0 - LZTD_HALO on (zeros outside it); s_cov: uint8[D_COV_BYTES].  Ends behind a
// barrier.
__device__ __forceinline__ void tile_items(const uint8_t *in, uint32_t n, uint32_t c0, uint8_t *s_in, uint8_t *s_cov, TileItems &it) {
    const uint32_t tid = threadIdx.x, org = c0 - LZTD_HALO;                      // (wraps for the first tile: s_in[q - org] is byte q all the same)
    const uint32_t slot = (n + 15) & ~15u;                                       // (the input slot holds whole units)
    for (uint32_t u = tid; u < D_IN_BYTES / 16; u += TT) {
        const uint32_t p = org + 16 * u;                                         // (a multiple of 16; beyond 2^31: in front of the stream)
        reinterpret_cast<uint4 *>(s_in)[u] = p < slot ? *reinterpret_cast<const uint4 *>(in + p) : make_uint4(0, 0, 0, 0);
    }
    for (uint32_t i = tid; i < D_COV_BYTES / 4; i += TT) reinterpret_cast<uint32_t *>(s_cov)[i] = 0;
    __syncthreads();
    // ---- a token begun in the tile before covers this one's first bytes
    if (tid < LZTD_REACH && c0 > tid) {
        const uint32_t p = c0 - 1 - tid;
        uint32_t ptr, len = 0, ttl = 0;
        if (s_in[p - org] == '<' && lzd_token(s_in, org, p, n, LZSS_TILE_DEC_OUT_MAX, ptr, len, ttl))
            for (uint32_t t = c0 - p; t < ttl; t++) s_cov[p + t - c0] = 1;
    }
    lzd_items(s_in, org, c0, n, LZSS_TILE_DEC_OUT_MAX, s_cov, it);
}

// ---------------------------------------------------------------- parse: a workgroup per stream tile
__global__ __launch_bounds__(TT) void k_lzss_tile_dec_parse(const SmallMember *__restrict__ tab, const uint8_t *__restrict__ base, uint32_t *__restrict__ scr, unsigned long long scr_words) {
    __shared__ __attribute__((aligned(16))) uint8_t s_in[D_IN_BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t s_cov[D_COV_BYTES];
    __shared__ uint32_t s_wave[TT / 64 + 4];
    __shared__ uint32_t s_need;
    const SmallMember m = tab[blockIdx.y];
    const uint32_t n = m.n, t = blockIdx.x, c0 = t * TILE;
    uint32_t *my = dec_scr(scr, scr_words, blockIdx.y);
    if (!my || n > LZSS_TILE_DEC_IN_MAX || c0 >= n) return;                      // (uniform; plan answers what parse leaves out)
    if (threadIdx.x == 0) s_need = 0;
    TileItems it;
    tile_items(base + m.in_off, n, c0, s_in, s_cov, it);
    uint32_t tot;
    const uint32_t at = block_scan<TT>(it.outl[0] + it.outl[1], s_wave, &tot);   // (every outl <= OUT_MAX < 2^19, 2048 of them: no overflow)
    // a token at the tile's output byte l starts inside the data iff ptr <= first + l: the tile's need is the largest ptr - l
    uint32_t need = 0;
    if (it.ttl[0] && it.tptr[0] > at) need = it.tptr[0] - at;
    if (it.ttl[1] && it.tptr[1] > at + it.outl[0]) need = max(need, it.tptr[1] - (at + it.outl[0]));
    if (need) atomicMax(&s_need, need);
    const bool bad = __syncthreads_or(it.bad);
    if (threadIdx.x == 0) {
        my[LZTD_SCR_CNT + t] = min(tot, LZSS_TILE_DEC_OUT_MAX + 1);
        my[LZTD_SCR_FLAG + t] = bad ? 1u : 0u;
        my[LZTD_SCR_NEED + t] = s_need;
    }
}

// ---------------------------------------------------------------- plan: a workgroup per member
__global__ __launch_bounds__(PT) void k_lzss_tile_dec_plan(const SmallMember *__restrict__ tab, uint8_t *__restrict__ base, uint32_t *__restrict__ scr, unsigned long long scr_words) {
    __shared__ uint32_t s_first[LZTD_IN_TILES_MAX + 1];
    __shared__ uint32_t s_wave[PT / 64 + 4];
    const SmallMember m = tab[blockIdx.x];
    const uint32_t n = m.n, tid = threadIdx.x;
    uint32_t *status = reinterpret_cast<uint32_t *>(base + m.status_off);
    uint32_t *my = dec_scr(scr, scr_words, blockIdx.x);
    if (!my || n == 0 || n > LZSS_TILE_DEC_IN_MAX) {                             // (the host does not send these)
        if (tid == 0) { if (my) my[LZTD_SCR_META + LZTD_META_VERDICT] = GROUP_BACK; *status = GROUP_BACK; }
        return;
    }
    const uint32_t T = lztd_tiles(n);
    const uint32_t cnt = tid < T ? my[LZTD_SCR_CNT + tid] : 0u;
    uint32_t E;
    const uint32_t first = block_scan<PT>(cnt, s_wave, &E);
    const bool bad = tid < T && (my[LZTD_SCR_FLAG + tid] != 0 || my[LZTD_SCR_NEED + tid] > first);
    if (tid < T) { s_first[tid] = first; my[LZTD_SCR_FIRST + tid] = first; }
    if (tid == 0) { s_first[T] = E; my[LZTD_SCR_FIRST + T] = E; }
    const bool back = __syncthreads_or(bad) || E == 0 || E > LZSS_TILE_DEC_OUT_MAX;   // (an empty result is the single call's to word)
    if (tid == 0) {
        my[LZTD_SCR_META + LZTD_META_VERDICT] = back ? GROUP_BACK : 0u;
        my[LZTD_SCR_META + LZTD_META_E] = back ? 0u : E;
        if (back) *status = GROUP_BACK;
    }
    if (back) return;
    for (uint32_t o = tid; o < lztd_tiles(E); o += PT) {
        const uint32_t t = lztd_entry_tile(s_first, T, o * TILE);
        my[LZTD_SCR_OT_TILE + o] = t;
        my[LZTD_SCR_OT_OFF + o] = o * TILE - s_first[t];
    }
}

// ---------------------------------------------------------------- resolve: a workgroup per output tile
__global__ __launch_bounds__(TT) void k_lzss_tile_dec_resolve(const SmallMember *__restrict__ tab, const uint8_t *__restrict__ base, uint32_t *__restrict__ scr, unsigned long long scr_words) {
    __shared__ __attribute__((aligned(16))) uint8_t s_in[D_IN_BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t s_cov[D_COV_BYTES];
    __shared__ uint32_t s_src[2 * TILE];                                         // [2][TILE]: where a byte of the tile comes from
    __shared__ uint8_t s_val[TILE];                                              // the tile's literals
    __shared__ uint32_t s_wave[TT / 64 + 4];
    const SmallMember m = tab[blockIdx.y];
    const uint32_t n = m.n, tid = threadIdx.x, o = blockIdx.x;
    uint32_t *my = dec_scr(scr, scr_words, blockIdx.y);
    if (!my || n == 0 || n > LZSS_TILE_DEC_IN_MAX || my[LZTD_SCR_META + LZTD_META_VERDICT] != 0) return;   // handed back by plan, which has stored the word
    const uint32_t E = my[LZTD_SCR_META + LZTD_META_E], T = lztd_tiles(n);
    if (o >= lztd_tiles(E)) return;
    const uint32_t s0 = o * TILE, s1 = s0 + lztd_tile_len(E, o);
    for (uint32_t r = tid; r < TILE; r += TT) { s_src[r] = s0 + r; s_val[r] = 0; }   // (every byte of the tile is an item's: the scans are parse's)
    for (uint32_t t = min(my[LZTD_SCR_OT_TILE + o], T - 1); t < T; t++) {
        const uint32_t first = my[LZTD_SCR_FIRST + t];
        if (first >= s1) break;                                                   // (uniform: every thread reads the same words)
        if (my[LZTD_SCR_CNT + t] == 0) continue;                                  // nothing but a token's text and zero-length tokens
        __syncthreads();                                                          // (the tile before is read: its LDS is this one's)
        const uint32_t c0 = t * TILE;
        TileItems it;
        tile_items(base + m.in_off, n, c0, s_in, s_cov, it);
        uint32_t tot;
        uint32_t a = first + block_scan<TT>(it.outl[0] + it.outl[1], s_wave, &tot);
        for (int k = 0; k < 2; k++) {
            if (!it.outl[k]) continue;
            const uint32_t lo = max(a, s0), hi = min(a + it.outl[k], s1);
            if (it.ttl[k]) for (uint32_t q = lo; q < hi; q++) s_src[q - s0] = q - min(it.tptr[k], q);   // (ptr <= a <= q: plan has checked it)
            else if (lo < hi) { s_src[a - s0] = a; s_val[a - s0] = s_in[c0 + 2 * tid + k - (c0 - LZTD_HALO)]; }
            a += it.outl[k];
        }
    }
    __syncthreads();
    const int cur = lzd_jump<TT, TILE>(s_src, s0, s1 - s0, D_ROUNDS);
    uint8_t *img = reinterpret_cast<uint8_t *>(my + LZTD_SCR_IMG);
    uint32_t *desc = my + LZTD_SCR_DESC;
    for (uint32_t r = tid; r < s1 - s0; r += TT) {
        const uint32_t x = s_src[cur * TILE + r];
        const bool here = x >= s0;                                                // a literal of the tile; otherwise a position of an earlier one
        if (here) img[s0 + r] = s_val[min(x - s0, TILE - 1)];                     // (x <= s0 + r: a source is the byte itself or lies before it)
        desc[s0 + r] = here ? LZTD_NONE : x;
    }
}

// ---------------------------------------------------------------- finish: a workgroup per member
__global__ __launch_bounds__(TT) void k_lzss_tile_dec_finish(const SmallMember *__restrict__ tab, uint8_t *base, uint32_t *scr, unsigned long long scr_words) {
    __shared__ uint8_t s_val[TILE];
    __shared__ __attribute__((aligned(16))) uint8_t s_res[D_IMG];
    __shared__ uint32_t s_wave[TT / 64 + 4];
    __shared__ uint32_t s_last;
    const SmallMember m = tab[blockIdx.x];
    const uint32_t n = m.n, tid = threadIdx.x;
    uint32_t *my = dec_scr(scr, scr_words, blockIdx.x);
    if (!my || n == 0 || n > LZSS_TILE_DEC_IN_MAX || my[LZTD_SCR_META + LZTD_META_VERDICT] != 0) return;
    const uint32_t E = my[LZTD_SCR_META + LZTD_META_E], OT = lztd_tiles(E);
    uint8_t *img = reinterpret_cast<uint8_t *>(my + LZTD_SCR_IMG);
    const uint32_t *desc = my + LZTD_SCR_DESC;
    uint8_t *dst = base + m.out_off;
    uint32_t plain = 0;                                                           // 1 + the last position in front of the tile whose byte is not 5C; 0: none
    uint32_t out_at = 0;                                                          // bytes of the result so far
    uint32_t dn[2] = {2 * tid < E ? desc[2 * tid] : LZTD_NONE, 2 * tid + 1 < E ? desc[2 * tid + 1] : LZTD_NONE};   // the tile's descriptors: resolve's, never written here
    for (uint32_t o = 0; o < OT; o++) {
        const uint32_t s0 = o * TILE, s1 = s0 + lztd_tile_len(E, o);
        const uint32_t q0 = min(s1, s0 + 2 * tid), q1 = min(s1, q0 + 2);
        for (uint32_t q = q0; q < q1; q++) {
            const uint32_t d = dn[q - q0];
            const uint8_t v = img[d == LZTD_NONE ? q : d];                       // (d < s0: final since its tile was finished)
            if (d != LZTD_NONE) img[q] = v;
            s_val[q - s0] = v;
        }
        for (int k = 0; k < 2; k++) { const uint32_t q = s0 + TILE + 2 * tid + k; dn[k] = q < E ? desc[q] : LZTD_NONE; }   // (the next tile's, on their way while this one is unescaped)
        __syncthreads();
        const uint32_t mine = lzd_last_plain(s_val, s0, q0, q1);
        const uint32_t before = max(plain, lzd_plain_before<TT>(mine, s_wave));
        if (tid == TT - 1) s_last = max(before, mine);
        uint32_t tot;
        const uint32_t at = block_scan<TT>(lzd_unesc_count(s_val, s0, q0, q1, before), s_wave, &tot);
        const uint32_t off0 = out_at, off1 = out_at + tot, u0 = lzt_image_first(off0);
        lzd_unesc_write(s_val, s0, q0, q1, before, s_res, off0 - u0 + at);
        __syncthreads();
        tile_store_out<TT>(dst, s_res, u0, off0, off1);                           // (off1 <= E: inside the slot, lzss_dec_out_slot)
        plain = s_last; out_at = off1;
        // ---- the tile is final.  Its bytes are read again by this workgroup alone, whose waves share the CU's cache: a release and an
        //      acquire at WORKGROUP scope around the barrier order every wave's stores of the tile before any wave's loads of the next.
        //      (An agent-scope fence here writes the L2 back and drops the L1 once a tile and wave, and buys nothing: no other workgroup
        //      reads the image, and the next launch begins behind this one's end.)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    if (tid == 0) __hip_atomic_store(reinterpret_cast<uint32_t *>(base + m.status_off), out_at, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

constexpr const char *DEC_WHAT = "lzss batch decompress";

// the launches of a group of g members; members: how many the slot must hold
int dec_launch(Ctx &c, hipStream_t s, uint32_t g, size_t members, const SmallMember *tab, uint8_t *base) {
    const unsigned long long scr_words = lztd_scr_at((uint32_t)members);
    void *p;
    const int rc = dev_buf(c, Slot::GD_LZSS_TILE_DEC, scr_words * 4, &p); if (rc) return rc;
    uint32_t *scr = (uint32_t *)p;
    RSN_LAUNCH("lzss_batch_tile_dec_parse", k_lzss_tile_dec_parse, dim3(LZTD_IN_TILES_MAX, g), dim3(TT), 0, s, tab, base, scr, scr_words);
    RSN_LAUNCH("lzss_batch_tile_dec_plan", k_lzss_tile_dec_plan, dim3(g), dim3(PT), 0, s, tab, base, scr, scr_words);
    RSN_LAUNCH("lzss_batch_tile_dec_resolve", k_lzss_tile_dec_resolve, dim3(LZTD_OUT_TILES_MAX, g), dim3(TT), 0, s, tab, base, scr, scr_words);
    RSN_LAUNCH("lzss_batch_tile_dec_finish", k_lzss_tile_dec_finish, dim3(g), dim3(TT), 0, s, tab, base, scr, scr_words);
    return RSN_OK;
}

// The device form: run_groups_dev's groups -- k_group_gather, the launches, k_group_scatter -- of up to LZSS_TILE_GROUP_BYTES of staging.
// Every member's output slot is the class's largest, so a group holds at most LZSS_TILE_GROUP_BYTES / that slot members (one, where a
// member alone is more), and its scratch is at most LZTD_SCR_PER_STAGING times its staging.
int tile_dec_run_dev(Ctx &c, hipStream_t s, const std::vector<size_t> &idx, const rsn_dev_member *mem, std::vector<uint32_t> &answers) {
    const size_t members = std::min(std::min(idx.size(), SMALL_GROUP_MAX), LZSS_TILE_GROUP_BYTES / lztd_out_slot() + 1);
    return run_groups_dev(c, s, DEC_WHAT, idx, mem, [&](size_t k) { return lztd_in_slot(mem[idx[k]].n); }, [&](size_t) { return lztd_out_slot(); },
        [&](hipStream_t s2, uint32_t g, const SmallMember *tab, uint8_t *base) { return dec_launch(c, s2, g, members, tab, base); }, answers, LZSS_TILE_GROUP_BYTES);
}

// the members of `rest` the class runs: the candidates by their length, sorted, when there are at least its minimum of them; they leave `rest`
template <class Len>
std::vector<size_t> dec_candidates(std::vector<size_t> &rest, Len len) {
    std::vector<size_t> cand, others;
    for (size_t i : rest) (lztd_candidate(len(i)) ? cand : others).push_back(i);
    if (cand.size() < LZSS_TILE_DEC_GROUP_MIN) return {};
    std::sort(cand.begin(), cand.end());
    rest.swap(others);
    return cand;
}

// The two offers (codecs.h: BehindClass; pool REST, so `rest` is the pool itself).  The kernels read the stream in pieces and keep a
// member's image in scratch, so they never run on pinned host memory: the host form goes through the device form (the tiled
// classes' common shape).  What the kernels hand back stays in `rest`.
int tile_dec_offer(Ctx &c, std::vector<size_t> &rest, std::vector<size_t> &, const uint8_t *const *ins, const size_t *lens, const SmallTake &take, size_t *failed) {
    std::vector<size_t> others = rest;                                    // (`rest` stays as it is when the run fails)
    const std::vector<size_t> idx = dec_candidates(others, [&](size_t i) { return lens[i]; });
    if (idx.empty()) return RSN_OK;
    const int rc = run_members_copied(c, DEC_WHAT, "a result", idx, ins, lens, [](size_t) { return lztd_out_slot(); },
        [&](hipStream_t s, const std::vector<size_t> &all, const rsn_dev_member *mem, std::vector<uint32_t> &answers) { return tile_dec_run_dev(c, s, all, mem, answers); },
        take, others, failed, nullptr);
    if (rc) return rc;
    std::sort(others.begin(), others.end());
    rest.swap(others);
    return RSN_OK;
}

int tile_dec_offer_dev(Ctx &c, hipStream_t s, std::vector<size_t> &rest, std::vector<size_t> &, const rsn_dev_member *mem, const DevPlans *,
                       std::vector<size_t> &idx, std::vector<uint32_t> &answers) {
    idx = dec_candidates(rest, [&](size_t i) { return (size_t)mem[i].n; });
    if (idx.empty()) return RSN_OK;
    return tile_dec_run_dev(c, s, idx, mem, answers);
}

}  // namespace

const BehindClass &lzss_tile_dec_class() {
    static const BehindClass dec = {BehindClass::REST, tile_dec_offer, tile_dec_offer_dev};
    return dec;
}

}  // namespace rsn
