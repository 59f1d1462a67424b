// huff_big.hip -- the Huffman encoder for the big members of a compress batch: above HUFF_MID_IN_MAX, where a member no longer fits one
// workgroup's LDS (huff_mid.hip), up to HUFF_BIG_IN_MAX bytes of a byte alphabet (codecs.h).
//
// Inside a batch such a member used to be the single call: about ten launches, three copy commands, the host's heap and a host wait, a
// member after the other.  Here a member is cut into TILES of HUFF_BIG_TILE bytes and a group of members is three launches, queued one
// behind the other with nothing on the host between them (huff_big_layout.h: the tiles, a member's scratch, the bit offsets, the bytes a
// tile stores):
//   count   k_huff_big_count, a workgroup per tile: the tile's 16 KiB, 16 bytes a thread, counted into per-wavefront LDS histograms as
//           huff_enc_body counts a member; the 128 counts and a "byte >= 0x80" flag go to the member's scratch.
//   plan    k_huff_big_plan, a workgroup per member: the tiles' counts summed; ranks and header entries by block scans and ONE wavefront
//           that builds the Go-exact tree and codes with wave_tree (huff_small_body.h), exactly as huff_enc_body does (the code
//           tests/huff_big_plan_test.cpp holds against huff_host.cpp at these counts); the header and the pad byte into the member's output
//           slot; every tile's bit length as sum(count x length) over the tile's OWN counts -- the input is not read for it -- and their
//           scan, the pad in front folded into the base.  The code table and the offsets stay in scratch.  A member it does not take --
//           a byte >= 0x80, one distinct byte, a code beyond 24 bits -- gets its status word here: GROUP_BACK_RUNES / GROUP_BACK.
//   emit    k_huff_big_emit, a workgroup per tile of a member that was taken: 16 bytes a thread again, their codes' first bits by a block
//           scan, ORed into an LDS image that starts at the 16-byte unit of the output the tile's first bit lies in (pack_codes16), and
//           stored 16 bytes at a time.  An output byte belongs to the tile its FIRST bit lies in: the tile codes on into the next tile's
//           first symbols until its last byte is full, and leaves the byte its own first bit lies in to the tile before.
// Ownership, the member's status word by the last of its tiles, the grid and the host form are the tiled classes' common shape (DESIGN
// 4.7; tile_dev.h); the done-counter is zeroed by the plan.  No workgroup waits for another; every loop is bounded by the tile, the
// alphabet or the tiles of a member.
#include "huff_small_body.h"
#include "huff_big_layout.h"
#include "tile_dev.h"

namespace rsn {
namespace {

constexpr int BG_T = 1024;                        // threads of a tile's workgroup: 16 bytes each are the tile
constexpr int BG_PT = 256;                        // threads of a member's planning workgroup
static_assert(HUFF_BIG_TILE == 16 * BG_T, "a tile is one round of 16 bytes a thread");
static_assert(BIGL_TILES_MAX <= BG_PT - 128 && BIGL_TILES_MAX <= 128, "the plan reads a tile's flag in a thread behind the 128 of the counts, and a tile's bits a thread");
// ---- the encoder's arithmetic at n <= HUFF_BIG_IN_MAX (what plan_tree, plan_codes and the scans rely on)
static_assert(HUFF_BIG_IN_MAX < PLAN_COUNT_LIMIT_WIDE, "every sum of counts is at most n");
static_assert(((unsigned long long)HUFF_BIG_IN_MAX << 8) < (1ull << 32), "a sum of counts and a node id pack into one word (plan_item)");
static_assert((unsigned long long)HUFF_BIG_IN_MAX * 24 + 8ull * HUFF_BIG_HDR_MAX + 8 < (1ull << 32), "a bit position in a member's output slot is one word");
static_assert(HUFF_BIG_HDR_MAX <= HUFF_HDR_MAX, "the counts cannot all be long: the class's header bound lies below the other classes'");
// a code of d bits needs counts that sum to at least fib(d + 2): fib(26) = 121393 is within the class, so codes of 24 bits occur and are
// taken; fib(27) = 196418 is too, so a code of 25 bits can occur and the plan hands such a member back -- the emit table is not widened
static_assert(plan_fib(26) <= HUFF_BIG_IN_MAX && plan_fib(27) == 196418 && plan_fib(27) <= HUFF_BIG_IN_MAX, "24-bit codes are taken, 25-bit codes are possible and handed back");
// the image of a tile: at most 24 bits a byte behind the up to 127 bits in front of its first (the 16-byte unit's), the next tile's up to 7
// symbols that fill its last byte, and the word pack_codes16 may OR zeros into behind the last
constexpr uint32_t BG_IMG_WORDS = HUFF_BIG_TILE * 24 / 32 + 16;
static_assert((127ull + (unsigned long long)HUFF_BIG_TILE * 24 + 7 + 24) / 32 + 2 <= BG_IMG_WORDS && BG_IMG_WORDS % 4 == 0, "the image holds the longest tile");
static_assert(BG_IMG_WORDS * 4 + 2048 <= 64 * 1024, "static LDS of k_huff_big_emit; two workgroups to a CU");

__global__ __launch_bounds__(BG_T) void k_huff_big_count(const SmallMember *__restrict__ tab, const uint8_t *__restrict__ base, uint32_t *__restrict__ scr) {
    __shared__ uint32_t s_cnt[BG_T / 64][128];
    const SmallMember m = tab[blockIdx.y];
    const uint32_t n = m.n, t = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    if (n > HUFF_BIG_IN_MAX || t >= big_tiles(n)) return;                 // (uniform: the whole workgroup)
    for (uint32_t i = tid; i < BG_T / 64 * 128; i += BG_T) (&s_cnt[0][0])[i] = 0;
    __syncthreads();
    const uint4 *in = reinterpret_cast<const uint4 *>(base + m.in_off) + (size_t)t * (HUFF_BIG_TILE / 16);
    const uint32_t len = big_tile_len(n, t);
    uint32_t high = 0;
    if (tid * 16 < len) {
        const uint4 v = in[tid];                                          // (the input slot holds whole units and zeros behind n)
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        const uint32_t valid = min(16u, len - tid * 16);
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t b = (w[j >> 2] >> (8 * (j & 3))) & 0xFF;
            if ((uint32_t)j < valid) { high |= b & 0x80; atomicAdd(&s_cnt[wave][b & 0x7F], 1u); }
        }
    }
    high = (uint32_t)__syncthreads_or((int)high);
    uint32_t *my = scr + (size_t)blockIdx.y * BIG_SCR_WORDS;
    if (tid < 128) {
        uint32_t c = 0;
        for (uint32_t w = 0; w < BG_T / 64; w++) c += s_cnt[w][tid];
        my[BIG_SCR_HIST + t * 128 + tid] = c;
    }
    if (tid == 0) my[BIG_SCR_FLAG + t] = high ? 1u : 0u;
}

__global__ __launch_bounds__(BG_PT) void k_huff_big_plan(const SmallMember *__restrict__ tab, uint8_t *__restrict__ base, uint32_t *__restrict__ scr) {
    __shared__ uint32_t s_tot[128], s_lf[128], s_tab[128], s_tb[BIGL_TILES_MAX];
    __shared__ uint8_t s_leaf[128];
    __shared__ uint32_t s_wave[BG_PT / 64 + 1];
    __shared__ uint32_t s_plan[2];                     // max code length, payload bits
    const SmallMember m = tab[blockIdx.x];
    uint32_t *status = reinterpret_cast<uint32_t *>(base + m.status_off);
    uint32_t *my = scr + (size_t)blockIdx.x * BIG_SCR_WORDS;
    const uint32_t n = m.n, tid = threadIdx.x, wave = tid >> 6;
    // a member that is not taken: no byte of it will be written, so its word is stored here; the emit launch reads the verdict and leaves
    auto hand_back = [&](uint32_t v) { if (tid == 0) { my[BIG_SCR_META + BIG_META_VERDICT] = v; *status = v; } };
    if (n < 2 || n > HUFF_BIG_IN_MAX) { hand_back(GROUP_BACK); return; }   // (the host never sends one)
    const uint32_t T = big_tiles(n);
    // ---- the tiles' counts summed (huffman.go:306-311)
    uint32_t c = 0, high = 0;
    if (tid < 128) {
        for (uint32_t t = 0; t < T; t++) c += my[BIG_SCR_HIST + t * 128 + tid];
        s_tot[tid] = c; s_tab[tid] = 0;
    } else if (tid - 128 < T) high = my[BIG_SCR_FLAG + tid - 128];
    high = (uint32_t)__syncthreads_or((int)high);
    const uint32_t a = (uint32_t)__syncthreads_count(tid < 128 && c != 0);
    if (high || a < 2) { hand_back(high ? GROUP_BACK_RUNES : GROUP_BACK); return; }
    // ---- leaves in (count asc, byte asc) order; the header's entries ascending by byte, '\\' first when it would be last (huffman.go:312-318)
    const bool above_bs = __syncthreads_or(tid > 0x5C && tid < 128 && c != 0);
    const bool bs_first = s_tot[0x5C] != 0 && !above_bs;
    const uint32_t e_len = tid < 128 && c ? plan_entry_len(c, tid) : 0u;
    if (tid < 128 && c) { const uint32_t r = plan_leaf_rank(s_tot, tid); s_lf[r] = c; s_leaf[r] = (uint8_t)tid; }
    uint32_t e_at = block_excl_scan<BG_PT / 64>(e_len, s_wave);
    const uint32_t E = s_wave[BG_PT / 64];                            // bytes of the entries
    if (bs_first) e_at = tid == 0x5C ? 0u : e_at + plan_entry_len(s_tot[0x5C], 0x5C);
    // ---- the tree and the codes: one wavefront (huffman.go:93-127)
    if (wave == 0) {
        const uint32_t au = (uint32_t)__builtin_amdgcn_readfirstlane((int)a);
        LaneStore<2> kids;
        LaneStore<4> code;
        wave_tree<8>(s_lf, au, kids, code);
        wave_codes_out(code, au, s_lf, s_leaf, s_tab, s_plan);
    }
    __syncthreads();
    const uint32_t max_len = s_plan[0], pay_bits = s_plan[1];
    const uint32_t H = E + 3, pad = (8 - pay_bits % 8) % 8;              // huffman.go:245-249
    const uint32_t total = H + (pay_bits + pad) / 8;
    if (big_plan_refuses(max_len, H, total, huff_big_enc_out_slot(n))) { hand_back(GROUP_BACK); return; }
    // ---- the header into the output slot; the table, the tiles' first bits and the member's words into scratch
    uint8_t *out = base + m.out_off;
    if (e_len) plan_entry(c, tid, out + e_at);
    if (tid == 0) { out[E] = '\\'; out[E + 1] = '\n'; out[E + 2] = (uint8_t)pad; }
    if (tid < 128) my[BIG_SCR_TAB + tid] = s_tab[tid];
    if (tid < T) s_tb[tid] = big_tile_bits(my + BIG_SCR_HIST + tid * 128, s_tab);
    __syncthreads();
    if (tid == 0) {
        big_tile_offsets(s_tb, T, 8 * H + pad, my + BIG_SCR_OFF);
        my[BIG_SCR_META + BIG_META_VERDICT] = 0; my[BIG_SCR_META + BIG_META_TOTAL] = total; my[BIG_SCR_META + BIG_META_DONE] = 0;
    }
}

__global__ __launch_bounds__(BG_T) void k_huff_big_emit(const SmallMember *__restrict__ tab, uint8_t *__restrict__ base, uint32_t *__restrict__ scr) {
    __shared__ __attribute__((aligned(16))) uint32_t s_img[BG_IMG_WORDS];
    __shared__ uint32_t s_tab[128];
    __shared__ uint32_t s_wave[BG_T / 64 + 1];
    const SmallMember m = tab[blockIdx.y];
    const uint32_t n = m.n, t = blockIdx.x, tid = threadIdx.x;
    if (n < 2 || n > HUFF_BIG_IN_MAX || t >= big_tiles(n)) return;        // (uniform: the whole workgroup)
    uint32_t *my = scr + (size_t)blockIdx.y * BIG_SCR_WORDS;
    if (my[BIG_SCR_META + BIG_META_VERDICT] != 0) return;                // handed back by the plan, which has stored its word
    const uint32_t T = big_tiles(n), b0 = my[BIG_SCR_OFF + t], b1 = my[BIG_SCR_OFF + t + 1], total = my[BIG_SCR_META + BIG_META_TOTAL];
    // the image's first byte is the output's byte u0, a 16-byte unit's first: bit positions below are the image's
    const uint32_t u0 = big_tile_origin(b0), i0 = b0 - 8 * u0, i1 = b1 - 8 * u0;
    const uint32_t img_words = min(BG_IMG_WORDS, (i1 + 31) / 32 + 3);    // what the tile and the symbols behind it can reach
    for (uint32_t i = tid; i < img_words; i += BG_T) s_img[i] = 0;
    if (tid < 128) s_tab[tid] = my[BIG_SCR_TAB + tid];
    __syncthreads();
    const uint8_t *inb = base + m.in_off;
    const uint32_t len = big_tile_len(n, t);
    const bool has = tid * 16 < len;
    const uint4 v = has ? (reinterpret_cast<const uint4 *>(inb) + (size_t)t * (HUFF_BIG_TILE / 16))[tid] : make_uint4(0, 0, 0, 0);
    const uint32_t valid = has ? min(16u, len - tid * 16) : 0u;
    const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
    uint32_t e[16], bits = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        e[j] = (uint32_t)j < valid ? s_tab[(w4[j >> 2] >> (8 * (j & 3))) & 0x7F] : 0u;
        bits += e[j] >> 24;
    }
    const uint32_t pos0 = i0 + block_excl_scan<BG_T / 64>(bits, s_wave);
    if (bits && pos0 + bits <= i1) pack_codes16(e, pos0, s_img);          // (the counts say so: the tile's bits end at i1)
    // ---- the next tile's first symbols, until this tile's last byte is full: at most 7, a code has a bit at least.  The last tile ends
    // on a byte (the pad lies in front), and a tile that ends the stream short of a byte does not exist.
    if (tid == 0 && (i1 & 7) && t + 1 < T) {
        const uint32_t stop = (i1 + 7) & ~7u;
        uint32_t p = i1;
        for (uint32_t j = 0; j < 7 && p < stop; j++) {
            const uint32_t at = (t + 1) * HUFF_BIG_TILE + j;
            if (at >= n) break;
            const uint32_t ent = s_tab[inb[at] & 0x7F], l = ent >> 24;
            if (!l) break;                                                // (a byte the counts do not know: cannot be)
            const unsigned long long val = (unsigned long long)(ent & 0xFFFFFFu) << (64 - (p & 31) - l);
            atomicOr(&s_img[p >> 5], __builtin_bswap32((uint32_t)(val >> 32)));
            if ((uint32_t)val) atomicOr(&s_img[(p >> 5) + 1], __builtin_bswap32((uint32_t)val));
            p += l;
        }
    }
    __syncthreads();
    // ---- the tile's own bytes out (the range may be empty, and begin in the unit behind u0), and the member's word by its last tile
    tile_store_out<BG_T>(base + m.out_off, reinterpret_cast<const uint8_t *>(s_img), u0, big_tile_first_byte(t, b0), big_tile_end_byte(b1));
    if (tile_finish(&my[BIG_SCR_META + BIG_META_DONE], T))
        __hip_atomic_store(reinterpret_cast<uint32_t *>(base + m.status_off), total, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

// the three launches of a group of g members; gx: tiles of the largest member the call holds
int big_launch(Ctx &c, hipStream_t s, uint32_t g, uint32_t gx, const SmallMember *tab, uint8_t *base) {
    void *p;
    const int rc = dev_buf(c, Slot::GD_BIG_TILES, (size_t)g * BIG_SCR_WORDS * 4, &p); if (rc) return rc;
    uint32_t *scr = (uint32_t *)p;
    RSN_LAUNCH("huff_batch_big_count", k_huff_big_count, dim3(gx, g), dim3(BG_T), 0, s, tab, (const uint8_t *)base, scr);
    RSN_LAUNCH("huff_batch_big_plan", k_huff_big_plan, dim3(g), dim3(BG_PT), 0, s, tab, base, scr);
    RSN_LAUNCH("huff_batch_big_emit", k_huff_big_emit, dim3(gx, g), dim3(BG_T), 0, s, tab, base, scr);
    return RSN_OK;
}

constexpr const char *BIG_WHAT = "huffman batch compress";
bool big_enc_takes(const uint8_t *, size_t n, int64_t) { return n > HUFF_MID_IN_MAX && n <= HUFF_BIG_IN_MAX; }   // (the length alone: both forms)
size_t big_out_bytes(size_t n) { return huff_big_enc_out_slot((uint32_t)n); }

// The device form: run_groups_dev's groups -- k_group_gather, the three launches, k_group_scatter -- of up to HUFF_BIG_GROUP_BYTES of staging.
int big_enc_run_dev(Ctx &c, hipStream_t s, const std::vector<size_t> &idx, const rsn_dev_member *mem, int64_t, const DevPlans *, std::vector<uint32_t> &answers) {
    const uint32_t gx = grid_tiles_of_largest(idx, mem, HUFF_BIG_IN_MAX, big_tiles);
    return run_groups_dev(c, s, BIG_WHAT, idx, mem, [&](size_t k) { return huff_enc_in_slot(mem[idx[k]].n); }, [&](size_t k) { return big_out_bytes(mem[idx[k]].n); },
        [&](hipStream_t s2, uint32_t g, const SmallMember *tab, uint8_t *base) { return big_launch(c, s2, g, gx, tab, base); }, answers, HUFF_BIG_GROUP_BYTES);
}

// The host form: the members through the device form above (the kernels read a member twice: never out of pinned host memory).
int big_enc_run(Ctx &c, const std::vector<size_t> &idx, const uint8_t *const *ins, const size_t *lens, int64_t window,
                const SmallTake &take, std::vector<size_t> &back, size_t *failed, std::vector<size_t> *back_runes) {
    return run_members_copied(c, BIG_WHAT, "a stream", idx, ins, lens, big_out_bytes,
        [&](hipStream_t s, const std::vector<size_t> &all, const rsn_dev_member *mem, std::vector<uint32_t> &answers) { return big_enc_run_dev(c, s, all, mem, window, nullptr, answers); },
        take, back, failed, back_runes);
}

}  // namespace
const BatchClass &huff_big_class() {
    static const BatchClass enc = {"huffman big compress", HUFF_BIG_GROUP_MIN, big_enc_takes, big_enc_run, big_enc_run_dev};
    return enc;
}

}  // namespace rsn
