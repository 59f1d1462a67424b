// huff_rune_mid.hip -- the grouped Huffman encoder for the mid-size members whose bytes are not all below 0x80 (rsn_huffman_compress_batch
// and its device and layered forms).  k_huff_mid_enc (huff_mid.hip) hands such a member back as GROUP_BACK_RUNES; when a call
// holds HUFF_RUNE_MID_GROUP_MIN of them, of more than HUFF_RUNE_IN_MAX and at most HUFF_RUNE_MID_IN_MAX bytes each, they come here instead
// of taking the single call one by one: ONE launch per group, ONE workgroup of 1024 threads per member, nothing on the host between the
// count and the emit.  It is k_huff_batch_rune_enc's algorithm (huff_rune.hip: the runes, the table, the plan, the header, the bits -- read
// there what each step is) at k_huff_mid_enc's shape: the member (64 KiB) and the image of its stream in dynamic LDS, one workgroup to a
// CU, 16 KiB of the member a round of the emit.  What differs from the 16 KiB kernel:
//   counts   a rune may occur 65535 times (PLAN_RUNE_MID_COUNT_MAX, huff_plan_rune.h): a heap item count << 9 | id still is one word, a
//            count still has five digits, so HUFF_RUNE_HDR_MAX still is the longest header;
//   depth    Fibonacci counts that sum to at most 65536 give a code of 22 bits, inside the packer's 24 (asserted below as huff_mid.hip does);
//   image    256 symbols have the flat 8-bit code as a prefix code and Huffman's is no longer, a rune is a byte at least: the payload is at
//            most n bytes, so the image is HUFF_RUNE_HDR_MAX + n and slack, not huff_rune_enc_out_slot's 9 n / 8 -- that would not fit;
//   rounds   four rounds of 1024 lanes: the scan's total carries from a round into the next, and a rune whose bytes lie across a round's
//            end is coded in the round of its START alone -- a lane classifies its unit with the words of both neighbours, whichever
//            round they belong to, and codes the starts among its own 16 positions.
// The counts take one LDS atomic a rune; aggregating a wavefront's equal runes first (64 lanes on the space character's slot) was not tried.
// Status word: the stream's length, or GROUP_BACK -- more than HUFF_RUNE_SYMS_MAX distinct runes, fewer than two, no rune >= 0x80, or a
// code beyond 24 bits (which cannot occur; the guard is the packer's).
// LDS: member 64 KiB + 16 B, image 68160 B, table 6 KiB, symbols and ranks 6 KiB: 146096 B, 142.7 KiB of the CU's 160 KiB, one workgroup a CU.
#include "huff_small_body.h"
#include "huff_plan_rune.h"
#include "huff_utf8.h"
#include "huff_rune_mid_select.h"

namespace rsn {
namespace {

constexpr uint32_t RM_T = 1024;
constexpr uint32_t RM_IN_MAX = HUFF_RUNE_MID_IN_MAX;
constexpr uint32_t RM_SYMS = PLAN_RUNE_SYMS_MAX;      // symbols at most: the first RM_SYMS threads hold them, two table slots each
constexpr uint32_t RM_SLOTS = PLAN_RUNE_SLOTS;
constexpr uint32_t RM_EMPTY = 0xFFFFFFFFu;            // (no rune)
constexpr uint32_t RM_IMG_WORDS = huff_rune_mid_enc_out_slot(RM_IN_MAX) / 4;
static_assert(RM_IN_MAX <= PLAN_RUNE_MID_COUNT_MAX && RM_IN_MAX <= HUFF_MID_IN_MAX && RM_IN_MAX > HUFF_RUNE_IN_MAX && HUFF_RUNE_SYMS_MAX == RM_SYMS,
              "the counts the plan takes, the members k_huff_mid_enc hands back, one alphabet");
static_assert(RM_SLOTS == 2 * RM_SYMS && RM_SYMS <= RM_T && RM_IMG_WORDS % 4 == 0 && RM_IN_MAX % 16 == 0, "two slots a symbol's thread, the image in 16-byte units");
// a code of d bits needs counts that sum to at least fib(d + 2): fib(24) = 46368 <= 65536 < fib(25)
constexpr unsigned long long rm_fib(int k) { unsigned long long a = 0, b = 1; for (int i = 0; i < k; i++) { const unsigned long long t = a + b; a = b; b = t; } return a; }
static_assert(rm_fib(24) <= RM_IN_MAX && rm_fib(25) > RM_IN_MAX, "the deepest code of a member is 22 bits: inside the 24 of the packer");
constexpr bool rm_sizes_hold() {
    for (uint32_t n = 2; n <= RM_IN_MAX; n++)
        if (huff_rune_mid_stream_max(n) + 3 > huff_rune_mid_enc_out_slot(n) || (n > HUFF_RUNE_IN_MAX && huff_rune_mid_enc_out_slot(n) > huff_compress_bound(n))) return false;
    return true;
}
static_assert(rm_sizes_hold(), "the slot holds the longest stream in whole words, and that of a member the class takes lies within huff_compress_bound");
// ---- LDS (dynamic; offsets in bytes).  Beside it the static: the table (3 x 512 words), the symbols and ranks (6 x 256), the scan's words
constexpr uint32_t RL_IN = 0;                                     // the member, and a unit of zeros behind its last
constexpr uint32_t RL_IMG = RL_IN + RM_IN_MAX + 16;               // the image of the stream
constexpr uint32_t RL_BYTES = RL_IMG + RM_IMG_WORDS * 4;
static_assert(RL_IMG % 16 == 0 && RL_BYTES + 3 * RM_SLOTS * 4 + 6 * RM_SYMS * 4 + 1024 <= 160 * 1024, "LDS of k_huff_mid_rune_enc");

// the 16 positions of unit u of the member in LDS (zeros behind its n bytes, a zero unit behind its last)
__device__ __forceinline__ uint32_t rm_classify(const uint4 *s_in, uint32_t u, uint32_t n, uint32_t rune[16]) {
    const uint4 v = s_in[u];
    const uint32_t w[6] = {u ? s_in[u - 1].w : 0u, v.x, v.y, v.z, v.w, s_in[u + 1].x};
    const uint32_t left = n - 16 * u;
    return classify16_words(w, left >= 16 ? 0xFFFFu : (1u << left) - 1u, rune);
}

__global__ __launch_bounds__(RM_T) void k_huff_mid_rune_enc(const SmallMember *__restrict__ tab, uint8_t *__restrict__ base) {
    extern __shared__ uint4 rm_lds[];
    uint4 *s_in = reinterpret_cast<uint4 *>(reinterpret_cast<uint8_t *>(rm_lds) + RL_IN);             // [RM_IN_MAX / 16 + 1]
    uint32_t *s_img = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(rm_lds) + RL_IMG);     // [RM_IMG_WORDS]
    __shared__ uint32_t s_key[RM_SLOTS], s_cnt[RM_SLOTS], s_code[RM_SLOTS];      // the table: rune, count, and once planned len << 24 | code
    __shared__ uint32_t s_rune[RM_SYMS], s_rcnt[RM_SYMS], s_rslot[RM_SYMS];      // the symbols compacted, in slot order
    __shared__ uint32_t s_lf[RM_SYMS], s_lslot[RM_SYMS];                         // the leaves in (count asc, rune asc) order: count, slot
    __shared__ uint32_t s_ord[RM_SYMS];                                          // the symbols ascending by rune: index into the compacted ones
    __shared__ uint32_t s_wave[RM_T / 64 + 1];
    __shared__ uint32_t s_meta[3];                     // distinct runes; more than the class takes; no rune >= 0x80
    __shared__ uint32_t s_plan[2];                     // max code length, payload bits
    const SmallMember m = tab[blockIdx.x];
    uint32_t *status = reinterpret_cast<uint32_t *>(base + m.status_off);
    const uint32_t n = m.n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (n < 2 || n > RM_IN_MAX) { block_done(status, GROUP_BACK); return; }    // (the host never sends one)
    if (tid < RM_SLOTS) { s_key[tid] = RM_EMPTY; s_cnt[tid] = 0; }
    for (uint32_t i = tid; i < RM_IMG_WORDS; i += RM_T) s_img[i] = 0;
    if (tid < 3) s_meta[tid] = 0;
    // ---- the member into LDS: its n bytes, zeros to the end of its last unit and one unit of zeros more
    const uint32_t units = (n + 15) / 16;
    const uint4 *hin = reinterpret_cast<const uint4 *>(base + m.in_off);
    for (uint32_t u = tid; u <= units; u += RM_T) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (u < units) {
            v = hin[u];
            const uint32_t rest = n - 16 * u;                             // bytes of this unit that are the member's (16 or more: all)
            if (rest < 16) {
                uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) {
                    const uint32_t keep = rest > 4 * k ? min(rest - 4 * k, 4u) : 0u;
                    w[k] = keep == 4 ? w[k] : keep == 0 ? 0u : w[k] & ((1u << (8 * keep)) - 1);
                }
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
        s_in[u] = v;
    }
    __syncthreads();
    // ---- distinct runes and their counts (huffman.go:306-311)
    for (uint32_t u = tid; u < units; u += RM_T) {
        uint32_t rune[16];
        const uint32_t mask = rm_classify(s_in, u, n, rune);
#pragma unroll 1
        for (uint32_t k = 0; k < 16; k++) {
            if (!((mask >> k) & 1u)) continue;
            if (*(volatile uint32_t *)&s_meta[1]) break;                  // the table holds more than the class takes: handed back below
            const uint32_t r = rune[k];
            uint32_t slot = plan_rune_hash(r), p = 0;
            for (; p < RM_SLOTS; p++) {
                const uint32_t old = atomicCAS(&s_key[slot], RM_EMPTY, r);
                if (old == RM_EMPTY && atomicAdd(&s_meta[0], 1u) >= HUFF_RUNE_SYMS_MAX) s_meta[1] = 1;
                if (old == RM_EMPTY || old == r) { atomicAdd(&s_cnt[slot], 1u); break; }
                slot = (slot + 1) & (RM_SLOTS - 1);
            }
            if (p == RM_SLOTS) s_meta[1] = 1;                             // (a full table: more than RM_SLOTS runes were on their way at once)
        }
    }
    __syncthreads();
    const uint32_t a = s_meta[0];
    if (s_meta[1] || a < 2) { block_done(status, GROUP_BACK); return; }
    // ---- the symbols side by side (two slots a thread of the first RM_SYMS), then ranked: leaves (count asc, rune asc), header entries (rune asc)
    {
        const uint32_t k0 = tid < RM_SYMS ? s_key[2 * tid] : RM_EMPTY, k1 = tid < RM_SYMS ? s_key[2 * tid + 1] : RM_EMPTY;
        uint32_t at = block_excl_scan<RM_T / 64>((uint32_t)(k0 != RM_EMPTY) + (uint32_t)(k1 != RM_EMPTY), s_wave);
        if (k0 != RM_EMPTY) { s_rune[at] = k0; s_rcnt[at] = s_cnt[2 * tid]; s_rslot[at] = 2 * tid; at++; }
        if (k1 != RM_EMPTY) { s_rune[at] = k1; s_rcnt[at] = s_cnt[2 * tid + 1]; s_rslot[at] = 2 * tid + 1; }
    }
    __syncthreads();
    if (tid < a) {
        uint32_t lr, rr;
        plan_rune_ranks(s_rune, s_rcnt, a, tid, &lr, &rr);
        s_lf[lr] = s_rcnt[tid]; s_lslot[lr] = s_rslot[tid];
        s_ord[rr] = tid;
        if (rr + 1 == a && s_rune[tid] < 0x80) s_meta[2] = 1;             // the last entry is no rune >= 0x80: '\\' could be it (huff_plan_rune.h)
    }
    __syncthreads();
    if (s_meta[2]) { block_done(status, GROUP_BACK); return; }
    // ---- the header's entries, ascending by rune (huffman.go:312-318): thread q writes entry q
    const uint32_t e_sym = tid < a ? s_ord[tid] : 0u;
    const uint32_t e_len = tid < a ? plan_rune_entry_len(s_rcnt[e_sym], s_rune[e_sym]) : 0u;
    const uint32_t e_at = block_excl_scan<RM_T / 64>(e_len, s_wave);
    const uint32_t E = s_wave[RM_T / 64];                              // bytes of the entries: at most HUFF_RUNE_HDR_MAX - 3
    if (e_len && E + 3 <= HUFF_RUNE_HDR_MAX) plan_rune_entry(s_rcnt[e_sym], s_rune[e_sym], reinterpret_cast<uint8_t *>(s_img) + e_at);
    // ---- the tree and the codes: one wavefront (huffman.go:93-127)
    if (wave == 0) {
        const uint32_t au = (uint32_t)__builtin_amdgcn_readfirstlane((int)a);
        LaneStore<4> heap, kids;
        LaneStore<8> code;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t l = lane + 64 * k;
            heap.r[k] = l < au ? plan_item<PLAN_RUNE_IDB>(s_lf[l], l) : 0u;
            kids.r[k] = 0;
        }
#pragma unroll
        for (int k = 0; k < 8; k++) code.r[k] = 0;
        const uint32_t root = plan_tree<PLAN_RUNE_IDB>(au, heap, kids);
        plan_codes<PLAN_RUNE_IDB>(au, root, kids, code);
        // leaf l is lane l % 64 of code.r[l / 64]
        uint32_t mx = 0, bits = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t l = lane + 64 * k;
            if (l < au) { const uint32_t cd = code.r[k], len = cd >> 24; s_code[s_lslot[l]] = cd; mx = max(mx, len); bits += s_lf[l] * len; }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { mx = max(mx, (uint32_t)__shfl_xor((int)mx, d, 64)); bits += (uint32_t)__shfl_xor((int)bits, d, 64); }
        if (lane == 0) { s_plan[0] = mx; s_plan[1] = bits; }
    }
    __syncthreads();
    const uint32_t max_len = s_plan[0], pay_bits = s_plan[1];
    const uint32_t H = E + 3, pad = (8 - pay_bits % 8) % 8;              // huffman.go:245-249
    const uint32_t total = H + (pay_bits + pad) / 8, out_words = (total + 3) / 4;
    if (max_len > 24 || H > HUFF_RUNE_HDR_MAX || out_words > RM_IMG_WORDS || 4 * out_words > huff_rune_mid_enc_out_slot(n)) { block_done(status, GROUP_BACK); return; }
    if (tid == 0) {
        uint8_t *h = reinterpret_cast<uint8_t *>(s_img);
        h[E] = '\\'; h[E + 1] = '\n'; h[E + 2] = (uint8_t)pad;
    }
    // ---- the code bits: 16 bytes a lane, 16 T bytes a round, a code for every rune that STARTS among them; at0 carries over the rounds
    uint32_t at0 = 8 * H + pad;
    for (uint32_t u0 = 0; u0 < units; u0 += RM_T) {
        const uint32_t u = u0 + tid;
        uint32_t e[16], bits = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) e[k] = 0;
        if (u < units) {
            uint32_t rune[16];
            const uint32_t mask = rm_classify(s_in, u, n, rune);
#pragma unroll
            for (int k = 0; k < 16; k++) {
                if ((mask >> k) & 1u) {
                    uint32_t slot = plan_rune_hash(rune[k]);
                    while (s_key[slot] != rune[k]) slot = (slot + 1) & (RM_SLOTS - 1);      // (counted above: it is there)
                    e[k] = s_code[slot];
                    bits += e[k] >> 24;
                }
            }
        }
        const uint32_t pos0 = at0 + block_excl_scan<RM_T / 64>(bits, s_wave);
        at0 += s_wave[RM_T / 64];
        if (bits) pack_codes16(e, pos0, s_img);
    }
    __syncthreads();
    uint4 *hout = reinterpret_cast<uint4 *>(base + m.out_off);
    for (uint32_t i = tid; i < (out_words + 3) / 4; i += RM_T) hout[i] = reinterpret_cast<const uint4 *>(s_img)[i];
    block_done(status, total);
}

struct RuneMidEncClass {
    static constexpr const char *what = "huffman batch compress";
    static size_t in_bytes(size_t n) { return huff_enc_in_slot(n); }
    static size_t out_bytes(size_t n) { return huff_rune_mid_enc_out_slot((uint32_t)n); }
    static int launch(Ctx &c, hipStream_t s, uint32_t g, const SmallMember *tab, uint8_t *base, int64_t) {
        const int rc = func_dyn_lds(c, reinterpret_cast<const void *>(k_huff_mid_rune_enc), RL_BYTES); if (rc) return rc;
        RSN_LAUNCH("huff_batch_rune_mid_enc", k_huff_mid_rune_enc, dim3(g), dim3(RM_T), RL_BYTES, s, tab, base);
        return RSN_OK;
    }
};

// The two offers (codecs.h: BehindClass, pool RUNES; huff_rune_mid_select.h choosing): the members the class runs leave the pool, the
// others STAY in it for the class listed behind this one (huff_rune.hip, which sends what it does not keep to `rest`).
int rune_mid_enc_offer(Ctx &c, std::vector<size_t> &runes, std::vector<size_t> &rest, const uint8_t *const *ins, const size_t *lens, const SmallTake &take, size_t *failed) {
    const std::vector<size_t> idx = rune_mid_class_members(runes, [&](size_t i) { return lens[i]; });
    return idx.empty() ? RSN_OK : class_run<RuneMidEncClass>(c, idx, ins, lens, 0, take, rest, failed, nullptr);
}
int rune_mid_enc_offer_dev(Ctx &c, hipStream_t s, std::vector<size_t> &runes, std::vector<size_t> &, const rsn_dev_member *mem, const DevPlans *,
                           std::vector<size_t> &idx, std::vector<uint32_t> &answers) {
    idx = rune_mid_class_members(runes, [&](size_t i) { return mem[i].n; });
    return idx.empty() ? RSN_OK : class_run_dev<RuneMidEncClass>(c, s, idx, mem, 0, nullptr, answers);
}

}  // namespace

const BehindClass &huff_rune_mid_class() {
    static const BehindClass enc = {BehindClass::RUNES, rune_mid_enc_offer, rune_mid_enc_offer_dev};
    return enc;
}

}  // namespace rsn
