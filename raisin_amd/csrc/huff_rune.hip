// huff_rune.hip -- the grouped Huffman encoder for members whose bytes are not all below 0x80: UTF-8 text, and bytes that are no UTF-8 at
// all (rsn_huffman_compress_batch and its device and layered forms).  The byte encoder k_huff_batch_enc (huff_small.hip) hands
// such a member back as GROUP_BACK_RUNES; when a call holds HUFF_RUNE_GROUP_MIN of them, of at most 16 KiB each, they come here instead
// of taking the single call one by one: ONE launch per group, ONE workgroup of 256 threads per member, nothing on the host between the
// count and the emit -- huff_enc_body's shape (huff_small_body.h) with another alphabet:
//   runes    as Go's `range string(b)` yields them (huffman.go:235,309; huff_utf8.h: classify16_words over the member in LDS): a byte
//            that starts no valid sequence is U+FFFD and consumes ONE byte; only the member's n bytes are data -- the block masks what
//            lies behind them in its last unit and keeps a unit of zeros behind that, so a sequence the member's end cuts off is U+FFFD
//            per byte whatever the staging or the caller's buffer holds there;
//   counts   an LDS table of HR_SLOTS slots, open addressing: atomicCAS on the key, atomicAdd on the count.  A literal EF BF BD and an
//            invalid byte are the same rune, so the same slot;
//   plan     the symbols compacted, ranked (huff_plan_rune.h) and ONE wavefront builds the Go-exact tree and codes of 2 to 256 leaves
//            with the heap (256 slots), the children (255 pairs) and the codes (511) in VGPRs through LaneStore, every index wave-uniform;
//   header   the entries ascending by rune at the positions a block scan of their lengths gives, then "\\\n" and the pad byte;
//   bits     every rune START contributes its code: a lane's 16 bytes hold 0 to 16 symbols, a block scan of the lanes' bits gives the
//            positions, pack_codes16 ORs them into the LDS image.  The starts and their slots are found again, not stored: a second
//            classification and probe cost less than the 32 KiB of LDS a slot index per byte would (3 workgroups a CU instead of 2).
// Status word: the stream's length, or GROUP_BACK -- more than HUFF_RUNE_SYMS_MAX distinct runes, fewer than two (the single-leaf tree,
// which the single call words), no rune >= 0x80 (the byte encoder's member: the batch flows never send one), or a code beyond 24 bits.
// The last cannot occur: the longest code of a tree over counts c is as long as the Fibonacci numbers that fit below sum(c), and those
// that sum to at most 16384 give 20 bits; the guard stays because the packer relies on it.
// LDS: member 16 KiB + 16 B, image 21072 B, table 6 KiB, symbols and ranks 6 KiB: 49.8 KiB, three workgroups to a CU's 160 KiB.
#include "huff_small_body.h"
#include "huff_plan_rune.h"
#include "huff_utf8.h"

namespace rsn {
namespace {

constexpr uint32_t HR_T = 256;
constexpr uint32_t HR_SLOTS = PLAN_RUNE_SLOTS;    // of the table: twice the symbols it may hold; plan_rune_hash gives a rune's first
constexpr uint32_t HR_EMPTY = 0xFFFFFFFFu;        // (no rune)
constexpr uint32_t HR_IMG_WORDS = huff_rune_enc_out_slot(HE_IN_MAX) / 4;
static_assert(HE_IN_MAX == HUFF_RUNE_IN_MAX && HE_IN_MAX <= PLAN_RUNE_COUNT_MAX && HUFF_RUNE_SYMS_MAX == PLAN_RUNE_SYMS_MAX, "one cutoff, one alphabet");
static_assert(HR_T == PLAN_RUNE_SYMS_MAX && HR_SLOTS == 2 * HR_T && HR_IMG_WORDS % 4 == 0, "a thread per symbol, two slots per thread, the image in 16-byte units");
constexpr bool hr_sizes_hold() {
    for (uint32_t n = 2; n <= HE_IN_MAX; n++)
        if (huff_rune_stream_max(n) + 3 > huff_rune_enc_out_slot(n) || huff_rune_stream_max(n) > huff_compress_bound(n)) return false;
    return true;
}
static_assert(hr_sizes_hold(), "the image fits the member's slot, and huff_compress_bound covers the stream");

// the 16 positions of unit u of the member in LDS (zeros behind its n bytes, a zero unit behind its last)
__device__ __forceinline__ uint32_t hr_classify(const uint4 *s_in, uint32_t u, uint32_t n, uint32_t rune[16]) {
    const uint4 v = s_in[u];
    const uint32_t w[6] = {u ? s_in[u - 1].w : 0u, v.x, v.y, v.z, v.w, s_in[u + 1].x};
    const uint32_t left = n - 16 * u;
    return classify16_words(w, left >= 16 ? 0xFFFFu : (1u << left) - 1u, rune);
}

__global__ __launch_bounds__(HR_T) void k_huff_batch_rune_enc(const SmallMember *__restrict__ tab, uint8_t *__restrict__ base) {
    __shared__ uint4 s_in[HE_IN_MAX / 16 + 1];
    __shared__ __attribute__((aligned(16))) uint32_t s_img[HR_IMG_WORDS];
    __shared__ uint32_t s_key[HR_SLOTS], s_cnt[HR_SLOTS], s_code[HR_SLOTS];      // the table: rune, count, and once planned len << 24 | code
    __shared__ uint32_t s_rune[HR_T], s_rcnt[HR_T], s_rslot[HR_T];               // the symbols compacted, in slot order
    __shared__ uint32_t s_lf[HR_T], s_lslot[HR_T];                               // the leaves in (count asc, rune asc) order: count, slot
    __shared__ uint32_t s_ord[HR_T];                                             // the symbols ascending by rune: index into the compacted ones
    __shared__ uint32_t s_wave[HR_T / 64 + 1];
    __shared__ uint32_t s_meta[3];                     // distinct runes; more than the class takes; no rune >= 0x80
    __shared__ uint32_t s_plan[2];                     // max code length, payload bits
    const SmallMember m = tab[blockIdx.x];
    uint32_t *status = reinterpret_cast<uint32_t *>(base + m.status_off);
    const uint32_t n = m.n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (n < 2 || n > HE_IN_MAX) { block_done(status, GROUP_BACK); return; }    // (the host never sends one)
    for (uint32_t i = tid; i < HR_SLOTS; i += HR_T) { s_key[i] = HR_EMPTY; s_cnt[i] = 0; }
    for (uint32_t i = tid; i < HR_IMG_WORDS; i += HR_T) s_img[i] = 0;
    if (tid < 3) s_meta[tid] = 0;
    // ---- the member into LDS: its n bytes, zeros to the end of its last unit and one unit of zeros more
    const uint32_t units = (n + 15) / 16;
    const uint4 *hin = reinterpret_cast<const uint4 *>(base + m.in_off);
    for (uint32_t u = tid; u <= units; u += HR_T) {
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
    for (uint32_t u = tid; u < units; u += HR_T) {
        uint32_t rune[16];
        const uint32_t mask = hr_classify(s_in, u, n, rune);
#pragma unroll 1
        for (uint32_t k = 0; k < 16; k++) {
            if (!((mask >> k) & 1u)) continue;
            if (*(volatile uint32_t *)&s_meta[1]) break;                  // the table holds more than the class takes: handed back below
            const uint32_t r = rune[k];
            uint32_t slot = plan_rune_hash(r), p = 0;
            for (; p < HR_SLOTS; p++) {
                const uint32_t old = atomicCAS(&s_key[slot], HR_EMPTY, r);
                if (old == HR_EMPTY && atomicAdd(&s_meta[0], 1u) >= HUFF_RUNE_SYMS_MAX) s_meta[1] = 1;
                if (old == HR_EMPTY || old == r) { atomicAdd(&s_cnt[slot], 1u); break; }
                slot = (slot + 1) & (HR_SLOTS - 1);
            }
            if (p == HR_SLOTS) s_meta[1] = 1;                             // (a full table: more than HR_SLOTS runes were on their way at once)
        }
    }
    __syncthreads();
    const uint32_t a = s_meta[0];
    if (s_meta[1] || a < 2) { block_done(status, GROUP_BACK); return; }
    // ---- the symbols side by side (two slots a thread), then ranked: leaves (count asc, rune asc), header entries (rune asc)
    {
        const uint32_t k0 = s_key[2 * tid], k1 = s_key[2 * tid + 1];
        uint32_t at = block_excl_scan<HR_T / 64>((uint32_t)(k0 != HR_EMPTY) + (uint32_t)(k1 != HR_EMPTY), s_wave);
        if (k0 != HR_EMPTY) { s_rune[at] = k0; s_rcnt[at] = s_cnt[2 * tid]; s_rslot[at] = 2 * tid; at++; }
        if (k1 != HR_EMPTY) { s_rune[at] = k1; s_rcnt[at] = s_cnt[2 * tid + 1]; s_rslot[at] = 2 * tid + 1; }
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
    const uint32_t e_at = block_excl_scan<HR_T / 64>(e_len, s_wave);
    const uint32_t E = s_wave[HR_T / 64];                              // bytes of the entries: at most HUFF_RUNE_HDR_MAX - 3
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
    if (max_len > 24 || H > HUFF_RUNE_HDR_MAX || out_words > HR_IMG_WORDS || 4 * out_words > huff_rune_enc_out_slot(n)) { block_done(status, GROUP_BACK); return; }
    if (tid == 0) {
        uint8_t *h = reinterpret_cast<uint8_t *>(s_img);
        h[E] = '\\'; h[E + 1] = '\n'; h[E + 2] = (uint8_t)pad;
    }
    // ---- the code bits: 16 bytes a lane, 16 T bytes a round, a code for every rune that STARTS among them
    uint32_t at0 = 8 * H + pad;
    for (uint32_t u0 = 0; u0 < units; u0 += HR_T) {
        const uint32_t u = u0 + tid;
        uint32_t e[16], bits = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) e[k] = 0;
        if (u < units) {
            uint32_t rune[16];
            const uint32_t mask = hr_classify(s_in, u, n, rune);
#pragma unroll
            for (int k = 0; k < 16; k++) {
                if ((mask >> k) & 1u) {
                    uint32_t slot = plan_rune_hash(rune[k]);
                    while (s_key[slot] != rune[k]) slot = (slot + 1) & (HR_SLOTS - 1);      // (counted above: it is there)
                    e[k] = s_code[slot];
                    bits += e[k] >> 24;
                }
            }
        }
        const uint32_t pos0 = at0 + block_excl_scan<HR_T / 64>(bits, s_wave);
        at0 += s_wave[HR_T / 64];
        if (bits) pack_codes16(e, pos0, s_img);
    }
    __syncthreads();
    uint4 *hout = reinterpret_cast<uint4 *>(base + m.out_off);
    for (uint32_t i = tid; i < (out_words + 3) / 4; i += HR_T) hout[i] = reinterpret_cast<const uint4 *>(s_img)[i];
    block_done(status, total);
}

struct RuneEncClass {
    static constexpr const char *what = "huffman batch compress";
    static size_t in_bytes(size_t n) { return huff_enc_in_slot(n); }
    static size_t out_bytes(size_t n) { return huff_rune_enc_out_slot((uint32_t)n); }
    static int launch(Ctx &c, hipStream_t s, uint32_t g, const SmallMember *tab, uint8_t *base, int64_t) {
        RSN_LAUNCH("huff_batch_rune_enc", k_huff_batch_rune_enc, dim3(g), dim3(HR_T), 0, s, tab, base);
        return RSN_OK;
    }
};

int rune_enc_offer(Ctx &c, std::vector<size_t> &runes, std::vector<size_t> &rest, const uint8_t *const *ins, const size_t *lens, const SmallTake &take, size_t *failed) {
    runes.resize(rune_class_members(runes, rest, [&](size_t i) { return lens[i]; }));
    const int rc = runes.empty() ? RSN_OK : class_run<RuneEncClass>(c, runes, ins, lens, 0, take, rest, failed, nullptr);
    runes.clear();
    return rc;
}
int rune_enc_offer_dev(Ctx &c, hipStream_t s, std::vector<size_t> &runes, std::vector<size_t> &rest, const rsn_dev_member *mem, const DevPlans *,
                       std::vector<size_t> &idx, std::vector<uint32_t> &answers) {
    runes.resize(rune_class_members(runes, rest, [&](size_t i) { return mem[i].n; }));
    idx.swap(runes);                                                      // (idx comes empty: the pool is left so)
    return idx.empty() ? RSN_OK : class_run_dev<RuneEncClass>(c, s, idx, mem, 0, nullptr, answers);
}

}  // namespace

const BehindClass &huff_rune_class() {
    static const BehindClass enc = {BehindClass::RUNES, rune_enc_offer, rune_enc_offer_dev};
    return enc;
}

}  // namespace rsn
