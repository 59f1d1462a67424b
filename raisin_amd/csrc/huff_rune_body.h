// huff_rune_body.h -- the one workgroup body of the grouped Huffman encoders for members whose bytes are not all below 0x80: UTF-8 text, and
// bytes that are no UTF-8 at all.  k_huff_batch_rune_enc (huff_rune.hip: 256 threads, members of at most 16 KiB, static LDS)
// and k_huff_mid_rune_enc (huff_rune_mid.hip: 1024 threads, members of 16 to 64 KiB, dynamic LDS) are this body at their shapes, as
// k_huff_batch_enc and k_huff_mid_enc are huff_enc_body (huff_small_body.h) -- whose shape this is, with another alphabet:
//   runes    as Go's `range string(b)` yields them (huffman.go:235,309; huff_utf8.h: classify16_words over the member in LDS): a byte
//            that starts no valid sequence is U+FFFD and consumes ONE byte; only the member's n bytes are data -- the block masks what
//            lies behind them in its last unit and keeps a unit of zeros behind that, so a sequence the member's end cuts off is U+FFFD
//            per byte whatever the staging or the caller's buffer holds there;
//   counts   an LDS table of PLAN_RUNE_SLOTS slots, open addressing: atomicCAS on the key, atomicAdd on the count.  A literal EF BF BD and
//            an invalid byte are the same rune, so the same slot;
//   plan     the symbols compacted, ranked (huff_plan_rune.h) and ONE wavefront builds the Go-exact tree and codes of 2 to 256 leaves
//            in its VGPRs (huff_small_body.h: wave_tree);
//   header   the entries ascending by rune at the positions a block scan of their lengths gives, then "\\\n" and the pad byte;
//   bits     every rune START contributes its code: a lane's 16 bytes hold 0 to 16 symbols, a block scan of the lanes' bits gives the
//            positions, pack_codes16 ORs them into the LDS image; 16 T bytes a round, the scan's total carried from a round into the next.
//            The starts and their slots are found again, not stored: a second classification and probe cost less than the LDS a slot
//            index per byte would (at 16 KiB: 32 KiB, 3 workgroups a CU instead of 2).
// Status word: the stream's length, or GROUP_BACK -- more than HUFF_RUNE_SYMS_MAX distinct runes, fewer than two (the single-leaf tree,
// which the single call words), no rune >= 0x80 (the byte encoder's member: the batch flows never send one), or a code beyond 24 bits.
// The last cannot occur at either kernel's member size (each unit says why); the guard stays because the packer relies on it.
#pragma once

#include "huff_small_body.h"
#include "huff_plan_rune.h"
#include "huff_utf8.h"

namespace rsn {
namespace {

// the 16 positions of unit u of the member in LDS (zeros behind its n bytes, a zero unit behind its last)
__device__ __forceinline__ uint32_t rune_classify(const uint4 *s_in, uint32_t u, uint32_t n, uint32_t rune[16]) {
    const uint4 v = s_in[u];
    const uint32_t w[6] = {u ? s_in[u - 1].w : 0u, v.x, v.y, v.z, v.w, s_in[u + 1].x};
    const uint32_t left = n - 16 * u;
    return classify16_words(w, left >= 16 ? 0xFFFFu : (1u << left) - 1u, rune);
}

// The encoder of one workgroup of T threads.  s_in: the member, IN_MAX bytes and a unit more; s_img: the output, IMG_WORDS words in whole
// 16-byte units -- header bytes, then the code bits (MSB first, words byte-swapped); slot(n): bytes of the output slot of a member of n bytes.
template <uint32_t T, uint32_t IN_MAX, uint32_t IMG_WORDS, class Slot>
__device__ __forceinline__ void huff_rune_enc_body(const SmallMember *__restrict__ tab, uint8_t *__restrict__ base, uint4 *s_in /*[IN_MAX / 16 + 1]*/, uint32_t *s_img, Slot slot) {
    constexpr uint32_t SYMS = PLAN_RUNE_SYMS_MAX;     // symbols at most: the first SYMS threads hold them, two table slots each
    constexpr uint32_t SLOTS = PLAN_RUNE_SLOTS;       // of the table: twice the symbols it may hold; plan_rune_hash gives a rune's first
    constexpr uint32_t EMPTY = 0xFFFFFFFFu;           // (no rune)
    static_assert(SLOTS == 2 * SYMS && SYMS <= T && HUFF_RUNE_SYMS_MAX == SYMS && IMG_WORDS % 4 == 0 && IN_MAX % 16 == 0, "two slots a symbol's thread, the image in 16-byte units");
    __shared__ uint32_t s_key[SLOTS], s_cnt[SLOTS], s_code[SLOTS];               // the table: rune, count, and once planned len << 24 | code
    __shared__ uint32_t s_rune[SYMS], s_rcnt[SYMS], s_rslot[SYMS];               // the symbols compacted, in slot order
    __shared__ uint32_t s_lf[SYMS], s_lslot[SYMS];                               // the leaves in (count asc, rune asc) order: count, slot
    __shared__ uint32_t s_ord[SYMS];                                             // the symbols ascending by rune: index into the compacted ones
    __shared__ uint32_t s_wave[T / 64 + 1];
    __shared__ uint32_t s_meta[3];                     // distinct runes; more than the class takes; no rune >= 0x80
    __shared__ uint32_t s_plan[2];                     // max code length, payload bits
    const SmallMember m = tab[blockIdx.x];
    uint32_t *status = reinterpret_cast<uint32_t *>(base + m.status_off);
    const uint32_t n = m.n, tid = threadIdx.x, wave = tid >> 6;
    if (n < 2 || n > IN_MAX) { block_done(status, GROUP_BACK); return; }    // (the host never sends one)
    for (uint32_t i = tid; i < SLOTS; i += T) { s_key[i] = EMPTY; s_cnt[i] = 0; }
    for (uint32_t i = tid; i < IMG_WORDS; i += T) s_img[i] = 0;
    if (tid < 3) s_meta[tid] = 0;
    // ---- the member into LDS: its n bytes, zeros to the end of its last unit and one unit of zeros more
    const uint32_t units = (n + 15) / 16;
    const uint4 *hin = reinterpret_cast<const uint4 *>(base + m.in_off);
    for (uint32_t u = tid; u <= units; u += T) s_in[u] = u < units ? unit_head(hin[u], n - 16 * u) : make_uint4(0, 0, 0, 0);
    __syncthreads();
    // ---- distinct runes and their counts (huffman.go:306-311)
    for (uint32_t u = tid; u < units; u += T) {
        uint32_t rune[16];
        const uint32_t mask = rune_classify(s_in, u, n, rune);
#pragma unroll 1
        for (uint32_t k = 0; k < 16; k++) {
            if (!((mask >> k) & 1u)) continue;
            if (*(volatile uint32_t *)&s_meta[1]) break;                  // the table holds more than the class takes: handed back below
            const uint32_t r = rune[k];
            uint32_t slot = plan_rune_hash(r), p = 0;
            for (; p < SLOTS; p++) {
                const uint32_t old = atomicCAS(&s_key[slot], EMPTY, r);
                if (old == EMPTY && atomicAdd(&s_meta[0], 1u) >= HUFF_RUNE_SYMS_MAX) s_meta[1] = 1;
                if (old == EMPTY || old == r) { atomicAdd(&s_cnt[slot], 1u); break; }
                slot = (slot + 1) & (SLOTS - 1);
            }
            if (p == SLOTS) s_meta[1] = 1;                                // (a full table: more than SLOTS runes were on their way at once)
        }
    }
    __syncthreads();
    const uint32_t a = s_meta[0];
    if (s_meta[1] || a < 2) { block_done(status, GROUP_BACK); return; }
    // ---- the symbols side by side (two slots a thread of the first SYMS), then ranked: leaves (count asc, rune asc), header entries (rune asc)
    {
        const bool mine = T == SYMS || tid < SYMS;
        const uint32_t k0 = mine ? s_key[2 * tid] : EMPTY, k1 = mine ? s_key[2 * tid + 1] : EMPTY;
        uint32_t at = block_excl_scan<T / 64>((uint32_t)(k0 != EMPTY) + (uint32_t)(k1 != EMPTY), s_wave);
        if (k0 != EMPTY) { s_rune[at] = k0; s_rcnt[at] = s_cnt[2 * tid]; s_rslot[at] = 2 * tid; at++; }
        if (k1 != EMPTY) { s_rune[at] = k1; s_rcnt[at] = s_cnt[2 * tid + 1]; s_rslot[at] = 2 * tid + 1; }
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
    const uint32_t e_at = block_excl_scan<T / 64>(e_len, s_wave);
    const uint32_t E = s_wave[T / 64];                                 // bytes of the entries: at most HUFF_RUNE_HDR_MAX - 3
    if (e_len && E + 3 <= HUFF_RUNE_HDR_MAX) plan_rune_entry(s_rcnt[e_sym], s_rune[e_sym], reinterpret_cast<uint8_t *>(s_img) + e_at);
    // ---- the tree and the codes: one wavefront (huffman.go:93-127)
    if (wave == 0) {
        const uint32_t au = (uint32_t)__builtin_amdgcn_readfirstlane((int)a);
        LaneStore<4> kids;
        LaneStore<8> code;
        wave_tree<PLAN_RUNE_IDB>(s_lf, au, kids, code);
        wave_codes_out(code, au, s_lf, s_lslot, s_code, s_plan);
    }
    __syncthreads();
    const uint32_t max_len = s_plan[0], pay_bits = s_plan[1];
    const uint32_t H = E + 3, pad = (8 - pay_bits % 8) % 8;              // huffman.go:245-249
    const uint32_t total = H + (pay_bits + pad) / 8, out_words = (total + 3) / 4;
    if (max_len > 24 || H > HUFF_RUNE_HDR_MAX || out_words > IMG_WORDS || 4 * out_words > slot(n)) { block_done(status, GROUP_BACK); return; }
    if (tid == 0) {
        uint8_t *h = reinterpret_cast<uint8_t *>(s_img);
        h[E] = '\\'; h[E + 1] = '\n'; h[E + 2] = (uint8_t)pad;
    }
    // ---- the code bits: 16 bytes a lane, 16 T bytes a round, a code for every rune that STARTS among them; at0 carries over the rounds
    uint32_t at0 = 8 * H + pad;
    for (uint32_t u0 = 0; u0 < units; u0 += T) {
        const uint32_t u = u0 + tid;
        uint32_t e[16], bits = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) e[k] = 0;
        if (u < units) {
            uint32_t rune[16];
            const uint32_t mask = rune_classify(s_in, u, n, rune);
#pragma unroll
            for (int k = 0; k < 16; k++) {
                if ((mask >> k) & 1u) {
                    uint32_t slot = plan_rune_hash(rune[k]);
                    while (s_key[slot] != rune[k]) slot = (slot + 1) & (SLOTS - 1);         // (counted above: it is there)
                    e[k] = s_code[slot];
                    bits += e[k] >> 24;
                }
            }
        }
        const uint32_t pos0 = at0 + block_excl_scan<T / 64>(bits, s_wave);
        at0 += s_wave[T / 64];
        if (bits) pack_codes16(e, pos0, s_img);
    }
    __syncthreads();
    uint4 *hout = reinterpret_cast<uint4 *>(base + m.out_off);
    for (uint32_t i = tid; i < (out_words + 3) / 4; i += T) hout[i] = reinterpret_cast<const uint4 *>(s_img)[i];
    block_done(status, total);
}

}  // namespace
}  // namespace rsn
