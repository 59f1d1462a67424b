// lzss_dec_body.h -- what the LZSS batch decoders share (lzss_small.hip, the parse only, and lzss_mid.hip: a member a workgroup;
// lzss_tile_dec.hip: a tile a workgroup), as __device__ functions: a token's parse (lzss.go:331-352), the items of a chunk of the stream two bytes a thread, the
// pointer jumping that settles the copy chains inside a tile of output, and DecodeOpeningSymbols (lzss.go:391-406) by the parity of the 5C
// run in front of a byte.  The counterpart of lzss_enc_body.h.
#pragma once

#include "block_dev.h"

namespace rsn {

#ifdef __HIPCC__
// The token whose '<' is the stream's byte p (s[q - org] is byte q, n the stream's length): "<" digits "," digits ">", at most 10 digits a
// number, values at most vmax, len <= ptr (lzss.go:350's slice stays inside the data).  true: ptr, len and ttl, the bytes of its text.
// false: malformed (ptr may be set; len and ttl are 0).
__device__ __forceinline__ bool lzd_token(const uint8_t *s, uint32_t org, uint32_t p, uint32_t n, uint32_t vmax, uint32_t &ptr, uint32_t &len, uint32_t &ttl) {
    uint32_t q = p + 1; unsigned long long v = 0; int nd = 0;
    while (q < n && nd < 10 && s[q - org] >= '0' && s[q - org] <= '9') { v = v * 10 + (s[q - org] - '0'); q++; nd++; }
    bool ok = nd && q < n && s[q - org] == ',' && v <= (unsigned long long)vmax;
    ptr = (uint32_t)v; q++; v = 0; nd = 0;
    while (ok && q < n && nd < 10 && s[q - org] >= '0' && s[q - org] <= '9') { v = v * 10 + (s[q - org] - '0'); q++; nd++; }
    ok = ok && nd && q < n && s[q - org] == '>' && v <= (unsigned long long)vmax && (uint32_t)v <= ptr;
    len = ok ? (uint32_t)v : 0u; ttl = ok ? q + 1 - p : 0u;
    return ok;
}

// The items of the chunk of the stream that begins at byte c0, two bytes of it a thread (2 * threadIdx.x and the next): every '<' parses
// its token and covers its text in s_cov (s_cov[q - c0] for byte q; zeroed by the caller but for what a token begun in front of c0
// covers).  ttl != 0: a token (its text's length), with tptr and tlen; outl: the bytes the item gives -- a token's tlen, 1 for a literal, 0
// for a byte of a token's text (an escaped stream holds no '<' of its own: once every token has parsed none lies in another's text).
// bad: a '<' of this thread's is no token.  s_in, org, n, vmax: lzd_token's.  outl is computed behind a barrier.
struct TileItems { uint32_t tptr[2], tlen[2], ttl[2], outl[2]; bool bad; };
__device__ __forceinline__ void lzd_items(const uint8_t *s_in, uint32_t org, uint32_t c0, uint32_t n, uint32_t vmax, uint8_t *s_cov, TileItems &it) {
    const uint32_t k0 = c0 + 2 * threadIdx.x;
    it.bad = false;
    for (int k = 0; k < 2; k++) {
        const uint32_t p = k0 + k;
        it.tptr[k] = 0; it.tlen[k] = 0; it.ttl[k] = 0;
        if (p >= n || s_in[p - org] != '<') continue;
        uint32_t ptr, len, text;                                                  // (scalars, not the arrays' elements: fewer VGPRs in k_lzss_mid_dec)
        const bool ok = lzd_token(s_in, org, p, n, vmax, ptr, len, text);
        it.tptr[k] = ptr;
        if (!ok) { it.bad = true; continue; }
        it.tlen[k] = len; it.ttl[k] = text;
        for (uint32_t t = 0; t < text; t++) s_cov[p - c0 + t] = 1;
    }
    __syncthreads();
    for (int k = 0; k < 2; k++) { const uint32_t p = k0 + k; it.outl[k] = p < n ? (it.ttl[k] ? it.tlen[k] : (s_cov[p - c0] ? 0u : 1u)) : 0u; }
}

// Every byte's source inside a tile of `cnt` output bytes that begins at s0: src <- src[src] while it lies in the tile and is not a literal
// (a literal is its own source; a copied byte lies before the byte that copies it).  s_src: uint32[2][TILE], the sources in [0]; returns
// which of the two holds them in the end.  `rounds` doublings at most, fewer when nothing moves.
template <int T, uint32_t TILE>
__device__ __forceinline__ int lzd_jump(uint32_t *s_src, uint32_t s0, uint32_t cnt, int rounds) {
    int cur = 0;
    for (int round = 0; round < rounds; round++) {
        bool moved = false;
        const uint32_t *sa = s_src + cur * TILE;
        uint32_t *sb = s_src + (cur ^ 1) * TILE;
        for (uint32_t r = threadIdx.x; r < cnt; r += T) {
            const uint32_t x = sa[r], y = x >= s0 ? sa[x - s0] : x;
            sb[r] = y; moved = moved || x != y;
        }
        cur ^= 1;
        if (!__syncthreads_or(moved)) break;
    }
    return cur;
}

// ---- DecodeOpeningSymbols: a byte is escaped iff the run of 5C right in front of it has odd length, counted from the last byte that is
// not 5C.  A thread holds the positions [q0, q1) of the escaped bytes (s_val[q - org] is byte q).
// 1 + the last of the thread's positions whose byte is not 5C; 0: none
__device__ __forceinline__ uint32_t lzd_last_plain(const uint8_t *s_val, uint32_t org, uint32_t q0, uint32_t q1) {
    uint32_t mine = 0;
    for (uint32_t q = q0; q < q1; q++) if (s_val[q - org] != 0x5C) mine = q + 1;
    return mine;
}
// the same for every position in front of the thread's (the threads hold consecutive runs in thread order)
template <int T>
__device__ __forceinline__ uint32_t lzd_plain_before(uint32_t mine, uint32_t *s_wave /*[T / 64]*/) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = mine, before = 0;
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d, 64); if (lane >= (uint32_t)d) inc = max(inc, o); }
    __syncthreads();
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    for (uint32_t w = 0; w < wave; w++) before = max(before, s_wave[w]);
    uint32_t prev = __shfl_up(inc, 1, 64);
    if (lane == 0) prev = 0;
    return max(before, prev);
}
// how many bytes the thread's positions give
__device__ __forceinline__ uint32_t lzd_unesc_count(const uint8_t *s_val, uint32_t org, uint32_t q0, uint32_t q1, uint32_t before) {
    uint32_t cnt = 0;
    for (uint32_t q = q0, bq = before; q < q1; q++) {
        const uint32_t b = s_val[q - org];
        cnt += (((q - bq) & 1u) || b != 0x5C) ? 1u : 0u;
        if (b != 0x5C) bq = q + 1;
    }
    return cnt;
}
// ... and the bytes, from s_res[o] on: an escaped byte as it is, FF -> 3C, every other byte as it is
__device__ __forceinline__ void lzd_unesc_write(const uint8_t *s_val, uint32_t org, uint32_t q0, uint32_t q1, uint32_t before, uint8_t *s_res, uint32_t o) {
    for (uint32_t q = q0, bq = before; q < q1; q++) {
        const uint32_t b = s_val[q - org];
        const bool esc = (q - bq) & 1u;
        if (esc || b != 0x5C) s_res[o++] = (uint8_t)(esc ? b : (b == 0xFF ? 0x3Cu : b));
        if (b != 0x5C) bq = q + 1;
    }
}
#endif

}  // namespace rsn
