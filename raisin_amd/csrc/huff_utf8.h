// huff_utf8.h -- Go's UTF-8 decoding (`range string(b)`, huffman.go:235,309) on the device, for the units that count and code runes:
// huff_encode.hip (the flat rune path, on global memory) and huff_rune_body.h (the grouped rune encoders' body, on a member held in LDS).
#pragma once

#include "huff_host.h"

namespace rsn {

// Length of the valid sequence starting with b0 (1 ASCII, 2..4), 0 if invalid
// (=> U+FFFD consuming one byte).  Accept ranges: go1.15 unicode/utf8.
__device__ __forceinline__ int seq_len(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3) {
    if (b0 < 0x80) return 1;
    if (b0 < 0xC2 || b0 > 0xF4) return 0;
    uint32_t lo = 0x80, hi = 0xBF;
    if (b0 == 0xE0) lo = 0xA0;
    else if (b0 == 0xED) hi = 0x9F;
    else if (b0 == 0xF0) lo = 0x90;
    else if (b0 == 0xF4) hi = 0x8F;
    if (b1 < lo || b1 > hi) return 0;
    if (b0 < 0xE0) return 2;
    if ((b2 & 0xC0) != 0x80) return 0;
    if (b0 < 0xF0) return 3;
    if ((b3 & 0xC0) != 0x80) return 0;
    return 4;
}

__device__ __forceinline__ uint32_t load_word_clamped(const uint8_t *in, size_t n, long long off) {
    // 4 bytes at `off` (multiple of 4); bytes outside [0,n) read as 0
    if (off < 0 || (size_t)off >= n) return 0;
    if ((size_t)off + 4 <= n) return *reinterpret_cast<const uint32_t *>(in + off);
    uint32_t w = 0;
    for (int k = 0; k < 4 && (size_t)off + k < n; k++) w |= (uint32_t)in[off + k] << (8 * k);
    return w;
}

// Classifies the 16 positions [P, P+16) from the six words w that hold the bytes [P - 4, P + 20), bytes outside the input zero; `valid`:
// a bit for every position below the input's end.  A position is a rune start unless a
// VALID multi-byte sequence begins 1..3 bytes before it (lead bytes are never
// continuation bytes, so every valid sequence start is itself a rune start:
// the decision is local, DESIGN.md "rune classification").  Returns the start
// mask; rune[k] is meaningful where bit k is set.
__device__ __forceinline__ uint32_t classify16_words(const uint32_t w[6], uint32_t valid, uint32_t rune[16]) {
    if (((w[0] | w[1] | w[2] | w[3] | w[4] | w[5]) & 0x80808080u) == 0) {
#pragma unroll
        for (int k = 0; k < 16; k++) rune[k] = (w[1 + (k >> 2)] >> (8 * (k & 3))) & 0xFF;
        return valid;
    }
    auto B = [&](int i) -> uint32_t { return (w[(i + 4) >> 2] >> (8 * ((i + 4) & 3))) & 0xFF; };   // i in [-4, 19]
    int v[19];
#pragma unroll
    for (int q = -3; q < 16; q++) v[q + 3] = seq_len(B(q), B(q + 1), B(q + 2), B(q + 3));
    uint32_t mask = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const bool consumed = v[k + 2] > 1 || v[k + 1] > 2 || v[k] > 3;
        if (!consumed) mask |= 1u << k;
        const int L = v[k + 3];
        const uint32_t b0 = B(k), b1 = B(k + 1), b2 = B(k + 2), b3 = B(k + 3);
        uint32_t r = b0;
        if (L == 0) r = kRuneError;
        else if (L == 2) r = ((b0 & 0x1F) << 6) | (b1 & 0x3F);
        else if (L == 3) r = ((b0 & 0x0F) << 12) | ((b1 & 0x3F) << 6) | (b2 & 0x3F);
        else if (L == 4) r = ((b0 & 0x07) << 18) | ((b1 & 0x3F) << 12) | ((b2 & 0x3F) << 6) | (b3 & 0x3F);
        rune[k] = r;
    }
    return mask & valid;
}

// the same on the input where it lies: in[0, n) in global memory
__device__ __forceinline__ uint32_t classify16(const uint8_t *__restrict__ in, size_t n, size_t P, uint32_t rune[16]) {
    uint32_t w[6];
#pragma unroll
    for (int j = 0; j < 6; j++) w[j] = load_word_clamped(in, n, (long long)P - 4 + 4 * j);
    const uint32_t valid = (P + 16 <= n) ? 0xFFFFu : (P < n ? ((1u << (n - P)) - 1u) : 0u);
    return classify16_words(w, valid, rune);
}

}  // namespace rsn
