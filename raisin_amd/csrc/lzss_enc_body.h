// lzss_enc_body.h -- what the LZSS batch encoders share (lzss_small.hip: a member a workgroup, brute force; lzss_mid.hip: a member a
// workgroup, hash chains; lzss_tile.hip: a tile a workgroup), the counterpart of lzss_dec_body.h: a key's item (lzss.go:143) as plain
// constexpr arithmetic, and as __device__ functions EncodeOpeningSymbols' rule for a byte (lzss.go:369-389), the hash-chain search, the
// greedy chain of a stretch of positions by pointer doubling (lzss.go:134-151) and the write of an item (lzss.go:318-320).  Every kernel
// keeps its own loops, LDS and launch bounds.
#pragma once

#include <cstdint>
#ifdef __HIPCC__                    // (a host program that includes this for the item arithmetic needs no HIP header)
#include "block_dev.h"
#include "lzss_match.h"             // lds_load8
#endif

namespace rsn {

// ---- the item of a key L << 16 | d: a match of L bytes at distance d (L = 0: a literal) is the token "<d,L>" of el bytes iff that is
// shorter than what it stands for (el < L), else its own bytes; sz: the bytes it puts out
constexpr uint32_t chain_digits(uint32_t v) { return v < 10 ? 1u : v < 100 ? 2u : v < 1000 ? 3u : v < 10000 ? 4u : 5u; }
struct LzssItem { uint32_t L, d, el, sz; };
constexpr LzssItem lzss_item(uint32_t L, uint32_t d) {
    const uint32_t el = L ? 3 + chain_digits(d) + chain_digits(L) : 0u;
    return LzssItem{L, d, el, L == 0 ? 1u : (el < L ? el : L)};
}

#ifdef __HIPCC__
// ---- EncodeOpeningSymbols: 3C -> FF; FF -> 5C FF; 5C -> 5C 5C.  How many bytes the byte b escapes to, and the write of them at fc[at]:
// returns the offset behind them.
__device__ __forceinline__ uint32_t lzss_esc_len(uint32_t b) { return (b == 0x5C || b == 0xFF) ? 2u : 1u; }
__device__ __forceinline__ uint32_t lzss_esc_put(uint8_t *fc, uint32_t at, uint32_t b) {
    if (b == 0x5C || b == 0xFF) { fc[at++] = 0x5C; fc[at++] = (uint8_t)b; } else fc[at++] = b == 0x3C ? (uint8_t)0xFF : (uint8_t)b;
    return at;
}

// ---- the hash-chain search of the grouped encoders (lzss_mid.hip, lzss_tile.hip).  The positions of a sub-tile of SUB threads join the
// chains of their two-byte keys (head[hash] <- i, ring[i & (RING - 1)] <- the head it replaced), so between sub-tiles a chain is in
// descending order and inside one in any order.
constexpr uint32_t CHAIN_NONE = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t chain_hash(uint32_t b0, uint32_t b1) { return ((b0 | (b1 << 8)) * 0x9E3779B1u) >> 20; }
// Position i of an escaped stream of E bytes walks the chain that begins at j: the longest L >= 2 with fc[i, i + L) inside the window
// (L <= distance <= W, L <= E - i), at its largest distance (lzss.go:166-184,418-421), as L << 16 | distance; 0: none.  s_fc[p - fc0] is
// the stream's byte p (fc0 a multiple of 4, at or below every position the walk reads: i - W rounded down to a sub-tile), with eleven
// readable bytes behind the last one a match may reach.  The walk is bounded by the ring, the eight-byte extensions are counted into
// `steps` and the walk ends once they exceed STEP_CAP: the caller hands the member back then.
template <uint32_t RING, uint32_t SUB, uint32_t STEP_CAP>
__device__ __forceinline__ uint32_t chain_best(const uint8_t *s_fc, const uint32_t *s_ring, uint32_t j, uint32_t i, uint32_t E, uint32_t W, uint32_t fc0, uint32_t &steps) {
    const uint32_t *fw = reinterpret_cast<const uint32_t *>(s_fc);
    const uint32_t cap = E - i;
    uint32_t best = 0;
    if (cap >= 2 && i >= 2) {
        const uint32_t jlo = i - min(i, W), floor_ = jlo & ~(uint32_t)(SUB - 1);   // (a chain entry below floor_: everything behind it is older still)
        const unsigned long long pat = lds_load8(fw, i - fc0);
        for (uint32_t visits = 0; j < E && j >= floor_ && visits < RING && steps <= STEP_CAP; visits++) {
            const uint32_t nxt = s_ring[j & (RING - 1)];
            if (j + 2 <= i && j >= jlo) {
                const uint32_t d = i - j, lim = min(d, cap), bl = best >> 16;
                // (a candidate counts if it is at least as long as the best so far: the byte at that length decides for most)
                if (lim >= bl && (bl == 0 || s_fc[j + bl - 1 - fc0] == s_fc[i + bl - 1 - fc0])) {
                    unsigned long long x = lds_load8(fw, j - fc0) ^ pat;
                    uint32_t L = x ? (uint32_t)__builtin_ctzll(x) >> 3 : 8u;
                    if (!x) {
                        uint32_t off = 8;
                        while (off < lim) {
                            x = lds_load8(fw, j + off - fc0) ^ lds_load8(fw, i + off - fc0);
                            steps++;
                            if (x) { off += (uint32_t)__builtin_ctzll(x) >> 3; break; }
                            off += 8;
                        }
                        L = off;
                    }
                    best = max(best, (min(L, lim) << 16) | d);        // longest, then farthest back (bytes.Index finds the leftmost, lzss.go:419)
                }
            }
            j = nxt;
        }
    }
    return best;
}

// ---- the greedy chain r -> r + max(1, L) (lzss.go:139-142) of a stretch of N positions, entered at `entry`, by pointer doubling: s_on[r]
// = 1 for every position the chain lands on, N standing for everything beyond the stretch.  The first R positions are real, s_key[r] their
// keys.  s_jmp: uint16[2][STRIDE], STRIDE > N; s_on: uint8[N + 1].  The whole workgroup of T threads calls it, behind the barrier that
// ends the keys' writes; it ends behind one.  (lzss_small.hip calls it; k_lzss_mid_enc and k_lzss_tile_chain keep the same loop over a
// tile of constant size as their own, which measured faster: LEDGER.)
template <int T, uint32_t STRIDE>
__device__ __forceinline__ void lzss_greedy_chain(const uint32_t *s_key, uint16_t *s_jmp, uint8_t *s_on, uint32_t N, uint32_t R, uint32_t entry) {
    for (uint32_t r = threadIdx.x; r <= N; r += T) {
        s_jmp[r] = (uint16_t)(r < R ? min(N, r + max(1u, s_key[r] >> 16)) : N);
        s_on[r] = r == entry;
    }
    __syncthreads();
    int cur = 0;
    for (uint32_t reach = 1; reach < N + 1; reach <<= 1) {                        // after the round: everything within 2 * reach - 1 steps of the entry
        const uint16_t *ja = s_jmp + cur * STRIDE;
        uint16_t *jb = s_jmp + (cur ^ 1) * STRIDE;
        for (uint32_t r = threadIdx.x; r < N; r += T) if (s_on[r]) s_on[ja[r]] = 1;
        for (uint32_t r = threadIdx.x; r <= N; r += T) jb[r] = ja[ja[r]];
        cur ^= 1;
        __syncthreads();
    }
}

// ---- the item at s_out[at]: "<" + itoa(d) + "," + itoa(L) + ">" (lzss.go:318-320), written backwards, or the sz bytes it stands for from
// the escaped stream (src: the item's position in it)
__device__ __forceinline__ void lzss_item_put(uint8_t *s_out, uint32_t at, const LzssItem &it, const uint8_t *src) {
    if (it.el < it.L) {
        uint32_t p = at + it.el;
        s_out[--p] = '>';
        for (uint32_t v = it.L; ; v /= 10) { s_out[--p] = (uint8_t)('0' + v % 10); if (v < 10) break; }
        s_out[--p] = ',';
        for (uint32_t v = it.d; ; v /= 10) { s_out[--p] = (uint8_t)('0' + v % 10); if (v < 10) break; }
        s_out[--p] = '<';
    } else for (uint32_t q = 0; q < it.sz; q++) s_out[at + q] = src[q];
}
#endif

}  // namespace rsn
