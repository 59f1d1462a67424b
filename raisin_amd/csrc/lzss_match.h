// lzss_match.h -- the two match searches that look at EVERY position of a strip (lzss_match.hip), as the encoder's driver
// (lzss_encode.hip) launches them: the packed sweep k_match2 (any window) and the bigram-bucket search k_match_hash (windows up to
// HWMAX).  The chain walk (lzss_encode.hip) evaluates only the positions a greedy chain lands on and hands strips back to these.
#pragma once

#include "rsn_common.h"

namespace rsn {

constexpr int MATCH_STRIP = 16384;      // positions per match block
constexpr uint32_t KEY_UNKNOWN = 0xFFFFFFFFu;                     // chain mode: no key evaluated for this position (the parse redoes the strip if the true chain lands here)

struct MatchArgs {
    const uint8_t *fc; uint32_t E; uint32_t W; uint32_t DW;   // DW = diagonals per wave
    uint32_t *keys;
    const uint32_t *only;                                      // non-null: sweep only the strips flagged here (k_match_hash's hand-backs), a flag per MATCH_STRIP positions
    uint32_t strip;                                            // positions per block: MATCH_STRIP, or a smaller multiple of 64 that divides it
};
constexpr int MW2_WIDE = 16;            // ... and where only a handful of strips are swept: a strip's latency is what the call waits for
constexpr int MW2 = 4;                  // wavefronts per block of the packed sweep: fewer, longer diagonal ranges (less pipeline fill)

constexpr int HT = 4096;                 // positions per block
constexpr int HTH = 512;                 // threads per block
constexpr int HSH = 9;                   // log2(HTH): entries of a bucket are ordered by staged offset >> HSH
constexpr int HWMAX = 4096;              // largest window this path takes
constexpr int HLMAX = 256;               // longest common prefix examined before the strip is handed back
constexpr int HNB = 8192;                // buckets
constexpr int H_STAGE = HWMAX + HT + HLMAX + 32;
constexpr uint32_t H_ITER_CAP = (HT / HTH) * 384;   // trips per lane before the strip is handed back (the sweep costs about as much as 250 trips per position)
static_assert(HWMAX + HT <= 8192, "an entry keeps the staged offset in 13 bits");
static_assert(MATCH_STRIP % HT == 0, "a strip is a whole number of hash tiles");
static_assert((1 << HSH) == HTH && (HWMAX + HT) % HTH == 0 && (HNB / 2) % HTH == 0, "round structure");

struct HashArgs { const uint8_t *fc; uint32_t E; uint32_t W; uint32_t *keys; uint32_t *heavy; const uint32_t *only; };

#ifdef __HIPCC__
// eight staged bytes from any byte offset: three aligned dwords and two v_alignbyte.  (gfx950's LDS takes unaligned accesses, and
// the compiler emits ONE ds_read_b64 for an align-1 load -- but an unaligned wave-instruction is replayed: the chain walk went from
// 37 to 70 ms with it, k_match_hash from 20 to 27.)
__device__ __forceinline__ unsigned long long lds_load8(const uint32_t *sw, uint32_t rel) {
    const uint32_t q = rel >> 2;
    const uint32_t w0 = sw[q], w1 = sw[q + 1], w2 = sw[q + 2];
    return (unsigned long long)__builtin_amdgcn_alignbyte(w1, w0, rel) | ((unsigned long long)__builtin_amdgcn_alignbyte(w2, w1, rel) << 32);   // v_alignbyte uses rel[1:0]
}

// ---- the hash-chain search of the grouped batch encoders (lzss_mid.hip: a member a workgroup; lzss_tile.hip: a tile a workgroup).  The
// positions of a sub-tile of SUB threads join the chains of their two-byte keys (head[hash] <- i, ring[i & (RING - 1)] <- the head it
// replaced), so between sub-tiles a chain is in descending order and inside one in any order.
constexpr uint32_t CHAIN_NONE = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t chain_hash(uint32_t b0, uint32_t b1) { return ((b0 | (b1 << 8)) * 0x9E3779B1u) >> 20; }
__device__ __forceinline__ uint32_t chain_digits(uint32_t v) { return v < 10 ? 1u : v < 100 ? 2u : v < 1000 ? 3u : v < 10000 ? 4u : 5u; }
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
// exclusive scan of one value per thread over a workgroup of T threads; *total: the sum
template <int T>
__device__ __forceinline__ uint32_t chain_scan(uint32_t v, uint32_t *s_wave /*[T / 64 + 1]*/, uint32_t *total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d, 64); if (lane >= (uint32_t)d) inc += o; }
    __syncthreads();                                                      // (the previous scan's readers are done with s_wave)
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    if (threadIdx.x < 64) {
        uint32_t w = threadIdx.x < T / 64 ? s_wave[threadIdx.x] : 0u, wi = w;
#pragma unroll
        for (int d = 1; d < T / 64; d <<= 1) { const uint32_t o = __shfl_up(wi, d, 64); if (lane >= (uint32_t)d) wi += o; }
        if (threadIdx.x < T / 64) s_wave[threadIdx.x] = wi - w;
        if (threadIdx.x == T / 64 - 1) s_wave[T / 64] = wi;
    }
    __syncthreads();
    *total = s_wave[T / 64];
    return s_wave[wave] + inc - v;
}
#endif

// the launches (lzss_match.hip); shmem2: k_match2's dynamic LDS for this window
int lzss_launch_match2(Ctx &c, hipStream_t s, const MatchArgs &m2, uint32_t n_blocks, size_t shmem2, bool wide = false);   // wide: MW2_WIDE wavefronts a block (m2.DW and shmem2 worked out for it)
int lzss_launch_match_hash(Ctx &c, hipStream_t s, const HashArgs &h);

}  // namespace rsn
