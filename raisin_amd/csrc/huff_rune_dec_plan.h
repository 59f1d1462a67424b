// huff_rune_dec_plan.h -- the grouped rune decoders' plan in front of the tree as a workgroup makes it, for the kernels of both classes
// (huff_rune_dec_body.h: rune_dec_body, k_huff_batch_rune_dec's and k_huff_mid_rune_dec's; k_huff_dev_rune_plan, k_huff_dev_rune_mid_plan).
// The steps are huff_parse_rune.h's -- the separator by a block-wide minimum, parse_rune_scan(...) by ONE lane into the LDS table, the
// counts' verdict and the stream's bounds -- at the limits of the class L (ParseRuneSmall, ParseRuneMid); the device form's plan kernels
// are this and 16 bytes of summary.
#pragma once

#include "huff_small_body.h"
#include "huff_parse_rune.h"

namespace rsn {
namespace {

static_assert(PARSE_RUNE_SCAN_MAX % 16 != 0, "the unit that holds the pad byte of the last separator looked for is one the header's load fetches");

constexpr int RP_T = 256;                                                      // threads of the plan kernels
constexpr uint32_t RD_HDR_UNITS = (PARSE_RUNE_SCAN_MAX + 15) / 16;             // 16-byte units of the header in LDS
constexpr uint32_t RD_TABLE_AT = (RD_HDR_UNITS + 1) * 16;                      // the table behind the header's bytes
constexpr uint32_t RD_PLAN_BYTES = RD_TABLE_AT + 2 * PARSE_RUNE_SLOTS * 4;
static_assert(PARSE_RUNE_SLOTS == 2 * RP_T, "two slots a thread");

// the header's bytes in LDS, a word fetched for every four consecutive bytes asked for
struct LdsBytes {
    const uint32_t *w;
    mutable uint32_t at = PARSE_NONE, cur = 0;
    __device__ __forceinline__ uint32_t get(uint32_t i) const {
        if ((i >> 2) != at) { at = i >> 2; cur = w[at]; }
        return (cur >> (8 * (i & 3))) & 0xFFu;
    }
};

// words of s_w
enum { W_SEP = 0, W_SCAN_OK, W_EXPECT, W_OVER, W_HIGH, W_DISTINCT, W_ROOT, W_MIN, W_MAX, W_WORDS };

// The plan in front of the tree, by a workgroup of T threads: the stream's first bytes into s_hdr under the gather's rule -- the unit that
// reaches beyond src + n is masked, nothing at or behind src + n rounded up to 16 is loaded -- the separator, the entries into the table,
// the counts' verdict and the stream's bounds.  false (the same for every thread): refused.  On return the table holds s_w[W_DISTINCT] runes.
template <int T, class L = ParseRuneSmall>
__device__ __forceinline__ bool rune_light_plan(const uint8_t *src_bytes, unsigned long long n64, uint4 *s_hdr /*[RD_HDR_UNITS + 1]*/, uint32_t *s_key, uint32_t *s_c1,
                                                uint32_t *s_w /*[W_WORDS]*/, HuffDevBounds &b, uint32_t *S, uint32_t *Tl) {
    const uint32_t tid = threadIdx.x;
    if (!parse_rune_length_ok<L>(n64)) return false;
    const uint32_t n = (uint32_t)n64, limit = parse_rune_scan_limit(n);
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(src_bytes);
        for (uint32_t u = tid; u * 16 < limit; u += T) s_hdr[u] = unit_head(src[u], n - 16 * u);      // (u * 16 < limit <= n)
    }
    for (uint32_t i = tid; i < PARSE_RUNE_SLOTS; i += T) { s_key[i] = PARSE_RUNE_EMPTY; s_c1[i] = 0; }
    if (tid < W_WORDS) s_w[tid] = tid == W_SEP ? PARSE_NONE : 0u;
    __syncthreads();
    const uint8_t *hb = reinterpret_cast<const uint8_t *>(s_hdr);
    {   // strings.SplitN(content, "\\\n", 2): the first separator among the bytes looked at -- a position at or behind n is never asked
        uint32_t mine = PARSE_NONE;
        for (uint32_t i = tid; i + 1 < limit; i += T) if (parse_sep_at(hb[i], hb[i + 1])) { mine = i; break; }
        if (mine != PARSE_NONE) atomicMin(&s_w[W_SEP], mine);
    }
    __syncthreads();
    const uint32_t sep = s_w[W_SEP];
    if (sep == PARSE_NONE || sep + 4 > n) return false;
    if (tid == 0) { LdsBytes h; h.w = reinterpret_cast<const uint32_t *>(s_hdr); s_w[W_SCAN_OK] = parse_rune_scan<L>(h, sep, s_key, s_c1, &s_w[W_DISTINCT]) ? 1u : 0u; }
    __syncthreads();
    if (!s_w[W_SCAN_OK]) return false;
    for (uint32_t i = tid; i < PARSE_RUNE_SLOTS; i += T) {
        const uint32_t r = s_key[i], c1 = s_c1[i];
        if (r == PARSE_RUNE_EMPTY) continue;
        if (c1 - 1 > L::COUNT_MAX) s_w[W_OVER] = 1;
        else atomicAdd(&s_w[W_EXPECT], parse_rune_bytes(r, c1));       // (256 symbols of at most COUNT_MAX * 4 bytes: no wrap)
        if (r >= 0x80) s_w[W_HIGH] = 1;
    }
    __syncthreads();
    if (!parse_rune_counts_ok<L>(s_w[W_DISTINCT], s_w[W_HIGH] != 0, s_w[W_OVER] != 0, s_w[W_EXPECT]) || !parse_rune_bounds<L>(n, sep, hb[sep + 2], b, S, Tl)) return false;
    b.expect = s_w[W_EXPECT];
    return true;
}

// ---- the device form's second plan launch: the light scan where the stream lies, a workgroup of RP_T threads a candidate, 16 bytes of
// summary each
template <class L>
__device__ __forceinline__ void rune_plan_body(const PlanEntry *__restrict__ tab, HuffDevSummary *__restrict__ sums) {
    __shared__ uint4 s_hdr[RD_HDR_UNITS + 1];
    __shared__ uint32_t s_key[PARSE_RUNE_SLOTS], s_c1[PARSE_RUNE_SLOTS];
    __shared__ uint32_t s_w[W_WORDS];
    const PlanEntry e = tab[blockIdx.x];
    HuffDevBounds b{};
    uint32_t S = 0, T = 0;
    const bool planned = rune_light_plan<RP_T, L>(e.src, e.n, s_hdr, s_key, s_c1, s_w, b, &S, &T);
    if (threadIdx.x == 0) sums[blockIdx.x] = planned ? HuffDevSummary{PARSE_PLANNED, b.A0, b.end - b.p0, b.expect} : HuffDevSummary{PARSE_NOT_MINE, 0, 0, 0};
}

}  // namespace
}  // namespace rsn
