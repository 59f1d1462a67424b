// lzss_small.hip -- the LZSS codec for a host buffer of at most 1 KiB to compress, 2 KiB to decompress (r06).
//
// The reference's own benchmark table is files of 13 to 25 bytes (README.md:153-167), and what BenchmarkFile times on them is one
// Compress and one Decompress (engine.go:379-406).  At that size the general path is all fixed cost: the check and its round trip, a
// chain walk that takes 0.17 ms however few the positions, a dozen launches, three host round trips -- 0.23 ms for 3.4 KB (r05).
// Here a call is ONE launch of ONE block that reads the caller's bytes from pinned host memory, does the whole codec in LDS and stores its
// result into pinned host memory; the host polls a word instead of waiting for the stream (as huff_small.hip).
//
//   compress    EncodeOpeningSymbols (lzss.go:369-389) by a block-wide scan; for EVERY escaped position the longest match that lies
//               entirely inside the window and its leftmost occurrence (lzss.go:166-184,418-421) by looking at every distance -- at
//               most 2048 x 2048 / 2 byte compares, a thread per position; the greedy chain from 0 (lzss.go:134-151) by pointer doubling
//               over next(i) = i + max(1, L); item sizes, a scan, the bytes (lzss.go:143,318-320).
//   decompress  every '<' parses its token (lzss.go:323-364); literal / token bytes get their output offsets from a scan; every output
//               byte its source (itself, or the byte `pointer` before it), resolved by pointer doubling; DecodeOpeningSymbols
//               (lzss.go:391-406) from the parity of the 5C run in front of every byte, a scan, the bytes.
// Many members at once (rsn_lzss_compress_batch / rsn_lzss_decompress_batch): k_lzss_batch_enc / _dec, the same bodies, a block per member
// of a group packed into pinned memory.
// What the path does not take returns 1 and goes through the general path, which also words the errors: inputs above the sizes below,
// streams whose tokens are malformed or point outside the data, outputs above 8 KiB.
#include "group_run.h"
#include "lzss_dec_body.h"
#include "lzss_enc_body.h"

namespace rsn {
namespace {

constexpr uint32_t SL_IN_MAX = 1024;            // bytes of input the encoder takes (measured: 0.04 / 0.06 / 0.10 ms for 256 / 512 / 1024 bytes of text, 0.25 for 2048 -- where the general path is as fast)
constexpr uint32_t SL_E_MAX = 2048;             // escaped positions (every byte of the input a 5C or an FF: twice its length)
constexpr uint32_t SL_DEC_IN_MAX = 2048;        // bytes of a compressed stream the decoder takes
constexpr uint32_t SL_DEC_E_MAX = 8192;         // bytes of the escaped stream it expands to, at most
constexpr int SLT = 1024;                       // threads of the one block

// pinned staging of one call: offsets into Ctx::pinned
constexpr size_t SP_IN = 0, SP_OUT = 4096, SP_FLAG = SP_OUT + SL_DEC_E_MAX + 64, SP_BYTES = SP_FLAG + 64;

// 0xFF in every byte of w that equals the byte c (exact per byte)
__device__ __forceinline__ uint32_t sl_bytes_equal(uint32_t w, uint32_t c) {
    const uint32_t t = w ^ (c * 0x01010101u);
    const uint32_t z = ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t | 0x7F7F7F7Fu);
    return (z >> 7) * 0xFFu;
}
constexpr uint32_t SL_STEP_CAP = 4096;          // eight-byte extension steps a thread spends before the call is handed to the general path (runs, short periods: every candidate matches as far as it may)

// ---------------------------------------------------------------- compress
// (r06, measured: the same search spread over sixteen blocks of two wavefronts with the last block to finish walking the chain was no
//  faster -- 0.05 / 0.12 / 0.18 ms for 256 / 1024 / 2048 bytes against 0.04 / 0.10 / 0.25 here: what a position's search costs is the
//  candidates of its wavefront's 64 different positions taken one after the other, not the CU's issue rate; hence the size limit.)
// (the codec of one member: the single call's kernel below and the grouped kernel further down are this body, inlined)
__device__ __forceinline__ void lzss_small_enc_body(const uint8_t *__restrict__ hin, uint32_t n, uint32_t W, uint8_t *__restrict__ hout, uint32_t *__restrict__ flag) {
    __shared__ __attribute__((aligned(16))) uint8_t s_in[SL_IN_MAX + 16];
    __shared__ __attribute__((aligned(16))) uint8_t s_fc[SL_E_MAX + 48];        // the escaped stream (lzss.go:369-389), zeros behind it
    __shared__ uint32_t s_key[SL_E_MAX];                                        // per position: L << 16 | distance (0: a literal)
    __shared__ uint16_t s_jmp[2][SL_E_MAX + 1];                                 // where the chain is 2^r steps on (E: beyond the end)
    __shared__ uint8_t s_on[SL_E_MAX + 1];                                      // the greedy chain from 0 lands here
    __shared__ __attribute__((aligned(16))) uint8_t s_out[SL_E_MAX + 32];
    __shared__ uint32_t s_wave[SLT / 64 + 1];
    __shared__ uint32_t s_bail;
    const uint32_t tid = threadIdx.x;
    if (tid * 16 < n) reinterpret_cast<uint4 *>(s_in)[tid] = reinterpret_cast<const uint4 *>(hin)[tid];   // (pinned host memory, zero behind n: one PCIe round trip)
    for (uint32_t i = tid; i < (SL_E_MAX + 48) / 4; i += SLT) reinterpret_cast<uint32_t *>(s_fc)[i] = 0;
    if (tid == 0) s_bail = 0;
    __syncthreads();
    // ---- EncodeOpeningSymbols: 3C -> FF; FF -> 5C FF; 5C -> 5C 5C.  Two input bytes per thread.
    uint32_t E;
    {
        const uint32_t i0 = 2 * tid;
        const uint32_t b0 = i0 < n ? s_in[i0] : 0u, b1 = i0 + 1 < n ? s_in[i0 + 1] : 0u;
        uint32_t at = block_scan<SLT>((i0 < n ? lzss_esc_len(b0) : 0u) + (i0 + 1 < n ? lzss_esc_len(b1) : 0u), s_wave, &E);
        if (E > SL_E_MAX) { block_done(flag, GROUP_BACK); return; }                 // (block-uniform)
        if (i0 < n) at = lzss_esc_put(s_fc, at, b0);
        if (i0 + 1 < n) at = lzss_esc_put(s_fc, at, b1);
    }
    __syncthreads();
    // ---- every position: the longest L >= 1 with fc[i, i + L) inside the window (L <= distance, L <= E - i), at its largest distance.
    // Sixteen candidates a load: the bytes equal to fc[i] among them are the candidates, each compared eight bytes at a time.
    const uint32_t Wc = W == 0 ? E : W;                                           // (0: the unbounded search buffer, lzss.go:125)
    const uint32_t *fw = reinterpret_cast<const uint32_t *>(s_fc);
    uint32_t steps = 0;
    for (uint32_t i = tid; i < E; i += SLT) {
        const uint32_t bi = s_fc[i], cap = E - i;
        const unsigned long long pat = lds_load8(fw, i);
        uint32_t best = 0;
        const uint32_t jlo = i - min(i, Wc);
        auto cand = [&](uint32_t j) {                                              // one candidate: fc[j] == fc[i], j in [jlo, i)
            const uint32_t d = i - j, lim = min(d, cap), bl = best >> 16;
            // (candidates come farthest first: a later one only counts if it is LONGER than the best so far -- the byte at that
            //  length decides for most of them before anything else is compared)
            if (lim <= bl || s_fc[j + bl] != s_fc[i + bl]) return;
            unsigned long long x = lds_load8(fw, j) ^ pat;
            uint32_t L = x ? (uint32_t)__builtin_ctzll(x) >> 3 : 8u;
            if (!x) {
                uint32_t off = 8;
                while (off < lim) {
                    x = lds_load8(fw, j + off) ^ lds_load8(fw, i + off);
                    steps++;
                    if (x) { off += (uint32_t)__builtin_ctzll(x) >> 3; break; }
                    off += 8;
                }
                L = off;
            }
            best = max(best, (min(L, lim) << 16) | d);                            // longest, then farthest back (bytes.Index finds the leftmost, lzss.go:419)
        };
        auto word = [&](uint32_t j0, uint32_t m) {                                 // the candidates among four bytes (m: 0xFF where the byte equals fc[i])
            while (m) { const uint32_t k = (uint32_t)__builtin_ctz(m) >> 3; m &= ~(0xFFu << (8 * k)); cand(j0 + k); }
        };
        // whole 16-byte units inside [jlo, i): one test for sixteen candidates; the ragged ends byte by byte
        const uint32_t u0 = (jlo + 15) & ~15u, u1 = i & ~15u;
        for (uint32_t j = jlo; j < min(u0, i); j++) if (s_fc[j] == bi) cand(j);
        for (uint32_t base = u0; base < u1 && steps <= SL_STEP_CAP; base += 16) {
            const uint4 q = *reinterpret_cast<const uint4 *>(s_fc + base);
            const uint32_t m0 = sl_bytes_equal(q.x, bi), m1 = sl_bytes_equal(q.y, bi), m2 = sl_bytes_equal(q.z, bi), m3 = sl_bytes_equal(q.w, bi);
            if (m0 | m1 | m2 | m3) { word(base, m0); word(base + 4, m1); word(base + 8, m2); word(base + 12, m3); }
        }
        for (uint32_t j = max(u1, u0); j < i; j++) if (s_fc[j] == bi) cand(j);
        s_key[i] = best;
    }
    if (steps > SL_STEP_CAP) s_bail = 1;
    __syncthreads();
    if (s_bail) { block_done(flag, GROUP_BACK); return; }
    // ---- the greedy chain from 0 over the whole stream
    lzss_greedy_chain<SLT, SL_E_MAX + 1>(s_key, &s_jmp[0][0], s_on, E, E, 0u);
    // ---- what every chain position puts out: a token iff it is shorter than what it stands for (lzss.go:143), else the bytes
    uint32_t total = 0;
    {
        const uint32_t i0 = 2 * tid;
        LzssItem it[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};                            // (sz 0: not on the chain)
        for (int k = 0; k < 2; k++) if (i0 + k < E && s_on[i0 + k]) it[k] = lzss_item(s_key[i0 + k] >> 16, s_key[i0 + k] & 0xFFFFu);
        uint32_t at = block_scan<SLT>(it[0].sz + it[1].sz, s_wave, &total);
        for (int k = 0; k < 2; k++) {
            if (!it[k].sz) continue;
            lzss_item_put(s_out, at, it[k], s_fc + i0 + k);
            at += it[k].sz;
        }
    }
    __syncthreads();
    if (tid * 16 < total) reinterpret_cast<uint4 *>(hout)[tid] = reinterpret_cast<const uint4 *>(s_out)[tid];
    block_done(flag, total);
}

// ---------------------------------------------------------------- decompress
__device__ __forceinline__ void lzss_small_dec_body(const uint8_t *__restrict__ hin, uint32_t n, uint8_t *__restrict__ hout, uint32_t *__restrict__ flag) {
    __shared__ __attribute__((aligned(16))) uint8_t s_in[SL_DEC_IN_MAX + 32];
    __shared__ uint8_t s_cov[SL_DEC_IN_MAX + 32];                                // the byte belongs to a token's text
    __shared__ uint16_t s_src[2][SL_DEC_E_MAX];                                  // per escaped byte: where it comes from (itself: a literal)
    __shared__ __attribute__((aligned(16))) uint8_t s_val[SL_DEC_E_MAX + 16];
    __shared__ uint32_t s_wave[SLT / 64 + 1];
    __shared__ uint32_t s_bad;
    const uint32_t tid = threadIdx.x;
    if (tid * 16 < n + 16) reinterpret_cast<uint4 *>(s_in)[tid] = tid * 16 < n ? reinterpret_cast<const uint4 *>(hin)[tid] : make_uint4(0, 0, 0, 0);
    for (uint32_t i = tid; i < SL_DEC_IN_MAX + 32; i += SLT) s_cov[i] = 0;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    // ---- the stream's items, two bytes of it per thread: the one chunk
    TileItems it;
    lzd_items(s_in, 0u, 0u, n, 0xFFFFu, s_cov, it);
    uint32_t E;
    uint32_t at = block_scan<SLT>(it.outl[0] + it.outl[1], s_wave, &E);
    if (E > SL_DEC_E_MAX || E == 0) { block_done(flag, E == 0 ? 0u : GROUP_BACK); return; }   // (a '<' that is no token counts as a literal: a malformed stream has E >= 1 and is answered below)
    if (it.bad) s_bad = 1;                                                        // malformed: the general path words the error
    for (int k = 0; k < 2; k++) {
        if (!it.outl[k]) continue;
        if (it.ttl[k]) {
            if (it.tptr[k] > at) s_bad = 1;                                       // the slice starts before the data (lzss.go:349)
            else for (uint32_t t = 0; t < it.tlen[k]; t++) s_src[0][at + t] = (uint16_t)(at + t - it.tptr[k]);
        } else { s_src[0][at] = (uint16_t)at; s_val[at] = s_in[2 * tid + k]; }
        at += it.outl[k];
    }
    __syncthreads();
    if (s_bad) { block_done(flag, GROUP_BACK); return; }
    // ---- every byte's literal: src <- src[src] until nothing moves (a copied byte always lies before the byte that copies it)
    int cur = 0;
    for (int round = 0; round < 14; round++) {
        bool moved = false;
        for (uint32_t q = tid; q < E; q += SLT) { const uint32_t a = s_src[cur][q], b = s_src[cur][a]; s_src[cur ^ 1][q] = (uint16_t)b; moved = moved || a != b; }
        cur ^= 1;
        if (!__syncthreads_or(moved)) break;
    }
    uint32_t v8[8];
    for (int k = 0; k < 8; k++) { const uint32_t q = 8 * tid + k; v8[k] = q < E ? s_val[s_src[cur][q]] : 0u; }
    __syncthreads();                                                               // (a literal's slot is read by its copies: all reads before the writes)
    for (int k = 0; k < 8; k++) if (8 * tid + k < E) s_val[8 * tid + k] = (uint8_t)v8[k];
    __syncthreads();
    // ---- DecodeOpeningSymbols (lzss.go:391-406): a byte is escaped iff the run of 5C right in front of it has odd length AND that run's
    //      first 5C is itself unescaped -- i.e. counting from the last byte that is not 5C.  last[q] = the last position <= q whose byte is
    //      not 5C (a max-scan); the run in front of q + 1 is q - last[q] long.
    //      (the unit's own copy of lzss_dec_body.h's lzd_* unescape: through the helpers, three passes over s_val, a single call measured 0.3 to 0.5 us slower; LEDGER)
    uint32_t mine = 0;                                                            // 1 + the last of this thread's eight positions whose byte is not 5C; 0: none
    for (int k = 0; k < 8; k++) { const uint32_t q = 8 * tid + k; if (q < E && s_val[q] != 0x5C) mine = q + 1; }
    uint32_t inc = mine;
    {
        const uint32_t lane = tid & 63, wave = tid >> 6;
        for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d, 64); if (lane >= (uint32_t)d) inc = max(inc, o); }
        __syncthreads();
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
    }
    uint32_t keep[8], ov[8], cnt = 0;
    // run of 5C in front of q: q - (last non-5C position before q, + 1)
    {
        uint32_t before_q = 0;                                                     // last non-5C position + 1 among positions < q
        {
            const uint32_t lane = tid & 63, wave = tid >> 6;
            uint32_t b = 0;
            for (uint32_t w = 0; w < wave; w++) b = max(b, s_wave[w]);
            uint32_t prev = __shfl_up(inc, 1, 64);
            if (lane == 0) prev = 0;
            before_q = max(b, prev);
        }
        for (int k = 0; k < 8; k++) {
            const uint32_t q = 8 * tid + k;
            keep[k] = 0; ov[k] = 0;
            if (q < E) {
                const uint32_t run = q - before_q, b = s_val[q];
                const bool esc = run & 1u;
                keep[k] = esc || b != 0x5C;
                ov[k] = esc ? b : (b == 0xFF ? 0x3Cu : b);
                cnt += keep[k];
                if (b != 0x5C) before_q = q + 1;
            }
        }
    }
    uint32_t total;
    uint32_t o = block_scan<SLT>(cnt, s_wave, &total);
    __shared__ __attribute__((aligned(16))) uint8_t s_res[SL_DEC_E_MAX + 16];
    for (int k = 0; k < 8; k++) if (keep[k]) s_res[o++] = (uint8_t)ov[k];
    __syncthreads();
    for (uint32_t u = tid; u * 16 < total; u += SLT) reinterpret_cast<uint4 *>(hout)[u] = reinterpret_cast<const uint4 *>(s_res)[u];
    block_done(flag, total);
}

__global__ __launch_bounds__(SLT) void k_lzss_small_enc(const uint8_t *__restrict__ hin, uint32_t n, uint32_t W, uint8_t *__restrict__ hout, uint32_t *__restrict__ flag) {
    lzss_small_enc_body(hin, n, W, hout, flag);
}
__global__ __launch_bounds__(SLT) void k_lzss_small_dec(const uint8_t *__restrict__ hin, uint32_t n, uint8_t *__restrict__ hout, uint32_t *__restrict__ flag) {
    lzss_small_dec_body(hin, n, hout, flag);
}

// ---------------------------------------------------------------- many members, one launch (the batch calls)
// A block per member, the member table in pinned host memory beside the packed members: the block reads its entry, then does exactly what
// the single call's kernel does for that member.  No block looks at another: the grid may be far larger than what is resident at once.
__global__ __launch_bounds__(SLT) void k_lzss_batch_enc(const SmallMember *__restrict__ tab, uint8_t *__restrict__ base, uint32_t W) {
    const SmallMember m = tab[blockIdx.x];
    lzss_small_enc_body(base + m.in_off, m.n, W, base + m.out_off, reinterpret_cast<uint32_t *>(base + m.status_off));
}
__global__ __launch_bounds__(SLT) void k_lzss_batch_dec(const SmallMember *__restrict__ tab, uint8_t *__restrict__ base) {
    const SmallMember m = tab[blockIdx.x];
    lzss_small_dec_body(base + m.in_off, m.n, base + m.out_off, reinterpret_cast<uint32_t *>(base + m.status_off));
}

// what the single calls and the batch classes below take
bool small_enc_takes(const uint8_t *, size_t n, int64_t window) { return n != 0 && n <= SL_IN_MAX && window <= 0xFFFF; }
bool small_dec_takes(const uint8_t *, size_t n, int64_t) { return n != 0 && n <= SL_DEC_IN_MAX; }

// The host side of a single call: the input and `pad` zero bytes behind it into the context's pinned staging, launch(in, out, flag), the
// wait for the flag.  1: the kernel handed the input back (the caller takes the general path).  *out: the result in the staging.
template <class Launch>
int small_call(Ctx &c, const uint8_t *in, size_t n, size_t pad, const uint8_t **out, size_t *out_n, const Launch &launch) {
    int rc = ctx_init(c); if (rc) return rc;
    hipStream_t s = c.own_stream;
    void *pp; rc = pinned_buf(c, SP_BYTES, &pp); if (rc) return rc;
    uint8_t *pin = (uint8_t *)pp;
    memcpy(pin + SP_IN, in, n);
    memset(pin + SP_IN + n, 0, pad);
    uint32_t *flag = (uint32_t *)(pin + SP_FLAG);
    *flag = GROUP_PENDING;
    rc = launch(s, (const uint8_t *)(pin + SP_IN), pin + SP_OUT, flag); if (rc) return rc;
    rc = flags_wait(c, s, flag, 1, "lzss"); if (rc) return rc;
    if (*flag == GROUP_BACK) return 1;
    *out = pin + SP_OUT; *out_n = *flag;
    return RSN_OK;
}

}  // namespace

// 1: not an input for this path (the caller takes the general one).  *out: the result in the context's pinned staging.
int lzss_small_compress(Ctx &c, const uint8_t *in, size_t n, int64_t window, const uint8_t **out, size_t *out_n) {
    if (!small_enc_takes(in, n, window)) return 1;
    return small_call(c, in, n, 16, out, out_n, [&](hipStream_t s, const uint8_t *pin, uint8_t *pout, uint32_t *flag) -> int {
        RSN_LAUNCH("lzss_small_enc", k_lzss_small_enc, dim3(1), dim3(SLT), 0, s, pin, (uint32_t)n, (uint32_t)(window <= 0 ? 0 : window), pout, flag);
        return RSN_OK;
    });
}
int lzss_small_decompress(Ctx &c, const uint8_t *in, size_t n, const uint8_t **out, size_t *out_n) {
    if (!small_dec_takes(in, n, 0)) return 1;
    return small_call(c, in, n, 32, out, out_n, [&](hipStream_t s, const uint8_t *pin, uint8_t *pout, uint32_t *flag) -> int {
        RSN_LAUNCH("lzss_small_dec", k_lzss_small_dec, dim3(1), dim3(SLT), 0, s, pin, (uint32_t)n, pout, flag);
        return RSN_OK;
    });
}

// ---------------------------------------------------------------- the two classes of the batch calls (codecs.h; the packers: group_run.h)
namespace {
struct SmallEncClass {
    static constexpr const char *what = "lzss batch compress";
    static size_t in_bytes(size_t n) { return lzss_in_slot(n); }
    static size_t out_bytes(size_t n) { return lzss_enc_out_slot(n, SL_E_MAX); }
    static int launch(Ctx &c, hipStream_t s, uint32_t g, const SmallMember *tab, uint8_t *base, int64_t window) {
        RSN_LAUNCH("lzss_batch_enc", k_lzss_batch_enc, dim3(g), dim3(SLT), 0, s, tab, base, (uint32_t)(window <= 0 ? 0 : window));
        return RSN_OK;
    }
};
struct SmallDecClass {
    static constexpr const char *what = "lzss batch decompress";
    static size_t in_bytes(size_t n) { return lzss_in_slot(n); }
    static size_t out_bytes(size_t) { return lzss_dec_out_slot(SL_DEC_E_MAX); }
    static int launch(Ctx &c, hipStream_t s, uint32_t g, const SmallMember *tab, uint8_t *base, int64_t) {
        RSN_LAUNCH("lzss_batch_dec", k_lzss_batch_dec, dim3(g), dim3(SLT), 0, s, tab, base);
        return RSN_OK;
    }
};
}  // namespace
const BatchClass &lzss_small_class(bool compress) {
    static const BatchClass enc = {"lzss small compress", 1, small_enc_takes, class_run<SmallEncClass>, class_run_dev<SmallEncClass>},
                            dec = {"lzss small decompress", 1, small_dec_takes, class_run<SmallDecClass>, class_run_dev<SmallDecClass>};
    return compress ? enc : dec;
}

}  // namespace rsn
