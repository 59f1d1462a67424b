// huff_small.hip -- the Huffman codec for a host buffer of at most 64 KiB (BASELINE configs[0]: the reference's own README case).
//
// At this size a call is its fixed costs: the general path is ~10 launches, five copy commands and three host round trips for work the
// device does in a few microseconds (r04: 89 us to compress 64 KiB, 129 us to decompress it).  Here a call is
//   compress    host memcpy into pinned memory -> k_small_hist (a block per 2 KiB tile reads it over PCIe, keeps a device copy, writes counts
//               straight back into pinned memory) -> the Go-exact tree, codes and header on the host (huffman.go:58-127,312-318)
//               -> k_small_emit (code table, header and tile bit positions in the KERNEL ARGUMENTS; a block per 2 KiB tile stores its words
//               into pinned memory) -> host memcpy into the result block:                    2 launches, no copy command
//   decompress  header and tree on the host (the stream is in host memory: huffman.go:196-227,261) -> host memcpy of the stream into pinned
//               memory -> k_small_dec (up to 32 blocks; the tree in the kernel arguments, every block builds its lookup table; lanes
//               take subsequences and settle where their codewords start -- see the kernel; decoded bytes into pinned memory)
//               -> host memcpy:                                                              1 launch, no copy command
// The host does not wait for the stream either: every block ends by setting a word in pinned memory that the host polls (block_done).
// 64 KiB of the README's text, host buffer to host buffer: compress 89 -> 32 us, decompress 129 -> 52 us (r05).
// Many streams at once (rsn_huffman_decompress_batch): k_huff_batch_dec, ONE block per stream with k_small_dec's body.
// Many inputs at once (rsn_huffman_compress_batch): k_huff_batch_enc, ONE block per input of 2 B to 16 KiB that builds its own tree.
// For byte alphabets (every symbol < 0x80); everything else -- runes, a single symbol,
// foreign headers, malformed streams and their error texts -- returns 1 and takes the general path, which words the errors.  (In a
// batch, runes have grouped kernels of their own behind these: huff_rune.hip to compress, huff_rune_dec.hip to decompress.)
#include "huff_small_body.h"
#include "huff_plan_small.h"

namespace rsn {
namespace {

// pinned staging of one call (Ctx::pinned): offsets
constexpr size_t PIN_IN = 0;                                        // the caller's bytes, zero-padded to 16
constexpr size_t PIN_OUT = PIN_IN + DEC_STREAM_MAX + 128;          // what the kernels produced
constexpr size_t PIN_CNT = PIN_OUT + SMALL_MAX + 64;               // encoder: every tile's 128 counts (u16), then a word per tile: a byte >= 0x80 was seen; decoder: status words
constexpr size_t PIN_BYTES = PIN_CNT + 32 * 128 * 2 + 2 * 32 * 4 + 256;
static_assert(PIN_OUT % 16 == 0 && PIN_CNT % 16 == 0, "16-byte stores");

// ---------------------------------------------------------------- compress, kernel 1: counts (huffman.go:306-311) + a device copy
// One block per tile of 2 KiB, a 16-byte load per lane straight from the caller's bytes in pinned host memory (one PCIe round trip for the
// whole kernel: r05, one block looping over 64 KiB: 15 us, four dependent round trips).  The tile's counts go back to pinned memory as
// they are: the host adds them up (the alphabet's counts) and, once it has the code lengths, turns them into every tile's bit position.
constexpr uint32_t ST = 2048;                   // bytes per tile
constexpr uint32_t ST_MAX = SMALL_MAX / ST;     // tiles
__global__ __launch_bounds__(128) void k_small_hist(const uint4 *__restrict__ hin, uint32_t n, uint4 *__restrict__ d_copy, uint16_t *__restrict__ tile_hist, uint32_t *__restrict__ tile_high) {
    __shared__ uint32_t s_h[2][128];
    __shared__ uint32_t s_high;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, at = blockIdx.x * ST + tid * 16;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (at < n) v = hin[at / 16];                                      // (host memory; the pad behind n is zero)
    s_h[0][tid] = 0; s_h[1][tid] = 0;
    if (tid == 0) s_high = 0;
    __syncthreads();
    if (at < n) {
        d_copy[at / 16] = v;
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        const uint32_t valid = min(16u, n - at);
        uint32_t high = 0;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t b = (w[j >> 2] >> (8 * (j & 3))) & 0xFF;
            if ((uint32_t)j < valid) { high |= b & 0x80; atomicAdd(&s_h[wave][b & 0x7F], 1u); }
        }
        if (high) s_high = 1;
    }
    __syncthreads();
    tile_hist[blockIdx.x * 128 + tid] = (uint16_t)(s_h[0][tid] + s_h[1][tid]);
    block_done(&tile_high[blockIdx.x], s_high);
}

// ---------------------------------------------------------------- compress, kernel 2: the stream (huffman.go:229-256,174-191)
// One block per tile again.  Code table, header and every tile's first bit position come in the KERNEL ARGUMENTS (no upload); a block packs
// its tile's codes into an LDS image of the words they touch and stores the words it owns into pinned host memory.  Two neighbours share
// the word a tile boundary falls into: it belongs to the LATER tile, which works out the earlier one's last few bits itself (from the up to
// 31 symbols before its first) -- no atomics on memory, no zeroed output, nothing between the blocks.
struct SmallEmitArgs {
    const uint8_t *d_copy; uint32_t *hout; uint32_t *done;   // done[tile]: FLAG_PENDING until the tile's words are out
    uint32_t n, H, total;                // input bytes; header bytes incl. "\\\n" and the pad byte; bytes of the stream
    uint32_t P[ST_MAX + 1];              // first code bit of every tile, counted from the stream's first byte (P[0] = 8 H + pad)
    uint32_t tab[128];                   // len << 24 | code (a 64 KiB input cannot produce a code beyond 22 bits)
    uint8_t hdr[HDR_MAX + 4];
};

constexpr uint32_t EMIT_IMG_WORDS = ST * 24 / 32 + (HDR_MAX + 3) / 4 + 8;
__global__ __launch_bounds__(256) void k_small_emit(SmallEmitArgs a) {
    __shared__ uint32_t s_img[EMIT_IMG_WORDS];       // the words this tile's bits fall into, in memory order (block 0: from the stream's first byte)
    __shared__ uint32_t s_tab[128];
    __shared__ uint32_t s_wave[5];
    __shared__ uint32_t s_prev[32];
    const uint32_t tid = threadIdx.x, b = blockIdx.x, n_tiles = gridDim.x;
    const uint32_t Pb = a.P[b], Pn = a.P[b + 1];
    const uint32_t W0 = b ? Pb >> 5 : 0u;                                        // the image's first word
    const uint32_t img_words = (Pn - (W0 << 5) + 31) >> 5;
    const uint32_t hw = b ? 0u : (a.H + 3) / 4;
    for (uint32_t w = tid; w < img_words + 1; w += 256) {
        uint32_t v = 0;
        if (w < hw) {
#pragma unroll
            for (int k = 0; k < 4; k++) { const uint32_t at = 4 * w + k; if (at < a.H) v |= (uint32_t)a.hdr[at] << (8 * k); }
        }
        s_img[w] = v;
    }
    if (tid < 128) s_tab[tid] = a.tab[tid];
    const uint32_t need = b ? Pb & 31 : 0u;                                      // bits of the tile before in this tile's first word
    if (need && tid < 32) s_prev[tid] = a.tab[a.d_copy[b * ST - 1 - tid] & 0x7F];   // (the tile before is a whole one: 2048 symbols, a bit each at least)
    // eight symbols a lane
    const uint32_t lo = b * ST + tid * 8;
    uint2 v = make_uint2(0, 0);
    if (lo < a.n) v = *reinterpret_cast<const uint2 *>(a.d_copy + lo);
    const uint32_t valid = lo < a.n ? min(8u, a.n - lo) : 0u;
    __syncthreads();
    uint32_t e[8], bits = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t byte = ((j < 4 ? v.x : v.y) >> (8 * (j & 3))) & 0x7F;
        e[j] = (uint32_t)j < valid ? s_tab[byte] : 0u;
        bits += e[j] >> 24;
    }
    const uint32_t pos0 = Pb - (W0 << 5) + block_excl_scan<4>(bits, s_wave);
    if (bits) {
        uint32_t w = pos0 >> 5, nacc = pos0 & 31;                     // the word being filled; bits of it that are in `acc` (the first nacc: a neighbour's, zero here)
        unsigned long long acc = 0;                                    // left-aligned
        bool first = true;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t l = e[j] >> 24;
            acc |= (unsigned long long)(e[j] & 0xFFFFFFu) << (64 - nacc - l);      // (l == 0: nothing)
            nacc += l;
            if (nacc >= 32) {
                const uint32_t be = __builtin_bswap32((uint32_t)(acc >> 32));
                if (first) atomicOr(&s_img[w], be); else s_img[w] = be;     // (the first word may be shared with the lane before)
                first = false;
                w++; acc <<= 32; nacc -= 32;
            }
        }
        if (nacc) atomicOr(&s_img[w], __builtin_bswap32((uint32_t)(acc >> 32)));   // (... the last with the lane after)
    }
    if (need && tid == 0) {                                            // the tile before ends in this tile's first word
        unsigned long long tail = 0;
        uint32_t have = 0;
        for (uint32_t k = 0; have < need; k++) { const uint32_t ent = s_prev[k]; tail |= (unsigned long long)(ent & 0xFFFFFFu) << have; have += ent >> 24; }
        const uint32_t t32 = (uint32_t)tail & ((1u << need) - 1u);
        atomicOr(&s_img[0], __builtin_bswap32(t32 << (32 - need)));
    }
    __syncthreads();
    // the words this tile owns: up to, not including, the one the next tile starts in; the last tile: to the stream's end
    const uint32_t own = b + 1 < n_tiles ? (Pn >> 5) - W0 : (a.total + 3) / 4 - W0;
    for (uint32_t i = tid; i < own; i += 256) a.hout[W0 + i] = s_img[i];
    block_done(&a.done[b], 0);
}

__global__ __launch_bounds__(DT) void k_small_dec(SmallDecArgs a) {
    __shared__ uint32_t s_pay[DEC_PAY_WORDS];                 // big-endian words of this block's part of the stream
    __shared__ __attribute__((aligned(16))) uint8_t s_out[DEC_OUT_CAP + 32];
    small_dec_body<DEC_PAY_WORDS, DEC_OUT_CAP, true, DL>(a, s_pay, s_out);
}

// ---------------------------------------------------------------- decompress, many streams in one launch (the batch call)
// ONE block per member, whatever the grid: the block copies its member's entry of the table (a SmallDecArgs in pinned memory: the tree,
// the stream's bounds, where its bytes and its output slot are) into LDS, builds its lookup table from it and decodes the whole stream
// with k_small_dec's lane maps.  No block waits for another.  What one block holds is the member cutoff: HB_PAY_MAX bytes of payload
// (256 lanes of at most HB_S_MAX bits) and HB_OUT_MAX decoded bytes (its LDS image of the output).
// (HB_S_MAX, HB_PAY_MAX, HB_OUT_MAX: huff_small_body.h -- huff_mid.hip takes what lies above them)
constexpr uint32_t HB_PAY_WORDS = DL * HB_S_MAX / 32 + 8;
__global__ __launch_bounds__(DT) void k_huff_batch_dec(const SmallDecArgs *__restrict__ tab) {
    __shared__ SmallDecArgs s_a;
    __shared__ uint32_t s_pay[HB_PAY_WORDS];
    __shared__ __attribute__((aligned(16))) uint8_t s_out[HB_OUT_MAX + 32];
    const uint32_t *src = reinterpret_cast<const uint32_t *>(tab + blockIdx.x);
    for (uint32_t i = threadIdx.x; i < sizeof(SmallDecArgs) / 4; i += DT) reinterpret_cast<uint32_t *>(&s_a)[i] = src[i];
    __syncthreads();
    small_dec_body<HB_PAY_WORDS, HB_OUT_MAX, false, DL>(s_a, s_pay, s_out);
}

// ---------------------------------------------------------------- compress, many members in one launch: huff_enc_body (huff_small_body.h)
__global__ __launch_bounds__(HE_T) void k_huff_batch_enc(const SmallMember *__restrict__ tab, uint8_t *__restrict__ base) {
    __shared__ uint4 s_in[HE_IN_MAX / 16];
    __shared__ uint32_t s_img[HE_IMG_WORDS];
    huff_enc_body<HE_T, HE_IN_MAX, HE_IMG_WORDS, false>(tab, base, s_in, s_img, [](uint32_t n) { return huff_small_enc_out_slot(n); });
}


}  // namespace

// 1: not an input for this path (the caller takes the general one)
int huff_small_compress(Ctx &c, const uint8_t *in, size_t n, const uint8_t **out, size_t *out_n) {
    if (n < 2 || n > SMALL_MAX) return 1;                                          // (r06: from 2 bytes up -- the README's own files are 13 and 25 bytes; one distinct symbol: the general path)
    int rc = ctx_init(c); if (rc) return rc;
    hipStream_t s = c.own_stream;
    void *pp; rc = pinned_buf(c, PIN_BYTES, &pp); if (rc) return rc;
    uint8_t *pin = (uint8_t *)pp;
    void *dp; rc = dev_buf(c, Slot::HS_INPUT, SMALL_MAX + 64, &dp); if (rc) return rc;
    memcpy(pin + PIN_IN, in, n);
    memset(pin + PIN_IN + n, 0, 16);
    const uint32_t n_tiles = (uint32_t)ceil_div(n, ST);
    uint16_t *th = (uint16_t *)(pin + PIN_CNT);
    uint32_t *hi = (uint32_t *)(th + ST_MAX * 128);
    uint32_t *done = hi + ST_MAX;
    for (uint32_t t = 0; t < n_tiles; t++) { hi[t] = FLAG_PENDING; done[t] = FLAG_PENDING; }
    RSN_LAUNCH("huff_small_hist", k_small_hist, dim3(n_tiles), dim3(128), 0, s, (const uint4 *)(pin + PIN_IN), (uint32_t)n, (uint4 *)dp, th, hi);
    rc = flags_wait(c, s, hi, n_tiles, "huffman"); if (rc) return rc;
    uint32_t cnt[128] = {0};
    for (uint32_t t = 0; t < n_tiles; t++) {
        if (hi[t]) return 1;                                                    // a byte >= 0x80: runes (huffman.go:309)
        for (uint32_t b = 0; b < 128; b++) cnt[b] += th[t * 128 + b];
    }
    std::vector<HuffSym> syms;
    for (uint32_t b = 0; b < 128; b++) if (cnt[b]) syms.push_back({b, cnt[b]});
    if (syms.size() < 2) return 1;
    std::string hdr, msg;
    emit_header(syms, hdr);
    HuffTree tree; HuffCodes codes;
    if (!build_tree(syms, tree, msg) || !assign_codes(tree, codes, msg, false)) return 1;
    if (codes.max_len > 24) return 1;
    const unsigned pad = (unsigned)((8 - codes.total_bits % 8) % 8);            // huffman.go:245-249
    hdr.append("\\\n");
    hdr.push_back((char)pad);
    const size_t H = hdr.size();
    const size_t total = H + (size_t)((codes.total_bits + pad) / 8);
    if (H > HDR_MAX || total > SMALL_MAX) return 1;
    SmallEmitArgs a{};
    a.d_copy = (const uint8_t *)dp; a.hout = (uint32_t *)(pin + PIN_OUT); a.done = done;
    a.n = (uint32_t)n; a.H = (uint32_t)H; a.total = (uint32_t)total;
    uint32_t len_of[128] = {0};
    for (uint32_t i = 0; i < tree.n_leaves; i++) { a.tab[tree.rune[i]] = ((uint32_t)codes.len[i] << 24) | (uint32_t)codes.code[i]; len_of[tree.rune[i]] = codes.len[i]; }
    a.P[0] = (uint32_t)(8 * H + pad);
    for (uint32_t t = 0; t < n_tiles; t++) {                                    // where every tile's first code bit goes
        uint32_t bits = 0;
        for (uint32_t b = 0; b < 128; b++) bits += th[t * 128 + b] * len_of[b];
        a.P[t + 1] = a.P[t] + bits;
    }
    memcpy(a.hdr, hdr.data(), H);
    RSN_LAUNCH("huff_small_emit", k_small_emit, dim3(n_tiles), dim3(256), 0, s, a);
    rc = flags_wait(c, s, done, n_tiles, "huffman"); if (rc) return rc;
    *out = pin + PIN_OUT; *out_n = total;
    return RSN_OK;
}

// The header parsed, the tree built and the kernel's view of the stream (everything in `a` but where its bytes are, the flags and the
// output): the stream's bytes from in + *A0 on are what the kernel reads, as a.pay.  `lanes`: subsequences the kernel has at most, of at
// most s_max bits.  1 = not for the small-input decoder (the caller takes the general one, which also words the errors).
int small_dec_plan(const uint8_t *in, size_t n, uint32_t lanes, uint32_t s_max, SmallDecArgs &a, size_t *A0, unsigned long long *expect_out, bool wide) {
    const size_t stream_max = wide ? PARSE_STREAM_MAX_WIDE : DEC_STREAM_MAX, out_max = wide ? PARSE_OUT_MAX_WIDE : SMALL_MAX;
    const unsigned long long count_max = wide ? PLAN_COUNT_LIMIT_WIDE - 1 : SMALL_MAX;
    if (n < 8 || n > stream_max) return 1;
    // ---- strings.SplitN(content, "\\\n", 2) (huffman.go:261); the counts (huffman.go:196-227)
    size_t sep = (size_t)-1;
    for (size_t i = 0; i + 1 < std::min<size_t>(n, HDR_MAX + 8); i++) if (in[i] == 0x5C && in[i + 1] == 0x0A) { sep = i; break; }
    if (sep == (size_t)-1 || sep + 4 > n) return 1;
    std::vector<HuffSym> syms; std::string msg;
    if (!parse_header(in, sep, syms, msg) || syms.size() < 2 || syms.size() > 128) return 1;
    unsigned long long expect = 0;
    for (const HuffSym &sy : syms) { if (sy.rune >= 0x80 || sy.freq > count_max) return 1; expect += sy.freq; }
    if (expect == 0 || expect > out_max) return 1;
    const size_t pay = sep + 3, sn = n - sep - 2;
    const unsigned diff = in[sep + 2];
    const unsigned long long nbits = (unsigned long long)(sn - 1) * 8;
    if (diff >= nbits) return 1;
    HuffTree tree; HuffCodes codes;
    if (!build_tree(syms, tree, msg) || !assign_codes(tree, codes, msg, false)) return 1;
    if (codes.max_len > 32 || codes.max_len == 0) return 1;
    // ---- the tree as the kernel wants it (every block fills its lookup table from it)
    a = SmallDecArgs{};
    const uint32_t A = tree.n_leaves;
    const size_t n_int = tree.freq.size() - A;
    for (size_t i = 0; i < n_int; i++) {
        const int32_t kids[2] = {tree.left[A + i], tree.right[A + i]};
        for (int b = 0; b < 2; b++) a.child[2 * i + b] = tree.is_leaf(kids[b]) ? (uint16_t)(0x8000u | tree.rune[kids[b]]) : (uint16_t)(kids[b] - (int32_t)A);
    }
    a.root = (uint32_t)(tree.root - (int32_t)A);
    *A0 = pay & ~(size_t)3;
    a.pay_words = (uint32_t)((n - *A0 + 3) / 4) + 8;
    a.p0 = (uint32_t)(8 * (pay - *A0) + diff);
    a.end = (uint32_t)(8 * (pay - *A0) + nbits);
    a.K = (uint32_t)std::min<unsigned>(codes.max_len, DEC_K); a.n_child = (uint32_t)(2 * n_int);
    const uint32_t span = a.end - a.p0;
    a.S = std::max<uint32_t>(64, (uint32_t)round_up(ceil_div(span, lanes), 32));
    if (a.S > s_max) return 1;
    a.T = (uint32_t)ceil_div(span, a.S);
    a.flat = codes.min_len == codes.max_len ? codes.max_len : 0u;
    *expect_out = expect;
    return RSN_OK;
}

int huff_small_decompress(Ctx &c, const uint8_t *in, size_t n, const uint8_t **out, size_t *out_n) {
    SmallDecArgs a;
    size_t A0 = 0; unsigned long long expect = 0;
    if (small_dec_plan(in, n, DEC_BLOCKS * DL, DEC_S_MAX, a, &A0, &expect) != RSN_OK) return 1;
    int rc = ctx_init(c); if (rc) return rc;
    hipStream_t s = c.own_stream;
    void *pp; rc = pinned_buf(c, PIN_BYTES, &pp); if (rc) return rc;
    uint8_t *pin = (uint8_t *)pp;
    void *dp; rc = dev_buf(c, Slot::HS_DEC_MAPS, (DEC_BLOCKS * 32 + DEC_BLOCKS) * 4, &dp); if (rc) return rc;      // the blocks' maps and flags
    // A flag holds the number of the call that set it: nothing to clear between calls on the same ALLOCATION.  Keyed on the allocation's
    // process-unique number, not its address (rsn_device_set / rsn_trim / the admission gate free the slot, and a later
    // hipMalloc can hand the same address back with other contents -- a stale flag equal to the current number would pass for this call's).
    static thread_local uint32_t seq = 0;
    static thread_local unsigned long long seq_of = 0;
    if (seq_of != c.buf(Slot::HS_DEC_MAPS).gen || ++seq == 0) { seq = 1; seq_of = c.buf(Slot::HS_DEC_MAPS).gen; RSN_HIP(hipMemsetAsync(dp, 0, (DEC_BLOCKS * 32 + DEC_BLOCKS) * 4, s)); }
    memcpy(pin + PIN_IN, in + A0, n - A0);
    memset(pin + PIN_IN + (n - A0), 0, 64);
    uint32_t *status = (uint32_t *)(pin + PIN_CNT);
    a.pay = (const uint32_t *)(pin + PIN_IN);
    const uint32_t n_blk = (uint32_t)ceil_div(a.T, DL);
    a.seq = seq;
    a.out_max = SMALL_MAX;
    a.hout = pin + PIN_OUT; a.status = status;
    a.g_maps = (uint32_t *)dp; a.g_flags = a.g_maps + DEC_BLOCKS * 32;
    for (uint32_t b = 0; b <= DEC_BLOCKS; b++) status[b] = FLAG_PENDING;
    RSN_LAUNCH("huff_small_dec", k_small_dec, dim3(n_blk), dim3(DT), 0, s, a);
    rc = flags_wait(c, s, status, n_blk, "huffman"); if (rc) return rc;
    for (uint32_t b = 0; b < n_blk; b++) if (status[b] != 0) return 1;
    *out = pin + PIN_OUT; *out_n = status[DEC_BLOCKS];
    return RSN_OK;
}

// The members of a decoding class: a stream the one-workgroup decoder cannot take -- runes, over the cutoff, anything small_dec_plan
// refuses -- goes to `back` untouched; the rest in groups (run_groups): the table entry is the plan's SmallDecArgs with its pointers into
// the staging, the input the stream from the 4-byte boundary the kernel reads from, and two status words (done / handed back, decoded bytes).
int huff_dec_run(Ctx &c, const HuffDecShape &shape, const HuffDecLaunch &launch, const std::vector<size_t> &idx, const uint8_t *const *ins, const size_t *lens,
                 const SmallTake &take, std::vector<size_t> &back, size_t *failed) {
    struct Plan { size_t i, A0; unsigned long long expect; SmallDecArgs a; };
    std::vector<Plan> plans;
    plans.reserve(idx.size());
    for (size_t i : idx) {
        Plan p; p.i = i;
        if (lens[i] < 8 || lens[i] > HDR_MAX + 8 + shape.pay_max || small_dec_plan(ins[i], lens[i], shape.lanes, shape.s_max, p.a, &p.A0, &p.expect) != RSN_OK ||
            p.expect > shape.out_max) { back.push_back(i); continue; }
        plans.push_back(p);
    }
    std::vector<size_t> handed;
    const int rc = run_groups<SmallDecArgs>(c, "huffman batch decompress", plans.size(),
        [&](size_t k) { const Plan &p = plans[k]; const size_t sn = lens[p.i] - p.A0; return GroupItem{p.i, ins[p.i] + p.A0, sn, huff_dec_in_slot(sn), huff_dec_out_slot(p.expect)}; },
        [&](SmallDecArgs &a, size_t k, uint8_t *base, const MemberSlots &o) {
            a = plans[k].a;
            a.pay = (const uint32_t *)(base + o.in);
            a.hout = base + o.out; a.out_max = (uint32_t)plans[k].expect;
            a.status = (uint32_t *)(base + o.status); a.status[1] = 0;
        },
        [&](hipStream_t s, uint32_t g, const SmallDecArgs *tab, uint8_t *) { return launch(c, s, g, tab); },
        [](const uint32_t *w) { return w[0] != 0 ? GROUP_BACK : w[1]; }, take, handed, failed);
    if (rc) return rc;
    // (members refused up front and members handed back, in index order)
    back.insert(back.end(), handed.begin(), handed.end());
    std::sort(back.begin(), back.end());
    return RSN_OK;
}

namespace {
int launch_batch_dec(Ctx &c, hipStream_t s, uint32_t g, const SmallDecArgs *tab) {
    RSN_LAUNCH("huff_batch_dec", k_huff_batch_dec, dim3(g), dim3(DT), 0, s, tab);
    return RSN_OK;
}
constexpr HuffDecShape BATCH_DEC_SHAPE = {DL, HB_S_MAX, HB_PAY_MAX, HB_OUT_MAX};
bool batch_dec_takes(const uint8_t *, size_t n, int64_t) { return n >= 8 && n <= HDR_MAX + 8 + BATCH_DEC_SHAPE.pay_max; }
// (the plan has been made: what huff_dec_run refuses behind it, asked here)
bool batch_dec_takes_plan(size_t n, const HuffDevSummary &sum) { return batch_dec_takes(nullptr, n, 0) && huff_dec_shape_takes(BATCH_DEC_SHAPE, sum); }
int batch_dec_run(Ctx &c, const std::vector<size_t> &idx, const uint8_t *const *ins, const size_t *lens, int64_t,
                  const SmallTake &take, std::vector<size_t> &back, size_t *failed, std::vector<size_t> *) {
    return huff_dec_run(c, BATCH_DEC_SHAPE, launch_batch_dec, idx, ins, lens, take, back, failed);
}
int batch_dec_run_dev(Ctx &c, hipStream_t s, const std::vector<size_t> &idx, const rsn_dev_member *mem, int64_t, const DevPlans *plans, std::vector<uint32_t> &answers) {
    return huff_dec_run_dev(c, s, BATCH_DEC_SHAPE, launch_batch_dec, idx, mem, *plans, answers);
}
bool batch_enc_takes(const uint8_t *, size_t n, int64_t) { return n >= 2 && n <= HE_IN_MAX; }
// (the kernel hands back runes and a single symbol)
struct SmallEncClass {
    static constexpr const char *what = "huffman batch compress";
    static size_t in_bytes(size_t n) { return huff_enc_in_slot(n); }
    static size_t out_bytes(size_t n) { return huff_small_enc_out_slot((uint32_t)n); }
    static int launch(Ctx &c, hipStream_t s, uint32_t g, const SmallMember *tab, uint8_t *base, int64_t) {
        RSN_LAUNCH("huff_batch_enc", k_huff_batch_enc, dim3(g), dim3(HE_T), 0, s, tab, base);
        return RSN_OK;
    }
};
}  // namespace
// fewer than two members for the grouped encoder: every member takes the pipeline (a group's one serial tree against the host's)
const BatchClass &huff_small_class(bool compress) {
    static const BatchClass enc = {"huffman small compress", 2, batch_enc_takes, class_run<SmallEncClass>, class_run_dev<SmallEncClass>},
                            dec = {"huffman small decompress", 1, batch_dec_takes, batch_dec_run, batch_dec_run_dev, batch_dec_takes_plan};
    return compress ? enc : dec;
}

}  // namespace rsn
