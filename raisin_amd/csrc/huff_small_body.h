// huff_small_body.h -- the device code that the Huffman kernels of huff_small.hip (a single small call, the batch kernels for members of
// up to 16 KiB), of huff_mid.hip (the batch kernels for members of 16 to 64 KiB) and of huff_big_dec.hip (the tiled decoder above that) share: the lane-map decoder of one workgroup, the
// one-workgroup encoder that builds its own tree, the tree in one wavefront's VGPRs (wave_tree: every kernel that builds one calls it,
// the rune kernels and the device plans too) and their scans; their last store is block_dev.h's block_done.  The bodies take what differs between the kernels
// -- lanes, LDS sizes, where the large LDS arrays live -- as template parameters and arguments; DESIGN 4.7.
#pragma once

#include "block_dev.h"
#include "group_run.h"
#include "huff_host.h"
#include "huff_pathmap.h"
#include "huff_plan_small.h"

namespace rsn {

// ---- what the host's plan of a stream and the decoding kernels share (huff_small.hip: small_dec_plan; one type for both units)
constexpr uint32_t SMALL_MAX = 65536;           // bytes of input (compress) / of output (decompress)
struct SmallDecArgs {
    const uint32_t *pay;      // the stream from a 4-byte boundary at or before its first payload byte (pinned host memory; zero behind its end)
    uint32_t pay_words;
    uint32_t p0, end;         // first code bit / the bit behind the last, counted from `pay`
    uint32_t K, root, n_child;  // index bits of the lookup table; the tree's root (an internal node)
    uint32_t S, T;            // bits per lane; lanes that have a subsequence
    uint32_t flat;            // every code has this length (0: lengths differ): the boundaries are where the arithmetic says -- as many phases as the code has bits, and none to find
    uint32_t seq;             // this call's number: what a block's flag holds once its map is out
    uint8_t *hout; uint32_t *status;      // status[b]: FLAG_PENDING, then 0 = block b done, 1 = not for this kernel; status[32]: decoded bytes (batch: status[1])
    uint32_t *g_maps, *g_flags;           // device memory: [block][32] (exit << 24 | symbols), [block] (k_small_dec; g_maps: k_huff_big_dec_map too, its member's scratch)
    uint32_t out_max, pad_[3];    // batch: bytes the member's output slot takes (k_small_dec: SMALL_MAX)
    uint16_t child[256];      // [2 * node + bit]: 0x8000 | byte for a leaf, else the internal node
};
static_assert(sizeof(SmallDecArgs) % 16 == 0, "a batch table entry is copied in dwords and the next one starts 16-aligned");
// The header parsed, the tree built and the kernel's view of the stream (huff_small.hip).  `lanes`: subsequences the kernel has at most, of
// at most s_max bits.  1 = not for the lane-map decoder (the caller takes the general one, which also words the errors).
// wide: the limits of the tiled class instead (huff_parse_small.h: PARSE_STREAM_MAX_WIDE, PARSE_OUT_MAX_WIDE, counts below PLAN_COUNT_LIMIT_WIDE).
int small_dec_plan(const uint8_t *in, size_t n, uint32_t lanes, uint32_t s_max, SmallDecArgs &a, size_t *A0, unsigned long long *expect_out, bool wide = false);

// ---- the decoding classes (huff_small.hip's k_huff_batch_dec, huff_mid.hip's k_huff_mid_dec) differ in what one workgroup holds and in the
// launch: the plan in front of the packer and the packing itself are huff_dec_run's (huff_small.hip; run_groups, group_run.h).
struct HuffDecShape {
    uint32_t lanes, s_max;                         // subsequences of one workgroup; bits of one at most
    uint32_t pay_max, out_max;                     // payload bytes / decoded bytes of a member at most
};
using HuffDecLaunch = std::function<int(Ctx &c, hipStream_t s, uint32_t members, const SmallDecArgs *tab)>;   // (a class's function, or the tiled class's three launches with their grid)
int huff_dec_run(Ctx &c, const HuffDecShape &shape, const HuffDecLaunch &launch, const std::vector<size_t> &idx, const uint8_t *const *ins, const size_t *lens,
                 const SmallTake &take, std::vector<size_t> &back, size_t *failed);
// The same classes on device buffers (huff_dev.hip): the members idx[k] of `mem`, every one with a planned summary that the class's
// takes_plan has accepted (asked again here, up front), through the one driver of groups on device staging (group_run.h:
// run_groups_staged) as the decoders' family -- a gather kernel copies each stream from its 4-byte boundary into its input slot and
// completes its SmallDecArgs from the plan table, the decoder is launched unchanged, and a scatter kernel copies what fits to d_out and
// turns the decoder's two status words into the answer: GROUP_BACK, or the decoded length.
// group_bytes: the staging of a group at most (a class whose members are large states a larger group of its own: huff_big_dec.hip).
int huff_dec_run_dev(Ctx &c, hipStream_t s, const HuffDecShape &shape, const HuffDecLaunch &launch, const std::vector<size_t> &idx, const rsn_dev_member *mem,
                     const DevPlans &plans, std::vector<uint32_t> &answers, size_t group_bytes = SMALL_GROUP_BYTES);
// What a stream's header promises, from a scan that allocates nothing (huff_mid.hip: the classes' takes() run it for every member of a
// batch): the payload behind "\\\n" and the pad byte, and the sum of the counts -- an upper bound that is exact for every header an
// encoder writes.  pay_open (may be null): asked with the payload before the counts are scanned; false ends the scan.  false: no separator.
bool huff_dec_promise(const uint8_t *in, size_t n, size_t *pay, unsigned long long *expect, bool (*pay_open)(size_t pay) = nullptr);
// what a decoding class asks of a planned stream beside its own cutoffs: its lanes hold the code bits
inline bool huff_dec_shape_takes(const HuffDecShape &shape, const HuffDevSummary &sum) {
    uint32_t S, T;
    return sum.expect <= shape.out_max && (sum.span + 7) / 8 <= shape.pay_max && parse_lanes(sum.span, shape.lanes, shape.s_max, &S, &T);
}

namespace {

constexpr uint32_t HDR_MAX = HUFF_HDR_MAX;
constexpr uint32_t DEC_STREAM_MAX = 65536 + 2048;   // bytes of a stream the decoder takes
constexpr int DEC_K = 9;                        // index bits of the decoder's table, at most (every block builds the table: 11 bits cost 2 us more than they save on 64 KiB)
constexpr int DEC_ROUNDS = 64;                  // rounds of the synchronisation before the general decoder is asked instead

// what a block's word holds until its last act (block_dev.h: block_done)
constexpr uint32_t FLAG_PENDING = 0xFFFFFFFFu;
static_assert(FLAG_PENDING == GROUP_PENDING, "flags_wait and group_wait poll the decoder's words too");

template <int WAVES>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *s_wave /*[WAVES + 1]*/) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d, 64); if (lane >= (uint32_t)d) inc += o; }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) { uint32_t acc = 0; for (int w = 0; w < WAVES; w++) { const uint32_t t = s_wave[w]; s_wave[w] = acc; acc += t; } s_wave[WAVES] = acc; }
    __syncthreads();
    return s_wave[wave] + inc - v;
}

// a 16-byte unit as loaded, of which the first `keep` bytes are the member's (16 or more: all): zeros from byte `keep` on
__device__ __forceinline__ uint4 unit_head(uint4 v, uint32_t keep) {
    if (keep >= 16) return v;
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        const uint32_t mine = keep > 4 * k ? min(keep - 4 * k, 4u) : 0u;
        w[k] = mine == 4 ? w[k] : mine == 0 ? 0u : w[k] & ((1u << (8 * mine)) - 1);
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// ---------------------------------------------------------------- decompress (huffman.go:131-153,258-297)
// The payload is one bit string without an index: a lane that takes the subsequence [lo, lo + S) does not know where its first codeword
// starts.  It starts at lo and trusts the code to synchronise; the lane before tells it where it really ended, the lane redoes its
// subsequence from there, and so on until nothing changes.  On most data two rounds settle it.  On PERIODIC data (the README's samiam.txt
// repeated to 64 KiB is that) a wrong start can stay a wrong parse for kilobytes -- a second phase the code is just as happy in -- and
// "redo from the predecessor's exit" then walks the stretch one lane a round (r05, first version: one block, 52 rounds, 48 of its 94 us).
// So a lane keeps a small MAP instead of one answer: for every start a predecessor might hand it (at most four), where it ends and how many
// symbols it takes.  A round only adds the starts not seen before -- with two phases every lane has both after two rounds, whoever is
// right -- and when no lane learns a new start the true path is a composition of the maps along the lanes (a wavefront scan).
// One CU decodes 64 KiB in 12 us a pass however it is arranged, so the lanes are spread over up to 16 BLOCKS, and the blocks must not wait
// for each other round by round: a block's FIRST lane answers all 32 starts its subsequence could be entered at (32 lanes, one each), the
// block composes its lanes into a map "entered at c -> left at c', n symbols", publishes it, and only then looks at the blocks before it
// (their maps, composed, give its true entry and its first output byte).  One wait per call, behind work that every block does alone.
constexpr int DL = 256;                          // lanes per block that take a subsequence
constexpr int DT = DL + 64;                      // ... and a fifth wavefront: the 32 entries of the block's first lane, beside the others' first guesses
constexpr uint32_t DEC_BLOCKS = 32;
constexpr uint32_t DEC_S_MAX = 96;               // bits per lane at most: (64 KiB + 2 KiB) * 8 / 8192 lanes, in whole words (at least 64: an exit lies within 32 bits of the next lane's first)
constexpr uint32_t DEC_PAY_WORDS = DL * DEC_S_MAX / 32 + 8;
constexpr uint32_t DEC_OUT_CAP = 32768;          // bytes one block may produce (text: 256 lanes * 96 bits / 3 bits = 8 KiB)
// what one workgroup of k_huff_batch_dec holds (huff_small.hip): 256 lanes of at most HB_S_MAX bits, HB_OUT_MAX decoded bytes
constexpr uint32_t HB_S_MAX = 512;
constexpr uint32_t HB_PAY_MAX = DL * HB_S_MAX / 8;              // 16384 bytes of payload (behind the header's "\\\n" and the pad byte)
constexpr uint32_t HB_OUT_MAX = 32768;                          // bytes of output
constexpr uint32_t OFF_BAD = 0xFF;               // an exit that is none: the path ran off the payload (or the entry cannot occur)


// a reader of the big-endian words in LDS: the next bits left-aligned in a register, a word fetched for every 32 consumed
struct BitReader {
    const uint32_t *pay; unsigned long long buf; uint32_t pos, nextw; int avail;
    __device__ __forceinline__ void seek(uint32_t p) {
        const uint32_t w = p >> 5, o = p & 31;
        buf = (((unsigned long long)pay[w] << 32) | pay[w + 1]) << o;
        avail = 64 - (int)o; nextw = w + 2; pos = p;
    }
    __device__ __forceinline__ void skip(uint32_t l) {
        buf <<= l; avail -= (int)l; pos += l;
        if (avail < 32) { buf |= (unsigned long long)pay[nextw++] << (32 - avail); avail += 32; }
    }
};
struct DecTab { const uint32_t *lut; const uint16_t *child; uint32_t K, end; };
// the codeword at the reader's position: its byte; the reader moves behind it (past `end`: the caller's to notice)
// (an entry of the table: one codeword or two, see the kernel's table walk)
__device__ __forceinline__ uint32_t ent_len1(uint32_t e) { return (e >> 16) & 31u; }
__device__ __forceinline__ uint32_t ent_len2(uint32_t e) { return (e >> 21) & 31u; }
__device__ __forceinline__ bool ent_two(uint32_t e) { return (e >> 26) & 1u; }
// a codeword longer than the table's K bits, from the internal node its first K bits lead to
__device__ __forceinline__ uint32_t dec_long(BitReader &r, const DecTab &t, uint32_t e) {
    uint32_t node = e & 0xFFFF;
    r.skip(t.K);
    for (;;) {
        const uint32_t bit = (uint32_t)(r.buf >> 63);
        r.skip(1);
        node = t.child[2 * node + bit];
        if ((node & 0x8000) || r.pos > t.end + 64) break;             // (garbage behind the end: stop)
    }
    return node & 0xFF;
}

// The kernel is launched for a few microseconds of work on CUs whose instruction caches are cold: its time is its CODE SIZE (r05: the
// first multi-block version, every loop inlined wherever it was used -- 36 KB of instructions, 56 us; the arithmetic is two).  So the two
// loops that walk codewords exist ONCE, as functions.
// the codewords that start in [from, hi): exit offset (from hi; OFF_BAD: the path ran off the payload) << 24 | their number
__device__ __noinline__ uint32_t run_path(const uint32_t *pay, const uint32_t *lut, const uint16_t *child, uint32_t K, uint32_t end, uint32_t from, uint32_t hi) {
    const DecTab tab{lut, child, K, end};
    BitReader r; r.pay = pay; r.seek(from);
    uint32_t c = 0;
    while (r.pos < hi) {
        const uint32_t e = lut[(uint32_t)(r.buf >> (64 - K))];
        if (e >> 31) { (void)dec_long(r, tab, e); c++; }
        else if (ent_two(e) && r.pos + ent_len1(e) < hi) { r.skip(ent_len2(e)); c += 2; }     // (the second one starts in this subsequence too)
        else { r.skip(ent_len1(e)); c++; }
        if (r.pos > end) break;
    }
    return (r.pos > end ? OFF_BAD : r.pos - hi) << 24 | c;
}
// `count` codewords from `from`, their bytes to out[0 ..)
__device__ __noinline__ void emit_path(const uint32_t *pay, const uint32_t *lut, const uint16_t *child, uint32_t K, uint32_t end, uint32_t from, uint32_t count, uint8_t *out) {
    const DecTab tab{lut, child, K, end};
    BitReader r; r.pay = pay; r.seek(from);
    for (uint32_t i = 0; i < count;) {
        const uint32_t e = lut[(uint32_t)(r.buf >> (64 - K))];
        if (e >> 31) out[i++] = (uint8_t)dec_long(r, tab, e);
        else if (ent_two(e) && i + 1 < count) { out[i] = (uint8_t)e; out[i + 1] = (uint8_t)(e >> 8); i += 2; r.skip(ent_len2(e)); }
        else { out[i++] = (uint8_t)e; r.skip(ent_len1(e)); }
    }
}
__device__ __forceinline__ uint32_t byte_of(uint32_t packed, uint32_t j) { return (packed >> (8 * j)) & 0xFF; }
// The decoder of one block.  MULTI: k_small_dec's up to DEC_BLOCKS blocks of one stream, each waiting for the maps of the blocks before it
// (they are co-resident: 32 blocks).  !MULTI: the whole stream in this one block, which waits for nobody -- the batch kernel's member.
// PAY_WORDS / OUT_CAP: the stream words and the output bytes one block holds in LDS.
// What the rune decoder (huff_rune_dec.hip) needs beside that: CHILD_MAX entries of `child` (the byte alphabets' 256 are a.child; a tree of
// 256 leaves has 510) and !STORE -- the decoded symbols stay in s_out[0 ..) for the caller, nothing is stored to a.hout and no status word
// is written.  Returns the symbols this block decoded, DEC_BODY_BACK where the stream is not for the lane maps (STORE: status 1 is out).
// TILE (huff_big_dec.hip: the MULTI form's two halves as two launches, so that no block waits for another; MULTI is set, block b is tile b
// of a stream whose tiles need not be co-resident).  TILE_MAP: the body up to the publication -- the tile's 32-entry map is stored to
// a.g_maps[b * 32 ..) and nothing else is.  TILE_EMIT: the body behind the wait -- the tile's true entry and its first output byte are
// given (a kernel between the two has composed the maps), only that entry of the first lane is answered, the bytes [tile_base, tile_base +
// count) are stored to a.hout and no status word is: a.out_max bounds the output as it does where one block holds the stream.
constexpr uint32_t DEC_BODY_BACK = 0xFFFFFFFFu;
constexpr int TILE_NONE = 0, TILE_MAP = 1, TILE_EMIT = 2;
template <uint32_t PAY_WORDS, uint32_t OUT_CAP, bool MULTI, int DLN, uint32_t CHILD_MAX, bool STORE, int TILE = TILE_NONE>
__device__ __forceinline__ uint32_t lane_dec_body(const SmallDecArgs &a, const uint16_t *child /*[a.n_child]*/, uint32_t *s_pay /*[PAY_WORDS]*/, uint8_t *s_out /*[OUT_CAP + 32], 16-aligned*/,
                                                  uint32_t tile_entry = 0, uint32_t tile_base = 0) {
    constexpr int DTN = DLN + 64;                             // the lanes and the wavefront of the block's first lane
    constexpr int PERC = (CHILD_MAX + DTN - 1) / DTN;         // entries of child[] a thread loads
    static_assert(STORE || !MULTI || TILE == TILE_MAP, "the symbols stay in LDS only where one block holds the whole stream");
    static_assert(TILE == TILE_NONE || MULTI, "a tile is a block of a stream of many");
    __shared__ uint32_t s_lut[1u << DEC_K];                   // byte | second byte << 8 | length << 16 | length of both << 21 | two << 26, or 0x80000000 | internal node reached after K bits
    __shared__ uint16_t s_child[CHILD_MAX];
    __shared__ uint32_t s_st[DLN], s_ex[DLN], s_n[DLN];          // per lane: its starts (offsets from its subsequence's first bit, a byte each), the exits that belong to them (offsets from the next subsequence's first bit), their number
    __shared__ uint32_t s_exmask;                             // ... the exits that occur among them, a bit each
    __shared__ uint32_t s_ex32[32], s_cn32[32];               // the block's first lane: exit and symbols for every start in its first 32 bits
    __shared__ uint32_t s_wto[DLN / 64 + 1], s_wc[DLN / 64 + 1][4];                 // the wavefronts' maps
    __shared__ uint32_t s_blk[4][2];                          // entry j of lane 1 -> (exit of the block's last lane, symbols of lanes 1..)
    __shared__ uint32_t s_all[MULTI && TILE == TILE_NONE ? DEC_BLOCKS * 32 : 1];   // the maps of the blocks before this one
    __shared__ uint32_t s_true[3];                            // this block's true entry (a start of its first lane), its first output byte, a failure
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = MULTI ? blockIdx.x : 0u, n_blk = MULTI ? gridDim.x : 1u;
    const uint32_t S = a.S;
    const uint32_t blk_lo = a.p0 + b * DLN * S;                                   // this block's first bit
    const uint32_t wlo = blk_lo >> 5;                                           // ... the word it is in: bit positions below are counted from it
    const uint32_t n_words = DLN * S / 32 + 6;
    {   // every load of the staging in flight at once (the bytes are in host memory, a round trip is microseconds); the table meanwhile
        constexpr int PER = (PAY_WORDS + DTN - 1) / DTN;
        uint32_t v[PER];
        uint32_t ch[PERC];                                                     // (asked for first: the table is built while the stream's words are on their way)
#pragma unroll
        for (int k = 0; k < PERC; k++) { const uint32_t i = tid + k * DTN; ch[k] = i < a.n_child ? child[i] : 0u; }
#pragma unroll
        for (int k = 0; k < PER; k++) { const uint32_t i = tid + k * DTN; v[k] = (i < n_words && wlo + i < a.pay_words) ? a.pay[wlo + i] : 0u; }
#pragma unroll
        for (int k = 0; k < PERC; k++) { const uint32_t i = tid + k * DTN; if (i < a.n_child) s_child[i] = (uint16_t)ch[k]; }
        __syncthreads();
        // window v of K bits: down the tree from the root, two windows a lane at a time (the steps depend on each other, the windows do
        // not); a leaf met with bits to spare sends the walk back to the root for a SECOND codeword: an entry holds up to two
        constexpr int G = 2;
        for (uint32_t v0 = tid * G; v0 < (1u << a.K); v0 += DTN * G) {
            uint32_t node[G], ent[G], got[G];
#pragma unroll
            for (int q = 0; q < G; q++) { node[q] = a.root; ent[q] = 0; got[q] = 0; }
            for (uint32_t d = 0; d < a.K; d++) {
#pragma unroll
                for (int q = 0; q < G; q++) {
                    if (got[q] == 2) continue;
                    const uint32_t bit = ((v0 + q) >> (a.K - 1 - d)) & 1;
                    node[q] = s_child[2 * node[q] + bit];
                    if (node[q] & 0x8000) {
                        if (got[q] == 0) ent[q] = (node[q] & 0xFF) | (d + 1) << 16;                     // byte, length
                        else ent[q] |= (node[q] & 0xFF) << 8 | (d + 1) << 21 | 1u << 26;             // second byte, length of both, "two"
                        got[q]++;
                        node[q] = a.root;
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < G; q++) if (v0 + q < (1u << a.K)) s_lut[v0 + q] = got[q] ? ent[q] : (0x80000000u | node[q]);
        }
#pragma unroll
        for (int k = 0; k < PER; k++) { const uint32_t i = tid + k * DTN; if (i < n_words + 2) s_pay[i] = i < n_words ? __builtin_bswap32(v[k]) : 0u; }
    }
    if (tid < 32) { s_ex32[tid] = OFF_BAD; s_cn32[tid] = 0; }
    if (tid == 0) s_exmask = 0;
    __syncthreads();
    const uint32_t base_bit = wlo << 5;
    const uint32_t end = a.end - base_bit;                                      // (all positions from here on: bits from s_pay[0])
    const uint32_t g = b * DLN + tid;                                            // the lane's subsequence
    const uint32_t L = min((uint32_t)DLN, a.T - b * DLN);                         // lanes of this block that have one
    const bool real = tid < L;                                                  // (the fifth wavefront's lanes: none)
    const uint32_t my_lo = blk_lo - base_bit + tid * S;
    const uint32_t my_hi = min(end, my_lo + S);                                 // (the next lane's first bit; the stream's last lane: the end)
    auto run_in = [&](uint32_t lo, uint32_t hi, uint32_t off, uint32_t &exit_off, uint32_t &count) {   // the codewords that start in [lo + off, hi)
        const uint32_t r = run_path(s_pay, s_lut, s_child, a.K, end, lo + off, hi);
        exit_off = r >> 24; count = r & 0xFFFFFFu;
    };
    // ---- the block's first lane, entered at every bit a codeword could start at (block 0: at the stream's first code bit, nowhere else)
    const uint32_t flat0 = a.flat ? (a.flat - (b * DLN * S) % a.flat) % a.flat : 0u;      // flat code: the one bit this block can be entered at
    if (tid >= DLN && tid < DLN + 32 && (TILE == TILE_EMIT ? (uint32_t)(tid - DLN) == tile_entry : b == 0 ? tid == DLN : (a.flat == 0 || (uint32_t)(tid - DLN) == flat0))) {
        const uint32_t hi0 = min(end, blk_lo - base_bit + S);
        uint32_t e, c;
        run_in(blk_lo - base_bit, hi0, tid - DLN, e, c);
        s_ex32[tid - DLN] = e; s_cn32[tid - DLN] = c;
        if (e < 32) atomicOr(&s_exmask, 1u << e);
    }
    uint32_t st[4] = {0, 0, 0, 0}, ex[4] = {OFF_BAD, OFF_BAD, OFF_BAD, OFF_BAD}, cn[4] = {0, 0, 0, 0}, n_ent = 0;
    auto add = [&](uint32_t off) {                                              // (n_ent < 4)
        uint32_t e, c;
        run_in(my_lo, my_hi, off, e, c);
#pragma unroll
        for (int j = 0; j < 4; j++) if ((uint32_t)j == n_ent) { st[j] = off; ex[j] = e; cn[j] = c; }
        n_ent++;
    };
    auto publish = [&] {
        s_st[tid] = st[0] | st[1] << 8 | st[2] << 16 | st[3] << 24;
        s_ex[tid] = ex[0] | ex[1] << 8 | ex[2] << 16 | ex[3] << 24;
        s_n[tid] = n_ent;
    };
    const bool chained = real && tid >= 1;                                      // lanes 1.. learn their starts from the lane before
    if (chained) add(a.flat ? (a.flat - (g * S) % a.flat) % a.flat : 0u);        // a first guess: the subsequence's first bit (flat code: the first boundary in it)
    if (tid < DLN) publish();
    bool lost = false;
    for (int round = 0;; round++) {
        __syncthreads();
        uint32_t fresh[4], n_fresh = 0;
        bool over = false;
        auto offer = [&](uint32_t off) {
            if (off == OFF_BAD) return;
            bool seen = false;
#pragma unroll
            for (int k = 0; k < 4; k++) seen |= ((uint32_t)k < n_ent && st[k] == off) || ((uint32_t)k < n_fresh && fresh[k] == off);
            if (seen) return;
            if (n_ent + n_fresh >= 4) { over = true; return; }
#pragma unroll
            for (int k = 0; k < 4; k++) if ((uint32_t)k == n_fresh) fresh[k] = off;
            n_fresh++;
        };
        if (chained && tid == 1) { for (uint32_t mk = s_exmask; mk; mk &= mk - 1) offer((uint32_t)__builtin_ctz(mk)); }
        else if (chained) {
            const uint32_t pe = s_ex[tid - 1], pn = s_n[tid - 1];
#pragma unroll
            for (int j = 0; j < 4; j++) if ((uint32_t)j < pn) offer(byte_of(pe, j));
        }
        __syncthreads();
#pragma unroll 1
        for (uint32_t k = 0; k < n_fresh; k++) add(k == 0 ? fresh[0] : k == 1 ? fresh[1] : k == 2 ? fresh[2] : fresh[3]);
        if (n_fresh) publish();                                                  // (only lanes 1 .. L - 1 ever have any)
        const int flags = __syncthreads_or((n_fresh ? 1 : 0) | (over ? 2 : 0));
        if (flags & 2) { lost = true; break; }                                  // more than four phases: the general decoder
        if (!flags) break;
        if (round >= DEC_ROUNDS) { lost = true; break; }
    }
    // ---- the lanes' maps composed: lane t's entry j leads to the entry of lane t + 1 whose start is j's exit
    PathMap m; m.to = PM_ID; m.c0 = m.c1 = m.c2 = m.c3 = 0;                     // (lane 0 and lanes without a subsequence: nothing)
    if (chained) {
        m.c0 = cn[0]; m.c1 = cn[1]; m.c2 = cn[2]; m.c3 = cn[3];
        if (tid + 1 < L) {
            const uint32_t ns = s_st[tid + 1], nn = s_n[tid + 1];
            m.to = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint32_t to = 7;
#pragma unroll
                for (int k = 0; k < 4; k++) if ((uint32_t)j < n_ent && (uint32_t)k < nn && ex[j] != OFF_BAD && byte_of(ns, k) == ex[j]) to = k;
                m.to |= to << (3 * j);
            }
        } else {                                                                // the block's last lane: its entries stay as they are (their exits are read below)
            m.to = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) m.to |= ((uint32_t)j < n_ent ? (uint32_t)j : 7u) << (3 * j);
        }
    }
    PathMap inc = m;                                                            // this wavefront's lanes up to and including this one
#pragma unroll 1
    for (int d = 1; d < 64; d <<= 1) { const PathMap o = pm_shfl_up(inc, d); if (lane >= (uint32_t)d) inc = pm_then(o, inc); }
    if (lane == 63) { s_wto[wave] = inc.to; s_wc[wave][0] = inc.c0; s_wc[wave][1] = inc.c1; s_wc[wave][2] = inc.c2; s_wc[wave][3] = inc.c3; }
    __syncthreads();
    if (tid == 0) {
        PathMap acc; acc.to = PM_ID; acc.c0 = acc.c1 = acc.c2 = acc.c3 = 0;
#pragma unroll 1
        for (int w = 0; w < DLN / 64; w++) {
            PathMap t; t.to = s_wto[w]; t.c0 = s_wc[w][0]; t.c1 = s_wc[w][1]; t.c2 = s_wc[w][2]; t.c3 = s_wc[w][3];
            s_wto[w] = acc.to; s_wc[w][0] = acc.c0; s_wc[w][1] = acc.c1; s_wc[w][2] = acc.c2; s_wc[w][3] = acc.c3;
            acc = pm_then(acc, t);
        }
    }
    __syncthreads();
    PathMap before; before.to = s_wto[wave]; before.c0 = s_wc[wave][0]; before.c1 = s_wc[wave][1]; before.c2 = s_wc[wave][2]; before.c3 = s_wc[wave][3];
    {
        const PathMap prev = pm_shfl_up(inc, 1);                                // (the lanes before this one, within the wavefront)
        if (lane) before = pm_then(before, prev);                               // entry j of lane 1 -> (entry of THIS lane, symbols of lanes 1 .. this - 1)
    }
    if (real && tid + 1 == L && L > 1) {                                        // the block's last lane: where every entry of lane 1 leaves the block
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t idx = pm_to(before, j);
            uint32_t e = OFF_BAD, c = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) if ((uint32_t)k == idx && idx < n_ent) { e = ex[k]; c = pm_c(before, j) + cn[k]; }
            s_blk[j][0] = e; s_blk[j][1] = c;
        }
    }
    __syncthreads();
    // ---- the block's map out, the earlier blocks' maps in
    auto lane1_index = [&](uint32_t off) -> uint32_t {                          // which entry of lane 1 starts at `off`
        const uint32_t s1 = s_st[1], n1 = s_n[1];
        uint32_t j = 7;
#pragma unroll
        for (int k = 0; k < 4; k++) if ((uint32_t)k < n1 && byte_of(s1, k) == off) j = k;
        return j;
    };
    if constexpr (MULTI && TILE != TILE_EMIT) {                                 // (one block alone: entered at its first bit, nothing to publish or wait for)
        if (tid < 32) {
            uint32_t e = s_ex32[tid], c = s_cn32[tid];
            if (L > 1 && e != OFF_BAD) { const uint32_t j = lane1_index(e); if (j < 4) { c += s_blk[j][1]; e = s_blk[j][0]; } else e = OFF_BAD; }
            if (lost) e = OFF_BAD;
            a.g_maps[b * 32 + tid] = e << 24 | (c & 0xFFFFFFu);
        }
        if constexpr (TILE == TILE_MAP) return 0;                               // (the launch's end publishes it)
        __threadfence();
        __syncthreads();
        if (tid == 0) {
            __hip_atomic_store(&a.g_flags[b], a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            for (uint32_t i = 0; i < b; i++) while (__hip_atomic_load(&a.g_flags[i], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != a.seq) __builtin_amdgcn_s_sleep(1);
        }
        __syncthreads();
        for (uint32_t i = tid; i < b * 32; i += DTN) s_all[i] = __hip_atomic_load(&a.g_maps[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
    }
    if (tid == 0) {
        uint32_t c = TILE ? tile_entry : 0u, base = TILE ? tile_base : 0u, fail = lost ? 1u : 0u;   // (block 0 is entered at its first bit)
        for (uint32_t i = 0; TILE == TILE_NONE && i < b && !fail; i++) {
            const uint32_t e = s_all[i * 32 + c];
            if ((e >> 24) == OFF_BAD || (e >> 24) >= 32) { fail = 1; break; }
            base += e & 0xFFFFFFu; c = e >> 24;
        }
        s_true[0] = c; s_true[1] = base; s_true[2] = fail;
    }
    __syncthreads();
    const uint32_t c_in = s_true[0], out_base = s_true[1];
    bool fail = s_true[2] != 0;
    // ---- the true path through this block
    uint32_t my_start = 0, my_cnt = 0, my_at = 0, my_exit = OFF_BAD;            // (my_at: symbols of this block before this lane's)
    if (!fail) {
        const uint32_t e0 = s_ex32[c_in];
        if (tid == 0) { my_start = c_in; my_cnt = s_cn32[c_in]; my_exit = e0; }
        else if (chained) {
            const uint32_t j1 = e0 == OFF_BAD ? 7u : lane1_index(e0);
            const uint32_t idx = pm_to(before, j1);
            my_at = s_cn32[c_in] + (j1 < 4 ? pm_c(before, j1) : 0u);
#pragma unroll
            for (int k = 0; k < 4; k++) if ((uint32_t)k == idx && idx < n_ent) { my_start = st[k]; my_cnt = cn[k]; my_exit = ex[k]; }
        }
    }
    const bool is_last_lane = real && g + 1 == a.T;
    const bool broken = !fail && real && (my_exit == OFF_BAD || (is_last_lane && my_exit != 0));   // off the payload, or the stream ends inside a codeword
    const uint32_t blk_cnt_hint = (real && tid + 1 == L) ? my_at + my_cnt : 0u;
    const int bad = __syncthreads_or((broken || fail) ? 1 : 0);
    if (real && tid + 1 == L) s_true[0] = blk_cnt_hint;
    __syncthreads();
    const uint32_t blk_cnt = s_true[0];
    if (bad || blk_cnt + (MULTI ? 16u : 0u) > OUT_CAP || out_base + blk_cnt > (MULTI && TILE == TILE_NONE ? SMALL_MAX : a.out_max)) {
        if constexpr (STORE && TILE == TILE_NONE) block_done(&a.status[b], 1);
        return DEC_BODY_BACK;
    }
    const uint32_t shift = out_base & 15;                                       // LDS byte i + shift <-> output byte out_base + i: 16-byte units line up
    if (real) emit_path(s_pay, s_lut, s_child, a.K, end, my_lo + my_start, my_cnt, s_out + my_at + shift);
    __syncthreads();
    if constexpr (STORE) {   // whole 16-byte units as they are; the first and the last are shared with the neighbours: their bytes one by one
        const uint32_t lo = shift, hi = shift + blk_cnt;                        // LDS byte range
        uint8_t *dst = a.hout + (out_base - shift);
        for (uint32_t u = tid; u * 16 < hi; u += DTN) {
            const uint32_t u0 = u * 16, u1 = u0 + 16;
            if (u0 >= lo && u1 <= hi) *reinterpret_cast<uint4 *>(dst + u0) = *reinterpret_cast<const uint4 *>(s_out + u0);
            else for (uint32_t x = max(u0, lo); x < min(u1, hi); x++) dst[x] = s_out[x];
        }
        if constexpr (TILE == TILE_NONE) {
            if (tid == 0 && b + 1 == n_blk) a.status[MULTI ? DEC_BLOCKS : 1u] = out_base + blk_cnt;
            block_done(&a.status[b], 0);
        }
    }
    return blk_cnt;
}
// the byte alphabets' decoder: the tree in the arguments, the bytes to a.hout, the status words written
template <uint32_t PAY_WORDS, uint32_t OUT_CAP, bool MULTI, int DLN>
__device__ __forceinline__ void small_dec_body(const SmallDecArgs &a, uint32_t *s_pay /*[PAY_WORDS]*/, uint8_t *s_out /*[OUT_CAP + 32], 16-aligned*/) {
    (void)lane_dec_body<PAY_WORDS, OUT_CAP, MULTI, DLN, 256, true>(a, a.child, s_pay, s_out);
}

// ---------------------------------------------------------------- compress, many members in one launch (the batch call)
// ONE block per member, whatever the grid, and nothing on the host between the histogram and the emit: the block loads its member (a
// SmallMember entry in pinned memory: where its bytes, its output slot and its status word are) into LDS once and counts it there, ranks
// the leaves, and ONE wavefront builds the Go-exact tree and codes (wave_tree below) with the heap, the children and the codes held in
// VGPRs, a slot per lane: a read is a readlane, a write a select in the one lane, both at a wave-uniform index.  The other wavefronts wait; the header's entries are already in place (a scan of their lengths).  Then every
// byte's first bit is a block scan of the code lengths and the codes are ORed into an LDS image of the output words, as k_small_emit does.
// Status word: the stream's length, GROUP_BACK_RUNES -- a byte >= 0x80 (runes, huffman.go:309) -- or GROUP_BACK: fewer than two distinct bytes, a code beyond
// 24 bits or a header beyond HDR_MAX (none of the last two below the member cutoff: counts below 2^15 give codes of at most 20 bits).
constexpr uint32_t HE_IN_MAX = 16384;            // member cutoff: 128 symbols code at most 7 bits a byte, so at most 14 KiB of payload
constexpr uint32_t HE_T = 256;
constexpr uint32_t HE_IMG_WORDS = (HDR_MAX + HE_IN_MAX * 7 / 8 + 64) / 4;
static_assert(huff_small_enc_out_slot(HE_IN_MAX) / 4 >= HE_IMG_WORDS, "the image fits the largest member's slot");

// `R` VGPRs of a wavefront as 64 R slots (slot i: register i / 64 of lane i % 64); every index wave-uniform
template <int R>
struct LaneStore {
    uint32_t r[R];
    __device__ __forceinline__ uint32_t get(uint32_t i) const {
        const uint32_t q = i >> 6, l = i & 63;
        uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)r[0], (int)l);
#pragma unroll
        for (int k = 1; k < R; k++) { const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)r[k], (int)l); v = q == (uint32_t)k ? w : v; }
        return v;
    }
    __device__ __forceinline__ void set(uint32_t i, uint32_t v) {              // (a compare and a select: lane i % 64 takes v)
        const uint32_t q = i >> 6, l = i & 63, me = __lane_id();
#pragma unroll
        for (int k = 0; k < R; k++) if (q == (uint32_t)k && me == l) r[k] = v;
    }
};

// The Go-exact tree and codes in ONE wavefront's VGPRs (huff_plan_small.h: plan_tree and plan_codes, the code the CPU tests hold against
// huff_host.cpp): the `a` leaves in rank order with their counts in s_lf[0 .. a), a wave-uniform and at most 64 R; the heap (64 R slots),
// the children (64 R - 1 pairs) and the codes (128 R - 1) in LaneStores.  IDB: bits of a node id (8 for the byte alphabets' R = 2,
// PLAN_RUNE_IDB for the runes' R = 4).  On return leaf l is lane l % 64 of code.r[l / 64], internal node a + k is lane k % 64 of
// kids.r[k / 64] (left | right << IDB).  Returns the root's id.  Every lane of the wavefront calls it; the other wavefronts wait.
template <uint32_t IDB, int R>
__device__ __forceinline__ uint32_t wave_tree(const uint32_t *s_lf, uint32_t a, LaneStore<R> &kids, LaneStore<2 * R> &code) {
    static_assert(128u * R <= (1u << IDB), "a node id has IDB bits");
    const uint32_t lane = threadIdx.x & 63;
    LaneStore<R> heap;
#pragma unroll
    for (int k = 0; k < R; k++) {
        const uint32_t l = lane + 64 * k;
        heap.r[k] = l < a ? plan_item<IDB>(s_lf[l], l) : 0u;
        kids.r[k] = 0;
    }
#pragma unroll
    for (int k = 0; k < 2 * R; k++) code.r[k] = 0;
    const uint32_t root = plan_tree<IDB>(a, heap, kids);
    plan_codes<IDB>(a, root, kids, code);
    return root;
}
// what the encoders take from it: leaf l's len << 24 | code to s_tab[s_at[l]], (deepest code, payload bits) to s_plan[0 .. 2)
template <int RC, class At>
__device__ __forceinline__ void wave_codes_out(const LaneStore<RC> &code, uint32_t a, const uint32_t *s_lf, const At *s_at, uint32_t *s_tab, uint32_t *s_plan) {
    const uint32_t lane = threadIdx.x & 63;
    uint32_t mx = 0, bits = 0;
#pragma unroll
    for (int k = 0; k < RC / 2; k++) {
        const uint32_t l = lane + 64 * k;
        if (l < a) { const uint32_t cd = code.r[k], len = cd >> 24; s_tab[s_at[l]] = cd; mx = max(mx, len); bits += s_lf[l] * len; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { mx = max(mx, (uint32_t)__shfl_xor((int)mx, d, 64)); bits += (uint32_t)__shfl_xor((int)bits, d, 64); }
    if (lane == 0) { s_plan[0] = mx; s_plan[1] = bits; }
}
// what the decoders' plans take from it: the shallowest and the deepest leaf, in every lane
template <int RC>
__device__ __forceinline__ void wave_depths(const LaneStore<RC> &code, uint32_t a, uint32_t *shallowest, uint32_t *deepest) {
    const uint32_t lane = threadIdx.x & 63;
    uint32_t mn = 255, mx = 0;
#pragma unroll
    for (int k = 0; k < RC / 2; k++) if (lane + 64 * k < a) { const uint32_t len = code.r[k] >> 24; mn = min(mn, len); mx = max(mx, len); }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { mn = min(mn, (uint32_t)__shfl_xor((int)mn, d, 64)); mx = max(mx, (uint32_t)__shfl_xor((int)mx, d, 64)); }
    *shallowest = mn; *deepest = mx;
}

// A lane's up to 16 codes (len << 24 | code, len <= 24; 0: none) into the image from bit pos0 on: MSB first, words byte-swapped; the
// lane's first and last words may be shared with its neighbours (LDS atomics), the words between are its own.
__device__ __forceinline__ void pack_codes16(const uint32_t e[16], uint32_t pos0, uint32_t *s_img) {
    uint32_t w = pos0 >> 5, nacc = pos0 & 31;
    unsigned long long acc = 0;
    bool first = true;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const uint32_t l = e[j] >> 24;
        if (l) acc |= (unsigned long long)(e[j] & 0xFFFFFFu) << (64 - nacc - l);
        nacc += l;
        if (nacc >= 32) {
            const uint32_t be = __builtin_bswap32((uint32_t)(acc >> 32));
            if (first) atomicOr(&s_img[w], be); else s_img[w] = be;
            first = false;
            w++; acc <<= 32; nacc -= 32;
        }
    }
    if (nacc) atomicOr(&s_img[w], __builtin_bswap32((uint32_t)(acc >> 32)));
}

// The encoder of one workgroup of T threads.  s_in: the member, IN_MAX bytes; s_img: the output, IMG_WORDS words -- header bytes, then the
// code bits (MSB first, words byte-swapped); slot(n): bytes of the output slot of a member of n bytes.  WIDE: the image leaves in 16-byte
// units (IMG_WORDS and the slot are whole units), else in words.
template <uint32_t T, uint32_t IN_MAX, uint32_t IMG_WORDS, bool WIDE, class Slot>
__device__ __forceinline__ void huff_enc_body(const SmallMember *__restrict__ tab, uint8_t *__restrict__ base, uint4 *s_in, uint32_t *s_img, Slot slot) {
    __shared__ uint32_t s_cnt[T / 64][128];
    __shared__ uint32_t s_tot[128], s_lf[128], s_tab[128];
    __shared__ uint8_t s_leaf[128];
    __shared__ uint32_t s_wave[T / 64 + 1];
    __shared__ uint32_t s_plan[2];                     // max code length, payload bits
    const SmallMember m = tab[blockIdx.x];
    uint32_t *status = reinterpret_cast<uint32_t *>(base + m.status_off);
    const uint32_t n = m.n, tid = threadIdx.x, wave = tid >> 6;
    if (n < 2 || n > IN_MAX) { block_done(status, GROUP_BACK); return; }    // (the host never sends one)
    for (uint32_t i = tid; i < T / 64 * 128; i += T) (&s_cnt[0][0])[i] = 0;
    for (uint32_t i = tid; i < IMG_WORDS; i += T) s_img[i] = 0;
    __syncthreads();
    // ---- the member into LDS, counted (huffman.go:306-311)
    const uint4 *hin = reinterpret_cast<const uint4 *>(base + m.in_off);
    uint32_t high = 0;
    for (uint32_t u = tid; u * 16 < n; u += T) {
        const uint4 v = hin[u];                                          // (pinned host memory; zero behind n)
        s_in[u] = v;
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        const uint32_t valid = min(16u, n - u * 16);
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t b = (w[j >> 2] >> (8 * (j & 3))) & 0xFF;
            if ((uint32_t)j < valid) { high |= b & 0x80; atomicAdd(&s_cnt[wave][b & 0x7F], 1u); }
        }
    }
    high = __syncthreads_or((int)high);
    uint32_t c = 0;
    if (tid < 128) {
        for (uint32_t w = 0; w < T / 64; w++) c += s_cnt[w][tid];
        s_tot[tid] = c;
    }
    const uint32_t a = (uint32_t)__syncthreads_count(tid < 128 && c != 0);
    if (high || a < 2) { block_done(status, high ? GROUP_BACK_RUNES : GROUP_BACK); return; }   // (runes: the rune encoder's, huff_rune.hip, when the call holds enough of them)
    // ---- leaves in (count asc, byte asc) order; the header's entries ascending by byte, '\\' first when it would be last (huffman.go:312-318)
    const bool above_bs = __syncthreads_or(tid > 0x5C && tid < 128 && c != 0);
    const bool bs_first = s_tot[0x5C] != 0 && !above_bs;
    const uint32_t e_len = tid < 128 && c ? plan_entry_len(c, tid) : 0u;
    if (tid < 128 && c) { const uint32_t r = plan_leaf_rank(s_tot, tid); s_lf[r] = c; s_leaf[r] = (uint8_t)tid; }
    uint32_t e_at = block_excl_scan<T / 64>(e_len, s_wave);
    const uint32_t E = s_wave[T / 64];                                // bytes of the entries
    if (bs_first) e_at = tid == 0x5C ? 0u : e_at + plan_entry_len(s_tot[0x5C], 0x5C);
    if (e_len && E + 3 <= HDR_MAX) plan_entry(c, tid, reinterpret_cast<uint8_t *>(s_img) + e_at);
    // ---- the tree and the codes: one wavefront (huffman.go:93-127)
    if (wave == 0) {
        const uint32_t au = (uint32_t)__builtin_amdgcn_readfirstlane((int)a);
        LaneStore<2> kids;
        LaneStore<4> code;
        wave_tree<8>(s_lf, au, kids, code);
        wave_codes_out(code, au, s_lf, s_leaf, s_tab, s_plan);
    }
    __syncthreads();
    const uint32_t max_len = s_plan[0], pay_bits = s_plan[1];
    const uint32_t H = E + 3, pad = (8 - pay_bits % 8) % 8;              // huffman.go:245-249
    const uint32_t total = H + (pay_bits + pad) / 8, out_words = (total + 3) / 4;
    if (max_len > 24 || H > HDR_MAX || out_words > IMG_WORDS || 4 * out_words > slot(n)) { block_done(status, GROUP_BACK); return; }
    if (tid == 0) {
        uint8_t *h = reinterpret_cast<uint8_t *>(s_img);
        h[E] = '\\'; h[E + 1] = '\n'; h[E + 2] = (uint8_t)pad;
    }
    // ---- the code bits: 16 bytes a lane, 16 T bytes a round; a lane's first and last words may be shared with its neighbours (LDS atomics)
    uint32_t at0 = 8 * H + pad;
    for (uint32_t r0 = 0; r0 < n; r0 += 16 * T) {
        const uint32_t lo = r0 + 16 * tid;
        const uint4 v = lo < n ? s_in[lo / 16] : make_uint4(0, 0, 0, 0);
        const uint32_t valid = lo < n ? min(16u, n - lo) : 0u;
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
        uint32_t e[16], bits = 0;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            e[j] = (uint32_t)j < valid ? s_tab[(w4[j >> 2] >> (8 * (j & 3))) & 0x7F] : 0u;
            bits += e[j] >> 24;
        }
        const uint32_t pos0 = at0 + block_excl_scan<T / 64>(bits, s_wave);
        at0 += s_wave[T / 64];
        if (bits) pack_codes16(e, pos0, s_img);
    }
    __syncthreads();
    if constexpr (WIDE) {
        uint4 *hout = reinterpret_cast<uint4 *>(base + m.out_off);
        for (uint32_t i = tid; i < (out_words + 3) / 4; i += T) hout[i] = reinterpret_cast<const uint4 *>(s_img)[i];
    } else {
        uint32_t *hout = reinterpret_cast<uint32_t *>(base + m.out_off);
        for (uint32_t i = tid; i < out_words; i += T) hout[i] = s_img[i];
    }
    block_done(status, total);
}

}  // namespace
}  // namespace rsn
