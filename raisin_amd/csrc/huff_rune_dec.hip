// huff_rune_dec.hip -- the grouped Huffman decoder for streams whose header names a rune >= 0x80: what k_huff_batch_rune_enc (huff_rune.hip)
// and the single call write for UTF-8 text and for bytes that are no UTF-8 at all (rsn_huffman_decompress_batch and its device, layered
// and round-trip forms).  The byte decoders' plans refuse such a stream; when a call holds HUFF_RUNE_DEC_GROUP_MIN of them they
// come here instead of taking the single call one by one: ONE launch per group, ONE workgroup of 320 threads per member, and the workgroup
// makes the plan itself -- the host form and the device form launch the same kernel and neither ships a tree:
//   header   rune_light_plan (huff_rune_dec_plan.h, k_huff_mid_rune_dec's too): the member's first min(n, PARSE_RUNE_SCAN_MAX) bytes into
//            LDS; the separator by a block-wide minimum; ONE lane's parse_rune_scan(...) puts the entries into an LDS table of
//            PARSE_RUNE_SLOTS slots, the encoder's hash -- a later entry for a rune finds its slot and replaces the count
//            (huff_parse_rune.h: the code the CPU test holds against parse_header);
//   tree     the symbols compacted, ranked a thread each (plan_rune_ranks over count + 1), and ONE wavefront builds the Go-exact tree of
//            2 to 256 leaves with the heap, the children and the depths in VGPRs through LaneStore, as the encoder does; the children
//            become child[] with a leaf's RANK where the byte decoders have its byte;
//   payload  lane_dec_body (huff_small_body.h): the byte decoders' lookup table, run_path / emit_path, four-entry maps and PathMap
//            composition, 256 lanes of at most 576 bits, with 510 entries of child[] and without its last store -- a leaf rank per symbol
//            stays in LDS;
//   expand   each thread takes a run of symbols, a block scan of utf8_len(leaf_rune[rank]) gives its first byte, every rune is written as
//            string(rune) into an LDS image, and the image leaves in whole 16-byte units inside the member's output slot.
// Status word: the decoded length in BYTES, or GROUP_BACK -- anything huff_parse_rune.h refuses, what lane_dec_body hands back (more than
// four phases, DEC_ROUNDS rounds, a path off the payload, a stream that ends inside a codeword), an output slot smaller than the header
// promises, and more decoded bytes than it promises.  Fewer is an answer.
// LDS: one block of 18464 B that is the header and the table, then the payload's words, then the output image (each dead before the next
// is written); the symbols 16416 B; the compacted symbols, leaves and child[] 5 KiB; lane_dec_body's own 6.6 KiB -- three workgroups to
// a CU's 160 KiB (DESIGN 4.7 has the compile remarks).
#include <iterator>

#include "huff_small_body.h"
#include "huff_parse_rune.h"
#include "huff_rune_dec_plan.h"

namespace rsn {
namespace {

static_assert(PARSE_RUNE_HDR_MAX == HUFF_RUNE_HDR_MAX && PARSE_RUNE_OUT_MAX == HUFF_RUNE_OUT_MAX && PARSE_RUNE_PAY_MAX == HUFF_RUNE_PAY_MAX &&
              PARSE_RUNE_STREAM_MAX == HUFF_RUNE_STREAM_MAX && PARSE_RUNE_SYMS_MAX == HUFF_RUNE_SYMS_MAX && PARSE_RUNE_LANES == (uint32_t)DL,
              "huff_parse_rune.h restates the class's limits without its headers");
constexpr int RD_T = DT;                                                       // lane_dec_body's threads: 256 lanes and the wavefront of the first lane
constexpr int RD_WAVES = RD_T / 64;
constexpr uint32_t RD_PAY_WORDS = DL * PARSE_RUNE_S_MAX / 32 + 8;
constexpr uint32_t RD_IMG_BYTES = HUFF_RUNE_OUT_MAX + 16;
constexpr uint32_t rd_max(uint32_t a, uint32_t b) { return a > b ? a : b; }
constexpr uint32_t RD_RAW_BYTES = (rd_max(rd_max(RD_PLAN_BYTES, RD_PAY_WORDS * 4), RD_IMG_BYTES) + 15) & ~15u;
static_assert(PARSE_RUNE_SLOTS <= 2 * RD_T && PARSE_RUNE_SYMS_MAX <= (uint32_t)RD_T, "two slots a thread, a thread a symbol");

__global__ __launch_bounds__(RD_T) void k_huff_batch_rune_dec(const SmallMember *__restrict__ tab, uint8_t *__restrict__ base) {
    __shared__ uint4 s_raw[RD_RAW_BYTES / 16];                      // the header and the table; then the payload's words; then the output image
    __shared__ __attribute__((aligned(16))) uint8_t s_sym[HUFF_RUNE_OUT_MAX + 32];   // a leaf rank per symbol
    __shared__ uint32_t s_rune[PARSE_RUNE_SYMS_MAX], s_rc1[PARSE_RUNE_SYMS_MAX];  // the symbols compacted, in slot order: rune, count + 1
    __shared__ uint32_t s_lf[PARSE_RUNE_SYMS_MAX], s_leaf_rune[PARSE_RUNE_SYMS_MAX];   // the leaves in (count asc, rune asc) order: count, rune
    __shared__ __attribute__((aligned(4))) uint16_t s_kid[PARSE_RUNE_CHILD_MAX + 2];
    __shared__ uint32_t s_wave[RD_WAVES + 1];
    __shared__ uint32_t s_w[W_WORDS];
    __shared__ SmallDecArgs s_a;
    const SmallMember m = tab[blockIdx.x];
    uint32_t *status = reinterpret_cast<uint32_t *>(base + m.status_off);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t *s_key = reinterpret_cast<uint32_t *>(s_raw) + RD_TABLE_AT / 4, *s_c1 = s_key + PARSE_RUNE_SLOTS;
    // every verdict below is the same for the whole workgroup: a hand-back is a return of all its threads
    HuffDevBounds b{};
    uint32_t S = 0, T = 0;
    if (!rune_light_plan<RD_T>(base + m.in_off, m.n, s_raw, s_key, s_c1, s_w, b, &S, &T)) { block_done(status, GROUP_BACK); return; }
    const uint32_t a = s_w[W_DISTINCT], expect = b.expect;
    if (huff_dec_out_slot(expect) > m.status_off - m.out_off) { block_done(status, GROUP_BACK); return; }   // (the host sized the slot from the same bytes: it holds)
    {   // the symbols side by side (two slots a thread), then ranked
        const uint32_t k0 = 2 * tid < PARSE_RUNE_SLOTS ? s_key[2 * tid] : PARSE_RUNE_EMPTY, k1 = 2 * tid < PARSE_RUNE_SLOTS ? s_key[2 * tid + 1] : PARSE_RUNE_EMPTY;
        uint32_t at = block_excl_scan<RD_WAVES>((uint32_t)(k0 != PARSE_RUNE_EMPTY) + (uint32_t)(k1 != PARSE_RUNE_EMPTY), s_wave);
        if (k0 != PARSE_RUNE_EMPTY) { s_rune[at] = k0; s_rc1[at] = s_c1[2 * tid]; at++; }
        if (k1 != PARSE_RUNE_EMPTY) { s_rune[at] = k1; s_rc1[at] = s_c1[2 * tid + 1]; }
    }
    __syncthreads();
    if (tid < a) {
        uint32_t lr, rr;
        plan_rune_ranks(s_rune, s_rc1, a, tid, &lr, &rr);
        s_lf[lr] = s_rc1[tid] - 1; s_leaf_rune[lr] = s_rune[tid];
    }
    __syncthreads();
    // ---- the tree, the depths and child[]: one wavefront, every index wave-uniform (huffman.go:93-127)
    if (wave == 0) {
        const uint32_t au = (uint32_t)__builtin_amdgcn_readfirstlane((int)a);
        LaneStore<4> kids;
        LaneStore<8> code;
        const uint32_t root = wave_tree<PLAN_RUNE_IDB>(s_lf, au, kids, code);
        uint32_t mn, mx;
        wave_depths(code, au, &mn, &mx);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t l = lane + 64 * k;                             // internal node l
            if (l + 1 < au) {
                s_kid[2 * l] = (uint16_t)parse_rune_child(kids.r[k] & ((1u << PLAN_RUNE_IDB) - 1), au);
                s_kid[2 * l + 1] = (uint16_t)parse_rune_child(kids.r[k] >> PLAN_RUNE_IDB, au);
            }
        }
        if (lane == 0) { s_w[W_ROOT] = root - au; s_w[W_MIN] = mn; s_w[W_MAX] = mx; }
    }
    __syncthreads();
    if (!parse_depths(s_w[W_MIN], s_w[W_MAX], b)) { block_done(status, GROUP_BACK); return; }
    if (tid == 0) {
        s_a.pay = reinterpret_cast<const uint32_t *>(base + m.in_off + b.A0);   // (A0 a multiple of 4, the slot 16-aligned, zeros behind the stream)
        s_a.pay_words = b.pay_words; s_a.p0 = b.p0; s_a.end = b.end;
        s_a.K = b.K; s_a.root = s_w[W_ROOT]; s_a.n_child = 2 * (a - 1);
        s_a.S = S; s_a.T = T; s_a.flat = b.flat; s_a.seq = 0;
        s_a.hout = nullptr; s_a.status = nullptr; s_a.g_maps = nullptr; s_a.g_flags = nullptr;
        s_a.out_max = HUFF_RUNE_OUT_MAX;
    }
    __syncthreads();                                                  // (the header and the table are dead: the payload's words take their place)
    const uint32_t n_sym = lane_dec_body<RD_PAY_WORDS, HUFF_RUNE_OUT_MAX, false, DL, PARSE_RUNE_CHILD_MAX + 2, false>(s_a, s_kid, reinterpret_cast<uint32_t *>(s_raw), s_sym);
    if (n_sym == DEC_BODY_BACK) { block_done(status, GROUP_BACK); return; }
    // ---- expand: a run of symbols a thread, their bytes' positions by a block scan, string(rune) into the image (the payload is dead)
    const uint32_t per = (n_sym + RD_T - 1) / RD_T, lo = min(tid * per, n_sym), hi = min(lo + per, n_sym);
    uint32_t bytes = 0;
    for (uint32_t i = lo; i < hi; i++) bytes += plan_rune_utf8_len(s_leaf_rune[s_sym[i]]);
    uint32_t at = block_excl_scan<RD_WAVES>(bytes, s_wave);
    const uint32_t total = s_wave[RD_WAVES];
    if (total == 0 || total > expect) { block_done(status, GROUP_BACK); return; }    // (more than the header promises: the single call's, as the byte decoders do with out_max)
    uint8_t *img = reinterpret_cast<uint8_t *>(s_raw);
    for (uint32_t i = lo; i < hi; i++) at += parse_rune_write(s_leaf_rune[s_sym[i]], img + at);
    __syncthreads();
    uint4 *hout = reinterpret_cast<uint4 *>(base + m.out_off);
    for (uint32_t u = tid; u * 16 < total; u += RD_T) hout[u] = s_raw[u];          // (total <= expect: inside the slot, huff_dec_out_slot(expect))
    block_done(status, total);
}

// ---- the device form's second plan launch (huff_rune_dec_plan.h: rune_plan_body), at this class's limits
__global__ __launch_bounds__(RP_T) void k_huff_dev_rune_plan(const PlanEntry *__restrict__ tab, HuffDevSummary *__restrict__ sums) { rune_plan_body<ParseRuneSmall>(tab, sums); }

int launch_rune_dec(Ctx &c, hipStream_t s, uint32_t g, const SmallMember *tab, uint8_t *base) {
    RSN_LAUNCH("huff_batch_rune_dec", k_huff_batch_rune_dec, dim3(g), dim3(RD_T), 0, s, tab, base);
    return RSN_OK;
}
const char *const RD_WHAT = "huffman batch decompress";

// The two offers (codecs.h: BehindClass; pool REST, so `rest` is the pool itself), huff_rune_select.h choosing.  The chosen run in the groups
// of the SmallMember classes, the input slot the whole stream, the output slot what the header promises.
int rune_dec_offer(Ctx &c, std::vector<size_t> &rest, std::vector<size_t> &, const uint8_t *const *ins, const size_t *lens, const SmallTake &take, size_t *failed) {
    const std::vector<size_t> cand = rune_dec_candidates(rest, [&](size_t i) { return lens[i] <= HUFF_RUNE_STREAM_MAX; });
    if (cand.empty()) return RSN_OK;
    std::vector<HuffDevSummary> sums;
    for (size_t i : cand) sums.push_back(parse_rune_light(ins[i], lens[i]));
    std::vector<size_t> idx, others = rest;                               // (`rest` stays as it is when the run fails)
    std::vector<uint32_t> expect;
    rune_dec_planned(cand, cand.size(), sums.data(), [&](size_t i) { return lens[i]; }, idx, expect);
    if (!rune_dec_leave(others, idx)) return RSN_OK;
    const int rc = run_member_groups(c, RD_WHAT, idx, ins, lens, [&](size_t k) { return huff_dec_in_slot(lens[idx[k]]); }, [&](size_t k) { return huff_dec_out_slot(expect[k]); },
        [&](hipStream_t s, uint32_t g, const SmallMember *tab, uint8_t *base) { return launch_rune_dec(c, s, g, tab, base); }, take, others, failed, nullptr);
    if (rc) return rc;
    std::sort(others.begin(), others.end());
    rest.swap(others);
    return RSN_OK;
}

int rune_dec_offer_dev(Ctx &c, hipStream_t s, std::vector<size_t> &rest, std::vector<size_t> &, const rsn_dev_member *mem, const DevPlans *plans,
                       std::vector<size_t> &idx, std::vector<uint32_t> &answers) {
    const std::vector<size_t> cand = rune_dec_candidates(rest, [&](size_t i) {
        const HuffDevSummary *v = plans->of(i);
        return v && v->verdict == PARSE_NOT_MINE && mem[i].n <= HUFF_RUNE_STREAM_MAX;
    });
    const size_t k = cand.size();
    if (k == 0) return RSN_OK;
    void *d_none; const HuffDevSummary *sums;
    const int rc = plan_where_they_lie(c, s, Slot::GD_RUNE_PLANS, 0, cand, mem, [&](const PlanEntry *d_tab, void *, HuffDevSummary *d_sum) {
        RSN_LAUNCH("huff_dev_rune_plan", k_huff_dev_rune_plan, dim3((uint32_t)k), dim3(RP_T), 0, s, d_tab, d_sum);
        return RSN_OK;
    }, &d_none, &sums);
    if (rc) return rc;
    std::vector<uint32_t> expect;
    auto len = [&](size_t i) { return (size_t)mem[i].n; };
    for (size_t q = 0; q < k; q++) if (sums[q].verdict > PARSE_NOT_MINE) {
        rune_dec_planned(cand, q, sums, len, idx, expect);                // (the failure is about the first member chosen in front of it)
        return c.fail(RSN_ERR_DEVICE, "%s: the rune plan kernel left a summary that is none", RD_WHAT);
    }
    rune_dec_planned(cand, k, sums, len, idx, expect);
    if (!rune_dec_leave(rest, idx)) return RSN_OK;
    return run_groups_dev(c, s, RD_WHAT, idx, mem, [&](size_t q) { return huff_dec_in_slot(mem[idx[q]].n); }, [&](size_t q) { return huff_dec_out_slot(expect[q]); },
        [&](hipStream_t s2, uint32_t g, const SmallMember *tab, uint8_t *base) { return launch_rune_dec(c, s2, g, tab, base); }, answers);
}

}  // namespace

const BehindClass &huff_rune_dec_class() {
    static const BehindClass dec = {BehindClass::REST, rune_dec_offer, rune_dec_offer_dev};
    return dec;
}

}  // namespace rsn
