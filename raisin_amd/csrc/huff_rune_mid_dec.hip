// huff_rune_mid_dec.hip -- the grouped Huffman decoder for the rune streams that promise more than HUFF_RUNE_OUT_MAX and at most
// HUFF_RUNE_MID_OUT_MAX bytes: what k_huff_mid_rune_enc (huff_rune_mid.hip) and the single call write for UTF-8 text of 16 to 64 KiB
// (rsn_huffman_decompress_batch and its device, layered, round-trip and suite forms).  k_huff_batch_rune_dec
// (huff_rune_dec.hip) ends at 16384 promised bytes; when a call holds HUFF_RUNE_MID_DEC_GROUP_MIN such streams they come here instead of
// taking the single call one by one: ONE launch per group, ONE workgroup of 1024 threads per member -- 960 lanes and the wavefront of the
// first lane's entries, k_huff_mid_dec's shape -- one workgroup to a CU.  The steps are the 16 KiB kernel's, with its code:
//   header   rune_light_plan<1024, ParseRuneMid> (huff_rune_dec_plan.h; huff_parse_rune.h at the mid limits): the stream's first
//            PARSE_RUNE_SCAN_MAX bytes into LDS, the separator, one lane's scan into the table, the counts' verdict, the bounds;
//   tree     the symbols compacted and ranked a thread each (plan_rune_ranks), ONE wavefront builds the Go-exact tree (wave_tree, wave_depths),
//            the children become child[] with a leaf's rank (parse_rune_child);
//   payload  lane_dec_body (huff_small_body.h) at 960 lanes of at most 576 bits, 510 entries of child[], without its last store: a leaf
//            rank per symbol stays in LDS, a.out_max = 65536 bounds the symbols;
//   expand   a run of symbols a thread, a block scan of utf8_len, string(rune) into an LDS image that takes the payload's place, and the
//            image leaves in whole 16-byte units inside huff_dec_out_slot(expect).
// Status word, the member's last store: the decoded length in BYTES, or GROUP_BACK -- anything huff_parse_rune.h refuses at these limits, a
// deepest code of 0 or more than 32 bits, what lane_dec_body hands back (a fifth phase, DEC_ROUNDS rounds, a path off the payload, an end
// inside a codeword), an output slot smaller than the promise needs, and more decoded bytes than promised.  Fewer is an answer.
// No workgroup waits for another; every loop is bounded by the member's size, the table's slots, the 510 nodes or a constant.
// LDS: dynamic 134720 B -- one block of 69152 B that is the header and the table, then the payload's words, then the output image (each
// dead before the next is written), and 65568 B of ranks; static: the symbols, leaves and child[] 5 KiB, lane_dec_body's own 15 KiB
// (DESIGN 4.7 has the compile remarks).
#include <iterator>

#include "huff_small_body.h"
#include "huff_parse_rune.h"
#include "huff_rune_dec_plan.h"
#include "huff_rune_mid_dec_select.h"

namespace rsn {
namespace {

using ML = ParseRuneMid;
static_assert(ML::OUT_MAX == HUFF_RUNE_MID_OUT_MAX && ML::PAY_MAX == HUFF_RUNE_MID_PAY_MAX && ML::STREAM_MAX == HUFF_RUNE_MID_STREAM_MAX && ML::LANES == HUFF_RUNE_MID_DEC_LANES &&
              ML::S_MAX == HUFF_RUNE_MID_DEC_S_MAX && ML::COUNT_MAX == PLAN_RUNE_MID_COUNT_MAX && PARSE_RUNE_SYMS_MAX == HUFF_RUNE_SYMS_MAX,
              "huff_parse_rune.h restates the class's limits without its headers");

constexpr int MD_T = 1024;                                                     // threads of a workgroup
constexpr int MD_DL = MD_T - 64;                                               // lane_dec_body's lanes; the sixteenth wavefront: the first lane's entries
constexpr int MD_WAVES = MD_T / 64;
static_assert((uint32_t)MD_DL == ML::LANES && PARSE_RUNE_SLOTS <= 2 * MD_T && PARSE_RUNE_SYMS_MAX <= (uint32_t)MD_T, "the class's lanes; two slots a thread, a thread a symbol");
constexpr uint32_t MD_PAY_WORDS = MD_DL * ML::S_MAX / 32 + 8;
constexpr uint32_t MD_IMG_BYTES = HUFF_RUNE_MID_OUT_MAX + 16;
constexpr uint32_t md_max(uint32_t a, uint32_t b) { return a > b ? a : b; }
// ---- LDS (dynamic; offsets in bytes)
constexpr uint32_t ML_RAW = 0;                                                 // the header and the table; then the payload's words; then the output image
constexpr uint32_t MD_RAW_BYTES = (md_max(md_max(RD_PLAN_BYTES, MD_PAY_WORDS * 4), MD_IMG_BYTES) + 15) & ~15u;
constexpr uint32_t ML_SYM = ML_RAW + MD_RAW_BYTES;                             // a leaf rank per symbol
constexpr uint32_t ML_BYTES = ML_SYM + HUFF_RUNE_MID_OUT_MAX + 32;
// beside it the static: 4 x 256 words of symbols and leaves, child[], the scan's words, the arguments, and lane_dec_body's own -- the 2 KiB
// table, child[] again, three words a lane, the maps.  The sum below is an ESTIMATE of that part, its large arrays and 2 KiB for the
// rest: the figure that counts is the compile remark's (20720 B static); growth of lane_dec_body's own LDS beyond the slack shows there
static_assert(ML_SYM % 16 == 0 && ML_BYTES + 4 * PARSE_RUNE_SYMS_MAX * 4 + 2 * (PARSE_RUNE_CHILD_MAX + 2) * 2 + (1u << DEC_K) * 4 + 3 * MD_DL * 4 + sizeof(SmallDecArgs) + 2048 <= 160 * 1024,
              "LDS of k_huff_mid_rune_dec");

__global__ __launch_bounds__(MD_T) void k_huff_mid_rune_dec(const SmallMember *__restrict__ tab, uint8_t *__restrict__ base) {
    extern __shared__ uint4 md_lds[];
    __shared__ uint32_t s_rune[PARSE_RUNE_SYMS_MAX], s_rc1[PARSE_RUNE_SYMS_MAX];  // the symbols compacted, in slot order: rune, count + 1
    __shared__ uint32_t s_lf[PARSE_RUNE_SYMS_MAX], s_leaf_rune[PARSE_RUNE_SYMS_MAX];   // the leaves in (count asc, rune asc) order: count, rune
    __shared__ __attribute__((aligned(4))) uint16_t s_kid[PARSE_RUNE_CHILD_MAX + 2];
    __shared__ uint32_t s_wave[MD_WAVES + 1];
    __shared__ uint32_t s_w[W_WORDS];
    __shared__ SmallDecArgs s_a;
    uint4 *s_raw = md_lds + ML_RAW / 16;
    uint8_t *s_sym = reinterpret_cast<uint8_t *>(md_lds) + ML_SYM;
    const SmallMember m = tab[blockIdx.x];
    uint32_t *status = reinterpret_cast<uint32_t *>(base + m.status_off);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t *s_key = reinterpret_cast<uint32_t *>(s_raw) + RD_TABLE_AT / 4, *s_c1 = s_key + PARSE_RUNE_SLOTS;
    // every verdict below is the same for the whole workgroup: a hand-back is a return of all its threads
    HuffDevBounds b{};
    uint32_t S = 0, T = 0;
    if (!rune_light_plan<MD_T, ML>(base + m.in_off, m.n, s_raw, s_key, s_c1, s_w, b, &S, &T)) { block_done(status, GROUP_BACK); return; }
    const uint32_t a = s_w[W_DISTINCT], expect = b.expect;
    if (huff_dec_out_slot(expect) > m.status_off - m.out_off) { block_done(status, GROUP_BACK); return; }   // (the host sized the slot from the same bytes: it holds)
    {   // the symbols side by side (two slots a thread), then ranked
        const uint32_t k0 = 2 * tid < PARSE_RUNE_SLOTS ? s_key[2 * tid] : PARSE_RUNE_EMPTY, k1 = 2 * tid < PARSE_RUNE_SLOTS ? s_key[2 * tid + 1] : PARSE_RUNE_EMPTY;
        uint32_t at = block_excl_scan<MD_WAVES>((uint32_t)(k0 != PARSE_RUNE_EMPTY) + (uint32_t)(k1 != PARSE_RUNE_EMPTY), s_wave);
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
        s_a.out_max = HUFF_RUNE_MID_OUT_MAX;
    }
    __syncthreads();                                                  // (the header and the table are dead: the payload's words take their place)
    const uint32_t n_sym = lane_dec_body<MD_PAY_WORDS, HUFF_RUNE_MID_OUT_MAX, false, MD_DL, PARSE_RUNE_CHILD_MAX + 2, false>(s_a, s_kid, reinterpret_cast<uint32_t *>(s_raw), s_sym);
    if (n_sym == DEC_BODY_BACK) { block_done(status, GROUP_BACK); return; }
    // ---- expand: a run of symbols a thread, their bytes' positions by a block scan, string(rune) into the image (the payload is dead)
    const uint32_t per = (n_sym + MD_T - 1) / MD_T, lo = min(tid * per, n_sym), hi = min(lo + per, n_sym);
    uint32_t bytes = 0;
    for (uint32_t i = lo; i < hi; i++) bytes += plan_rune_utf8_len(s_leaf_rune[s_sym[i]]);
    uint32_t at = block_excl_scan<MD_WAVES>(bytes, s_wave);
    const uint32_t total = s_wave[MD_WAVES];
    if (total == 0 || total > expect) { block_done(status, GROUP_BACK); return; }    // (more than the header promises: the single call's, as the byte decoders do with out_max)
    uint8_t *img = reinterpret_cast<uint8_t *>(s_raw);
    for (uint32_t i = lo; i < hi; i++) at += parse_rune_write(s_leaf_rune[s_sym[i]], img + at);
    __syncthreads();
    uint4 *hout = reinterpret_cast<uint4 *>(base + m.out_off);
    for (uint32_t u = tid; u * 16 < total; u += MD_T) hout[u] = s_raw[u];          // (total <= expect <= 65536: inside the image and the slot, huff_dec_out_slot(expect))
    block_done(status, total);
}

// ---- the device form's plan launch: k_huff_dev_rune_plan's body (huff_rune_dec_plan.h) at this class's limits, under its own name
__global__ __launch_bounds__(RP_T) void k_huff_dev_rune_mid_plan(const PlanEntry *__restrict__ tab, HuffDevSummary *__restrict__ sums) { rune_plan_body<ML>(tab, sums); }

int launch_rune_mid_dec(Ctx &c, hipStream_t s, uint32_t g, const SmallMember *tab, uint8_t *base) {
    const int rc = func_dyn_lds(c, reinterpret_cast<const void *>(k_huff_mid_rune_dec), ML_BYTES); if (rc) return rc;
    RSN_LAUNCH("huff_batch_rune_mid_dec", k_huff_mid_rune_dec, dim3(g), dim3(MD_T), ML_BYTES, s, tab, base);
    return RSN_OK;
}
const char *const MD_WHAT = "huffman batch decompress";

// The two offers (codecs.h: BehindClass; pool REST, so `rest` is the pool itself), huff_rune_mid_dec_select.h choosing among what the 16 KiB
// class left.  The chosen run in the groups of the SmallMember classes, the input slot the whole stream, the output slot what the header
// promises.
int rune_mid_dec_offer(Ctx &c, std::vector<size_t> &rest, std::vector<size_t> &, const uint8_t *const *ins, const size_t *lens, const SmallTake &take, size_t *failed) {
    auto len = [&](size_t i) { return lens[i]; };
    const std::vector<size_t> cand = rune_mid_dec_candidates(rest, [](size_t) { return true; }, len);
    if (cand.empty()) return RSN_OK;
    std::vector<HuffDevSummary> sums;
    for (size_t i : cand) sums.push_back(parse_rune_light<ML>(ins[i], lens[i]));
    std::vector<size_t> idx, others = rest;                               // (`rest` stays as it is when the run fails)
    std::vector<uint32_t> expect;
    rune_mid_dec_planned(cand, cand.size(), sums.data(), len, idx, expect);
    if (!rune_mid_dec_leave(others, idx)) return RSN_OK;
    const int rc = run_member_groups(c, MD_WHAT, idx, ins, lens, [&](size_t k) { return huff_dec_in_slot(lens[idx[k]]); }, [&](size_t k) { return huff_dec_out_slot(expect[k]); },
        [&](hipStream_t s, uint32_t g, const SmallMember *tab, uint8_t *base) { return launch_rune_mid_dec(c, s, g, tab, base); }, take, others, failed, nullptr);
    if (rc) return rc;
    std::sort(others.begin(), others.end());
    rest.swap(others);
    return RSN_OK;
}

int rune_mid_dec_offer_dev(Ctx &c, hipStream_t s, std::vector<size_t> &rest, std::vector<size_t> &, const rsn_dev_member *mem, const DevPlans *plans,
                           std::vector<size_t> &idx, std::vector<uint32_t> &answers) {
    auto len = [&](size_t i) { return (size_t)mem[i].n; };
    const std::vector<size_t> cand = rune_mid_dec_candidates(rest, [&](size_t i) {
        const HuffDevSummary *v = plans->of(i);
        return v && v->verdict == PARSE_NOT_MINE;
    }, len);
    const size_t k = cand.size();
    if (k == 0) return RSN_OK;
    void *d_none; const HuffDevSummary *sums;
    const int rc = plan_where_they_lie(c, s, Slot::GD_RUNE_MID_PLANS, 0, cand, mem, [&](const PlanEntry *d_tab, void *, HuffDevSummary *d_sum) {
        RSN_LAUNCH("huff_dev_rune_mid_plan", k_huff_dev_rune_mid_plan, dim3((uint32_t)k), dim3(RP_T), 0, s, d_tab, d_sum);
        return RSN_OK;
    }, &d_none, &sums);
    if (rc) return rc;
    std::vector<uint32_t> expect;
    for (size_t q = 0; q < k; q++) if (sums[q].verdict > PARSE_NOT_MINE) {
        rune_mid_dec_planned(cand, q, sums, len, idx, expect);            // (the failure is about the first member chosen in front of it)
        return c.fail(RSN_ERR_DEVICE, "%s: the mid rune plan kernel left a summary that is none", MD_WHAT);
    }
    rune_mid_dec_planned(cand, k, sums, len, idx, expect);
    if (!rune_mid_dec_leave(rest, idx)) return RSN_OK;
    return run_groups_dev(c, s, MD_WHAT, idx, mem, [&](size_t q) { return huff_dec_in_slot(mem[idx[q]].n); }, [&](size_t q) { return huff_dec_out_slot(expect[q]); },
        [&](hipStream_t s2, uint32_t g, const SmallMember *tab, uint8_t *base) { return launch_rune_mid_dec(c, s2, g, tab, base); }, answers);
}

}  // namespace

const BehindClass &huff_rune_mid_dec_class() {
    static const BehindClass dec = {BehindClass::REST, rune_mid_dec_offer, rune_mid_dec_offer_dev};
    return dec;
}

}  // namespace rsn
