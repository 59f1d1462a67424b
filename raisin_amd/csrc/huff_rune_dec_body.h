// huff_rune_dec_body.h -- the one kernel body and the one pair of offers of the grouped rune decoders (huff_rune_dec.hip: k_huff_batch_rune_dec,
// 16 KiB; huff_rune_mid_dec.hip: k_huff_mid_rune_dec, 64 KiB), the counterpart of huff_rune_body.h.  A unit is its LDS, a
// one-line kernel and a small class struct; a class is its limits L (huff_parse_rune.h: ParseRuneSmall, ParseRuneMid).
// ONE workgroup of L::LANES + 64 threads per member -- the lanes and the wavefront of the first lane's entries -- makes the plan itself;
// the host form and the device form launch the same kernel and neither ships a tree:
//   header   rune_light_plan (huff_rune_dec_plan.h): the member's first min(n, PARSE_RUNE_SCAN_MAX) bytes into LDS; the separator by a
//            block-wide minimum; ONE lane's parse_rune_scan(...) puts the entries into an LDS table of PARSE_RUNE_SLOTS slots, the encoder's
//            hash -- a later entry for a rune finds its slot and replaces the count (huff_parse_rune.h: the code the CPU tests hold against
//            parse_header); the counts' verdict and the stream's bounds at L's limits;
//   tree     the symbols compacted, ranked a thread each (plan_rune_ranks over count + 1), and ONE wavefront builds the Go-exact tree of
//            2 to 256 leaves with the heap, the children and the depths in VGPRs through LaneStore, as the encoder does; the children
//            become child[] with a leaf's RANK where the byte decoders have its byte;
//   payload  lane_dec_body (huff_small_body.h): the byte decoders' lookup table, run_path / emit_path, four-entry maps and PathMap
//            composition, L::LANES lanes of at most L::S_MAX bits, with 510 entries of child[] and without its last store -- a leaf rank
//            per symbol stays in LDS, a.out_max = L::OUT_MAX bounds the symbols;
//   expand   each thread takes a run of symbols, a block scan of utf8_len(leaf_rune[rank]) gives its first byte, every rune is written as
//            string(rune) into an LDS image that takes the payload's place, and the image leaves in whole 16-byte units inside the
//            member's output slot, huff_dec_out_slot(expect).
// Status word, the member's last store: the decoded length in BYTES, or GROUP_BACK -- anything huff_parse_rune.h refuses at L's limits, a
// deepest code of 0 or more than 32 bits, what lane_dec_body hands back (more than four phases, DEC_ROUNDS rounds, a path off the payload,
// a stream that ends inside a codeword), an output slot smaller than the header promises, and more decoded bytes than it promises.  Fewer
// is an answer.  No workgroup waits for another; every loop is bounded by the member's size, the table's slots, the 510 nodes or a constant.
// LDS: the unit gives the two large arrays (RuneDecLds<L>: their sizes) -- s_raw, one block that is the header and the table, then the
// payload's words, then the output image, each dead before the next is written; s_sym, a leaf rank per symbol -- the body declares the
// small ones: the compacted symbols, leaves and child[] 5 KiB, beside lane_dec_body's own.
#pragma once

#include "huff_small_body.h"
#include "huff_parse_rune.h"
#include "huff_rune_dec_plan.h"

namespace rsn {
namespace {

template <class L>
struct RuneDecLds {
    static constexpr int T = L::LANES + 64;                                    // threads of a workgroup
    static constexpr uint32_t PAY_WORDS = L::LANES * L::S_MAX / 32 + 8, IMG_BYTES = L::OUT_MAX + 16;
    static constexpr uint32_t max2(uint32_t a, uint32_t b) { return a > b ? a : b; }
    static constexpr uint32_t RAW_BYTES = (max2(max2(RD_PLAN_BYTES, PAY_WORDS * 4), IMG_BYTES) + 15) & ~15u, SYM_BYTES = L::OUT_MAX + 32;
    static_assert(PARSE_RUNE_SLOTS <= 2 * T && PARSE_RUNE_SYMS_MAX <= (uint32_t)T, "two slots a thread, a thread a symbol");
};

template <class L>
__device__ __forceinline__ void rune_dec_body(const SmallMember *__restrict__ tab, uint8_t *__restrict__ base, uint4 *s_raw /*[RAW_BYTES / 16]*/, uint8_t *s_sym /*[SYM_BYTES], 16-aligned*/) {
    using D = RuneDecLds<L>;
    constexpr int T = D::T, WAVES = T / 64;
    __shared__ uint32_t s_rune[PARSE_RUNE_SYMS_MAX], s_rc1[PARSE_RUNE_SYMS_MAX];  // the symbols compacted, in slot order: rune, count + 1
    __shared__ uint32_t s_lf[PARSE_RUNE_SYMS_MAX], s_leaf_rune[PARSE_RUNE_SYMS_MAX];   // the leaves in (count asc, rune asc) order: count, rune
    __shared__ __attribute__((aligned(4))) uint16_t s_kid[PARSE_RUNE_CHILD_MAX + 2];
    __shared__ uint32_t s_wave[WAVES + 1];
    __shared__ uint32_t s_w[W_WORDS];
    __shared__ SmallDecArgs s_a;
    const SmallMember m = tab[blockIdx.x];
    uint32_t *status = reinterpret_cast<uint32_t *>(base + m.status_off);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t *s_key = reinterpret_cast<uint32_t *>(s_raw) + RD_TABLE_AT / 4, *s_c1 = s_key + PARSE_RUNE_SLOTS;
    // every verdict below is the same for the whole workgroup: a hand-back is a return of all its threads
    HuffDevBounds b{};
    uint32_t S = 0, Tl = 0;
    if (!rune_light_plan<T, L>(base + m.in_off, m.n, s_raw, s_key, s_c1, s_w, b, &S, &Tl)) { block_done(status, GROUP_BACK); return; }
    const uint32_t a = s_w[W_DISTINCT], expect = b.expect;
    if (huff_dec_out_slot(expect) > m.status_off - m.out_off) { block_done(status, GROUP_BACK); return; }   // (the host sized the slot from the same bytes: it holds)
    {   // the symbols side by side (two slots a thread), then ranked
        const uint32_t k0 = 2 * tid < PARSE_RUNE_SLOTS ? s_key[2 * tid] : PARSE_RUNE_EMPTY, k1 = 2 * tid < PARSE_RUNE_SLOTS ? s_key[2 * tid + 1] : PARSE_RUNE_EMPTY;
        uint32_t at = block_excl_scan<WAVES>((uint32_t)(k0 != PARSE_RUNE_EMPTY) + (uint32_t)(k1 != PARSE_RUNE_EMPTY), s_wave);
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
        s_a.S = S; s_a.T = Tl; s_a.flat = b.flat; s_a.seq = 0;
        s_a.hout = nullptr; s_a.status = nullptr; s_a.g_maps = nullptr; s_a.g_flags = nullptr;
        s_a.out_max = L::OUT_MAX;
    }
    __syncthreads();                                                  // (the header and the table are dead: the payload's words take their place)
    const uint32_t n_sym = lane_dec_body<D::PAY_WORDS, L::OUT_MAX, false, (int)L::LANES, PARSE_RUNE_CHILD_MAX + 2, false>(s_a, s_kid, reinterpret_cast<uint32_t *>(s_raw), s_sym);
    if (n_sym == DEC_BODY_BACK) { block_done(status, GROUP_BACK); return; }
    // ---- expand: a run of symbols a thread, their bytes' positions by a block scan, string(rune) into the image (the payload is dead)
    const uint32_t per = (n_sym + T - 1) / T, lo = min(tid * per, n_sym), hi = min(lo + per, n_sym);
    uint32_t bytes = 0;
    for (uint32_t i = lo; i < hi; i++) bytes += plan_rune_utf8_len(s_leaf_rune[s_sym[i]]);
    uint32_t at = block_excl_scan<WAVES>(bytes, s_wave);
    const uint32_t total = s_wave[WAVES];
    if (total == 0 || total > expect) { block_done(status, GROUP_BACK); return; }    // (more than the header promises: the single call's, as the byte decoders do with out_max)
    uint8_t *img = reinterpret_cast<uint8_t *>(s_raw);
    for (uint32_t i = lo; i < hi; i++) at += parse_rune_write(s_leaf_rune[s_sym[i]], img + at);
    __syncthreads();
    uint4 *hout = reinterpret_cast<uint4 *>(base + m.out_off);
    for (uint32_t u = tid; u * 16 < total; u += T) hout[u] = s_raw[u];             // (total <= expect <= L::OUT_MAX: inside the image and the slot, huff_dec_out_slot(expect))
    block_done(status, total);
}

// ---- the two offers of a class C (codecs.h: BehindClass; pool REST, so `rest` is the pool itself), huff_rune_select.h choosing at C::L's
// rules.  C says what differs: L; `slot`, the scratch of the device form's plans; plan_launch, the class's plan kernel (rune_plan_body<L>)
// under its launch label; `plan_name`, the word its error text calls that kernel; launch, the decode kernel under its label.  The chosen
// run in the groups of the SmallMember classes, the input slot the whole stream, the output slot what the header promises.
constexpr const char *RUNE_DEC_WHAT = "huffman batch decompress";

template <class C>
int rune_dec_offer(Ctx &c, std::vector<size_t> &rest, std::vector<size_t> &, const uint8_t *const *ins, const size_t *lens, const SmallTake &take, size_t *failed) {
    using L = typename C::L;
    auto len = [&](size_t i) { return lens[i]; };
    const std::vector<size_t> cand = rune_dec_candidates<L>(rest, [](size_t) { return true; }, len);
    if (cand.empty()) return RSN_OK;
    std::vector<HuffDevSummary> sums;
    for (size_t i : cand) sums.push_back(parse_rune_light<L>(ins[i], lens[i]));
    std::vector<size_t> idx, others = rest;                               // (`rest` stays as it is when the run fails)
    std::vector<uint32_t> expect;
    rune_dec_planned<L>(cand, cand.size(), sums.data(), len, idx, expect);
    if (!rune_dec_leave<L>(others, idx)) return RSN_OK;
    const int rc = run_member_groups(c, RUNE_DEC_WHAT, idx, ins, lens, [&](size_t k) { return huff_dec_in_slot(lens[idx[k]]); }, [&](size_t k) { return huff_dec_out_slot(expect[k]); },
        [&](hipStream_t s, uint32_t g, const SmallMember *tab, uint8_t *base) { return C::launch(c, s, g, tab, base); }, take, others, failed, nullptr);
    if (rc) return rc;
    std::sort(others.begin(), others.end());
    rest.swap(others);
    return RSN_OK;
}

template <class C>
int rune_dec_offer_dev(Ctx &c, hipStream_t s, std::vector<size_t> &rest, std::vector<size_t> &, const rsn_dev_member *mem, const DevPlans *plans,
                       std::vector<size_t> &idx, std::vector<uint32_t> &answers) {
    using L = typename C::L;
    auto len = [&](size_t i) { return (size_t)mem[i].n; };
    const std::vector<size_t> cand = rune_dec_candidates<L>(rest, [&](size_t i) {
        const HuffDevSummary *v = plans->of(i);
        return v && v->verdict == PARSE_NOT_MINE;
    }, len);
    const size_t k = cand.size();
    if (k == 0) return RSN_OK;
    void *d_none; const HuffDevSummary *sums;
    const int rc = plan_where_they_lie(c, s, C::slot, 0, cand, mem, [&](const PlanEntry *d_tab, void *, HuffDevSummary *d_sum) { return C::plan_launch(c, s, (uint32_t)k, d_tab, d_sum); },
                                       &d_none, &sums);
    if (rc) return rc;
    std::vector<uint32_t> expect;
    for (size_t q = 0; q < k; q++) if (sums[q].verdict > PARSE_NOT_MINE) {
        rune_dec_planned<L>(cand, q, sums, len, idx, expect);             // (the failure is about the first member chosen in front of it)
        return c.fail(RSN_ERR_DEVICE, "%s: the %s plan kernel left a summary that is none", RUNE_DEC_WHAT, C::plan_name);
    }
    rune_dec_planned<L>(cand, k, sums, len, idx, expect);
    if (!rune_dec_leave<L>(rest, idx)) return RSN_OK;
    return run_groups_dev(c, s, RUNE_DEC_WHAT, idx, mem, [&](size_t q) { return huff_dec_in_slot(mem[idx[q]].n); }, [&](size_t q) { return huff_dec_out_slot(expect[q]); },
        [&](hipStream_t s2, uint32_t g, const SmallMember *tab, uint8_t *base) { return C::launch(c, s2, g, tab, base); }, answers);
}

}  // namespace
}  // namespace rsn
