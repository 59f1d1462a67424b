// huff_dev.hip -- the Huffman decompress batch on device buffers (rsn_huffman_decompress_batch_dev, rsn.h).
// The grouped decoders (k_huff_batch_dec, k_huff_mid_dec) decode from a SmallDecArgs table entry that the host form fills from the header's
// bytes (small_dec_plan, huff_small.hip).  A stream that lies in device memory would have to come down for that; here the plan is made
// where the stream lies:
//   k_huff_dev_plan    a workgroup per candidate member: the first min(n, HDR_MAX + 8) bytes into LDS, the separator by a block-wide
//                      minimum, the entries by one lane's scan of the LDS bytes (an entry's skip decides where the next begins), the leaves
//                      ranked a thread each, the Go-exact tree built by ONE wavefront with the heap, the children and the depths in VGPRs
//                      (huff_parse_small.h / huff_plan_small.h: the code the CPU tests hold against the host's) -- the pointer-free part of
//                      a SmallDecArgs into the plan table, 16 bytes of summary for the host
//   k_huff_dev_gather  a workgroup per member of a group: the stream from its 4-byte boundary into the input slot (zeros behind it), its
//                      SmallDecArgs completed from the plan table and the group's offsets, the status words set
//   (the class's decoder, launched unchanged)
//   k_huff_dev_scatter the decoder's two status words into the answer, what fits into the member's buffer
// What crosses PCIe per member: 16 bytes up and 16 down for the plan, 64 up for the group's table and 4 down for the answer.
// No workgroup waits for another; every loop is bounded by HDR_MAX + 8, by the 255 nodes or by a slot's size.
#include "huff_small_body.h"
#include "huff_parse_small.h"

namespace rsn {

namespace {

static_assert(PARSE_HDR_MAX == HDR_MAX && PARSE_STREAM_MAX == DEC_STREAM_MAX && PARSE_OUT_MAX == SMALL_MAX && PARSE_K_MAX == (uint32_t)DEC_K,
              "huff_parse_small.h restates the decoders' limits without their headers");
static_assert(PLAN_COUNT_LIMIT <= SMALL_MAX, "a count the plan takes is one small_dec_plan takes");
static_assert(PARSE_OUT_MAX_WIDE == HUFF_BIG_OUT_MAX && PARSE_PAY_MAX_WIDE == HUFF_BIG_PAY_MAX, "... and the wide form's are the tiled decoder's class (codecs.h)");

constexpr int HP_T = 128;                                     // threads of the plan kernel: a thread per byte of the alphabet, two wavefronts
constexpr uint32_t HP_UNITS = (PARSE_SCAN_MAX + 15) / 16;     // 16-byte units of the header in LDS
constexpr int GD_THREADS = 256;

// the header's bytes in LDS, a word fetched for every four consecutive bytes asked for
struct LdsBytes {
    const uint32_t *w;
    mutable uint32_t at = PARSE_NONE, cur = 0;
    __device__ __forceinline__ uint32_t get(uint32_t i) const {
        if ((i >> 2) != at) { at = i >> 2; cur = w[at]; }
        return (cur >> (8 * (i & 3))) & 0xFFu;
    }
};

__global__ __launch_bounds__(HP_T) void k_huff_dev_plan(const PlanEntry *__restrict__ tab, HuffDevPlan *__restrict__ plans, HuffDevSummary *__restrict__ sums) {
    __shared__ uint4 s_hdr[HP_UNITS + 1];
    __shared__ uint32_t s_cnt1[PLAN_SYMS_MAX], s_lf[PLAN_SYMS_MAX];
    __shared__ uint8_t s_leaf[PLAN_SYMS_MAX];
    __shared__ __attribute__((aligned(4))) uint16_t s_child[256];
    __shared__ uint32_t s_w[8];                               // the separator, the scan's verdict, the counts' sum, the largest count, root, shortest, deepest
    static_assert(HP_T == PLAN_SYMS_MAX, "a thread per byte of the alphabet");
    const PlanEntry e = tab[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // every verdict below is the same for the whole workgroup: a refusal is a return of all its threads
    auto refuse = [&] { if (tid == 0) sums[blockIdx.x] = HuffDevSummary{PARSE_NOT_MINE, 0, 0, 0}; };
    if (!parse_length_ok(e.n, true)) { refuse(); return; }     // (the wide form is allowed: huff_parse_small.h says which streams it judges)
    const uint32_t n = (uint32_t)e.n, limit = parse_scan_limit(n);
    {   // the header into LDS under the gather's rule: the unit that reaches beyond src + n is masked, nothing at or behind src + n rounded up to 16 is loaded
        const uint4 *src = reinterpret_cast<const uint4 *>(e.src);
        for (uint32_t u = tid; u * 16 < limit; u += HP_T) s_hdr[u] = unit_head(src[u], n - 16 * u);      // (u * 16 < limit <= n)
    }
    s_cnt1[tid] = 0;
    reinterpret_cast<uint32_t *>(s_child)[tid] = 0;
    if (tid < 8) s_w[tid] = tid == 0 ? PARSE_NONE : 0u;
    __syncthreads();
    const uint8_t *hb = reinterpret_cast<const uint8_t *>(s_hdr);
    {   // strings.SplitN(content, "\\\n", 2): the first separator among the bytes looked at -- a position at or behind n is never asked
        uint32_t mine = PARSE_NONE;
        for (uint32_t i = tid; i + 1 < limit; i += HP_T) if (parse_sep_at(hb[i], hb[i + 1])) { mine = i; break; }
        if (mine != PARSE_NONE) atomicMin(&s_w[0], mine);
    }
    __syncthreads();
    const uint32_t sep = s_w[0];
    if (sep == PARSE_NONE || sep + 4 > n) { refuse(); return; }
    if (tid == 0) { LdsBytes h; h.w = reinterpret_cast<const uint32_t *>(s_hdr); s_w[1] = parse_scan(h, sep, s_cnt1, PLAN_COUNT_LIMIT_WIDE) ? 1u : 0u; }
    __syncthreads();
    if (!s_w[1]) { refuse(); return; }
    const uint32_t c1 = s_cnt1[tid];
    if (c1) { atomicAdd(&s_w[2], c1 - 1); atomicMax(&s_w[3], c1 - 1); }
    const uint32_t a = (uint32_t)__syncthreads_count(c1 != 0);
    HuffDevBounds b{};
    const bool wide = parse_is_wide(true, n, s_w[2]);
    if (!parse_counts_ok(a, s_w[3] >= parse_count_limit(wide), s_w[2], wide) || !parse_bounds(n, sep, hb[sep + 2], b)) { refuse(); return; }
    b.expect = s_w[2];
    if (c1) { const uint32_t r = plan_leaf_rank(s_cnt1, tid); s_lf[r] = c1 - 1; s_leaf[r] = (uint8_t)tid; }
    __syncthreads();
    if (wave == 0) {   // the tree, the depths and child[]: one wavefront, every index wave-uniform (huff_small_body.h: LaneStore)
        const uint32_t au = (uint32_t)__builtin_amdgcn_readfirstlane((int)a);
        LaneStore<2> kids;
        LaneStore<4> code;
        const uint32_t root = wave_tree<8>(s_lf, au, kids, code);
        uint32_t mn, mx;
        wave_depths(code, au, &mn, &mx);
        // internal node k is lane k of kids.r[0], node 64 + k lane k of kids.r[1]
        if (lane + 1 < au) { s_child[2 * lane] = (uint16_t)parse_child(kids.r[0] & 0xFFu, au, s_leaf); s_child[2 * lane + 1] = (uint16_t)parse_child(kids.r[0] >> 8, au, s_leaf); }
        if (lane + 65 < au) { s_child[2 * lane + 128] = (uint16_t)parse_child(kids.r[1] & 0xFFu, au, s_leaf); s_child[2 * lane + 129] = (uint16_t)parse_child(kids.r[1] >> 8, au, s_leaf); }
        if (lane == 0) { s_w[4] = root - au; s_w[5] = mn; s_w[6] = mx; }
    }
    __syncthreads();
    if (!parse_depths(s_w[5], s_w[6], b)) { refuse(); return; }
    b.root = s_w[4]; b.n_child = 2 * (a - 1); b.verdict = PARSE_PLANNED;
    HuffDevPlan *out = plans + blockIdx.x;
    reinterpret_cast<uint32_t *>(out->child)[tid] = reinterpret_cast<const uint32_t *>(s_child)[tid];     // (zeros behind n_child)
    if (tid == 0) { out->b = b; sums[blockIdx.x] = HuffDevSummary{PARSE_PLANNED, b.A0, b.end - b.p0, b.expect}; }
}

// a member of a decoding group: where its stream begins (d_in + A0: 4-byte aligned), where its result goes, its slots in the staging and its plan
struct DecEntry {
    const uint8_t *src; uint8_t *dst;
    unsigned long long cap;                       // bytes of dst (0: a size query, dst may be null)
    uint32_t n, in_off, in_bytes, out_off, out_bytes, status_off, plan, pad_[3];
};
static_assert(sizeof(DecEntry) == 64, "64 bytes a member go up with its group");
constexpr size_t HD_ENTRY = sizeof(SmallDecArgs) + sizeof(DecEntry);
static_assert(HD_ENTRY % 16 == 0, "a group's two tables are whole 16-byte units");

// A workgroup per member.  k_group_gather's copy (group_dev.hip) from a source that is only 4-byte aligned: whole units with 16-byte loads
// at that alignment, the unit the stream ends in a dword at a time -- the dword that reaches beyond src + n is masked, and nothing is loaded
// at or behind src + n rounded up to 4 (d_in is 16-byte aligned and A0 a multiple of 4: inside d_in + n rounded up to 16).  Zeros from
// byte n to the slot's end, as the decoders' loads rely on.  Then the member's SmallDecArgs: the plan's part as it is, S and T for this
// class's lanes, the pointers into the staging, out_max = expect, and the status words -- GROUP_PENDING, 0.
__global__ __launch_bounds__(GD_THREADS) void k_huff_dev_gather(const DecEntry *__restrict__ tab, uint8_t *__restrict__ base, const HuffDevPlan *__restrict__ plans,
                                                                 uint32_t lanes, uint32_t s_max) {
    const DecEntry e = tab[blockIdx.x];
    const uint32_t *src = reinterpret_cast<const uint32_t *>(e.src);
    uint4 *dst = reinterpret_cast<uint4 *>(base + e.in_off);
    const uint32_t units = e.in_bytes / 16, full = e.n / 16;
    for (uint32_t u = threadIdx.x; u < units; u += GD_THREADS) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (u < full) { const rsn_u32x4_a4 x = *reinterpret_cast<const rsn_u32x4_a4 *>(src + 4 * u); v = make_uint4(x.x, x.y, x.z, x.w); }
        else if (u == full) {
            uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                const uint32_t at = 16 * u + 4 * k;
                if (at < e.n) { const uint32_t keep = min(e.n - at, 4u); w[k] = src[4 * u + k]; if (keep < 4) w[k] &= (1u << (8 * keep)) - 1; }
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        dst[u] = v;
    }
    const HuffDevPlan *p = plans + e.plan;
    SmallDecArgs *a = reinterpret_cast<SmallDecArgs *>(base) + blockIdx.x;
    if (threadIdx.x < 128) reinterpret_cast<uint32_t *>(a->child)[threadIdx.x] = reinterpret_cast<const uint32_t *>(p->child)[threadIdx.x];
    if (threadIdx.x == 0) {
        const HuffDevBounds b = p->b;
        uint32_t S, T;
        (void)parse_lanes(b.end - b.p0, lanes, s_max, &S, &T);          // (the host has asked the same of the same span: it holds)
        uint32_t *status = reinterpret_cast<uint32_t *>(base + e.status_off);
        a->pay = reinterpret_cast<const uint32_t *>(base + e.in_off);
        a->pay_words = b.pay_words; a->p0 = b.p0; a->end = b.end;
        a->K = b.K; a->root = b.root; a->n_child = b.n_child;
        a->S = S; a->T = T; a->flat = b.flat; a->seq = 0;
        a->hout = base + e.out_off; a->status = status;
        a->g_maps = nullptr; a->g_flags = nullptr;
        a->out_max = b.expect; a->pad_[0] = a->pad_[1] = a->pad_[2] = 0;
        status[0] = GROUP_PENDING; status[1] = 0;
    }
}

// A workgroup per member, behind the decoder on the stream.  The decoder's words: w[0] still GROUP_PENDING -- no kernel answered; w[0] != 0
// -- handed back; else w[1] is the decoded length.  From there k_group_scatter's rules: a length beyond the output slot goes down as
// GROUP_PENDING, only what fits the member's buffer is copied, whole 16-byte units then the tail, never a byte at or behind dst + len.
__global__ __launch_bounds__(GD_THREADS) void k_huff_dev_scatter(const DecEntry *__restrict__ tab, const uint8_t *__restrict__ base, uint32_t *__restrict__ answers) {
    const DecEntry e = tab[blockIdx.x];
    const uint32_t *w = reinterpret_cast<const uint32_t *>(base + e.status_off);
    const uint32_t w0 = w[0];
    uint32_t v = w0 == GROUP_PENDING ? GROUP_PENDING : w0 != 0 ? GROUP_BACK : w[1];
    if (v < GROUP_BACK && v > e.out_bytes) v = GROUP_PENDING;
    if (threadIdx.x == 0) answers[blockIdx.x] = v;
    if (v >= GROUP_BACK_RUNES || v > e.cap) return;
    const uint4 *src = reinterpret_cast<const uint4 *>(base + e.out_off);
    uint4 *dst = reinterpret_cast<uint4 *>(e.dst);
    const uint32_t full = v / 16;
    for (uint32_t u = threadIdx.x; u < full; u += GD_THREADS) dst[u] = src[u];
    const uint32_t i = full * 16 + threadIdx.x;
    if (threadIdx.x < 16 && i < v) e.dst[i] = base[e.out_off + i];
}

}  // namespace

int huff_dev_plan(Ctx &c, hipStream_t s, size_t n, const rsn_dev_member *mem, DevPlans &plans) {
    plans.at.assign(n, DEV_PLAN_NONE);
    plans.sum.clear();
    plans.d_table = nullptr;
    std::vector<size_t> cand;
    for (size_t i = 0; i < n; i++) if (mem[i].n >= 8 && mem[i].n <= HDR_MAX + 8 + HUFF_BIG_PAY_MAX) { plans.at[i] = (uint32_t)cand.size(); cand.push_back(i); }
    const size_t k = cand.size();
    if (k == 0) return RSN_OK;
    if (k >= DEV_PLAN_NONE) return c.fail(RSN_ERR_LIMIT, "huffman: a batch of %zu members", k);
    void *d_plans; const HuffDevSummary *h_sum;
    const int rc = plan_where_they_lie(c, s, Slot::GD_PLANS, k * sizeof(HuffDevPlan), cand, mem, [&](const PlanEntry *d_tab, void *d_table, HuffDevSummary *d_sum) {
        RSN_LAUNCH("huff_dev_plan", k_huff_dev_plan, dim3((uint32_t)k), dim3(HP_T), 0, s, d_tab, (HuffDevPlan *)d_table, d_sum);
        return RSN_OK;
    }, &d_plans, &h_sum);
    if (rc) return rc;
    plans.sum.assign(h_sum, h_sum + k);
    plans.d_table = (const HuffDevPlan *)d_plans;
    for (const HuffDevSummary &v : plans.sum)
        if (v.verdict > PARSE_NOT_MINE || (v.verdict == PARSE_PLANNED && (v.A0 & 3u))) return c.fail(RSN_ERR_DEVICE, "huffman batch decompress: the plan kernel left a summary that is none");
    return RSN_OK;
}

// The decoding classes through the one driver (group_run.h: run_groups_staged), every member asked up front whether it is of the class.
// The gather kernel completes the layout's SmallDecArgs on the device, so only the DecEntry table goes up, behind them.
int huff_dec_run_dev(Ctx &c, hipStream_t s, const HuffDecShape &shape, const HuffDecLaunch &launch, const std::vector<size_t> &idx, const rsn_dev_member *mem,
                     const DevPlans &plans, std::vector<uint32_t> &answers, size_t group_bytes) {
    const char *what = "huffman batch decompress";
    answers.assign(idx.size(), GROUP_PENDING);
    for (size_t i : idx) {
        const HuffDevSummary *v = plans.of(i);
        if (!v || v->verdict != PARSE_PLANNED || v->A0 > mem[i].n || !huff_dec_shape_takes(shape, *v)) return c.fail(RSN_ERR_DEVICE, "%s: internal error: member %zu is not of the class", what, i);
    }
    return run_groups_staged<HD_ENTRY, sizeof(DecEntry)>(c, s, what, idx.size(), group_bytes,
        [&](size_t k) { return huff_dec_in_slot(mem[idx[k]].n - plans.of(idx[k])->A0); }, [&](size_t k) { return huff_dec_out_slot(plans.of(idx[k])->expect); },
        [&](uint8_t *tab, size_t, size_t q, size_t k, const MemberSlots &o, size_t ib, size_t ob) {
            const rsn_dev_member &m = mem[idx[k]];
            const HuffDevSummary &v = *plans.of(idx[k]);
            ((DecEntry *)tab)[q] = DecEntry{(const uint8_t *)m.d_in + v.A0, (uint8_t *)m.d_out, m.d_out ? (unsigned long long)m.out_cap : 0ull,
                                            (uint32_t)(m.n - v.A0), o.in, (uint32_t)ib, o.out, (uint32_t)ob, o.status, plans.at[idx[k]], {0, 0, 0}};
        }, [](size_t g) { return g * sizeof(SmallDecArgs); },
        [&](uint32_t g, uint8_t *base, uint8_t *d_tab, uint32_t *d_ans) {
            const DecEntry *d_gat = (const DecEntry *)d_tab;
            RSN_LAUNCH("huff_dev_gather", k_huff_dev_gather, dim3(g), dim3(GD_THREADS), 0, s, d_gat, base, plans.d_table, shape.lanes, shape.s_max);
            const int rc = launch(c, s, g, (const SmallDecArgs *)base); if (rc) return rc;
            RSN_LAUNCH("huff_dev_scatter", k_huff_dev_scatter, dim3(g), dim3(GD_THREADS), 0, s, d_gat, (const uint8_t *)base, d_ans);
            return RSN_OK;
        }, answers);
}

}  // namespace rsn
