// huff_rune.hip -- the grouped Huffman encoder for members whose bytes are not all below 0x80: UTF-8 text, and bytes that are no UTF-8 at
// all (rsn_huffman_compress_batch and its device and layered forms).  The byte encoder k_huff_batch_enc (huff_small.hip) hands
// such a member back as GROUP_BACK_RUNES; when a call holds HUFF_RUNE_GROUP_MIN of them, of at most 16 KiB each, they come here instead
// of taking the single call one by one: ONE launch per group, ONE workgroup of 256 threads per member, nothing on the host between the
// count and the emit.  The kernel is huff_rune_enc_body (huff_rune_body.h: the runes, the table, the plan, the header, the bits and the
// status word -- read there what each step is) with the member and the image in static LDS; this unit holds its limits and its class.
// A code beyond 24 bits cannot occur: the longest code of a tree over counts c is as long as the Fibonacci numbers that fit below sum(c),
// and those that sum to at most 16384 give 20 bits.
// LDS: member 16 KiB + 16 B, image 21072 B, table 6 KiB, symbols and ranks 6 KiB: 49.8 KiB, three workgroups to a CU's 160 KiB.
#include "huff_rune_body.h"

namespace rsn {
namespace {

constexpr uint32_t HR_T = 256;
constexpr uint32_t HR_IMG_WORDS = huff_rune_enc_out_slot(HE_IN_MAX) / 4;
static_assert(HE_IN_MAX == HUFF_RUNE_IN_MAX && HE_IN_MAX <= PLAN_RUNE_COUNT_MAX && HUFF_RUNE_SYMS_MAX == PLAN_RUNE_SYMS_MAX, "one cutoff, one alphabet");
static_assert(HR_T == PLAN_RUNE_SYMS_MAX && PLAN_RUNE_SLOTS == 2 * HR_T && HR_IMG_WORDS % 4 == 0, "a thread per symbol, two slots per thread, the image in 16-byte units");
constexpr bool hr_sizes_hold() {
    for (uint32_t n = 2; n <= HE_IN_MAX; n++)
        if (huff_rune_stream_max(n) + 3 > huff_rune_enc_out_slot(n) || huff_rune_stream_max(n) > huff_compress_bound(n)) return false;
    return true;
}
static_assert(hr_sizes_hold(), "the image fits the member's slot, and huff_compress_bound covers the stream");

__global__ __launch_bounds__(HR_T) void k_huff_batch_rune_enc(const SmallMember *__restrict__ tab, uint8_t *__restrict__ base) {
    __shared__ uint4 s_in[HE_IN_MAX / 16 + 1];
    __shared__ __attribute__((aligned(16))) uint32_t s_img[HR_IMG_WORDS];
    huff_rune_enc_body<HR_T, HE_IN_MAX, HR_IMG_WORDS>(tab, base, s_in, s_img, [](uint32_t n) { return huff_rune_enc_out_slot(n); });
}

struct RuneEncClass {
    static constexpr const char *what = "huffman batch compress";
    static size_t in_bytes(size_t n) { return huff_enc_in_slot(n); }
    static size_t out_bytes(size_t n) { return huff_rune_enc_out_slot((uint32_t)n); }
    static int launch(Ctx &c, hipStream_t s, uint32_t g, const SmallMember *tab, uint8_t *base, int64_t) {
        RSN_LAUNCH("huff_batch_rune_enc", k_huff_batch_rune_enc, dim3(g), dim3(HR_T), 0, s, tab, base);
        return RSN_OK;
    }
};

int rune_enc_offer(Ctx &c, std::vector<size_t> &runes, std::vector<size_t> &rest, const uint8_t *const *ins, const size_t *lens, const SmallTake &take, size_t *failed) {
    runes.resize(rune_class_members(runes, rest, [&](size_t i) { return lens[i]; }));
    const int rc = runes.empty() ? RSN_OK : class_run<RuneEncClass>(c, runes, ins, lens, 0, take, rest, failed, nullptr);
    runes.clear();
    return rc;
}
int rune_enc_offer_dev(Ctx &c, hipStream_t s, std::vector<size_t> &runes, std::vector<size_t> &rest, const rsn_dev_member *mem, const DevPlans *,
                       std::vector<size_t> &idx, std::vector<uint32_t> &answers) {
    runes.resize(rune_class_members(runes, rest, [&](size_t i) { return mem[i].n; }));
    idx.swap(runes);                                                      // (idx comes empty: the pool is left so)
    return idx.empty() ? RSN_OK : class_run_dev<RuneEncClass>(c, s, idx, mem, 0, nullptr, answers);
}

}  // namespace

const BehindClass &huff_rune_class() {
    static const BehindClass enc = {BehindClass::RUNES, rune_enc_offer, rune_enc_offer_dev};
    return enc;
}

}  // namespace rsn
