// huff_rune_mid.hip -- the grouped Huffman encoder for the mid-size members whose bytes are not all below 0x80 (rsn_huffman_compress_batch
// and its device and layered forms).  k_huff_mid_enc (huff_mid.hip) hands such a member back as GROUP_BACK_RUNES; when a call
// holds HUFF_RUNE_MID_GROUP_MIN of them, of more than HUFF_RUNE_IN_MAX and at most HUFF_RUNE_MID_IN_MAX bytes each, they come here instead
// of taking the single call one by one: ONE launch per group, ONE workgroup of 1024 threads per member, nothing on the host between the
// count and the emit.  The kernel is huff_rune_enc_body (huff_rune_body.h: the runes, the table, the plan, the header, the bits -- read
// there what each step is), the body of k_huff_batch_rune_enc too, at k_huff_mid_enc's shape: the member (64 KiB) and the image of its
// stream in dynamic LDS, one workgroup to a CU, 16 KiB of the member a round of the emit.  What differs from the 16 KiB kernel:
//   counts   a rune may occur 65535 times (PLAN_RUNE_MID_COUNT_MAX, huff_plan_rune.h): a heap item count << 9 | id still is one word, a
//            count still has five digits, so HUFF_RUNE_HDR_MAX still is the longest header;
//   depth    Fibonacci counts that sum to at most 65536 give a code of 22 bits, inside the packer's 24 (asserted below as huff_mid.hip does);
//   image    256 symbols have the flat 8-bit code as a prefix code and Huffman's is no longer, a rune is a byte at least: the payload is at
//            most n bytes, so the image is HUFF_RUNE_HDR_MAX + n and slack, not huff_rune_enc_out_slot's 9 n / 8 -- that would not fit;
//   rounds   four rounds of 1024 lanes: the scan's total carries from a round into the next, and a rune whose bytes lie across a round's
//            end is coded in the round of its START alone -- a lane classifies its unit with the words of both neighbours, whichever
//            round they belong to, and codes the starts among its own 16 positions.
// The counts take one LDS atomic a rune; aggregating a wavefront's equal runes first (64 lanes on the space character's slot) was not tried.
// Status word: the stream's length, or GROUP_BACK -- more than HUFF_RUNE_SYMS_MAX distinct runes, fewer than two, no rune >= 0x80, or a
// code beyond 24 bits (which cannot occur; the guard is the packer's).
// LDS: member 64 KiB + 16 B, image 68160 B, table 6 KiB, symbols and ranks 6 KiB: 146096 B, 142.7 KiB of the CU's 160 KiB, one workgroup a CU.
#include "huff_rune_body.h"
#include "huff_rune_mid_select.h"

namespace rsn {
namespace {

constexpr uint32_t RM_T = 1024;
constexpr uint32_t RM_IN_MAX = HUFF_RUNE_MID_IN_MAX;
constexpr uint32_t RM_SYMS = PLAN_RUNE_SYMS_MAX;      // symbols at most: the first RM_SYMS threads hold them, two table slots each
constexpr uint32_t RM_SLOTS = PLAN_RUNE_SLOTS;
constexpr uint32_t RM_IMG_WORDS = huff_rune_mid_enc_out_slot(RM_IN_MAX) / 4;
static_assert(RM_IN_MAX <= PLAN_RUNE_MID_COUNT_MAX && RM_IN_MAX <= HUFF_MID_IN_MAX && RM_IN_MAX > HUFF_RUNE_IN_MAX && HUFF_RUNE_SYMS_MAX == RM_SYMS,
              "the counts the plan takes, the members k_huff_mid_enc hands back, one alphabet");
static_assert(RM_SLOTS == 2 * RM_SYMS && RM_SYMS <= RM_T && RM_IMG_WORDS % 4 == 0 && RM_IN_MAX % 16 == 0, "two slots a symbol's thread, the image in 16-byte units");
// a code of d bits needs counts that sum to at least fib(d + 2): fib(24) = 46368 <= 65536 < fib(25)
static_assert(plan_fib(24) <= RM_IN_MAX && plan_fib(25) > RM_IN_MAX, "the deepest code of a member is 22 bits: inside the 24 of the packer");
constexpr bool rm_sizes_hold() {
    for (uint32_t n = 2; n <= RM_IN_MAX; n++)
        if (huff_rune_mid_stream_max(n) + 3 > huff_rune_mid_enc_out_slot(n) || (n > HUFF_RUNE_IN_MAX && huff_rune_mid_enc_out_slot(n) > huff_compress_bound(n))) return false;
    return true;
}
static_assert(rm_sizes_hold(), "the slot holds the longest stream in whole words, and that of a member the class takes lies within huff_compress_bound");
// ---- LDS (dynamic; offsets in bytes).  Beside it the static: the table (3 x 512 words), the symbols and ranks (6 x 256), the scan's words
constexpr uint32_t RL_IN = 0;                                     // the member, and a unit of zeros behind its last
constexpr uint32_t RL_IMG = RL_IN + RM_IN_MAX + 16;               // the image of the stream
constexpr uint32_t RL_BYTES = RL_IMG + RM_IMG_WORDS * 4;
static_assert(RL_IMG % 16 == 0 && RL_BYTES + 3 * RM_SLOTS * 4 + 6 * RM_SYMS * 4 + 1024 <= 160 * 1024, "LDS of k_huff_mid_rune_enc");

__global__ __launch_bounds__(RM_T) void k_huff_mid_rune_enc(const SmallMember *__restrict__ tab, uint8_t *__restrict__ base) {
    extern __shared__ uint4 rm_lds[];
    uint8_t *sm = reinterpret_cast<uint8_t *>(rm_lds);
    huff_rune_enc_body<RM_T, RM_IN_MAX, RM_IMG_WORDS>(tab, base, reinterpret_cast<uint4 *>(sm + RL_IN), reinterpret_cast<uint32_t *>(sm + RL_IMG),
                                                      [](uint32_t n) { return huff_rune_mid_enc_out_slot(n); });
}

struct RuneMidEncClass {
    static constexpr const char *what = "huffman batch compress";
    static size_t in_bytes(size_t n) { return huff_enc_in_slot(n); }
    static size_t out_bytes(size_t n) { return huff_rune_mid_enc_out_slot((uint32_t)n); }
    static int launch(Ctx &c, hipStream_t s, uint32_t g, const SmallMember *tab, uint8_t *base, int64_t) {
        const int rc = func_dyn_lds(c, reinterpret_cast<const void *>(k_huff_mid_rune_enc), RL_BYTES); if (rc) return rc;
        RSN_LAUNCH("huff_batch_rune_mid_enc", k_huff_mid_rune_enc, dim3(g), dim3(RM_T), RL_BYTES, s, tab, base);
        return RSN_OK;
    }
};

// The two offers (codecs.h: BehindClass, pool RUNES; huff_rune_mid_select.h choosing): the members the class runs leave the pool, the
// others STAY in it for the class listed behind this one (huff_rune.hip, which sends what it does not keep to `rest`).
int rune_mid_enc_offer(Ctx &c, std::vector<size_t> &runes, std::vector<size_t> &rest, const uint8_t *const *ins, const size_t *lens, const SmallTake &take, size_t *failed) {
    const std::vector<size_t> idx = rune_mid_class_members(runes, [&](size_t i) { return lens[i]; });
    return idx.empty() ? RSN_OK : class_run<RuneMidEncClass>(c, idx, ins, lens, 0, take, rest, failed, nullptr);
}
int rune_mid_enc_offer_dev(Ctx &c, hipStream_t s, std::vector<size_t> &runes, std::vector<size_t> &, const rsn_dev_member *mem, const DevPlans *,
                           std::vector<size_t> &idx, std::vector<uint32_t> &answers) {
    idx = rune_mid_class_members(runes, [&](size_t i) { return mem[i].n; });
    return idx.empty() ? RSN_OK : class_run_dev<RuneMidEncClass>(c, s, idx, mem, 0, nullptr, answers);
}

}  // namespace

const BehindClass &huff_rune_mid_class() {
    static const BehindClass enc = {BehindClass::RUNES, rune_mid_enc_offer, rune_mid_enc_offer_dev};
    return enc;
}

}  // namespace rsn
