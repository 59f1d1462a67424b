// huff_rune_mid_dec.hip -- the grouped Huffman decoder for the rune streams that promise more than HUFF_RUNE_OUT_MAX and at most
// HUFF_RUNE_MID_OUT_MAX bytes: what k_huff_mid_rune_enc (huff_rune_mid.hip) and the single call write for UTF-8 text of 16 to 64 KiB
// (rsn_huffman_decompress_batch and its device, layered, round-trip and suite forms).  k_huff_batch_rune_dec
// (huff_rune_dec.hip) ends at 16384 promised bytes; when a call holds HUFF_RUNE_MID_DEC_GROUP_MIN such streams among what that class left
// they come here instead of taking the single call one by one: ONE launch per group, ONE workgroup of 1024 threads per member -- 960 lanes
// and the wavefront of the first lane's entries, k_huff_mid_dec's shape -- one workgroup to a CU.  The kernel is rune_dec_body and the
// offers are rune_dec_offer / rune_dec_offer_dev (huff_rune_dec_body.h: read there what each step is), the 16 KiB kernel's, at
// ParseRuneMid's limits (huff_parse_rune.h): counts up to 65536, 960 lanes of at most 576 bits, a promise of 16385 to 65536 bytes from a
// stream of at least 516.  What is this unit's own:
// LDS, dynamic 134720 B: s_raw 69152 B (the payload's words are its largest tenant) and 65568 B of ranks; static: the body's 5 KiB and
// lane_dec_body's own 15 KiB (DESIGN 4.7 has the compile remarks).
#include "huff_rune_dec_body.h"

namespace rsn {
namespace {

using ML = ParseRuneMid;
using MD = RuneDecLds<ML>;
// ---- LDS (dynamic; offsets in bytes)
constexpr uint32_t ML_RAW = 0;                                                 // the header and the table; then the payload's words; then the output image
constexpr uint32_t ML_SYM = ML_RAW + MD::RAW_BYTES;                            // a leaf rank per symbol
constexpr uint32_t ML_BYTES = ML_SYM + MD::SYM_BYTES;
// beside it the static: 4 x 256 words of symbols and leaves, child[], the scan's words, the arguments, and lane_dec_body's own -- the 2 KiB
// table, child[] again, three words a lane, the maps.  The sum below is an ESTIMATE of that part, its large arrays and 2 KiB for the
// rest: the figure that counts is the compile remark's (20720 B static); growth of lane_dec_body's own LDS beyond the slack shows there
static_assert(ML_SYM % 16 == 0 && ML_BYTES + 4 * PARSE_RUNE_SYMS_MAX * 4 + 2 * (PARSE_RUNE_CHILD_MAX + 2) * 2 + (1u << DEC_K) * 4 + 3 * ML::LANES * 4 + sizeof(SmallDecArgs) + 2048 <= 160 * 1024,
              "LDS of k_huff_mid_rune_dec");

__global__ __launch_bounds__(MD::T) void k_huff_mid_rune_dec(const SmallMember *__restrict__ tab, uint8_t *__restrict__ base) {
    extern __shared__ uint4 md_lds[];
    rune_dec_body<ML>(tab, base, md_lds + ML_RAW / 16, reinterpret_cast<uint8_t *>(md_lds) + ML_SYM);
}

// ---- the device form's plan launch: k_huff_dev_rune_plan's body (huff_rune_dec_plan.h) at this class's limits, under its own name
__global__ __launch_bounds__(RP_T) void k_huff_dev_rune_mid_plan(const PlanEntry *__restrict__ tab, HuffDevSummary *__restrict__ sums) { rune_plan_body<ML>(tab, sums); }

struct RuneMidDecClass {
    using L = ML;
    static constexpr Slot slot = Slot::GD_RUNE_MID_PLANS;
    static constexpr const char *plan_name = "mid rune";
    static int plan_launch(Ctx &c, hipStream_t s, uint32_t k, const PlanEntry *d_tab, HuffDevSummary *d_sum) {
        RSN_LAUNCH("huff_dev_rune_mid_plan", k_huff_dev_rune_mid_plan, dim3(k), dim3(RP_T), 0, s, d_tab, d_sum);
        return RSN_OK;
    }
    static int launch(Ctx &c, hipStream_t s, uint32_t g, const SmallMember *tab, uint8_t *base) {
        const int rc = func_dyn_lds(c, reinterpret_cast<const void *>(k_huff_mid_rune_dec), ML_BYTES); if (rc) return rc;
        RSN_LAUNCH("huff_batch_rune_mid_dec", k_huff_mid_rune_dec, dim3(g), dim3(MD::T), ML_BYTES, s, tab, base);
        return RSN_OK;
    }
};

}  // namespace

const BehindClass &huff_rune_mid_dec_class() {
    static const BehindClass dec = {BehindClass::REST, rune_dec_offer<RuneMidDecClass>, rune_dec_offer_dev<RuneMidDecClass>};
    return dec;
}

}  // namespace rsn
