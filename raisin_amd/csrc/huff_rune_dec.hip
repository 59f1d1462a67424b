// huff_rune_dec.hip -- the grouped Huffman decoder for streams whose header names a rune >= 0x80: what k_huff_batch_rune_enc (huff_rune.hip)
// and the single call write for UTF-8 text and for bytes that are no UTF-8 at all (rsn_huffman_decompress_batch and its device, layered
// and round-trip forms).  The byte decoders' plans refuse such a stream; when a call holds HUFF_RUNE_DEC_GROUP_MIN of them they
// come here instead of taking the single call one by one: ONE launch per group, ONE workgroup of 320 threads per member.  The kernel is
// rune_dec_body and the offers are rune_dec_offer / rune_dec_offer_dev (huff_rune_dec_body.h: the header, the tree, the payload, the
// expand step, the status word -- read there what each step is), k_huff_mid_rune_dec's too, at ParseRuneSmall's limits
// (huff_parse_rune.h): 256 lanes of at most 576 bits, a promise of at most 16384 bytes.  What is this unit's own:
// LDS, static: s_raw 18464 B (the header and the table are its largest tenant), the symbols 16416 B; with the body's 5 KiB and
// lane_dec_body's own 6.6 KiB three workgroups to a CU's 160 KiB (DESIGN 4.7 has the compile remarks).
#include "huff_rune_dec_body.h"

namespace rsn {
namespace {

using RS = ParseRuneSmall;
using RD = RuneDecLds<RS>;
static_assert(RD::T == DT, "lane_dec_body's threads at the byte decoders' shape: 256 lanes and the wavefront of the first lane");

__global__ __launch_bounds__(RD::T) void k_huff_batch_rune_dec(const SmallMember *__restrict__ tab, uint8_t *__restrict__ base) {
    __shared__ uint4 s_raw[RD::RAW_BYTES / 16];                     // the header and the table; then the payload's words; then the output image
    __shared__ __attribute__((aligned(16))) uint8_t s_sym[RD::SYM_BYTES];   // a leaf rank per symbol
    rune_dec_body<RS>(tab, base, s_raw, s_sym);
}

// ---- the device form's second plan launch (huff_rune_dec_plan.h: rune_plan_body), at this class's limits
__global__ __launch_bounds__(RP_T) void k_huff_dev_rune_plan(const PlanEntry *__restrict__ tab, HuffDevSummary *__restrict__ sums) { rune_plan_body<RS>(tab, sums); }

struct RuneDecClass {
    using L = RS;
    static constexpr Slot slot = Slot::GD_RUNE_PLANS;
    static constexpr const char *plan_name = "rune";
    static int plan_launch(Ctx &c, hipStream_t s, uint32_t k, const PlanEntry *d_tab, HuffDevSummary *d_sum) {
        RSN_LAUNCH("huff_dev_rune_plan", k_huff_dev_rune_plan, dim3(k), dim3(RP_T), 0, s, d_tab, d_sum);
        return RSN_OK;
    }
    static int launch(Ctx &c, hipStream_t s, uint32_t g, const SmallMember *tab, uint8_t *base) {
        RSN_LAUNCH("huff_batch_rune_dec", k_huff_batch_rune_dec, dim3(g), dim3(RD::T), 0, s, tab, base);
        return RSN_OK;
    }
};

}  // namespace

const BehindClass &huff_rune_dec_class() {
    static const BehindClass dec = {BehindClass::REST, rune_dec_offer<RuneDecClass>, rune_dec_offer_dev<RuneDecClass>};
    return dec;
}

}  // namespace rsn
