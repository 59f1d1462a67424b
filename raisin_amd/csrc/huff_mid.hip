// huff_mid.hip -- the Huffman codec for the mid-size members of a batch: above the cutoffs of huff_small.hip's batch kernels (16 KiB of
// input; 16 KiB of payload or 32 KiB of output), up to HUFF_MID_IN_MAX bytes to compress and HUFF_MID_PAY_MAX bytes of payload that decode
// to at most HUFF_MID_OUT_MAX bytes.
//
// Inside a batch such a member used to be a single call: two launches and two host round trips to compress, one launch of up to 32
// workgroups to decompress.  Here it is ONE workgroup of a launch that holds many members, with the bodies of the small batch kernels
// (huff_small_body.h) at a larger shape:
//   compress    huff_enc_body at 1024 threads: the member in LDS (64 KiB), counted there; ranks and header entries by block scans; one
//               wavefront builds the Go-exact tree (huff_plan_small.h); every byte's first bit from a block scan of the code lengths, 16 KiB
//               of the member a round; the codes ORed into an LDS image of the stream (57 KiB + the header) that leaves in 16-byte units.
//   decompress  small_dec_body, one block alone, at 960 lanes of at most 480 bits (and the wavefront of the first lane's entry): the payload
//               in LDS (56 KiB), the lanes' maps of up to four phases, a wavefront scan, the output image in LDS (64 KiB).
// Both take about 130 KiB of the CU's 160 KiB of LDS, so a CU holds one workgroup, and 1024 threads are what fills its four SIMDs.
// What a kernel does not take it hands back (GROUP_BACK / status 1), and that member goes through the single call, which words the errors.
// No workgroup waits for another; every loop is bounded by the member's size or a constant; the status word is a member's last store.
#include "huff_small_body.h"

namespace rsn {
namespace {

constexpr int HM_T = 1024;                        // threads of a workgroup
// ---- the encoder's arithmetic at n <= HUFF_MID_IN_MAX (what huff_enc_body and huff_plan_small.h rely on)
static_assert(HUFF_MID_IN_MAX == SMALL_MAX, "the class ends where the single call's small path ends");
static_assert(HUFF_MID_IN_MAX - 1 < PLAN_COUNT_LIMIT, "two distinct bytes at least: every count is at most n - 1 = 65535");
static_assert(((unsigned long long)HUFF_MID_IN_MAX << 8) < (1ull << 32) && HUFF_MID_IN_MAX < (1u << 24), "a sum of counts and a node id pack into one word (plan_item)");
static_assert(128 * (5 + 1 + 1) + 1 + 3 <= HDR_MAX, "128 entries of five digits, '|' and a byte (the newline's: two), \"\\\\\\n\" and the pad byte");
// a code of d bits needs counts that sum to at least fib(d + 2) (Fibonacci counts are the worst case): fib(24) = 46368 <= 65536 < fib(25)
static_assert(plan_fib(24) <= HUFF_MID_IN_MAX && plan_fib(25) > HUFF_MID_IN_MAX, "the deepest code of a member is 22 bits: inside the 24 of the emit table");
// the flat 7-bit code is a prefix code of a byte alphabet, and Huffman's is no longer than any: the payload is at most 7 n / 8 bytes
static_assert((unsigned long long)HUFF_MID_IN_MAX * 7 <= (unsigned long long)HUFF_MID_PAY_MAX * 8, "the payload of the largest member");
constexpr uint32_t HM_IMG_WORDS = ((HDR_MAX + HUFF_MID_PAY_MAX + 64) / 4 + 3) & ~3u;
static_assert(huff_mid_enc_out_slot(HUFF_MID_IN_MAX) / 4 <= HM_IMG_WORDS && HM_IMG_WORDS % 4 == 0, "the image holds the largest member's slot, in 16-byte units");
// ---- LDS of the encoder (dynamic; offsets in bytes).  Beside it huff_enc_body's own: 16 x 128 counts, the tables, the scan's words
constexpr uint32_t EL_IN = 0;                                    // the member
constexpr uint32_t EL_IMG = EL_IN + HUFF_MID_IN_MAX;             // the image of the stream
constexpr uint32_t EL_BYTES = EL_IMG + HM_IMG_WORDS * 4;
static_assert(EL_IMG % 16 == 0 && EL_BYTES + 12 * 1024 <= 160 * 1024, "LDS of k_huff_mid_enc");

// ---- the decoder's shape: 15 wavefronts of lanes and the sixteenth for the first lane's entry
constexpr int HM_DL = HM_T - 64;
constexpr uint32_t HM_S_MAX = 480;                               // bits per lane at most, in whole words
static_assert((unsigned long long)HM_DL * HM_S_MAX >= (unsigned long long)HUFF_MID_PAY_MAX * 8, "960 lanes of 480 bits hold the largest payload");
constexpr uint32_t HM_PAY_WORDS = HM_DL * HM_S_MAX / 32 + 8;
// ---- LDS of the decoder (dynamic).  Beside it small_dec_body's own: the 2 KiB table, the tree, 960 lanes' maps (11 KiB), the member's entry
constexpr uint32_t DL_OUT = 0;                                   // the output image
constexpr uint32_t DL_PAY = DL_OUT + ((HUFF_MID_OUT_MAX + 32 + 15) & ~15u);   // the payload's words
constexpr uint32_t DL_BYTES = DL_PAY + HM_PAY_WORDS * 4;
static_assert(DL_BYTES + 16 * 1024 <= 160 * 1024, "LDS of k_huff_mid_dec");

__global__ __launch_bounds__(HM_T) void k_huff_mid_enc(const SmallMember *__restrict__ tab, uint8_t *__restrict__ base) {
    extern __shared__ uint4 hm_lds[];
    uint8_t *sm = reinterpret_cast<uint8_t *>(hm_lds);
    huff_enc_body<HM_T, HUFF_MID_IN_MAX, HM_IMG_WORDS, true>(tab, base, reinterpret_cast<uint4 *>(sm + EL_IN), reinterpret_cast<uint32_t *>(sm + EL_IMG),
                                                             [](uint32_t n) { return huff_mid_enc_out_slot(n); });
}

__global__ __launch_bounds__(HM_T) void k_huff_mid_dec(const SmallDecArgs *__restrict__ tab) {
    extern __shared__ uint4 hm_lds[];
    __shared__ SmallDecArgs s_a;
    uint8_t *sm = reinterpret_cast<uint8_t *>(hm_lds);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(tab + blockIdx.x);
    for (uint32_t i = threadIdx.x; i < sizeof(SmallDecArgs) / 4; i += HM_T) reinterpret_cast<uint32_t *>(&s_a)[i] = src[i];
    __syncthreads();
    small_dec_body<HM_PAY_WORDS, HUFF_MID_OUT_MAX, false, HM_DL>(s_a, reinterpret_cast<uint32_t *>(sm + DL_PAY), sm + DL_OUT);
}

int launch_mid_dec(Ctx &c, hipStream_t s, uint32_t g, const SmallDecArgs *tab) {
    const int rc = func_dyn_lds(c, reinterpret_cast<const void *>(k_huff_mid_dec), DL_BYTES); if (rc) return rc;
    RSN_LAUNCH("huff_batch_mid_dec", k_huff_mid_dec, dim3(g), dim3(HM_T), DL_BYTES, s, tab);
    return RSN_OK;
}

// The header alone decides (huffman.go:196-227,261): the payload is what lies behind "\\\n" and the pad byte, the output is the sum of the
// counts.  This runs for every member of a decompress batch, the small kernel's thousands included, so it allocates nothing and looks at
// the header only where the stream's length leaves the class open: a symbol takes a bit at least, so a payload of 4 KiB cannot promise more
// than huff_batch_dec holds.  The sum is parse_header's scan of the counts without its table: an entry that occurs twice counts twice,
// and runes are not looked at -- an upper bound that is exact for every header an encoder writes.  The group's own plan
// (small_dec_plan) is exact and hands back what it refuses.
constexpr HuffDecShape MID_DEC_SHAPE = {HM_DL, HM_S_MAX, HUFF_MID_PAY_MAX, HUFF_MID_OUT_MAX};
// the class's cutoffs, stated once for both forms of takes: within what one workgroup holds here, and beyond what k_huff_batch_dec's does
bool mid_dec_wants(size_t pay, unsigned long long expect) {
    if (pay > MID_DEC_SHAPE.pay_max || expect > MID_DEC_SHAPE.out_max) return false;
    return pay > HB_PAY_MAX || expect > HB_OUT_MAX;                    // (the rest is k_huff_batch_dec's)
}
bool mid_dec_takes(const uint8_t *in, size_t n, int64_t) {
    if (n < 8 || n > HDR_MAX + 8 + HUFF_MID_PAY_MAX || 8 * n <= HB_OUT_MAX) return false;
    size_t pay = 0; unsigned long long expect = 0;
    return huff_dec_promise(in, n, &pay, &expect, [](size_t p) { return p <= HUFF_MID_PAY_MAX && !(p <= HB_PAY_MAX && 8 * p <= HB_OUT_MAX); }) && mid_dec_wants(pay, expect);
}
// ... and from the plan's figures, once k_huff_dev_plan has read the header where it lies: the code bits in whole bytes stand for the payload
// (the same number for every stream whose pad byte is below 8, as an encoder writes it)
bool mid_dec_takes_plan(size_t n, const HuffDevSummary &sum) {
    return n >= 8 && n <= HDR_MAX + 8 + HUFF_MID_PAY_MAX && mid_dec_wants((sum.span + 7) / 8, sum.expect) && huff_dec_shape_takes(MID_DEC_SHAPE, sum);
}

bool mid_enc_takes(const uint8_t *, size_t n, int64_t) { return n > HE_IN_MAX && n <= HUFF_MID_IN_MAX; }   // (asked after the small class)
struct MidEncClass {
    static constexpr const char *what = "huffman batch compress";
    static size_t in_bytes(size_t n) { return huff_enc_in_slot(n); }
    static size_t out_bytes(size_t n) { return huff_mid_enc_out_slot((uint32_t)n); }
    static int launch(Ctx &c, hipStream_t s, uint32_t g, const SmallMember *tab, uint8_t *base, int64_t) {
        const int rc = func_dyn_lds(c, reinterpret_cast<const void *>(k_huff_mid_enc), EL_BYTES); if (rc) return rc;
        RSN_LAUNCH("huff_batch_mid_enc", k_huff_mid_enc, dim3(g), dim3(HM_T), EL_BYTES, s, tab, base);
        return RSN_OK;
    }
};
int mid_dec_run(Ctx &c, const std::vector<size_t> &idx, const uint8_t *const *ins, const size_t *lens, int64_t,
                const SmallTake &take, std::vector<size_t> &back, size_t *failed, std::vector<size_t> *) {
    return huff_dec_run(c, MID_DEC_SHAPE, launch_mid_dec, idx, ins, lens, take, back, failed);
}
int mid_dec_run_dev(Ctx &c, hipStream_t s, const std::vector<size_t> &idx, const rsn_dev_member *mem, int64_t, const DevPlans *plans, std::vector<uint32_t> &answers) {
    return huff_dec_run_dev(c, s, MID_DEC_SHAPE, launch_mid_dec, idx, mem, *plans, answers);
}
}  // namespace
// (the scan above, for the tiled class too: huff_big_dec.hip)
bool huff_dec_promise(const uint8_t *in, size_t n, size_t *pay_out, unsigned long long *expect_out, bool (*pay_open)(size_t pay)) {
    size_t sep = (size_t)-1;
    for (size_t i = 0; i + 1 < std::min<size_t>(n, HDR_MAX + 8); i++) if (in[i] == 0x5C && in[i + 1] == 0x0A) { sep = i; break; }
    if (sep == (size_t)-1 || sep + 4 > n) return false;
    const size_t pay = n - sep - 3;
    if (pay_open && !pay_open(pay)) return false;
    unsigned long long expect = 0, acc = 0;
    for (size_t i = 0; i < sep; i++) {
        const uint8_t ch = in[i];
        if (ch >= '0' && ch <= '9') { acc = std::min<unsigned long long>(acc * 10 + (ch - '0'), 1ull << 40); continue; }
        if (ch != '|') continue;
        expect += acc; acc = 0;
        i += (i + 2 < sep && in[i + 1] == 0x5C && in[i + 2] == 'n') ? 2 : 1;      // the entry's byte is not a count's digit
    }
    *pay_out = pay; *expect_out = expect;
    return true;
}
const BatchClass &huff_mid_class(bool compress) {
    static const BatchClass enc = {"huffman mid compress", HUFF_MID_GROUP_MIN, mid_enc_takes, class_run<MidEncClass>, class_run_dev<MidEncClass>},
                            dec = {"huffman mid decompress", HUFF_MID_GROUP_MIN, mid_dec_takes, mid_dec_run, mid_dec_run_dev, mid_dec_takes_plan};
    return compress ? enc : dec;
}

}  // namespace rsn
