// codecs.h -- device-resident codec entry points shared between translation units.
#pragma once

#include <algorithm>
#include <functional>

#include "group_layout.h"
#include "huff_host.h"
#include "lzss_legacy.h"
#include "rsn_common.h"
#include "huff_parse_small.h"   // (behind the HIP runtime: its functions are __host__ __device__ under hipcc)
#include "huff_rune_select.h"
#include "huff_rune_mid_select.h"
#include "huff_parse_rune.h"    // (the rune decoders' limits, named below)
#include "huff_big_layout.h"      // (the tiled classes' layout headers, behind the HIP runtime as well: their limits are stated there and named here)
#include "huff_big_dec_layout.h"
#include "lzss_tile_layout.h"
#include "lzss_tile_dec_layout.h"

namespace rsn {

// an optimal prefix code never costs more than the fixed-length code: <= 21 bits per rune
constexpr size_t huff_compress_bound(size_t n) { return n * 21 / 8 + (n < kMaxRune ? n : (size_t)kMaxRune) * 26 + 96; }
size_t lzss_compress_bound(size_t n);

// All four: buffers are device pointers (16-byte aligned), the call synchronises
// `s` before returning, *out_n is the exact result size; on RSN_ERR_CAPACITY it
// is the capacity that would have sufficed.
int huff_encode_dev(Ctx &c, hipStream_t s, const uint8_t *d_in, size_t n, uint8_t *d_out, size_t out_cap, size_t *out_n,
                    HuffTree *tree_out, HuffCodes *codes_out);
// the same in two halves, for one stream out of several slices of the input (rsn_huffman_compress_sharded, rsn_api.hip)
struct HuffSlice { uint32_t tile = 0, n_tiles = 0; uint32_t *d_tile_hist = nullptr; uint16_t *d_smask = nullptr; bool ascii = true; std::vector<HuffSym> syms; };
int huff_slice_hist(Ctx &c, hipStream_t s, const uint8_t *d_in, size_t n, HuffSlice &sl);
int huff_slice_emit(Ctx &c, hipStream_t s, const uint8_t *d_in, size_t n, const HuffSlice &sl, const HuffTree &tree, const HuffCodes &codes, bool flat,
                    const std::string &hdr, unsigned long long base_bits, unsigned long long slice_bits, uint8_t *d_out);
bool huff_flat_code(const HuffTree &tree, const HuffCodes &codes);
// A host-buffer decode in SLICES (rsn_api.hip: the upload is still running while the first slices decode, and their bytes go down while
// the later ones decode): the decoder asks for its input as it needs it and announces its output as it becomes final.  The stream is one
// bit string without a block index (huffman.go:258-297), so a slice starts exactly where its predecessor's last codeword ended -- the
// hand-over is that bit position and the output offset, nothing else.
struct SliceStream {
    std::function<bool(size_t)> need_in;            // returns once d_in[0, bytes) is on the device; false: give up (the call fails)
    std::function<bool(size_t, size_t)> have_out;   // d_out[off, off + len) is final; false: give up
    std::function<size_t()> in_so_far;              // how much of d_in is on the device now (does not wait; may be empty)
    size_t slice_bytes = (size_t)32 << 20;          // payload bytes per slice (a multiple of 8 KiB: whole blocks of subsequences)
};
int huff_decode_dev(Ctx &c, hipStream_t s, const uint8_t *d_in, size_t n, uint8_t *d_out, size_t out_cap, size_t *out_n, const SliceStream *st = nullptr);
int lzss_encode_dev(Ctx &c, hipStream_t s, const uint8_t *d_in, size_t n, int64_t window, uint8_t *d_out, size_t out_cap, size_t *out_n);
// the same in SECTIONS as the input lands (a host-buffer call, rsn_api.hip): returns 1 when the input is not for it -- something in it needs
// an escape, or the window is not one the sections take -- and the caller encodes it whole.  slice_bytes = positions per section.
int lzss_encode_sliced(Ctx &c, hipStream_t s, const uint8_t *d_in, size_t n, int64_t window, uint8_t *d_out, size_t out_cap, size_t *out_n, const SliceStream &st);
// host buffers of at most 64 KiB, byte alphabets (huff_small.hip): two launches / one launch, no copy command; 1 = not for this path.
// *out: the result in the context's pinned staging (valid until the thread's next call), for the caller to copy
int huff_small_compress(Ctx &c, const uint8_t *in, size_t n, const uint8_t **out, size_t *out_n);
int huff_small_decompress(Ctx &c, const uint8_t *in, size_t n, const uint8_t **out, size_t *out_n);
// host buffers of at most 2 KiB (lzss_small.hip): one launch of one block each way, no copy command; 1 = not for this path
int lzss_small_compress(Ctx &c, const uint8_t *in, size_t n, int64_t window, const uint8_t **out, size_t *out_n);
int lzss_small_decompress(Ctx &c, const uint8_t *in, size_t n, const uint8_t **out, size_t *out_n);
int lzss_decode_dev(Ctx &c, hipStream_t s, const uint8_t *d_in, size_t n, uint8_t *d_out, size_t out_cap, size_t *out_n);

// ---- many members in one launch (the batch calls, rsn_api.hip).  A CLASS of members is what one grouped kernel takes, a
// workgroup per member: the small and the mid-size members of each layer and direction, eight rows -- and four whose
// members take a workgroup per TILE, the big members of Huffman compress (huff_big.hip), of Huffman decompress (huff_big_dec.hip), of
// LZSS compress (lzss_tile.hip) and, behind the rows, of LZSS decompress (lzss_tile_dec.hip).
// The contract of every row:
//   takes(in, n, window)   whether the member is of the class, asked in the order of batch_classes' rows (a later row need not exclude
//                          what an earlier one takes).  Fewer than group_min members of a class in a call are not grouped: a workgroup each
//                          against the whole device a single call has (the minimums are measured).
//   run(...)               the members `idx` (indexes into ins / lens, all of the class) are packed into the calling thread's pinned
//                          staging in groups of at most SMALL_GROUP_MAX members and SMALL_GROUP_BYTES, and each group is ONE launch
//                          (run_groups, group_run.h).  take(i, p, len) receives member i's result (p: in the staging, valid during the
//                          call; a non-zero return stops the call with that code); a member the kernel hands back -- or, for the Huffman
//                          decoders, one whose header the host's plan refuses -- is appended to `back`, in index order, for the caller's
//                          single call.  A failure returns its code with *failed = the group's first member (staging, launch, wait) or
//                          the member itself (take).  back_runes (may be null): receives, instead of `back`, the members a kernel hands
//                          back as GROUP_BACK_RUNES (group_layout.h) -- the Huffman byte encoders' "a byte >= 0x80 and nothing else".
struct SmallMember { uint32_t in_off, n, out_off, status_off; };   // byte offsets into the group's staging
constexpr size_t SMALL_GROUP_BYTES = (size_t)16 << 20;             // staging of one group (a member larger than that is a group of its own)
constexpr size_t SMALL_GROUP_MAX = 4096;                           // members of one group
using SmallTake = std::function<int(size_t i, const uint8_t *p, size_t len)>;
// what the Huffman decompress batch on device buffers knows of its members before it classifies them (huff_dev.hip: huff_dev_plan): the
// candidates' summaries as k_huff_dev_plan wrote them and the device table of their plans.  at[i]: member i's entry in both, DEV_PLAN_NONE
// where the member is no candidate.
constexpr uint32_t DEV_PLAN_NONE = 0xFFFFFFFFu;
struct DevPlans {
    std::vector<uint32_t> at;
    std::vector<HuffDevSummary> sum;
    const HuffDevPlan *d_table = nullptr;
    const HuffDevSummary *of(size_t i) const { return at[i] == DEV_PLAN_NONE ? nullptr : &sum[at[i]]; }
};
struct BatchClass {
    const char *name;
    size_t group_min;
    bool (*takes)(const uint8_t *in, size_t n, int64_t window);
    int (*run)(Ctx &c, const std::vector<size_t> &idx, const uint8_t *const *ins, const size_t *lens, int64_t window,
               const SmallTake &take, std::vector<size_t> &back, size_t *failed, std::vector<size_t> *back_runes);
    // the device-buffer form (the batch calls on device buffers; group_run.h: run_groups_staged): the members `idx` of `mem` through the same
    // groups and the same kernel on `s`, the staging in device scratch; answers[k]: GROUP_BACK, or member idx[k]'s length -- its bytes are in
    // its d_out when that is at most its out_cap.  plans: null but for the Huffman decoders, whose table entries are completed on the device
    // from the plans.
    int (*run_dev)(Ctx &c, hipStream_t s, const std::vector<size_t> &idx, const rsn_dev_member *mem, int64_t window, const DevPlans *plans, std::vector<uint32_t> &answers);
    // takes() for a member whose bytes lie in device memory, from its length and its plan's summary (a planned one): the same cutoffs.
    // Null where takes() looks at no byte of the member and serves both forms.
    bool (*takes_plan)(size_t n, const HuffDevSummary &sum) = nullptr;
};
// lzss_small.hip: what lzss_small_compress / _decompress take (1 KiB with a window <= 0xFFFF; 2 KiB of stream).
// lzss_mid.hip: a workgroup keeps the member's whole escaped stream in LDS.  The encoder takes LZSS_MID_IN_MAX bytes with a window of 1 to
// 4096 and hands back what escapes to more than LZSS_MID_E_MAX bytes (what LDS holds beside the search structure); the decoder takes a
// stream of at most LZSS_MID_E_MAX bytes that expands to at most as many -- so every stream the encoder writes is one the decoder takes.
// A group takes as long as its largest member, 6.7 ms for 64 KiB of text; from LZSS_MID_GROUP_MIN members on it is no slower than the
// loop of single calls at every size.  Mirrored as raisin_amd.lz.MID_IN_MAX / MID_E_MAX / MID_GROUP_MIN.
constexpr uint32_t LZSS_MID_IN_MAX = 65536;
constexpr uint32_t LZSS_MID_E_MAX = 69632;
constexpr size_t LZSS_MID_GROUP_MIN = 64;
const BatchClass &lzss_small_class(bool compress), &lzss_mid_class(bool compress);
// lzss_tile.hip: the compress direction above the mid class.  A member of more than LZSS_MID_IN_MAX and at most LZSS_TILE_IN_MAX bytes
// (window 1 to 4096) does not fit a workgroup, and a workgroup a member would leave the device idle, so its escaped stream is cut into
// tiles of LZSS_TILE_POS positions and a group is FOUR launches with nothing on the host between them: a workgroup per member escapes it
// into scratch, a workgroup per tile searches it (the window in front and the look-ahead behind in LDS; the chain walk is the mid
// kernel's, lzss_enc_body.h), a workgroup per member walks the greedy chain and sizes the items, and a workgroup per tile stores its bytes
// (lzss_tile_layout.h: the tiles, the scratch, which tile stores which byte).  It hands back what escapes to more than LZSS_TILE_E_MAX
// bytes or to more than one and a half times the member, and -- as the mid class -- runs and short periods (the step cap).  Both forms
// run on device staging, in groups of up to LZSS_TILE_GROUP_BYTES.  The streams decode through the tiled decoder below inside a
// decompress batch.  LZSS_TILE_IN_MAX, LZSS_TILE_GROUP_MIN: DESIGN 4.7 and profiles/lzss_tile_batch.txt.
// Mirrored as raisin_amd.lz.TILE_IN_MAX / TILE_E_MAX / TILE_POS / TILE_GROUP_MIN / TILE_GROUP_BYTES.
// A PROBE build widens the class to measure where it should end (scripts/probes/lzss_tile_batch.py; Makefile: EXTRA=-DRSN_LZSS_TILE_IN_MAX=...
// -DRSN_LZSS_TILE_GROUP_MIN=...); every other build has the two measured values (RSN_LZSS_TILE_IN_MAX's: lzss_tile_layout.h).
#ifndef RSN_LZSS_TILE_GROUP_MIN
#define RSN_LZSS_TILE_GROUP_MIN 16
#endif
constexpr uint32_t LZSS_TILE_IN_MAX = LZT_IN_MAX;
constexpr uint32_t LZSS_TILE_E_MAX = LZT_E_MAX;
constexpr uint32_t LZSS_TILE_POS = LZT_TILE;
constexpr size_t LZSS_TILE_GROUP_MIN = RSN_LZSS_TILE_GROUP_MIN;
constexpr size_t LZSS_TILE_GROUP_BYTES = 67108864;
static_assert(LZT_IN_MIN == LZSS_MID_IN_MAX, "the tiled class begins where the mid class ends");
static_assert(LZSS_TILE_E_MAX < (1u << 31) && 4096 < (1u << 15) && LZSS_TILE_IN_MAX > LZSS_MID_IN_MAX && LZSS_TILE_GROUP_MIN >= 2,
              "a key is L << 16 | distance with its top bit free: L <= distance <= the window, 13 bits each, exact whatever E is; positions are words");
const BatchClass &lzss_tile_class();
// huff_small.hip: inputs of 2 B to 16 KiB (two members at least: a group's one serial tree against the host's); streams short enough for
// k_huff_batch_dec's workgroup.
// huff_mid.hip: a workgroup of 1024 threads keeps the whole member and the whole image of its stream in LDS, one workgroup to a CU.  The
// encoder takes more than 16 KiB and at most HUFF_MID_IN_MAX bytes of a byte alphabet (every byte < 0x80, two distinct bytes at least) and
// hands the rest back; a byte of such an alphabet codes in at most 7 bits, so its payload is at most 7/8 of the input: HUFF_MID_PAY_MAX.
// The decoder takes, by its header, a stream that promises at most HUFF_MID_OUT_MAX bytes from at most HUFF_MID_PAY_MAX bytes of payload,
// and that k_huff_batch_dec's workgroup does not hold -- so every stream the encoder writes is one a grouped decoder takes.  Two such
// members lose to the loop of single calls (0.6x to compress), from HUFF_MID_GROUP_MIN on no size does in either direction.
// Mirrored as raisin_amd.huffman.MID_IN_MAX / MID_PAY_MAX / MID_OUT_MAX / MID_GROUP_MIN.
constexpr uint32_t HUFF_MID_IN_MAX = 65536;
constexpr uint32_t HUFF_MID_PAY_MAX = 57344;
constexpr uint32_t HUFF_MID_OUT_MAX = 65536;
constexpr size_t HUFF_MID_GROUP_MIN = 4;
static_assert((unsigned long long)HUFF_MID_PAY_MAX * 8 >= (unsigned long long)HUFF_MID_IN_MAX * 7 && HUFF_MID_OUT_MAX >= HUFF_MID_IN_MAX,
              "the decoder takes every stream the encoder writes");
const BatchClass &huff_small_class(bool compress), &huff_mid_class(bool compress);
// huff_big.hip: the compress direction above the mid class.  A member of more than HUFF_MID_IN_MAX and at most HUFF_BIG_IN_MAX bytes of a
// byte alphabet does not fit a workgroup, so it is cut into tiles of HUFF_BIG_TILE bytes and a group is THREE launches with nothing on
// the host between them: a workgroup per tile counts it, a workgroup per member sums the tiles' counts, builds the Go-exact tree in one
// wavefront (huff_plan_small.h), writes the header and scans the tiles' bit lengths, and a workgroup per tile codes it at its bit offset
// (huff_big_layout.h: the tiles, the scratch, which tile stores which byte).  It hands back what the mid class hands back, and a member
// whose deepest code has more than the 24 bits of the emit table's entry -- possible from fib(27) = 196418 bytes on.  Both forms run on
// device staging: the host form copies a run's inputs up and its results down (a member is read twice: never out of pinned host memory).
// Its groups hold up to HUFF_BIG_GROUP_BYTES of staging: a group of the other classes' 16 MiB would hold 32 members of 256 KiB, two tiles a CU.  The streams
// decode through the tiled decoder below inside a decompress batch.  HUFF_BIG_GROUP_MIN, HUFF_BIG_IN_MAX: measured,
// DESIGN 4.7 and profiles/huff_big_batch.txt.  Mirrored as raisin_amd.huffman.BIG_IN_MAX / BIG_TILE / BIG_GROUP_MIN / BIG_GROUP_BYTES.
constexpr uint32_t HUFF_BIG_IN_MAX = BIGL_IN_MAX;
constexpr uint32_t HUFF_BIG_TILE = BIGL_TILE;
constexpr size_t HUFF_BIG_GROUP_MIN = 4;
constexpr size_t HUFF_BIG_GROUP_BYTES = 67108864;
const BatchClass &huff_big_class();
// huff_big_dec.hip: the way back.  A stream of a byte alphabet that promises more than HUFF_MID_OUT_MAX and at most HUFF_BIG_OUT_MAX bytes
// from at most HUFF_BIG_PAY_MAX bytes of payload is cut into tiles of its PAYLOAD (huff_big_dec_layout.h: 960 lanes of 64 code bits, 7680
// bytes) and a group is three launches with nothing on the host between them: a workgroup per tile answers all 32 bits the tile could be
// entered at (lane_dec_body's map, huff_small_body.h), a wavefront per member composes the tiles' maps into every tile's true entry, first
// output byte and symbol count and gives the whole verdict, and a workgroup per tile of a taken member decodes it from its entry and stores
// its own output bytes.  No workgroup waits for another.  Handed back, to the single call: what the wide plan refuses (huff_parse_small.h:
// runes, foreign headers, codes beyond 32 bits), more than four phases or DEC_ROUNDS in a tile, a tile of more symbols than the emit
// image holds (below 1.9 bits a symbol over a whole tile), malformed streams.  Both forms run on device staging, in groups of up to
// HUFF_BIG_GROUP_BYTES, as the encoder's do.  HUFF_BIG_DEC_GROUP_MIN, HUFF_BIG_OUT_MAX: DESIGN 4.7 and profiles/huff_big_dec_batch.txt.
// Mirrored as raisin_amd.huffman.BIG_OUT_MAX / BIG_PAY_MAX / BIG_DEC_GROUP_MIN / BIG_DEC_LANES / BIG_DEC_LANE_BITS / BIG_DEC_OUT_CAP.
constexpr uint32_t HUFF_BIG_OUT_MAX = BIGD_OUT_MAX;
constexpr uint32_t HUFF_BIG_PAY_MAX = BIGD_PAY_MAX;
constexpr size_t HUFF_BIG_DEC_GROUP_MIN = 4;
static_assert((unsigned long long)HUFF_BIG_PAY_MAX * 8 >= (unsigned long long)HUFF_BIG_IN_MAX * 7 && HUFF_BIG_OUT_MAX >= HUFF_BIG_IN_MAX,
              "the decoder takes every stream the encoder writes");
const BatchClass &huff_big_dec_class();
// ---- the second stage.  A class BEHIND the rows has no takes(): what the rows' kernels answered says which members are its.  Once the
// rows have run, every flow (rsn_api.hip: batch_front, layer_batch_run) OFFERS it one POOL of members -- RUNES: those the rows handed back
// as GROUP_BACK_RUNES; REST: everything left for the single call so far -- in one loop over what batch_classes lists behind the rows, and
// it runs grouped those it chooses when there are at least its minimum of them (huff_rune_select.h: the rules).
//   offer       host form: the members it runs leave the pool, take() receives their results; what its kernel hands back joins `rest`
//               (a REST pool is `rest`), which the flow sorts afterwards.  *failed as run() sets it.  The classes of a RUNES pool are
//               offered it in the order listed: one that is not the last leaves in the pool, sorted, whatever it does not run, for the
//               next; the LAST sends whatever else the pool held to `rest` and leaves the pool empty.
//   offer_dev   device form, the same choice: the members it runs leave the pool for `idx` (which comes empty), answers[k] is idx[k]'s, and the flow settles
//               them as a row's.  A failure is about behind_failed: the first member chosen, or, when none was yet, the lowest offered.
struct BehindClass {
    enum Pool { RUNES, REST } pool;
    int (*offer)(Ctx &c, std::vector<size_t> &pool, std::vector<size_t> &rest, const uint8_t *const *ins, const size_t *lens, const SmallTake &take, size_t *failed);
    int (*offer_dev)(Ctx &c, hipStream_t s, std::vector<size_t> &pool, std::vector<size_t> &rest, const rsn_dev_member *mem, const DevPlans *plans,
                     std::vector<size_t> &idx, std::vector<uint32_t> &answers);
};
inline size_t behind_failed(const std::vector<size_t> &idx, const std::vector<size_t> &pool) { return !idx.empty() ? idx[0] : pool.empty() ? 0 : *std::min_element(pool.begin(), pool.end()); }
// huff_rune.hip: the members of at most HUFF_RUNE_IN_MAX bytes that k_huff_batch_enc hands back as GROUP_BACK_RUNES -- UTF-8 text, bytes
// that are no UTF-8 at all -- a workgroup each in k_huff_batch_rune_enc (its body: huff_rune_body.h): the runes as Go's `range string(b)` yields them counted in an
// LDS table, the Go-exact tree of 2 to HUFF_RUNE_SYMS_MAX leaves in one wavefront (huff_plan_rune.h), header and code bits as the byte
// encoder writes them.  It hands back more distinct runes than that, and a single one.  Behind the rows of Huffman compress, pool RUNES:
// a call that holds at least HUFF_RUNE_GROUP_MIN such members runs them; fewer take the single call, as every one did before.
// HUFF_RUNE_GROUP_MIN = 16 is the floor, not a crossover: calls with up to 12 such members keep their launches as they were, and at 16
// members the grouped route already is 8 to 27 times as fast as the single calls it replaces, at 25 B, 1 KiB and 16 KiB, from host and
// from device buffers -- no count tried (16 to 4096) loses at any size (profiles/huff_rune_batch.txt).
// Mirrored as raisin_amd.huffman.RUNE_SYMS_MAX / RUNE_GROUP_MIN.
constexpr uint32_t HUFF_RUNE_SYMS_MAX = 256;
const BehindClass &huff_rune_class();
// huff_rune_mid.hip: the same for the members of more than HUFF_RUNE_IN_MAX and at most HUFF_RUNE_MID_IN_MAX bytes that k_huff_mid_enc hands
// back as GROUP_BACK_RUNES -- a workgroup of 1024 threads each in k_huff_mid_rune_enc, the member and the image of its stream in LDS, one
// workgroup to a CU as in the mid class: the 16 KiB kernel's body (huff_rune_body.h) with its runes, table, plan and header, counts up to 65535 (PLAN_RUNE_MID_COUNT_MAX),
// the bits a round of 16 KiB at a time.  It hands back what the 16 KiB class hands back: more than HUFF_RUNE_SYMS_MAX distinct runes, a
// single one.  Behind the rows of Huffman compress, pool RUNES, listed AHEAD of huff_rune_class (which would send these members to `rest`,
// where nothing says any more that they were rune members): a call that holds at least HUFF_RUNE_MID_GROUP_MIN such members runs them and
// leaves the others in the pool; fewer stay in the pool, all of them, and take the single call as every one did before.  Rune members above
// HUFF_RUNE_MID_IN_MAX (huff_big.hip's hand-backs) are not this class's.  Its streams decode grouped too, through huff_rune_mid_dec_class
// below (the 16 KiB rune decoder ends at HUFF_RUNE_OUT_MAX).  HUFF_RUNE_MID_GROUP_MIN = 16 is the floor, for the reason HUFF_RUNE_GROUP_MIN
// gives, not a crossover: at 16 members the grouped route is 6.8 to 11 times as fast as the single calls it replaces, at 20, 32 and 64 KiB,
// from host and from device buffers, and no count tried (16 to 256) loses at any size, so HUFF_RUNE_MID_IN_MAX stays at the mid class's
// 65536 (profiles/huff_rune_mid_batch.txt).  Mirrored as raisin_amd.huffman.RUNE_MID_IN_MAX / RUNE_MID_GROUP_MIN.
const BehindClass &huff_rune_mid_class();
// huff_rune_dec.hip: the way back.  A stream whose header names a rune >= 0x80 -- what the byte decoders' plans refuse -- a workgroup each
// in k_huff_batch_rune_dec: the workgroup parses the header itself (huff_parse_rune.h: at most HUFF_RUNE_SYMS_MAX distinct runes, the
// Go-exact tree in one wavefront), decodes the payload with the byte decoders' lane maps (huff_small_body.h: lane_dec_body) to a leaf rank
// per symbol, and writes every rune as string(rune).  It takes a stream of at most HUFF_RUNE_STREAM_MAX bytes that promises at most
// HUFF_RUNE_OUT_MAX bytes from at most HUFF_RUNE_PAY_MAX bytes of payload (huff_parse_rune.h: ParseRuneSmall) -- so every stream the rune encoder writes for a
// member of valid UTF-8 is one this decoder takes; a byte that is no UTF-8 comes back as the three bytes of U+FFFD, so a lossy member's
// stream may promise up to three times the member's size and goes to the single call when that passes HUFF_RUNE_OUT_MAX -- and hands back what the byte decoders hand back, a code beyond 32 bits, and a stream that decodes to more
// bytes than its header promises.  Behind the rows of Huffman decompress, pool REST: the host form plans its candidates with a scan of the
// header that allocates nothing (parse_rune_light), the device form -- whose candidates are what k_huff_dev_plan answered PARSE_NOT_MINE
// -- with ONE more plan launch over them where they lie (k_huff_dev_rune_plan: one copy down, one host wait), and it runs when at least
// HUFF_RUNE_DEC_GROUP_MIN are candidates and as many of them are planned.  What the kernel hands back stays in `rest`, and so does a rune
// stream that promises more than HUFF_RUNE_OUT_MAX bytes: huff_rune_mid_dec_class, listed behind this one, is offered it next.
// HUFF_RUNE_DEC_GROUP_MIN: see DESIGN 4.7 for what was measured.  Mirrored as raisin_amd.huffman.RUNE_OUT_MAX / RUNE_PAY_MAX /
// RUNE_DEC_GROUP_MIN.
constexpr bool huff_rune_dec_takes_the_encoder() {
    for (uint32_t n = 2; n <= HUFF_RUNE_IN_MAX; n++) {
        const uint32_t hdr = (n < 256 ? n : 256u) * 10 + 3, pay = huff_rune_stream_max(n) - hdr;
        if (n > HUFF_RUNE_OUT_MAX || hdr > HUFF_RUNE_HDR_MAX || pay > HUFF_RUNE_PAY_MAX || huff_rune_stream_max(n) > HUFF_RUNE_STREAM_MAX) return false;
    }
    return true;
}
static_assert(huff_rune_dec_takes_the_encoder(), "header, payload and length of every stream the rune encoder writes are ones the rune decoder takes; valid UTF-8 decodes to the member's own n bytes");
const BehindClass &huff_rune_dec_class();
// huff_rune_mid_dec.hip: the way back for what k_huff_mid_rune_enc writes.  A rune stream of at most HUFF_RUNE_MID_STREAM_MAX bytes whose
// header promises MORE than HUFF_RUNE_OUT_MAX and at most HUFF_RUNE_MID_OUT_MAX bytes from at most HUFF_RUNE_MID_PAY_MAX bytes of payload
// (huff_parse_rune.h: ParseRuneMid) -- the lower bound is the promise, not the payload: a stream that promises less from more than
// HUFF_RUNE_PAY_MAX bytes, which no encoder writes, stays the single call's -- a workgroup of 1024 threads each in k_huff_mid_rune_dec:
// the 16 KiB kernel's steps with its code (huff_rune_dec_body.h: one body, one pair of offers; huff_parse_rune.h at ParseRuneMid's limits: counts up to
// PLAN_RUNE_MID_COUNT_MAX; lane_dec_body at 960 lanes of 576 bits), payload, ranks and image in dynamic LDS, one workgroup to a CU.  It
// hands back what the 16 KiB class hands back.  Behind the rows of Huffman decompress, pool REST, listed behind huff_rune_dec_class: its
// candidates are what that class left in `rest` with at least HUFF_RUNE_MID_DEC_PAY_MIN bytes of payload (fewer cannot decode to more than
// HUFF_RUNE_OUT_MAX), planned as that class plans -- parse_rune_light<ParseRuneMid> on the host, ONE launch of k_huff_dev_rune_mid_plan
// over what k_huff_dev_plan answered PARSE_NOT_MINE on the device -- and it runs when at least HUFF_RUNE_MID_DEC_GROUP_MIN are candidates
// and as many of them are planned.  HUFF_RUNE_MID_DEC_GROUP_MIN = 16 is the rune classes' floor (DESIGN 4.7 says what was measured).
// Mirrored as raisin_amd.huffman.RUNE_MID_OUT_MAX / RUNE_MID_PAY_MAX / RUNE_MID_DEC_GROUP_MIN.
constexpr bool huff_rune_mid_dec_takes_the_encoder() {
    for (uint32_t n = HUFF_RUNE_IN_MAX + 1; n <= HUFF_RUNE_MID_IN_MAX; n++) {
        const uint32_t hdr = (n < 256 ? n : 256u) * 10 + 3, pay = huff_rune_mid_stream_max(n) - hdr;
        if (n <= HUFF_RUNE_OUT_MAX || n > HUFF_RUNE_MID_OUT_MAX || hdr > HUFF_RUNE_HDR_MAX || pay > HUFF_RUNE_MID_PAY_MAX ||
            ((n + 3) / 4 + 7) / 8 < HUFF_RUNE_MID_DEC_PAY_MIN ||                  // (a rune is four bytes at most and takes a bit at least: the prefilter passes it)
            huff_rune_mid_stream_max(n) > HUFF_RUNE_MID_STREAM_MAX) return false;
    }
    return true;
}
static_assert(huff_rune_mid_dec_takes_the_encoder(), "header, payload and length of every stream the mid-size rune encoder writes are ones the mid-size rune decoder takes; valid UTF-8 promises the member's own n bytes (a lossy member up to 3 n: the single call's above HUFF_RUNE_MID_OUT_MAX)");
const BehindClass &huff_rune_mid_dec_class();
// lzss_tile_dec.hip: the way back for what no workgroup holds.  A stream of at most LZSS_TILE_DEC_IN_MAX bytes that expands to at most
// LZSS_TILE_DEC_OUT_MAX escaped bytes is cut into tiles of LZSS_TILE_POS bytes -- of the stream for the parse, of the escaped output for
// the copies -- and a group is FOUR launches with nothing on the host between them: a workgroup per stream tile parses its tokens, a
// workgroup per member scans the tiles' outputs and gives the verdict, a workgroup per output tile settles the copy chains inside the
// tile and leaves a descriptor for every byte that copies an earlier tile, and a workgroup per member finishes its tiles in order, unescapes
// them and stores the result (lzss_tile_dec_layout.h: the tiles, the scratch, which tile stores which byte).  What a stream expands to is
// not known before it is parsed -- a stream the mid class takes by its length is handed back when it expands beyond LZSS_MID_E_MAX, the
// ordinary case for what lzss_tile.hip writes -- so the class stands behind the rows of LZSS decompress, pool REST: its candidates are the
// members left for the single call whose stream is longer than the small decoder's 2 KiB and at most LZSS_TILE_DEC_IN_MAX, and it runs
// when there are at least LZSS_TILE_DEC_GROUP_MIN of them.  It hands back malformed streams, a pointer that starts before the data, an
// empty result and more than LZSS_TILE_DEC_OUT_MAX escaped bytes; they stay in `rest`, and the single call words the errors.  Both forms
// run on device staging, in groups of up to LZSS_TILE_GROUP_BYTES.  LZSS_TILE_DEC_GROUP_MIN: DESIGN 4.7.
// Mirrored as raisin_amd.lz.TILE_DEC_IN_MAX / TILE_DEC_OUT_MAX / TILE_DEC_GROUP_MIN.
constexpr uint32_t LZSS_TILE_DEC_IN_MAX = LZTD_IN_MAX;
constexpr uint32_t LZSS_TILE_DEC_OUT_MAX = LZTD_OUT_MAX;
// A PROBE build lowers the minimum to measure where it should be (scripts/probes/lzss_tile_dec_batch.py; Makefile: EXTRA=-DRSN_LZSS_TILE_DEC_GROUP_MIN=2).
#ifndef RSN_LZSS_TILE_DEC_GROUP_MIN
#define RSN_LZSS_TILE_DEC_GROUP_MIN 8
#endif
constexpr size_t LZSS_TILE_DEC_GROUP_MIN = RSN_LZSS_TILE_DEC_GROUP_MIN;
static_assert(LZSS_TILE_DEC_GROUP_MIN >= 2, "a group of one is the single call's");
// (lzss_tile_layout.h: a taken member's stream has at most lzt_e_cap(n) <= LZSS_TILE_E_MAX bytes -- an item is never longer than what it
// stands for -- and its escaped length is at most the same)
static_assert(LZSS_TILE_DEC_IN_MAX >= lzt_e_cap(LZSS_TILE_IN_MAX) && LZSS_TILE_DEC_OUT_MAX >= LZSS_TILE_E_MAX && lzt_e_cap(LZSS_TILE_IN_MAX) <= LZSS_TILE_E_MAX,
              "the decoder takes every stream the encoder writes");
const BehindClass &lzss_tile_dec_class();
// the rows of a layer and direction in order of precedence, and the classes behind them: LZSS asks its small class first, Huffman
// decompress its mid class (a short stream may promise more output than k_huff_batch_dec's workgroup holds) and then its tiled class, for
// the same reason: the small class takes by the stream's length alone, and 8 KiB of payload can promise more than HUFF_MID_OUT_MAX bytes
enum class BatchLayer { HUFFMAN, LZSS };
struct BatchRows {
    const BatchClass *const *first; size_t n;
    const BehindClass *const *behind = nullptr; size_t n_behind = 0;
    template <size_t N> BatchRows(const BatchClass *const (&rows)[N]) : first(rows), n(N) {}
    template <size_t N, size_t M> BatchRows(const BatchClass *const (&rows)[N], const BehindClass *const (&after)[M]) : first(rows), n(N), behind(after), n_behind(M) {}
};
inline BatchRows batch_classes(BatchLayer layer, bool compress) {
    static const BatchClass *const huff_enc[] = {&huff_small_class(true), &huff_mid_class(true), &huff_big_class()}, *const huff_dec[] = {&huff_mid_class(false), &huff_big_dec_class(), &huff_small_class(false)};
    static const BehindClass *const huff_enc_behind[] = {&huff_rune_mid_class(), &huff_rune_class()}, *const huff_dec_behind[] = {&huff_rune_dec_class(), &huff_rune_mid_dec_class()}, *const lzss_dec_behind[] = {&lzss_tile_dec_class()};
    static const BatchClass *const lzss_enc[] = {&lzss_small_class(true), &lzss_mid_class(true), &lzss_tile_class()}, *const lzss_dec[] = {&lzss_small_class(false), &lzss_mid_class(false)};
    if (layer == BatchLayer::HUFFMAN) return compress ? BatchRows(huff_enc, huff_enc_behind) : BatchRows(huff_dec, huff_dec_behind);
    return compress ? BatchRows(lzss_enc) : BatchRows(lzss_dec, lzss_dec_behind);
}
// until none of flags[0 .. n) is GROUP_PENDING (group_layout.h; the single small calls): polled for 5 ms, then the stream is waited for the
// ordinary way -- a kernel that has not answered by then is RSN_ERR_DEVICE
int flags_wait(Ctx &c, hipStream_t s, const uint32_t *flags, uint32_t n, const char *what);
// until every member's status word (base + off[k]) differs from `pending`: polled for 5 ms, then the stream is queried until a time limit --
// a kernel that never answers is RSN_ERR_DEVICE, the host never spins for ever
int group_wait(Ctx &c, hipStream_t s, const uint8_t *base, const std::vector<uint32_t> &off, uint32_t pending, const char *what);

// the decoder in SLICES as the stream lands (a host-buffer call, rsn_api.hip): 1 = not a stream for it (a 5C, huge tokens): the caller decodes it whole;
// RSN_ERR_CAPACITY: it expands beyond out_cap (what the caller's sample promised)
int lzss_decode_sliced(Ctx &c, hipStream_t s, const uint8_t *d_in, size_t n, uint8_t *d_out, size_t out_cap, size_t *out_n, const SliceStream &st);

// the layered round trip's two passes (huff_encode.hip, beside k_byte_hist): both only queue work on `s`.  d_hist: 256 counts, zeroed
// here; *d_first: the lowest offset below n at which d_a and d_b differ, ~0 when none does.  Buffers 16-byte aligned.
int byte_hist256_dev(Ctx &c, hipStream_t s, const uint8_t *d_in, size_t n, unsigned long long *d_hist);
int bytes_differ_dev(Ctx &c, hipStream_t s, const uint8_t *d_a, const uint8_t *d_b, size_t n, unsigned long long *d_first);

// ---- the adaptive arithmetic codec (arith.hip): one wave per member, in slices of at most ARITH_SLICE_SYMBOLS symbols a launch
// (mirrored as raisin_amd.arithmetic.SLICE_SYMBOLS).  One member is one wave's serial work, so its size is limited:
// ARITH_MAX_BYTES of input to the encoder and of output from the decoder, RSN_ERR_LIMIT beyond.
constexpr uint32_t ARITH_SLICE_SYMBOLS = 65536;
constexpr size_t ARITH_MAX_BYTES = RSN_ARITH_MAX_BYTES;
size_t arith_compress_bound(size_t n);
// the members `idx` of a batch (the single call: a batch of one) through the two kernels, in groups, on the thread's own stream; take(i, p,
// len) receives member i's result.  A failure returns the lowest failing member's code with *failed = that member.
int arith_compress_members(Ctx &c, const std::vector<size_t> &idx, const uint8_t *const *ins, const size_t *lens, const SmallTake &take, size_t *failed);
int arith_decompress_members(Ctx &c, const std::vector<size_t> &idx, const uint8_t *const *ins, const size_t *lens, const SmallTake &take, size_t *failed);
// device buffers, under the contract of the four at the top; out_cap == the exact size is taken, and *out_n on RSN_ERR_CAPACITY is it
int arith_encode_dev(Ctx &c, hipStream_t s, const uint8_t *d_in, size_t n, uint8_t *d_out, size_t out_cap, size_t *out_n);
int arith_decode_dev(Ctx &c, hipStream_t s, const uint8_t *d_in, size_t n, uint8_t *d_out, size_t out_cap, size_t *out_n);
// the batch calls on device buffers (rsn.h): the n members where they lie, a wave each, in the host form's groups, on `s`,
// which is synchronised.  out_lens[i]: the exact size of member i's result, complete in its d_out when that is at most its out_cap (a null
// d_out counts as none).  RSN_ERR_CAPACITY: some member did not fit, *failed the lowest of them, every member has run; any other code:
// the lowest failing member's, *failed that member (out_lens is then the caller's to clear).  The messages are the single calls'.
int arith_members_dev(Ctx &c, hipStream_t s, bool enc, size_t n, const rsn_dev_member *mem, size_t *out_lens, size_t *failed);

// the Huffman decompress batch on device buffers (rsn.h; huff_dev.hip): ONE launch of k_huff_dev_plan over the members a grouped
// decoder could take (8 <= n <= HUFF_HDR_MAX + 8 + HUFF_BIG_PAY_MAX), a workgroup each -- the header parsed, the tree built and the stream's
// bounds computed where the stream lies -- then ONE copy down, 16 bytes a candidate, and the one host wait the classes' slots need.
int huff_dev_plan(Ctx &c, hipStream_t s, size_t n, const rsn_dev_member *mem, DevPlans &plans);

// the layered batch calls' mover (rsn.h; layers_batch.hip): `tiles` entries of at most LB_TILE bytes each (layers_batch_layout.h),
// src and dst 16-byte aligned device pointers -- h_tab (pinned) goes up to d_tab in one copy and ONE launch of k_members_move, a workgroup
// an entry, moves them.  Only queues work on `s`: h_tab is the caller's until the stream has been synchronised.
struct MoveEntry { const uint8_t *src; uint8_t *dst; unsigned long long len; };
int members_move(Ctx &c, hipStream_t s, const MoveEntry *h_tab, MoveEntry *d_tab, size_t tiles);

// the batch round trip's verify pass (rsn.h; roundtrip_batch.hip): `tiles` entries of h_tab (pinned; roundtrip_batch_layout.h)
// over the run's m members go up into d_slot -- a block of verify_layout(both, tiles, m, hists).bytes (suite_layout.h) -- in one copy, ONE
// memset clears the stats block behind the table and ONE launch of k_members_verify, a workgroup an entry, fills it.  both: the instance
// that counts both sides (profile name members_verify); otherwise the batch suite's for the further lists of a run (DESIGN 4.13;
// members_verify_dec), which compares as the first and counts the decompressed side alone, 256 counters a member.  Only queues work on `s`.
struct RbEntry;
int members_verify(Ctx &c, hipStream_t s, bool both, const RbEntry *h_tab, size_t tiles, size_t m, bool hists, void *d_slot);

// exclusive scan of n counts on the stream (huff_encode.hip); *total (may be null) receives the sum; in and out must not overlap
int scan_u64(Ctx &c, hipStream_t s, const char *name, const unsigned long long *in, unsigned long long *out, uint32_t n, unsigned long long *total);

}  // namespace rsn
