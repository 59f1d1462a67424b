/*
 * rsn.h -- C ABI of librsn: the MI355X (gfx950) implementation of raisin's
 * Huffman, LZSS and arithmetic codecs (go-compression/raisin compressor/huffman,
 * compressor/lz, compressor/arithmetic).  This is the drop-in boundary: a Go host binds these entry
 * points with cgo in place of the per-package Compress/Decompress functions
 * (binding shown in INTEGRATION.md).  Plain pointers and sizes only.
 *
 * All compute runs in hand-written HIP kernels; there is NO CPU fallback.  If
 * no HIP device can be initialised every codec call fails with RSN_ERR_DEVICE.
 *
 * Threading: every entry point is re-entrant and may be called concurrently
 * from any number of host threads (the reference engine runs codecs from
 * concurrent goroutines, engine/engine.go:235-244).  State is per calling
 * thread; nothing is process-global (unlike huffman.go:56,129,193-194).
 *
 * Errors: the reference panics (check(e), index out of range); this library
 * returns a negative code and a thread-local message instead and never aborts.
 * The cgo shim turns a non-zero code back into panic() to keep engine behaviour
 * (engine.go:315-328 recovers it into a "failed" row).  "Never aborts" includes
 * the C++ side's own failures: every entry point below runs inside a guard that
 * turns std::bad_alloc / std::system_error / anything thrown into RSN_ERR_NOMEM
 * or RSN_ERR_DEVICE, and the helper threads of the pipelined calls come from a
 * pool that answers "none to be had" (the call then takes its serial form)
 * instead of throwing -- csrc/rsn_helpers.h, tests/thread_fail_test.cpp.
 */
#ifndef RSN_H
#define RSN_H

#include <stddef.h>
#include <stdint.h>

/* The library is built with -fvisibility=hidden: the entry points below are its whole dynamic symbol table. */
#if defined(__GNUC__) || defined(__clang__)
#define RSN_API __attribute__((visibility("default")))
#else
#define RSN_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define RSN_OK 0
#define RSN_ERR_ARG (-1)      /* bad argument (e.g. negative level, lzss.go:43-45) */
#define RSN_ERR_EMPTY (-2)    /* huffman of empty input: reference panics in heap.Pop (huffman.go:102) */
#define RSN_ERR_FORMAT (-3)   /* malformed compressed stream: reference panics (index/slice out of range) */
#define RSN_ERR_DEVICE (-4)   /* HIP runtime / device failure */
#define RSN_ERR_NOMEM (-5)
#define RSN_ERR_LIMIT (-6)    /* outside implementation limits (documented in DESIGN.md) */
#define RSN_ERR_CAPACITY (-7) /* caller-provided device output buffer too small */

#define RSN_LZSS_DEFAULT_WINDOW 4096 /* lzss.go:35 DefaultWindowSize */

/* ---- library / device ------------------------------------------------- */
/* Select the HIP device used by the calling thread.  A thread that never calls this uses device 0,
 * or what RSN_DEVICE says: a number, or "rr" = new thread contexts take the visible devices in turn. */
RSN_API int rsn_device_set(int device);
/* Number of visible HIP devices, or a negative error. */
RSN_API int rsn_device_count(void);
RSN_API const char *rsn_last_error(void); /* thread-local, valid until the next call on this thread */
RSN_API const char *rsn_version(void);
/* Releases what the library keeps between calls: the calling thread's device scratch and pinned
 * staging, the contexts parked by threads that have exited, and the recycled result buffers.
 * Safe at any time between calls; the next call re-allocates what it needs. */
RSN_API void rsn_trim(void);
RSN_API void rsn_free(void *p);           /* releases buffers returned through `out` below (only rsn_free may: they carry a
                                     library header; large ones are recycled for the next result) */

/* ---- host-buffer entry points (what the cgo shim binds) ----------------
 * Input is borrowed for the duration of the call and never modified -- the same
 * bytes may be handed to several calls at once (the pipelined calls pin them in
 * place under a shared, reference-counted table).  Output is allocated by the
 * library and released with rsn_free().                                     */

/* replaces huffman.Compress([]byte) []byte            huffman.go:299 */
RSN_API int rsn_huffman_compress(const uint8_t *in, size_t n, uint8_t **out, size_t *out_n);
/* replaces huffman.Decompress([]byte) []byte          huffman.go:327 */
RSN_API int rsn_huffman_decompress(const uint8_t *in, size_t n, uint8_t **out, size_t *out_n);
/* replaces lz.CompressAsync([]byte, bool, int) []byte lzss.go:109
 * (the engine path: Writer.Write lzss.go:53-57).  window <= 0 = unbounded
 * search buffer (lzss.go:125).  The progress-bar argument has no equivalent. */
RSN_API int rsn_lzss_compress(const uint8_t *in, size_t n, int64_t window, uint8_t **out, size_t *out_n);
/* replaces lz.Compress([]byte, bool, int) []byte      lzss.go:224 -- the older synchronous encoder.
 * FOR SMALL INPUTS ONLY: it is the reference's O(n * window) loop (O(n^2) for window <= 0) on the calling
 * thread; inputs above 64 MiB (above 1 MiB for window <= 0 or > 65536) return RSN_ERR_LIMIT instead of
 * blocking a cgo call for hours (RSN_LEGACY_NO_LIMIT=1 lifts the bound).
 * Not on the .rsn path (the engine calls CompressAsync) and not accelerated: a host-side
 * restatement for API completeness, quirks included (every-second-byte FindReverse :425-431,
 * offsets computed from the unsliced buffer :249-257, `<=` token threshold :272).  Needs no device. */
RSN_API int rsn_lzss_compress_legacy(const uint8_t *in, size_t n, int64_t window, uint8_t **out, size_t *out_n);
/* replaces lz.Decompress([]byte, bool) []byte         lzss.go:323 */
RSN_API int rsn_lzss_decompress(const uint8_t *in, size_t n, uint8_t **out, size_t *out_n);

/* Batch form for independent chunks (one .rsn segment per chunk, as
 * engine.CompressFiles produces one file per input, engine.go:150-154).  By default the batch
 * stays on the calling thread's device; with RSN_BATCH_DEVICES=<G>|all the chunks are dealt out
 * over G visible devices -- chunk k -> worker k mod G, worker w on device (calling thread's
 * device + w) mod visible.  On each device chunk k+1's upload, chunk k's encode and chunk k-1's
 * download run at once.  Nothing is exchanged between devices.  Each outs[i] equals what
 * rsn_huffman_compress() returns for ins[i]; on any error every outs[i] is NULL.
 * When at least two chunks are of 2 B to 16 KiB, those run grouped first, on the calling thread:
 * one launch per group, a workgroup per chunk that builds the chunk's own tree.
 * Chunks above 16 KiB and up to 64 KiB run grouped the same way through a kernel of their own when the call holds at least
 * four of them.  A grouped chunk with a single distinct byte is handed back to the pipeline.  Chunks of at most 16 KiB with a
 * byte >= 0x80 -- UTF-8 text, or no UTF-8 at all -- run grouped too, through an encoder of their own that counts runes as Go's
 * `range string` yields them, when the call holds at least 16 of them; one with more than 256 distinct runes, or with a single
 * one, is handed back to the pipeline, as every such chunk is in a call with fewer, and as chunks above 16 KiB are.
 * (RSN_BATCH_WORKERS, RSN_BATCH_KEEP_MIB: see rsn_api.hip / INTEGRATION.md.) */
RSN_API int rsn_huffman_compress_batch(size_t n_chunks, const uint8_t *const *ins, const size_t *lens,
                               uint8_t **outs, size_t *out_lens);

/* Batch forms of the other three host-buffer calls, for many independent members at once (engine.CompressFiles /
 * DecompressFiles loop over files, engine.go:150-154,175-185).  outs[i] / out_lens[i] are byte for byte what the single call
 * (rsn_huffman_decompress, rsn_lzss_compress(..., window, ...), rsn_lzss_decompress) returns for ins[i], empty members included;
 * each outs[i] is released with rsn_free.  n == 0 returns RSN_OK.  If any member fails, every outs[i] is NULL, the return code
 * is that of the lowest-index failing member and rsn_last_error() reads "member <i>: " followed by the single call's message.
 * Null arrays, or a null ins[i] with a non-zero length, return RSN_ERR_ARG; without a device every call returns RSN_ERR_DEVICE.
 * Small members run many to a launch, a workgroup each, on the calling thread: LZSS compress inputs of at most
 * 1 KiB (window <= 0xFFFF) and, through a kernel of their own, of at most 64 KiB (window 1 to 4096) that escape to at most 68 KiB;
 * LZSS compress inputs above 64 KiB and up to 256 KiB (window 1 to 4096), cut into tiles over the whole device, when the call holds
 * at least 16 such members;
 * LZSS streams of at most 2 KiB that expand to at most 8 KiB and, likewise, of at most 68 KiB that expand to at most 68 KiB
 * (the mid-size classes only when the call holds at least 64 such members); Huffman streams of a byte alphabet
 * (2 to 128 symbols, codes of at most 32 bits) with at most 16 KiB of payload and 32 KiB of output and, through a kernel of
 * their own when the call holds at least four such streams, with at most 56 KiB of payload and 64 KiB of output; Huffman streams of
 * a rune alphabet (a symbol >= 0x80 among the header's 2 to 256; what the encoders write for UTF-8 text) that promise at most 16 KiB
 * from at most 18 KiB of payload, through a decoder of their own when the call holds at least 16 such streams.  Every other member -- and
 * one a kernel hands back -- takes the single call's path, in index order; RSN_BATCH_WORKERS / RSN_BATCH_DEVICES deal those
 * over workers as rsn_huffman_compress_batch deals its chunks.  The same input bytes may be passed to several calls at once. */
RSN_API int rsn_huffman_decompress_batch(size_t n, const uint8_t *const *ins, const size_t *lens, uint8_t **outs, size_t *out_lens);
RSN_API int rsn_lzss_compress_batch(size_t n, const uint8_t *const *ins, const size_t *lens, int64_t window, uint8_t **outs,
                                    size_t *out_lens);
RSN_API int rsn_lzss_decompress_batch(size_t n, const uint8_t *const *ins, const size_t *lens, uint8_t **outs, size_t *out_lens);

/* ONE stream from `shards` slices of ONE input (intra-file sharding): per-slice histograms are summed, one tree and one
 * header are built, every slice is encoded at its exact bit offset (the format has a single front pad, huffman.go:245-255) by a
 * worker of its own, and the pieces are stitched on the way down.  The result is byte for byte rsn_huffman_compress(in, n).
 * shards <= 0: RSN_HUFF_SHARDS, else one per device used.  Worker w runs on device (calling thread's + w mod D) mod visible,
 * D = RSN_BATCH_DEVICES (default 1: the workers share the caller's device).  rsn_huffman_compress itself takes this path
 * when RSN_HUFF_SHARDS > 1 is set in the environment.                                                                    */
RSN_API int rsn_huffman_compress_sharded(const uint8_t *in, size_t n, int shards, uint8_t **out, size_t *out_n);

/* ---- device-resident entry points --------------------------------------
 * d_in / d_out are HIP device pointers on the calling thread's device; stream
 * is a hipStream_t (NULL = the thread's own stream).  The call returns after
 * the result size is known on the host; d_out is complete once `stream` has
 * been synchronised (the calls below synchronise it before returning).
 * d_in and d_out must both be 16-byte aligned (RSN_ERR_ARG otherwise: the
 * kernels load and store 16 bytes at a time from both bases); [d_in, d_in+n)
 * and [d_out, d_out+out_cap) must not overlap (RSN_ERR_ARG).  Only the n bytes
 * of the input are read as data: the result never depends on what lies before
 * d_in or behind d_in + n.  A d_out of rsn_*_bound(n) bytes always suffices
 * for the two compress calls.                                                */
RSN_API size_t rsn_huffman_compress_bound(size_t n);
RSN_API size_t rsn_lzss_compress_bound(size_t n);
RSN_API int rsn_huffman_compress_dev(const void *d_in, size_t n, void *d_out, size_t out_cap, size_t *out_n, void *stream);
/* The decoded size is only known after the header is parsed.  When the buffer is too small -- or
 * d_out is NULL / out_cap 0, the size query -- the call returns RSN_ERR_CAPACITY, sets the error
 * string, and stores in *out_n a capacity that WOULD suffice (the exact size rounded up to 16, plus
 * 16 -- plus 32 from rsn_huffman_compress_dev: not the exact size); call again with a buffer of at least
 * that many bytes, the second call returns RSN_OK and the exact size.  rsn_lzss_decompress_dev and the two
 * compress_dev calls follow the same contract, with that one figure apart.  An empty input (n == 0) has nothing
 * to size: the two LZSS calls return RSN_OK and size 0 for it, the query included (rsn_huffman_compress_dev
 * returns RSN_ERR_EMPTY, rsn_huffman_decompress_dev RSN_ERR_FORMAT).  How small a buffer may be: rsn_huffman_decompress_dev, rsn_lzss_compress_dev and rsn_lzss_decompress_dev
 * take out_cap == the exact result size, whatever its remainder mod 16.  rsn_huffman_compress_dev needs the result size rounded
 * up to 16, plus 32 (its emit kernels clear and fill whole words up to there); with less -- the exact size included -- it returns
 * RSN_ERR_CAPACITY and stores that figure.  On RSN_ERR_FORMAT and on RSN_ERR_CAPACITY the contents of d_out are unspecified (the decoders
 * write while they validate, and what fits a too-small buffer may have been written before the total is known; nothing
 * is ever written outside [d_out, d_out + out_cap)).  (The Huffman query with d_out NULL is answered from the header's counts alone,
 * without touching the payload: a foreign stream whose payload decodes to more than its header
 * announces reports the larger need on the call that follows.)                                  */
RSN_API int rsn_huffman_decompress_dev(const void *d_in, size_t n, void *d_out, size_t out_cap, size_t *out_n, void *stream);
RSN_API int rsn_lzss_compress_dev(const void *d_in, size_t n, int64_t window, void *d_out, size_t out_cap, size_t *out_n, void *stream);
RSN_API int rsn_lzss_decompress_dev(const void *d_in, size_t n, void *d_out, size_t out_cap, size_t *out_n, void *stream);

/* ---- layered calls -------------------------------------------------------
 * The engine's unit of work: a LIST of layers over one buffer (engine.go:443-479; the CLI's default is lzss,huffman).  `layers` is
 * always in COMPRESS order, as the engine's `algorithms` is; rsn_layers_decompress undoes them last to first.  The result is byte for
 * byte what the chain of the single calls above returns -- rsn_lzss_compress(..., RSN_LZSS_DEFAULT_WINDOW, ...) / rsn_huffman_compress
 * in order, rsn_*_decompress in reverse, the Huffman codec's lossy treatment of bytes that are not UTF-8 included -- but between the
 * layers the stream stays on the device, in the calling thread's scratch: the input goes up once and the last layer's output comes
 * down once.  n_layers == 0 returns a copy of the input; n_layers == 1 IS the single call (same small-input paths, same pipelining,
 * same launches).  Host buffers of at most 64 KiB run the chain of single host calls instead: at that size a call is its launches, and
 * the single calls' one-launch paths read and write pinned host memory without a copy command.
 * Errors: a null `layers` with n_layers > 0, an unknown layer id or n_layers > RSN_LAYERS_MAX is RSN_ERR_ARG, checked before the
 * device is touched; without a device RSN_ERR_DEVICE; otherwise the failing layer's own code, and rsn_last_error() reads
 * "layer <k> (<name>): " followed by the single call's message, k counting in compress order whichever direction runs (Huffman of an
 * empty stream is RSN_ERR_EMPTY: [lzss, huffman] on an empty input fails in layer 1).  *out stays NULL on every failure.           */
#define RSN_LAYER_LZSS 1    /* lz.CompressAsync(..., 4096) / lz.Decompress: what engine.Writers["lzss"] does */
#define RSN_LAYER_HUFFMAN 2
#define RSN_LAYERS_MAX 8
RSN_API int rsn_layers_compress(const uint8_t *in, size_t n, const int *layers, size_t n_layers, uint8_t **out, size_t *out_n);
RSN_API int rsn_layers_decompress(const uint8_t *in, size_t n, const int *layers, size_t n_layers, uint8_t **out, size_t *out_n);
/* The same on device buffers, under the contract of the rsn_*_dev calls above: d_in and d_out 16-byte aligned and not overlapping
 * (RSN_ERR_ARG), synchronised before returning; when d_out is too small -- or NULL / out_cap 0, the size query -- the call returns
 * RSN_ERR_CAPACITY and stores in *out_n a capacity that would suffice.  The size of a layered result is only known once the chain has
 * run: the query of two or more layers (and of one compress layer) costs the whole chain, its last layer writing into scratch, and a
 * buffer that turns out too small costs the chain up to its last layer; a caller that can bound the result (the compress bounds
 * applied in turn, or the original's size when decompressing) should pass a buffer of that size.  The smallest out_cap that is
 * taken is the last step's own: the exact size, except behind a last Huffman compress layer (rounded up to 16, plus 32).          */
RSN_API int rsn_layers_compress_dev(const void *d_in, size_t n, const int *layers, size_t n_layers, void *d_out, size_t out_cap, size_t *out_n, void *stream);
RSN_API int rsn_layers_decompress_dev(const void *d_in, size_t n, const int *layers, size_t n_layers, void *d_out, size_t out_cap, size_t *out_n, void *stream);

/* engine.BenchmarkFile's body (engine.go:357-441) in one call: upload once, compress, decompress, compare and count the bytes, all on
 * the device; only `res` comes down -- and the compressed stream, if `compressed` is not NULL (released with rsn_free).  When a layer
 * fails, `res` is left zeroed and the code is the layer's.                                                                        */
typedef struct {
    uint64_t original_n, compressed_n, decompressed_n;
    int lossless;                    /* decompressed == original, byte for byte and in length */
    uint64_t first_difference;       /* lowest differing offset; min(original_n, decompressed_n) if one is a prefix of the other; UINT64_MAX if lossless */
    uint64_t hist_original[256];     /* byte counts of the input             (engine.go:367-370) */
    uint64_t hist_decompressed[256]; /* byte counts of what came back        (engine.go:412-415) */
    double compress_ms, decompress_ms; /* host wall clock of the two halves, for the caller's "time taken" */
} rsn_roundtrip_result;
RSN_API int rsn_layers_roundtrip(const uint8_t *in, size_t n, const int *layers, size_t n_layers, rsn_roundtrip_result *res,
                                 uint8_t **compressed, size_t *compressed_n);

/* ---- the adaptive arithmetic codec ---------------------------------------
 * replaces arithmetic.Compress([]byte) []byte / arithmetic.Decompress([]byte) []byte (compressor/arithmetic/arithmetic.go:15,27):
 * an adaptive 16-bit arithmetic coder over a 257-symbol model (bytes and an end symbol) that freezes once its total reaches 16383;
 * streams are byte for byte the reference's.  An empty input compresses to 01 ff (which, as in the reference, does not decompress).
 * One stream is SERIAL work: each member runs on one wavefront, and the device is used by running many members at once -- the batch
 * calls are the fast path.  A member above RSN_ARITH_MAX_BYTES (input of a compress call, output of a decompress call;
 * for a stream handed to decompress, rsn_arithmetic_compress_bound of it) returns RSN_ERR_LIMIT.
 * Decompress returns RSN_ERR_FORMAT where the reference panics -- no 1 bit in the stream, or fewer than 14 bits behind the first --
 * and, the one deliberate deviation, where the reference would decode for ever: a stream that has not reached its end symbol after
 * more than RSN_ARITH_TAIL_BITS bits have been shifted in from behind its end (the 1, 0 the decoder appends and the zeros that follow;
 * a stream the reference's encoder wrote needs at most 16 plus the pending bits it dropped).
 * The host-buffer and batch calls follow the contracts of their neighbours above: results released with rsn_free; n == 0 members
 * return RSN_OK; outs[i] is byte for byte the single call's (the single call IS a batch of one: every member goes through the same
 * two kernels); if any member fails every outs[i] is NULL, the code is the lowest failing member's and rsn_last_error() reads
 * "member <i>: ..."; null arrays or a null member of non-zero length are RSN_ERR_ARG before a device is looked for; without a device
 * RSN_ERR_DEVICE.  The _dev calls follow the device-resident contract above (16-byte alignment, no overlap, synchronised before
 * returning); on RSN_ERR_CAPACITY -- or the size query, d_out NULL / out_cap 0 -- *out_n is the EXACT result size, and out_cap equal
 * to it is accepted; nothing is ever written outside [d_out, d_out + out_cap).  A buffer of rsn_arithmetic_compress_bound(n) bytes
 * always suffices for rsn_arithmetic_compress_dev (a symbol causes at most 16 shifts: 2 * n + 4).                                  */
#define RSN_ARITH_TAIL_BITS 4096
#define RSN_ARITH_MAX_BYTES ((size_t)64 << 20)
RSN_API size_t rsn_arithmetic_compress_bound(size_t n);
RSN_API int rsn_arithmetic_compress(const uint8_t *in, size_t n, uint8_t **out, size_t *out_n);
RSN_API int rsn_arithmetic_decompress(const uint8_t *in, size_t n, uint8_t **out, size_t *out_n);
RSN_API int rsn_arithmetic_compress_batch(size_t n, const uint8_t *const *ins, const size_t *lens, uint8_t **outs, size_t *out_lens);
RSN_API int rsn_arithmetic_decompress_batch(size_t n, const uint8_t *const *ins, const size_t *lens, uint8_t **outs, size_t *out_lens);
RSN_API int rsn_arithmetic_compress_dev(const void *d_in, size_t n, void *d_out, size_t out_cap, size_t *out_n, void *stream);
RSN_API int rsn_arithmetic_decompress_dev(const void *d_in, size_t n, void *d_out, size_t out_cap, size_t *out_n, void *stream);

/* ---- batch calls on device buffers ---------------------------------------
 * Many independent members that already lie in device memory, in one call: `members` is a HOST array of n descriptors, each under
 * the contract of the device-resident entry points above -- d_in / d_out device pointers on the calling thread's device, both
 * 16-byte aligned (RSN_ERR_ARG otherwise), only the n bytes of a member's input read as data: nothing in front of d_in or behind
 * d_in + n reaches a result, so members may be packed back to back in one allocation at 16-byte offsets.  Member i's result is byte
 * for byte what the single call (rsn_lzss_compress_dev(..., window, ...), rsn_lzss_decompress_dev, rsn_arithmetic_compress_dev,
 * rsn_arithmetic_decompress_dev) writes for the same input -- which is the host batch call's and the reference's -- and lies at
 * members[i].d_out[0 .. out_lens[i]); empty members behave as in the single call.  The work is queued on `stream` (NULL = the
 * thread's own), which is synchronised before the call returns.  The members' bytes never cross to the host: LZSS members of the
 * host batch calls' classes (same sizes, same window rules, same minimum counts) are gathered on the device into the grouped
 * kernels' staging, run one launch a group and are scattered to their buffers; arithmetic members are coded where they lie, a
 * wavefront each; every other LZSS member -- and one a grouped kernel hands back -- runs the single call on the same stream, in
 * index order.
 * Arguments, all checked before a device is looked for (RSN_ERR_ARG): n == 0 returns RSN_OK; null `members` or `out_lens`; a null
 * d_in with n > 0; a d_in or d_out that is not 16-byte aligned; a null d_out with out_cap != 0 (a null d_out with out_cap == 0 is a
 * size query for that member); an output range that overlaps ANY member's input range, or another member's output range (empty
 * ranges overlap nothing; inputs may overlap each other).  `window` is rsn_lzss_compress_dev's.  Without a device: RSN_ERR_DEVICE.
 * Failures: if a member fails with a code other than RSN_ERR_CAPACITY the call returns the lowest-index such member's code,
 * rsn_last_error() reads "member <i>: " followed by the single call's message, and every out_lens[i] is 0.  Otherwise, if some
 * members did not fit their buffers, the call returns RSN_ERR_CAPACITY and names the lowest such member; every member has still
 * been processed: out_lens[i] <= out_cap marks a member that fits -- its bytes are complete and out_lens[i] is exact -- and
 * out_lens[i] > out_cap one that did not, the value being a capacity that suffices, as the single call reports it (LZSS: the exact
 * size rounded up to 16, plus 16; arithmetic: the exact size).  A buffer of rsn_lzss_compress_bound(n) / rsn_arithmetic_compress_bound(n)
 * bytes always suffices for a compress member, and an out_cap equal to the exact result size is accepted whatever its remainder
 * mod 16.  Nothing is ever written outside [d_out, d_out + out_cap) of any member; what a member that did not fit, or the members of
 * a failed call, hold is unspecified.
 * Huffman (rsn_huffman_compress_batch_dev, rsn_huffman_decompress_batch_dev; the single calls are rsn_huffman_compress_dev /
 * rsn_huffman_decompress_dev) runs the host batch calls' classes the same way.  To compress, members of 2 bytes to 64 KiB of a byte
 * alphabet (every byte below 0x80, two distinct bytes at least) are gathered and coded by the grouped encoders, which build their
 * trees themselves.  To decompress, one more kernel in front reads every candidate stream's header WHERE IT LIES -- separator, counts,
 * the reference's tree and the stream's bit bounds, a workgroup a member -- and 16 bytes a member come down for the host to size the
 * slots; streams of a byte alphabet that promise at most 64 KiB from at most 56 KiB of payload then run the grouped decoders.  What
 * still takes the single call on the same stream, in index order: to decompress, rune alphabets (a symbol >= 0x80 among the header's)
 * unless the call holds at least 16 such streams that promise at most 16 KiB from at most 18 KiB of payload with 2 to 256 distinct
 * runes -- ONE more plan kernel reads those headers where they lie (16 more bytes a member come down, one more host wait, only in calls
 * that hold such members), and they run grouped through a decoder of their own that parses its header and builds its tree itself;
 * to compress, members with a byte >= 0x80 unless the call holds at least 16 of them of at most 16 KiB -- those run grouped as well,
 * through an encoder of their own that counts runes as Go's `range string` yields them (2 to 256 distinct runes; more, or one, take
 * the single call); in both directions a single distinct byte, headers the device-side plan refuses (a count of 65536 or more, foreign or malformed headers --
 * the single call decodes them or words their error), members above 64 KiB, and classes below their minimum count.  An empty member
 * fails rsn_huffman_compress_batch_dev with RSN_ERR_EMPTY, as in the single call, before a device is looked for.
 * Huffman capacities: a buffer of rsn_huffman_compress_bound(n) always suffices.  A member that takes the single call needs what
 * rsn_huffman_compress_dev / rsn_huffman_decompress_dev need (compress: the exact size rounded up to 16, plus 32); a grouped member is
 * written by the scatter kernel, and an out_cap equal to its exact size is accepted.  On RSN_ERR_CAPACITY out_lens[i] of a member
 * that did not fit is the single call's figure whichever path it took -- compress: the exact size rounded up to 16, plus 32;
 * decompress: rounded up to 16, plus 16 -- so a second call with the reported figures always succeeds. */
typedef struct { const void *d_in; size_t n; void *d_out; size_t out_cap; } rsn_dev_member;
RSN_API int rsn_huffman_compress_batch_dev(size_t n, const rsn_dev_member *members, size_t *out_lens, void *stream);
RSN_API int rsn_huffman_decompress_batch_dev(size_t n, const rsn_dev_member *members, size_t *out_lens, void *stream);
RSN_API int rsn_lzss_compress_batch_dev(size_t n, const rsn_dev_member *members, int64_t window, size_t *out_lens, void *stream);
RSN_API int rsn_lzss_decompress_batch_dev(size_t n, const rsn_dev_member *members, size_t *out_lens, void *stream);
RSN_API int rsn_arithmetic_compress_batch_dev(size_t n, const rsn_dev_member *members, size_t *out_lens, void *stream);
RSN_API int rsn_arithmetic_decompress_batch_dev(size_t n, const rsn_dev_member *members, size_t *out_lens, void *stream);

/* ---- layered batch calls -------------------------------------------------
 * The engine's whole unit of work: a LIST of layers over MANY members (engine.CompressFiles / DecompressFiles; the CLI's default is
 * lzss,huffman), in one call.  Member i's result is byte for byte what rsn_layers_compress(ins[i], ...) / rsn_layers_compress_dev returns
 * for the same layer list -- the chain of the single calls at RSN_LZSS_DEFAULT_WINDOW, the Huffman codec's lossy treatment of bytes that
 * are not UTF-8 included; decompress undoes the layers last to first.  `layers` is in compress order, holds RSN_LAYER_LZSS /
 * RSN_LAYER_HUFFMAN only and at most RSN_LAYERS_MAX entries.  The layers run LAYER-MAJOR: every member through one layer -- the batch
 * calls' grouped kernels, thousands of small members to a launch -- before the next, and between the layers every member stays on the
 * device, in slots of the calling thread's scratch.  Members are taken in runs of consecutive members whose slots fit a
 * budget (1 GiB; RSN_LAYERS_BATCH_BUDGET=<bytes>, read at every call); a member above the budget is a run of its own.
 * Arguments, all checked before a device is looked for (RSN_ERR_ARG): n == 0 returns RSN_OK before anything else is looked at; then the
 * arrays and members as in the neighbouring batch calls -- host form: null arrays, a null ins[i] of non-zero length; device form: null
 * arrays, a null d_in with n > 0, alignment, a null d_out with an out_cap, the overlap rule over the CALLER's ranges; then the layer list as
 * in rsn_layers_compress.  Without a device: RSN_ERR_DEVICE.
 * Failures: the first layer, in run order, at which some member fails with a code other than RSN_ERR_CAPACITY ends the call with that
 * layer's lowest failing member's code; rsn_last_error() reads "member <i>: layer <k> (<name>): " followed by the single call's message, k
 * counting in compress order; every outs[i] is then NULL and every out_lens[i] 0.  [lzss, huffman] with an empty member fails as
 * "member <i>: layer 1 (huffman): ..." with RSN_ERR_EMPTY; a list without Huffman takes empty members, and their result is empty.
 * Host form: runs on the calling thread's device; a run's inputs go up in ONE copy, its results are packed on the device and come down
 * in ONE copy; each outs[i] is released with rsn_free.
 * Device form: under the contract of the batch calls on device buffers above; intermediates never cross to the host.  Only the last step
 * writes caller memory, and its contract holds: a size query per member (d_out NULL with out_cap 0); on RSN_ERR_CAPACITY -- the message
 * names the lowest member that did not fit -- every member has been processed, out_lens[i] <= out_cap marks a member that fits, complete
 * and exact, out_lens[i] > out_cap one that did not, the value being a capacity that suffices on a second call (the last step's figure:
 * the exact size rounded up to 16, plus 16 -- plus 32 behind a last Huffman compress layer); the smallest out_cap taken is the last
 * step's own (the exact size; a member the last Huffman compress layer runs through the single call: rounded up to 16, plus 32).
 * Nothing is ever written outside [d_out, d_out + out_cap).  n_layers == 1 IS the codec's batch call on device buffers at window
 * RSN_LZSS_DEFAULT_WINDOW -- the same launches -- with the layer named in the message.  n_layers == 0 copies each member; a member that
 * does not fit reports its size rounded up to 16, plus 16.  The stream is synchronised before the call returns. */
RSN_API int rsn_layers_compress_batch(size_t n, const uint8_t *const *ins, const size_t *lens, const int *layers, size_t n_layers, uint8_t **outs, size_t *out_lens);
RSN_API int rsn_layers_decompress_batch(size_t n, const uint8_t *const *ins, const size_t *lens, const int *layers, size_t n_layers, uint8_t **outs, size_t *out_lens);
RSN_API int rsn_layers_compress_batch_dev(size_t n, const rsn_dev_member *members, const int *layers, size_t n_layers, size_t *out_lens, void *stream);
RSN_API int rsn_layers_decompress_batch_dev(size_t n, const rsn_dev_member *members, const int *layers, size_t n_layers, size_t *out_lens, void *stream);

/* ---- batch round trip ----------------------------------------------------
 * engine.BenchmarkFile's body over MANY members in one call (the reference's benchmark loop, ai/helpers/compressor.py:89-108 over
 * engine.go:213-309): every member is compressed under the layer list, decompressed again, compared with its original and its bytes
 * counted, all on the device.  res[i] holds, field for field, what rsn_layers_roundtrip(ins[i], lens[i], layers, n_layers,
 * ...) reports for member i alone; `hists` is NULL or n * 512 counters: hists[512 * i .. + 256) the byte counts of member i's input,
 * hists[512 * i + 256 .. + 512) of what came back -- that call's two histograms as 32-bit counts.  No compressed bytes are handed out
 * (rsn_layers_compress_batch does that), and there are no per-member times: the caller times the call.
 * The layer list follows rsn_layers_compress_batch's rules: compress order, RSN_LAYER_LZSS / RSN_LAYER_HUFFMAN only, at most
 * RSN_LAYERS_MAX entries, LZSS at RSN_LZSS_DEFAULT_WINDOW.  n_layers == 0: compressed and decompressed both equal the input.  An empty
 * member under a list without Huffman: all sizes 0, lossless, first_difference UINT64_MAX.  The members run layer-major in the layered
 * batch calls' runs (RSN_LAYERS_BATCH_BUDGET applies) -- the compress pass, the decompress pass from where the first left every member,
 * then ONE launch that compares and counts all members of the run; per run one table goes up and one block of answers comes down (8 bytes
 * a member, plus 2 KiB a member when `hists` is given).  Nothing else of a member crosses to the host; in the host form a run's inputs go
 * up in one copy, in the device form the members are read where they lie and never written.
 * Arguments, all checked before a device is looked for (RSN_ERR_ARG): n == 0 returns RSN_OK before anything else is looked at.  Host form:
 * null `ins`, `lens` or `res`, a null ins[i] with a non-zero length.  Device form: null `members` or `res`; a null d_in with n > 0; a d_in
 * that is not 16-byte aligned; every member's d_out must be NULL and its out_cap 0 -- both are RESERVED in this call, which writes no
 * caller memory on the device.  Then the layer list as in rsn_layers_compress.  Without a device: RSN_ERR_DEVICE.
 * Failures are all or nothing.  A round trip is 2 * n_layers steps: compress layers 0 .. L-1, then decompress layers L-1 .. 0.  The call
 * ends with the EARLIEST step in that order at which some member fails, and with that step's lowest failing member, however the members
 * were cut into runs; rsn_last_error() reads "member <i>: layer <k> (<name>): " followed by the single call's message, k counting in
 * compress order.  Every res[i] is then zeroed and `hists` unspecified.  Behind the passes, a member whose original or decompressed
 * length exceeds UINT32_MAX (the counters are 32 bits) fails the call with RSN_ERR_LIMIT and "member <i>: ...": one large buffer is
 * rsn_layers_roundtrip's job.  Anything thrown leaves every res[i] zeroed.
 * The device form queues its work on `stream` (NULL = the thread's own), which is synchronised before the call returns. */
typedef struct {
    uint64_t original_n, compressed_n, decompressed_n;
    uint64_t first_difference;   /* as rsn_roundtrip_result: lowest differing offset; min(original_n, decompressed_n) if one is a
                                    prefix of the other; UINT64_MAX if lossless */
    int lossless;
} rsn_roundtrip_member;
RSN_API int rsn_layers_roundtrip_batch(size_t n, const uint8_t *const *ins, const size_t *lens, const int *layers, size_t n_layers,
                                       rsn_roundtrip_member *res, uint32_t *hists);
RSN_API int rsn_layers_roundtrip_batch_dev(size_t n, const rsn_dev_member *members, const int *layers, size_t n_layers,
                                           rsn_roundtrip_member *res, uint32_t *hists, void *stream);

/* ---- batch suite ---------------------------------------------------------
 * The reference's whole benchmark loop in one call: MANY members under SEVERAL layer lists (files x algorithm lists, then the best list
 * per file: ai/helpers/compressor.py:89-108 and ai/helpers/files.py:67-78; engine.BenchmarkSuite, engine.go:213-309), with everything the
 * lists have in common done once.  lists[l] is a layer list in compress order under rsn_layers_compress_batch's rules; at
 * most RSN_SUITE_LISTS_MAX lists.  `res` holds n_lists * n rows, list-major: for every list l that succeeds, res[l * n + i] equals, field
 * for field, res[i] of rsn_layers_roundtrip_batch(n, ins, lens, lists[l].layers, lists[l].n_layers, ...) -- of rsn_layers_roundtrip_batch_dev
 * for the device form.  `hists_original` is NULL or n * 256 counters, `hists_decompressed` NULL or n_lists * n * 256, list-major:
 * hists_original[256 * i .. + 256) and hists_decompressed[256 * (l * n + i) .. + 256) are the two halves of that call's
 * hists[512 * i .. + 512).  hists_original is complete when at least one list succeeded.
 * What is shared: the lists form a prefix tree over their layers.  Per run (the layered batch calls' runs; RSN_LAYERS_BATCH_BUDGET applies,
 * the outputs that are kept counted in) the members are staged and go up once (host form) or are read where they lie (device form), every
 * distinct non-empty prefix is compressed once -- [lzss] and [lzss, huffman] run the LZSS encoder once -- and the originals' bytes are
 * counted once.  The decompress passes and the compare are per list: a Huffman layer is lossy on bytes that are not UTF-8, so two lists'
 * streams are not assumed equal on the way back.  Of equal lists one is run and its rows are copied.
 * best: NULL or n entries; best[i] is the index of the list with the smallest compressed_n for member i among the lists that succeeded,
 * the lowest index among equals (best_result compares ratios with a strict `<` and does not look at `lossless`); UINT32_MAX when no list
 * succeeded.  It is computed on the host from the rows.
 * Arguments, all checked before a device is looked for (RSN_ERR_ARG, every row zeroed), in this order: n == 0 returns RSN_OK before
 * anything else is looked at; the arrays and members as in rsn_layers_roundtrip_batch / _dev (the device form's d_out and out_cap are
 * reserved: NULL and 0; the call writes no caller memory on the device); n_lists == 0 returns RSN_OK with nothing written; a null `lists`
 * or `res`; n_lists > RSN_SUITE_LISTS_MAX; then every list as in rsn_layers_compress, the message prefixed "list <l>: " -- for example
 * "list 1: layer 1: unknown layer id 3".  Without a device: RSN_ERR_DEVICE.
 * Failures are per list: the reference's loop catches a failure per file and algorithm and goes on (compressor.py:96-100).  A list fails
 * exactly when rsn_layers_roundtrip_batch fails for it alone, with that call's code -- the earliest step's lowest member, however the
 * members were cut into runs, and RSN_ERR_LIMIT for a length above UINT32_MAX -- and only its own rows are zeroed; its
 * hists_decompressed rows are unspecified.  Every other list's rows are complete and valid.  list_rc is NULL or n_lists codes:
 * list_rc[l] is the code of list l (RSN_OK: it succeeded).  The call returns RSN_OK when every list succeeded, otherwise the code of
 * the failing list of the lowest index, and rsn_last_error() reads "list <l>: " followed by that call's message.
 * A failure of the call as a whole -- an argument, no device, an allocation, anything thrown -- leaves every row zeroed and does not write
 * list_rc or best: a caller that fills list_rc with a value that is no code beforehand tells the two apart.
 * The device form queues its work on `stream` (NULL = the thread's own), which is synchronised before the call returns. */
#define RSN_SUITE_LISTS_MAX 16
typedef struct { const int *layers; size_t n_layers; } rsn_layer_list;   /* compress order; rsn_layers_compress_batch's rules */
RSN_API int rsn_layers_suite_batch(size_t n, const uint8_t *const *ins, const size_t *lens, size_t n_lists, const rsn_layer_list *lists,
                                   rsn_roundtrip_member *res, int *list_rc, uint32_t *hists_original, uint32_t *hists_decompressed,
                                   uint32_t *best);
RSN_API int rsn_layers_suite_batch_dev(size_t n, const rsn_dev_member *members, size_t n_lists, const rsn_layer_list *lists,
                                       rsn_roundtrip_member *res, int *list_rc, uint32_t *hists_original,
                                       uint32_t *hists_decompressed, uint32_t *best, void *stream);

/* ---- measurement --------------------------------------------------------
 * When enabled, every kernel launch of the calling thread is bracketed by HIP
 * events on the launch stream; rsn_prof_get() reports per-kernel totals since
 * the last rsn_prof_reset().                                               */
typedef struct {
    char name[48];
    uint64_t launches;
    double total_ms;
} rsn_prof_entry;
RSN_API void rsn_prof_enable(int on);
RSN_API void rsn_prof_reset(void);
RSN_API int rsn_prof_get(rsn_prof_entry *entries, int cap); /* returns the number of entries */
/* Bytes the library has queued on host-to-device and device-to-host COPY COMMANDS since the last rsn_prof_reset(): process-wide
 * atomic counters, the helper threads' copies included, counted while the most recent rsn_prof_enable() of any thread was (1).
 * Kernels that read or write pinned host memory directly (the small-input paths) issue no copy command and count nothing. */
RSN_API void rsn_prof_copied(uint64_t *h2d_bytes, uint64_t *d2h_bytes);

/* Introspection used by the parity tests: the code table the encoder builds for
 * `in` (device buffer not needed; runs the histogram on the device, the tree on
 * the host).  Arrays hold `cap` entries in printCodes DFS order (huffman.go:110);
 * returns the symbol count or a negative error. */
RSN_API int64_t rsn_huffman_table(const uint8_t *in, size_t n, uint32_t *runes, uint64_t *freqs,
                          uint64_t *codes, uint8_t *lens, size_t cap);

/* ---- host-side helpers (no device needed) --------------------------------
 * The part of the Huffman codec that stays on the host by design: the Go-exact
 * tree (buildTree huffman.go:58-103 with container/heap order), the codes
 * (printCodes :110-127) and the textual header (:312-318 / decodeTree :196-227).
 * Exposed so that the host logic can be checked on a machine without a GPU.   */

/* (rune,count) pairs in any order -> codes in printCodes DFS order plus the
 * header this library writes (ascending rune, '\\' never last).  Returns the
 * symbol count, or a negative error.  header may be NULL.                      */
RSN_API int64_t rsn_huffman_plan(const uint32_t *runes, const uint64_t *counts, size_t n_syms,
                         uint32_t *out_runes, uint64_t *out_codes, uint8_t *out_lens,
                         uint8_t *header, size_t header_cap, size_t *header_len);
/* decodeTree's scan of a header (bytes before "\\\n").  Returns the number of
 * distinct symbols (ascending rune), or a negative error where the reference
 * would index out of range.                                                   */
RSN_API int64_t rsn_huffman_parse_header(const uint8_t *header, size_t n, uint32_t *runes, uint64_t *counts, size_t cap);

/* Where rsn_huffman_compress_sharded cuts `in` into slices: cuts[0] = 0 < ... < cuts[S] = n, every cut on a rune start of Go's
 * decoding of the whole input (huffman.go:309: a UTF-8 sequence is never split).  Returns S (<= shards; short inputs get fewer
 * slices), or a negative error; cuts must hold shards + 1 entries.                                                           */
RSN_API int64_t rsn_huffman_slice_cuts(const uint8_t *in, size_t n, int shards, size_t *cuts, size_t cap);

#ifdef __cplusplus
}
#endif
#endif
