"""Mirror of /root/reference/compressor/huffman (huffman.go) over librsn."""
import io

from . import _lib


def Compress(fileContents):
    """huffman.go:299 Compress([]byte) []byte"""
    return _lib.call_host(_lib.lib().rsn_huffman_compress, fileContents)


def Decompress(fileContents):
    """huffman.go:327 Decompress([]byte) []byte"""
    return _lib.call_host(_lib.lib().rsn_huffman_decompress, fileContents)


def CompressSharded(fileContents, shards=0):
    """ONE stream from `shards` slices of one input (rsn_huffman_compress_sharded): per-slice histograms summed, one tree, every slice
    encoded at its bit offset by a worker of its own (a device of its own with RSN_BATCH_DEVICES).  Equals Compress(fileContents)."""
    return _lib.call_host(_lib.lib().rsn_huffman_compress_sharded, fileContents, int(shards))


def CompressBatch(chunks):
    """One complete .rsn segment per chunk, as engine.CompressFiles writes one file per input (engine.go:150-154).
    rsn_huffman_compress_batch runs chunks of 2 to BATCH_COMPRESS_INPUT_MAX bytes many to a launch, a workgroup each that builds the
    chunk's own tree on the device (byte alphabets; a chunk with a single distinct byte is handed back, one with a byte >= 0x80 goes to
    the rune class below, RUNE_GROUP_MIN), when at least two chunks are of that size.  Chunks above that and up to MID_IN_MAX bytes are the mid class (csrc/huff_mid.hip: the same kernel body at
    1024 threads, the whole chunk in LDS), grouped the same way when the call holds at least MID_GROUP_MIN of them; those of them with a byte >= 0x80 go to the mid-size rune class below, RUNE_MID_GROUP_MIN.  Chunks above that and up to BIG_IN_MAX bytes are the big class
    (csrc/huff_big.hip: tiles of BIG_TILE bytes, three launches a group) when the call holds at least BIG_GROUP_MIN of them.  The other chunks are dealt out over the batch workers (chunk k -> device k mod G) and go through a
    pipeline of upload / encode / download per device.  Each result equals Compress(chunk)."""
    return _lib.call_batch(_lib.lib().rsn_huffman_compress_batch, chunks)


# The largest chunk the batch encoder's grouped kernel takes (csrc/huff_small.hip HE_IN_MAX): its output -- at most 7 bits
# a byte of payload -- stays inside what one workgroup of the batch decoder holds, so the round trip is grouped both ways.
BATCH_COMPRESS_INPUT_MAX = 16384

# What one workgroup of the batch decoder holds (csrc/huff_small.hip HB_PAY_MAX / HB_OUT_MAX): a stream with more payload
# bytes (behind the header's backslash-newline and the pad byte), or more output, goes through the single call's path inside the batch.
BATCH_GROUP_PAYLOAD_MAX = 16384
BATCH_GROUP_OUTPUT_MAX = 32768


# The mid class of the two batch calls (csrc/codecs.h HUFF_MID_IN_MAX / HUFF_MID_PAY_MAX / HUFF_MID_OUT_MAX / HUFF_MID_GROUP_MIN):
# chunks above BATCH_COMPRESS_INPUT_MAX and up to MID_IN_MAX bytes, and streams beyond the two limits above whose header promises at most
# MID_OUT_MAX bytes from at most MID_PAY_MAX bytes of payload -- 7/8 of MID_IN_MAX, what a byte alphabet codes to at most -- go a workgroup
# each through one launch per group when a call holds at least MID_GROUP_MIN of them.
MID_IN_MAX = 65536
MID_PAY_MAX = 57344
MID_OUT_MAX = 65536
MID_GROUP_MIN = 4

# The big class of the compress batch calls (csrc/codecs.h HUFF_BIG_IN_MAX / HUFF_BIG_TILE / HUFF_BIG_GROUP_MIN / HUFF_BIG_GROUP_BYTES;
# csrc/huff_big.hip): chunks above MID_IN_MAX and up to BIG_IN_MAX bytes of a byte alphabet are cut into tiles of BIG_TILE bytes,
# a workgroup each, and go through three launches per group -- count, plan, emit -- when a call holds at least BIG_GROUP_MIN of them; a
# group holds up to BIG_GROUP_BYTES of staging.  A chunk whose deepest code has more than 24 bits (possible from 196418 bytes on) is handed
# back to the single call's path, like one with a single distinct byte or a byte >= 0x80.
BIG_IN_MAX = 262144
BIG_TILE = 16384
BIG_GROUP_MIN = 4
BIG_GROUP_BYTES = 67108864
# The way back (csrc/codecs.h HUFF_BIG_OUT_MAX / HUFF_BIG_PAY_MAX / HUFF_BIG_DEC_GROUP_MIN; csrc/huff_big_dec_layout.h BIGD_LANES / BIGD_S /
# BIGD_OUT_CAP; csrc/huff_big_dec.hip): streams of a byte alphabet whose header promises more than MID_OUT_MAX and at most
# BIG_OUT_MAX bytes from at most BIG_PAY_MAX bytes of payload are cut into tiles of BIG_DEC_LANES lanes of BIG_DEC_LANE_BITS code bits, a
# workgroup each, and go through three launches per group -- map, chain, emit -- when a decompress batch holds at least BIG_DEC_GROUP_MIN
# of them.  A stream with a tile of more than BIG_DEC_OUT_CAP - 16 symbols (fewer than 1.875 bits a symbol over the whole tile), one whose
# tiles need more than four phases a lane, and a malformed one take the single call's path inside the batch.  Every stream the big class
# above writes is one of the class.
BIG_OUT_MAX = 262144
BIG_PAY_MAX = 229376
BIG_DEC_GROUP_MIN = 4
BIG_DEC_LANES = 960
BIG_DEC_LANE_BITS = 64
BIG_DEC_OUT_CAP = 32768

# The rune class of the compress batch calls (csrc/codecs.h HUFF_RUNE_SYMS_MAX / HUFF_RUNE_GROUP_MIN; csrc/huff_rune.hip): chunks
# of at most BATCH_COMPRESS_INPUT_MAX bytes that hold a byte >= 0x80 -- UTF-8 text, or no UTF-8 at all -- go a workgroup each through one
# launch per group when a call holds at least RUNE_GROUP_MIN of them; a chunk with more than RUNE_SYMS_MAX distinct runes, or with one, takes
# the single call's path inside the batch, as every such chunk does in a call with fewer.
# The way back (csrc/huff_parse_rune.h HUFF_RUNE_DEC_GROUP_MIN / HUFF_RUNE_OUT_MAX / HUFF_RUNE_PAY_MAX; csrc/huff_rune_dec.hip): streams
# whose header names a rune >= 0x80, at most RUNE_SYMS_MAX distinct runes, and promises at most RUNE_OUT_MAX bytes from at most RUNE_PAY_MAX
# bytes of payload go a workgroup each through one launch per group when a decompress batch holds at least RUNE_DEC_GROUP_MIN of them; the
# others take the single call's path inside the batch.  Every stream the rune class above writes is one of them.
RUNE_SYMS_MAX = 256
RUNE_GROUP_MIN = 16
RUNE_OUT_MAX = 16384
RUNE_PAY_MAX = 18432
RUNE_DEC_GROUP_MIN = 16
# The mid-size rune class of the compress batch calls (csrc/huff_rune_mid_select.h HUFF_RUNE_MID_IN_MAX / HUFF_RUNE_MID_GROUP_MIN;
# csrc/huff_rune_mid.hip): chunks of more than BATCH_COMPRESS_INPUT_MAX and at most RUNE_MID_IN_MAX bytes that hold a byte >= 0x80
# go a workgroup each through one launch per group when a call holds at least RUNE_MID_GROUP_MIN of them; what it hands back is what the rune
# class above hands back.
# The way back (csrc/huff_parse_rune.h HUFF_RUNE_MID_OUT_MAX / HUFF_RUNE_MID_PAY_MAX / HUFF_RUNE_MID_DEC_GROUP_MIN;
# csrc/huff_rune_mid_dec.hip): rune streams that promise more than RUNE_OUT_MAX and at most RUNE_MID_OUT_MAX bytes from at most
# RUNE_MID_PAY_MAX bytes of payload go a workgroup each through one launch per group when a decompress batch holds at least
# RUNE_MID_DEC_GROUP_MIN of them.  Every stream the mid-size rune class writes for valid UTF-8 is one of them.
RUNE_MID_IN_MAX = 65536
RUNE_MID_GROUP_MIN = 16
RUNE_MID_OUT_MAX = 65536
RUNE_MID_PAY_MAX = 69120
RUNE_MID_DEC_GROUP_MIN = 16


def DecompressBatch(streams):
    """Decompress(stream) for every stream of the list in one call (rsn_huffman_decompress_batch): small streams many to a launch, a
    workgroup each; streams of up to MID_PAY_MAX bytes of payload that decode to at most MID_OUT_MAX bytes likewise (csrc/huff_mid.hip)
    when the call holds at least MID_GROUP_MIN of them; streams of a rune alphabet that decode to at most RUNE_OUT_MAX bytes likewise
    (csrc/huff_rune_dec.hip) when it holds at least RUNE_DEC_GROUP_MIN of them, and those that promise more than that and at most RUNE_MID_OUT_MAX
    bytes (csrc/huff_rune_mid_dec.hip) when it holds at least RUNE_MID_DEC_GROUP_MIN of them; streams of a byte alphabet that decode to more than MID_OUT_MAX and at most
    BIG_OUT_MAX bytes in tiles, three launches a group (csrc/huff_big_dec.hip), when it holds at least BIG_DEC_GROUP_MIN of them; the rest through the single call's path.  Each result equals Decompress(stream); a failing stream raises for the
    whole list (the message names the lowest failing index: "member <i>: ...")."""
    return _lib.call_batch(_lib.lib().rsn_huffman_decompress_batch, streams)


class Writer(_lib.Writer):
    """huffman.go:368-386: Write compresses the whole buffer once and returns len(compressed)."""

    def __init__(self, w):
        super().__init__(w, lambda data: Compress(data))


class Reader(_lib.Reader):
    """huffman.go:388-422: the first Read drains the source and decompresses everything."""

    def __init__(self, r):
        super().__init__(r, lambda data: Decompress(data))


def NewWriter(w):
    """huffman.go:372 NewWriter(io.Writer) io.WriteCloser"""
    return Writer(w)


def NewReader(r):
    """huffman.go:395 NewReader(io.Reader) io.Reader"""
    if isinstance(r, (bytes, bytearray)):
        r = io.BytesIO(r)
    return Reader(r)


def table(data):
    """[(rune, freq, code, len)] in printCodes order (huffman.go:110) as built by the library."""
    import ctypes

    import numpy as np
    L = _lib.lib()
    data = bytes(data)
    cap = 0x110000
    runes = np.zeros(cap, dtype=np.uint32)
    freqs = np.zeros(cap, dtype=np.uint64)
    codes = np.zeros(cap, dtype=np.uint64)
    lens = np.zeros(cap, dtype=np.uint8)
    a = L.rsn_huffman_table(data, len(data), runes.ctypes.data, freqs.ctypes.data, codes.ctypes.data, lens.ctypes.data, cap)
    if a < 0:
        _lib.check(int(a))
    return [(int(runes[i]), int(freqs[i]), int(codes[i]), int(lens[i])) for i in range(a)]


def plan(counts):
    """Host-only: {rune: count} -> ([(rune, code, len)] in printCodes order, header bytes).
    Runs the library's Go-exact tree builder without touching a device."""
    import ctypes

    import numpy as np
    L = _lib.lib()
    items = sorted(counts.items())
    runes = np.array([r for r, _ in items], dtype=np.uint32)
    cnts = np.array([c for _, c in items], dtype=np.uint64)
    n = len(items)
    o_r = np.zeros(max(n, 1), dtype=np.uint32)
    o_c = np.zeros(max(n, 1), dtype=np.uint64)
    o_l = np.zeros(max(n, 1), dtype=np.uint8)
    hdr = np.zeros(32 * max(n, 1), dtype=np.uint8)
    hl = ctypes.c_size_t(0)
    a = L.rsn_huffman_plan(runes.ctypes.data, cnts.ctypes.data, n, o_r.ctypes.data, o_c.ctypes.data, o_l.ctypes.data,
                           hdr.ctypes.data, hdr.size, ctypes.byref(hl))
    if a < 0:
        _lib.check(int(a))
    return [(int(o_r[i]), int(o_c[i]), int(o_l[i])) for i in range(a)], bytes(hdr[:hl.value])


def parse_header(header):
    """Host-only: decodeTree's header scan (huffman.go:196-227) -> [(rune, count)] ascending."""
    import numpy as np
    L = _lib.lib()
    header = bytes(header)
    cap = max(len(header), 1)
    runes = np.zeros(cap, dtype=np.uint32)
    cnts = np.zeros(cap, dtype=np.uint64)
    a = L.rsn_huffman_parse_header(header, len(header), runes.ctypes.data, cnts.ctypes.data, cap)
    if a < 0:
        _lib.check(int(a))
    return [(int(runes[i]), int(cnts[i])) for i in range(a)]


# ---- device-resident form (torch tensors as plain device memory) -----------
def compress_bound(n):
    return int(_lib.lib().rsn_huffman_compress_bound(n))


def compress_tensor(src, out=None, stream=None):
    """src: uint8 CUDA tensor.  Returns a uint8 tensor holding the .rsn bytes: a view of `out` when it was large
    enough, otherwise (RSN_ERR_CAPACITY) a view of a fresh tensor of the capacity the library asked for."""
    n = src.numel()
    return _lib.dev_tensor(_lib.lib().rsn_huffman_compress_dev, src, out, stream, n + n // 8 + (1 << 16))


def decompress_tensor(src, out=None, stream=None):
    """below 1 MiB of stream a generous guess costs less than a second call; from there the size query first"""
    n = src.numel()
    return _lib.dev_tensor(_lib.lib().rsn_huffman_decompress_dev, src, out, stream, 8 * n + (1 << 16) if n < (1 << 20) else None)


def compress_tensors(srcs, outs=None, stream=None):
    """compress_tensor for a list of 1-D uint8 CUDA tensors in ONE call (rsn_huffman_compress_batch_dev): the members of CompressBatch's
    classes run grouped on the device, the others the single call's codec; nothing of a member crosses to the host.  -> a list of
    tensors; without `outs`, views of one allocation of compress_bound(n) bytes a member.  An empty member raises, as Compress does."""
    return _lib.dev_tensors(_lib.lib().rsn_huffman_compress_batch_dev, srcs, outs, stream, compress_bound, retry=False)


def decompress_tensors(srcs, outs=None, stream=None):
    """decompress_tensor for a list of streams in ONE call (rsn_huffman_decompress_batch_dev): the headers are read on the device.  Without
    `outs`: a guess of eight times the stream plus 4 KiB a member (a two-symbol stream expands eightfold at most per payload byte); the
    members it does not hold are run once more."""
    return _lib.dev_tensors(_lib.lib().rsn_huffman_decompress_batch_dev, srcs, outs, stream, lambda n: 8 * n + 4096)
