"""Mirror of /root/reference/compressor/arithmetic (arithmetic.go) over librsn: the adaptive arithmetic codec.

One stream is one wavefront's serial work: the batch calls, which run a wavefront per member, are the fast path."""
import io

from . import _lib

# symbols a kernel launch codes per member at most (csrc/codecs.h ARITH_SLICE_SYMBOLS): longer members carry their state from launch to launch
SLICE_SYMBOLS = 65536
# bits the decoder shifts in from behind a stream's end before it gives up on an end symbol (include/rsn.h RSN_ARITH_TAIL_BITS)
TAIL_BITS = 4096
# the largest member: input of Compress, output of Decompress (include/rsn.h RSN_ARITH_MAX_BYTES)
MAX_BYTES = 64 << 20


def Compress(fileContents):
    """arithmetic.go:15 Compress([]byte) []byte"""
    return _lib.call_host(_lib.lib().rsn_arithmetic_compress, fileContents)


def Decompress(fileContents):
    """arithmetic.go:27 Decompress([]byte) []byte -- RsnError (-3) where the reference panics, and where it would decode for ever"""
    return _lib.call_host(_lib.lib().rsn_arithmetic_decompress, fileContents)


def CompressBatch(files):
    """Compress(f) for every buffer of the list in one call (rsn_arithmetic_compress_batch), a wavefront per member; each result
    equals Compress(f)."""
    return _lib.call_batch(_lib.lib().rsn_arithmetic_compress_batch, files)


def DecompressBatch(streams):
    """Decompress(s) for every stream of the list in one call (rsn_arithmetic_decompress_batch); each result equals Decompress(s).  A
    failing stream raises for the whole list (the message names the lowest failing index: "member <i>: ...")."""
    return _lib.call_batch(_lib.lib().rsn_arithmetic_decompress_batch, streams)


class Writer(_lib.Writer):
    """arithmetic.go:312-332: Write compresses the whole buffer once and returns len(compressed)."""

    def __init__(self, w):
        super().__init__(w, lambda data: Compress(data))


class Reader(_lib.Reader):
    """arithmetic.go:335-370: the first Read drains the source and decompresses everything."""

    def __init__(self, r):
        super().__init__(r, lambda data: Decompress(data))


def NewWriter(w):
    """arithmetic.go:317 NewWriter(io.Writer) io.WriteCloser"""
    return Writer(w)


def NewReader(r):
    """arithmetic.go:343 NewReader(io.Reader) io.Reader"""
    if isinstance(r, (bytes, bytearray)):
        r = io.BytesIO(r)
    return Reader(r)


# ---- device-resident form (torch tensors as plain device memory) -----------
def compress_bound(n):
    return int(_lib.lib().rsn_arithmetic_compress_bound(n))


def compress_tensor(src, out=None, stream=None):
    """src: uint8 CUDA tensor.  Returns a uint8 tensor holding the stream."""
    return _lib.dev_tensor(_lib.lib().rsn_arithmetic_compress_dev, src, out, stream, compress_bound(src.numel()), floor=16)


def decompress_tensor(src, out=None, stream=None):
    """The decoded size is not in the stream: a guess of eight times the stream first, the exact size on the second call if that was
    too small."""
    return _lib.dev_tensor(_lib.lib().rsn_arithmetic_decompress_dev, src, out, stream, 8 * src.numel() + 4096, floor=16)


def compress_tensors(srcs, outs=None, stream=None):
    """compress_tensor for a list of 1-D uint8 CUDA tensors in ONE call (rsn_arithmetic_compress_batch_dev): a wavefront per member, the
    members coded where they lie -- the fast path for data that is on the device already.  Each tensor's data_ptr must be 16-byte aligned
    (slices of one allocation at 16-byte offsets are).  Returns the streams, trimmed; without `outs` they are views of one allocation of
    bound-sized slots."""
    return _lib.dev_tensors(_lib.lib().rsn_arithmetic_compress_batch_dev, srcs, outs, stream, compress_bound)


def decompress_tensors(srcs, outs=None, stream=None):
    """decompress_tensor for a list of streams in ONE call (rsn_arithmetic_decompress_batch_dev).  Without `outs`: a guess of eight times
    the stream plus 4 KiB per member; the members that decode to more are run once more with the exact sizes the call reports."""
    return _lib.dev_tensors(_lib.lib().rsn_arithmetic_decompress_batch_dev, srcs, outs, stream, lambda n: 8 * n + 4096)
