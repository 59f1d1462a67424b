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


class Writer:
    """arithmetic.go:312-332: Write compresses the whole buffer once and returns len(compressed)."""

    def __init__(self, w):
        self.w = w

    def Write(self, data):
        compressed = Compress(data)
        self.w.write(compressed)
        return len(compressed)

    write = Write

    def Close(self):
        return None

    close = Close


class Reader:
    """arithmetic.go:335-370: the first Read drains the source and decompresses everything."""

    def __init__(self, r):
        self.r = r
        self.decompressed = None
        self.pos = 0

    def Read(self, size=-1):
        if self.decompressed is None:
            self.decompressed = Decompress(self.r.read())
        if size is None or size < 0:
            size = len(self.decompressed) - self.pos
        chunk = self.decompressed[self.pos:self.pos + size]
        self.pos += len(chunk)
        return chunk

    read = Read


def NewWriter(w):
    """arithmetic.go:317 NewWriter(io.Writer) io.WriteCloser"""
    return Writer(w)


def NewReader(r):
    """arithmetic.go:343 NewReader(io.Reader) io.Reader"""
    if isinstance(r, (bytes, bytearray)):
        r = io.BytesIO(r)
    return Reader(r)


# ---- device-resident form (torch tensors as plain device memory) -----------
from ._lib import own_stream as _own_stream  # noqa: E402


def compress_bound(n):
    return int(_lib.lib().rsn_arithmetic_compress_bound(n))


def _dev_tensor(fn, src, out, stream, guess):
    """`fn` over src -> a view of `out` when it was large enough, otherwise (RSN_ERR_CAPACITY: .needed is the exact size) a view of a
    fresh tensor of that size."""
    import torch
    n = src.numel()
    st = _own_stream(src, stream)
    if out is None:
        out = torch.empty(guess, dtype=torch.uint8, device=src.device)
    try:
        got = _lib.call_dev(fn, src.data_ptr(), n, out.data_ptr(), out.numel(), st)
    except _lib.RsnError as e:
        if e.code != _lib.RSN_ERR_CAPACITY:
            raise
        out = torch.empty(max(e.needed, 16), dtype=torch.uint8, device=src.device)
        got = _lib.call_dev(fn, src.data_ptr(), n, out.data_ptr(), out.numel(), st)
    return out[:got]


def compress_tensor(src, out=None, stream=None):
    """src: uint8 CUDA tensor.  Returns a uint8 tensor holding the stream."""
    return _dev_tensor(_lib.lib().rsn_arithmetic_compress_dev, src, out, stream, compress_bound(src.numel()))


def decompress_tensor(src, out=None, stream=None):
    """The decoded size is not in the stream: a guess of eight times the stream first, the exact size on the second call if that was
    too small."""
    return _dev_tensor(_lib.lib().rsn_arithmetic_decompress_dev, src, out, stream, 8 * src.numel() + 4096)
