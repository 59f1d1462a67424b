"""Mirror of /root/reference/compressor/lz (lzss.go) over librsn."""
import io

from . import _lib

DefaultWindowSize = 4096  # lzss.go:35
# The mid-size members of a batch (csrc/codecs.h: LZSS_MID_IN_MAX, LZSS_MID_E_MAX, LZSS_MID_GROUP_MIN; tests/test_lzss_mid_host.py holds
# the two together): inputs above 1 KiB and up to MID_IN_MAX bytes (window 1 to 4096) and streams above 2 KiB and up to MID_E_MAX bytes
# go many to a launch, a workgroup each, when a call holds at least MID_GROUP_MIN of them.
MID_IN_MAX = 65536
MID_E_MAX = 69632
MID_GROUP_MIN = 64
# The members of a compress batch above MID_IN_MAX (csrc/codecs.h: LZSS_TILE_IN_MAX, LZSS_TILE_E_MAX, LZSS_TILE_POS, LZSS_TILE_GROUP_MIN,
# LZSS_TILE_GROUP_BYTES; tests/test_lzss_tile_host.py holds the two together): inputs up to TILE_IN_MAX bytes (window 1 to 4096) are cut
# into tiles of TILE_POS escaped positions, a workgroup each, and a group of them is four launches, when a call holds at least
# TILE_GROUP_MIN of them.  A member that escapes to more than TILE_E_MAX bytes, or to more than one and a half times its length, and
# a member of runs or short periods take the single call's path.
TILE_IN_MAX = 262144
TILE_E_MAX = 278528
TILE_POS = 2048
TILE_GROUP_MIN = 16
TILE_GROUP_BYTES = 67108864
# The way back (csrc/codecs.h: LZSS_TILE_DEC_IN_MAX, LZSS_TILE_DEC_OUT_MAX, LZSS_TILE_DEC_GROUP_MIN; tests/test_lzss_tile_dec_host.py holds
# the two together): the streams of a decompress batch that the small and the mid class leave -- longer than 2 KiB and at most
# TILE_DEC_IN_MAX bytes, expanding to at most TILE_DEC_OUT_MAX escaped bytes -- are cut into tiles of TILE_POS bytes and a group of them is
# four launches, when a call holds at least TILE_DEC_GROUP_MIN of them.  Every stream the tiled encoder writes is one of them.
TILE_DEC_IN_MAX = TILE_E_MAX
TILE_DEC_OUT_MAX = TILE_E_MAX
TILE_DEC_GROUP_MIN = 8


def CompressAsync(fileContents, useProgressBar=False, maxSearchBufferLength=DefaultWindowSize):
    """lzss.go:109 CompressAsync([]byte, bool, int) []byte -- the engine/.rsn path
    (Writer.Write, lzss.go:53-57).  The progress bar has no equivalent."""
    return _lib.call_host(_lib.lib().rsn_lzss_compress, fileContents, int(maxSearchBufferLength))


def Compress(fileContents, useProgressBar=False, maxSearchBufferLength=DefaultWindowSize):
    """lzss.go:224 Compress([]byte, bool, int) []byte -- the older synchronous encoder (not the .rsn
    path; host-side, quirks included: see include/rsn.h)."""
    return _lib.call_host(_lib.lib().rsn_lzss_compress_legacy, fileContents, int(maxSearchBufferLength))


def Decompress(fileContents, useProgressBar=False):
    """lzss.go:323 Decompress([]byte, bool) []byte"""
    return _lib.call_host(_lib.lib().rsn_lzss_decompress, fileContents)


def CompressAsyncBatch(files, maxSearchBufferLength=DefaultWindowSize):
    """CompressAsync(f, False, maxSearchBufferLength) for every buffer of the list in one call (rsn_lzss_compress_batch): inputs of at most
    1 KiB many to a launch, a workgroup each; inputs up to MID_IN_MAX bytes likewise, through a kernel of their own, when the window is 1 to
    4096 and the list holds at least MID_GROUP_MIN of them; inputs above that and up to TILE_IN_MAX bytes tiled over the whole device, four
    launches a group, when the list holds at least TILE_GROUP_MIN of them; the rest through the single call's path.  Each result equals
    CompressAsync(f)."""
    return _lib.call_batch(_lib.lib().rsn_lzss_compress_batch, files, int(maxSearchBufferLength))


def DecompressBatch(streams):
    """Decompress(s) for every stream of the list in one call (rsn_lzss_decompress_batch); each result equals Decompress(s): streams of
    at most 2 KiB many to a launch, streams up to MID_E_MAX bytes likewise (at least MID_GROUP_MIN of them), what those leave up to
    TILE_DEC_IN_MAX bytes tiled over workgroups (at least TILE_DEC_GROUP_MIN of them), the rest through the single call's path.  A failing
    stream raises for the whole list (the message names the lowest failing index: "member <i>: ...")."""
    return _lib.call_batch(_lib.lib().rsn_lzss_decompress_batch, streams)


class Writer(_lib.Writer):
    """lzss.go:29-61"""

    def __init__(self, w, windowSize):
        super().__init__(w, lambda data: CompressAsync(data, self.useProgressBar, self.windowSize))
        self.windowSize = windowSize
        self.useProgressBar = True


class Reader(_lib.Reader):
    """lzss.go:63-106"""

    def __init__(self, r):
        super().__init__(r, lambda data: Decompress(data, True))

    def Close(self):
        return None


def NewWriterLevel(w, level):
    """lzss.go:42-51: level is the window size; negative levels are an error."""
    if level < 0:
        raise ValueError("lzss: invalid compression level: %d" % level)
    return Writer(w, level)


def NewWriter(w):
    """lzss.go:37 NewWriter(io.Writer) io.WriteCloser (window 4096)"""
    return NewWriterLevel(w, DefaultWindowSize)


def NewReader(r):
    """lzss.go:98 NewReader(io.Reader) io.Reader"""
    if isinstance(r, (bytes, bytearray)):
        r = io.BytesIO(r)
    return Reader(r)


def compress_bound(n):
    return int(_lib.lib().rsn_lzss_compress_bound(n))


def compress_tensor(src, window=DefaultWindowSize, out=None, stream=None):
    """no second call here: an `out` that is too small raises (RsnError.needed: the size that suffices)"""
    return _lib.dev_tensor(_lib.lib().rsn_lzss_compress_dev, src, out, stream, compress_bound(src.numel()), int(window), retry=False)


def decompress_tensor(src, out=None, stream=None):
    """below 1 MiB of stream a generous guess costs less than a second call; from there the size query first"""
    n = src.numel()
    return _lib.dev_tensor(_lib.lib().rsn_lzss_decompress_dev, src, out, stream, 16 * n + (1 << 16) if n < (1 << 20) else None)


def compress_tensors(srcs, window=DefaultWindowSize, outs=None, stream=None):
    """compress_tensor for a list of 1-D uint8 CUDA tensors in ONE call (rsn_lzss_compress_batch_dev): the members of CompressAsyncBatch's
    classes many to a launch without leaving the device, the rest through the single call's path.  Each tensor's data_ptr must be 16-byte
    aligned (slices of one allocation at 16-byte offsets are).  Returns the streams, trimmed; without `outs` they are views of one
    allocation of bound-sized slots.  An `out` that is too small raises (RsnError.out_lens: sizes that suffice)."""
    return _lib.dev_tensors(_lib.lib().rsn_lzss_compress_batch_dev, srcs, outs, stream, compress_bound, int(window), retry=False)


def decompress_tensors(srcs, outs=None, stream=None):
    """decompress_tensor for a list of streams in ONE call (rsn_lzss_decompress_batch_dev).  Without `outs`: a guess of sixteen times the
    stream plus 4 KiB per member, and the members that expand further are run once more with the capacities the call reports."""
    return _lib.dev_tensors(_lib.lib().rsn_lzss_decompress_batch_dev, srcs, outs, stream, lambda n: 16 * n + 4096)
