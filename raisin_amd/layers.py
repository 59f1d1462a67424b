"""The engine's unit of work over librsn: a LIST of layers applied to one buffer (engine.go:443-479), with the stream kept on the device
between the layers (rsn_layers_*, include/rsn.h), and the same over MANY buffers in one call, layer-major, every member on the device from
the first layer to the last (rsn_layers_*_batch, rsn_layers_*_batch_dev).  Layers are given by the engine's names, in compress order."""
import ctypes

from . import _lib

LZSS, HUFFMAN = 1, 2          # RSN_LAYER_LZSS, RSN_LAYER_HUFFMAN
LAYERS_MAX = 8                # RSN_LAYERS_MAX
IDS = {"lzss": LZSS, "huffman": HUFFMAN}


def ids(layers):
    """(ctypes int array, count) of the engine's layer names"""
    try:
        v = [IDS[a] for a in layers]
    except KeyError as e:
        raise ValueError("unknown layer %r (this build carries: lzss, huffman)" % (e.args[0],)) from None
    return (ctypes.c_int * max(len(v), 1))(*v), len(v)


def Compress(data, layers):
    """engine.compress(data, layers): byte for byte the chain of lz.CompressAsync / huffman.Compress in order."""
    arr, k = ids(layers)
    return _lib.call_host(_lib.lib().rsn_layers_compress, data, arr, k)


def Decompress(data, layers):
    """engine.decompress(data, layers): the layers undone last to first."""
    arr, k = ids(layers)
    return _lib.call_host(_lib.lib().rsn_layers_decompress, data, arr, k)


def compress_tensor(src, layers, out=None, stream=None):
    """src: uint8 CUDA tensor -> a uint8 tensor holding the layered stream (a view of `out` when it was large enough)."""
    n = src.numel()
    return _lib.dev_tensor(_lib.lib().rsn_layers_compress_dev, src, out, stream, n + n // 4 + (1 << 16), *ids(layers), floor=16)


def decompress_tensor(src, layers, out=None, stream=None):
    """from 1 MiB of stream up the size query first (d_out NULL): it runs the chain once, rsn.h"""
    n = src.numel()
    return _lib.dev_tensor(_lib.lib().rsn_layers_decompress_dev, src, out, stream, 8 * n + (1 << 16) if n < (1 << 20) else None, *ids(layers), floor=16)


def CompressBatch(datas, layers):
    """engine.CompressFiles' work on a list of buffers: element i is byte for byte Compress(datas[i], layers)."""
    arr, k = ids(layers)
    return _lib.call_batch(_lib.lib().rsn_layers_compress_batch, datas, arr, k)


def DecompressBatch(datas, layers):
    """engine.DecompressFiles' work on a list of streams: element i is byte for byte Decompress(datas[i], layers)."""
    arr, k = ids(layers)
    return _lib.call_batch(_lib.lib().rsn_layers_decompress_batch, datas, arr, k)


def compress_bound(n, layers):
    """a capacity that always suffices for the layered stream of n bytes: the codecs' bounds applied in turn"""
    L = _lib.lib()
    for a in layers:
        n = L.rsn_huffman_compress_bound(n) if IDS[a] == HUFFMAN else L.rsn_lzss_compress_bound(n)
    return n


def compress_tensors(srcs, layers, outs=None, stream=None):
    """a list of uint8 CUDA tensors (16-byte aligned) -> the list of their layered streams, in one call (rsn_layers_compress_batch_dev);
    without `outs`, views of one allocation with a slot of compress_bound bytes a member."""
    arr, k = ids(layers)
    return _lib.dev_tensors(_lib.lib().rsn_layers_compress_batch_dev, srcs, outs, stream, lambda n: compress_bound(n, layers), arr, k)


def decompress_tensors(srcs, layers, outs=None, stream=None):
    """the list of layered streams -> the list of what they hold (rsn_layers_decompress_batch_dev); a member that outgrows its slot of
    8 * n + 64 KiB -- or its `out` -- is run once more, with the others of its kind, into an allocation of the size the call reported."""
    arr, k = ids(layers)
    return _lib.dev_tensors(_lib.lib().rsn_layers_decompress_batch_dev, srcs, outs, stream, lambda n: 8 * n + (1 << 16), arr, k)


def RoundTrip(data, layers, keep_compressed=False):
    """engine.BenchmarkFile's body on the device (rsn_layers_roundtrip): returns (RoundTripResult, compressed bytes or None)."""
    L = _lib.lib()
    arr, k = ids(layers)
    data = bytes(data)
    res = _lib.RoundTripResult()
    if not keep_compressed:
        _lib.check(L.rsn_layers_roundtrip(data, len(data), arr, k, ctypes.byref(res), None, None))
        return res, None
    out = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_size_t(0)
    _lib.check(L.rsn_layers_roundtrip(data, len(data), arr, k, ctypes.byref(res), ctypes.byref(out), ctypes.byref(n)))
    try:
        return res, ctypes.string_at(out, n.value)
    finally:
        L.rsn_free(out)
