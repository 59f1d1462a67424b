"""The engine's unit of work over librsn: a LIST of layers applied to one buffer (engine.go:443-479), with the stream kept on the device
between the layers (rsn_layers_*, include/rsn.h).  Layers are given by the engine's names, in compress order."""
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
