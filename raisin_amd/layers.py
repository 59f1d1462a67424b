"""The engine's unit of work over librsn: a LIST of layers applied to one buffer (engine.go:443-479), with the stream kept on the device
between the layers (rsn_layers_*, include/rsn.h), and the same over MANY buffers in one call, layer-major, every member on the device from
the first layer to the last (rsn_layers_*_batch, rsn_layers_*_batch_dev) -- and the benchmark's whole body over many buffers, compressed,
undone, compared and counted on the device (rsn_layers_roundtrip_batch, rsn_layers_roundtrip_batch_dev), under one layer list or under
several that share their common prefixes' work (rsn_layers_suite_batch, rsn_layers_suite_batch_dev).  Layers are given by the engine's
names, in compress order."""
import ctypes
from dataclasses import dataclass

from . import _lib

LZSS, HUFFMAN = 1, 2          # RSN_LAYER_LZSS, RSN_LAYER_HUFFMAN
LAYERS_MAX = 8                # RSN_LAYERS_MAX
SUITE_LISTS_MAX = 16          # RSN_SUITE_LISTS_MAX
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


@dataclass
class RoundTripMember:
    """rsn_roundtrip_member, and the member's two histograms (lists of 256 counts) when they were asked for"""
    original_n: int
    compressed_n: int
    decompressed_n: int
    first_difference: int
    lossless: bool
    hist_original: list = None
    hist_decompressed: list = None


def _roundtrip_batch(k, hists, call):
    """call(res, counts) over k members -> the list of RoundTripMember"""
    import numpy as np
    res = (_lib.RoundTripMember * max(k, 1))()
    counts = np.zeros(512 * max(k, 1), dtype=np.uint32) if hists else None
    _lib.check(call(res, counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if hists else None))
    out = []
    for i in range(k):
        r = res[i]
        m = RoundTripMember(int(r.original_n), int(r.compressed_n), int(r.decompressed_n), int(r.first_difference), bool(r.lossless))
        if hists:
            m.hist_original = counts[512 * i:512 * i + 256].tolist()
            m.hist_decompressed = counts[512 * i + 256:512 * i + 512].tolist()
        out.append(m)
    return out


def RoundTripBatch(datas, layers, hists=True):
    """engine.BenchmarkFile's body over a list of buffers in one call (rsn_layers_roundtrip_batch): element i holds what
    RoundTrip(datas[i], layers) reports -- the sizes, lossless or not, where the buffers first differ -- and, with `hists`, both byte
    histograms.  If any member fails the call raises, naming the member and the layer."""
    arr, k = ids(layers)
    L = _lib.lib()
    datas = [bytes(d) for d in datas]
    n = len(datas)
    ins = (ctypes.c_char_p * max(n, 1))(*datas)
    lens = (ctypes.c_size_t * max(n, 1))(*[len(d) for d in datas])
    return _roundtrip_batch(n, hists, lambda res, counts: L.rsn_layers_roundtrip_batch(n, ins, lens, arr, k, res, counts))


def roundtrip_tensors(srcs, layers, hists=True, stream=None):
    """the same for a list of uint8 CUDA tensors (16-byte aligned), read where they lie and never written (rsn_layers_roundtrip_batch_dev);
    only the answers come down."""
    arr, k = ids(layers)
    srcs = list(srcs)
    if not srcs:
        return []
    L = _lib.lib()
    st = _lib.own_stream(srcs[0], stream)
    n = len(srcs)
    mem = (_lib.DevMember * n)(*[_lib.DevMember(t.data_ptr() if t.numel() else None, t.numel(), None, 0) for t in srcs])
    return _roundtrip_batch(n, hists, lambda res, counts: L.rsn_layers_roundtrip_batch_dev(n, mem, arr, k, res, counts, st))


def _suite(n, lists, hists, call):
    """call(L, n_lists, arr, res, codes, ho, hd, best) over n members under `lists` -> (rows, best, list_errors)"""
    import numpy as np
    k = len(lists)
    keep = [ids(a) for a in lists]                        # (unknown names raise here, before the library is looked for)
    L = _lib.lib()
    arr = (_lib.LayerList * max(k, 1))(*[_lib.LayerList(ctypes.cast(a, ctypes.POINTER(ctypes.c_int)), c) for a, c in keep])
    res = (_lib.RoundTripMember * max(k * n, 1))()
    NOT_RUN = 1                                           # no code of the library's: the call writes the codes only when it ran its lists
    codes = (ctypes.c_int * max(k, 1))(*([NOT_RUN] * max(k, 1)))
    best = np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32)
    ho = np.zeros(256 * max(n, 1), dtype=np.uint32) if hists else None
    hd = np.zeros(256 * max(k * n, 1), dtype=np.uint32) if hists else None
    u32p = ctypes.POINTER(ctypes.c_uint32)
    rc = call(L, k, arr, res, codes, ho.ctypes.data_as(u32p) if hists else None, hd.ctypes.data_as(u32p) if hists else None, best.ctypes.data_as(u32p))
    if n == 0 or k == 0:
        _lib.check(rc)
        return [[] for _ in range(k)], [None] * n, [None] * k
    if rc and any(codes[l] == NOT_RUN for l in range(k)):
        _lib.check(rc)                                    # the call as a whole failed
    message = L.rsn_last_error().decode("utf-8", "replace") if rc else ""
    errors, first = [], True
    for l in range(k):
        if codes[l] == 0:
            errors.append(None)
            continue
        errors.append(_lib.RsnError(codes[l], message if first else "list %d: failed" % l))
        first = False
    rows = []
    for l in range(k):
        if errors[l] is not None:
            rows.append(None)
            continue
        row = []
        for i in range(n):
            r = res[l * n + i]
            m = RoundTripMember(int(r.original_n), int(r.compressed_n), int(r.decompressed_n), int(r.first_difference), bool(r.lossless))
            if hists:
                m.hist_original = ho[256 * i:256 * i + 256].tolist()
                m.hist_decompressed = hd[256 * (l * n + i):256 * (l * n + i) + 256].tolist()
            row.append(m)
        rows.append(row)
    return rows, [None if b == 0xFFFFFFFF else int(b) for b in best[:n]], errors


def SuiteBatch(datas, lists, hists=True):
    """The benchmark loop of files x layer lists in one call (rsn_layers_suite_batch): -> (rows, best, list_errors).  rows[l][i] holds what
    RoundTripBatch(datas, lists[l])[i] holds -- every shared prefix of the lists is compressed once, the members go up once and their bytes
    are counted once -- or rows[l] is None where list l failed, list_errors[l] then being the RsnError that call raises for it alone (the
    message: of the failing list of the lowest index; the code: of every one) and None otherwise.  best[i]: the list with the smallest
    compressed size of member i among those that succeeded, the lowest index among equals; None when none did."""
    datas = [bytes(d) for d in datas]
    n = len(datas)
    ins = (ctypes.c_char_p * max(n, 1))(*datas)
    lens = (ctypes.c_size_t * max(n, 1))(*[len(d) for d in datas])
    return _suite(n, list(lists), hists, lambda L, k, arr, res, codes, ho, hd, best: L.rsn_layers_suite_batch(n, ins, lens, k, arr, res, codes, ho, hd, best))


def suite_tensors(srcs, lists, hists=True, stream=None):
    """the same for a list of uint8 CUDA tensors (16-byte aligned), read where they lie and never written (rsn_layers_suite_batch_dev)"""
    lists, srcs = list(lists), list(srcs)
    if not srcs:
        for a in lists:
            ids(a)                                        # (unknown names raise all the same)
        return [[] for _ in lists], [], [None] * len(lists)
    st = _lib.own_stream(srcs[0], stream)
    n = len(srcs)
    mem = (_lib.DevMember * n)(*[_lib.DevMember(t.data_ptr() if t.numel() else None, t.numel(), None, 0) for t in srcs])
    return _suite(n, lists, hists, lambda L, k, arr, res, codes, ho, hd, best: L.rsn_layers_suite_batch_dev(n, mem, k, arr, res, codes, ho, hd, best, st))
