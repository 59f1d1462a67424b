"""ctypes binding of librsn.so (include/rsn.h).  The library is the product: if
it is missing or cannot reach a HIP device every call raises -- there is no
Python or CPU fallback anywhere in this package."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RSN_LIB_PATH") or os.path.join(_HERE, "librsn.so")   # RSN_LIB_PATH: another BUILD of librsn (A/B of compile-time switches)

RSN_OK = 0
RSN_ERR_CAPACITY = -7

# RSN_NO_TORCH=1: this package never imports torch -- bytes, numpy and ctypes only.  librsn then runs on the HIP runtime it is linked
# against (the system's /opt/rocm, ROCm 7.2), which is the runtime a C or Go (cgo) host gets; with torch imported first the process
# resolves libamdhip64.so.7 to the copy torch bundles (ROCm 7.0.2, same SONAME) and librsn runs on THAT one -- the two differ in
# behaviour (under torch's, a download does not start while an upload runs: DESIGN 0, INTEGRATION.md "Which HIP runtime").  The
# parity suites that only need the host-buffer API run once in each mode (tests/test_gpu_no_torch.py).
NO_TORCH = os.environ.get("RSN_NO_TORCH") == "1"


class RsnError(RuntimeError):
    """Raised where the reference would panic (check(e) / index out of range)."""

    def __init__(self, code, msg):
        super().__init__("librsn error %d: %s" % (code, msg))
        self.code = code


class ProfEntry(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 48), ("launches", ctypes.c_uint64), ("total_ms", ctypes.c_double)]


class RoundTripResult(ctypes.Structure):
    """rsn_roundtrip_result (include/rsn.h)"""
    _fields_ = [("original_n", ctypes.c_uint64), ("compressed_n", ctypes.c_uint64), ("decompressed_n", ctypes.c_uint64),
                ("lossless", ctypes.c_int), ("first_difference", ctypes.c_uint64),
                ("hist_original", ctypes.c_uint64 * 256), ("hist_decompressed", ctypes.c_uint64 * 256),
                ("compress_ms", ctypes.c_double), ("decompress_ms", ctypes.c_double)]


class RoundTripMember(ctypes.Structure):
    """rsn_roundtrip_member (include/rsn.h): one member's answer of the batch round trip"""
    _fields_ = [("original_n", ctypes.c_uint64), ("compressed_n", ctypes.c_uint64), ("decompressed_n", ctypes.c_uint64),
                ("first_difference", ctypes.c_uint64), ("lossless", ctypes.c_int)]


class LayerList(ctypes.Structure):
    """rsn_layer_list (include/rsn.h): one layer list of the batch suite, in compress order"""
    _fields_ = [("layers", ctypes.POINTER(ctypes.c_int)), ("n_layers", ctypes.c_size_t)]


class DevMember(ctypes.Structure):
    """rsn_dev_member (include/rsn.h): one member of a batch call on device buffers"""
    _fields_ = [("d_in", ctypes.c_void_p), ("n", ctypes.c_size_t), ("d_out", ctypes.c_void_p), ("out_cap", ctypes.c_size_t)]


_lib = None

SYMBOLS = [
    "rsn_device_set", "rsn_device_count", "rsn_last_error", "rsn_version", "rsn_free", "rsn_trim",
    "rsn_huffman_compress", "rsn_huffman_decompress", "rsn_lzss_compress", "rsn_lzss_decompress", "rsn_lzss_compress_legacy",
    "rsn_huffman_compress_batch", "rsn_huffman_compress_sharded",
    "rsn_huffman_decompress_batch", "rsn_lzss_compress_batch", "rsn_lzss_decompress_batch",
    "rsn_huffman_compress_bound", "rsn_lzss_compress_bound",
    "rsn_huffman_compress_dev", "rsn_huffman_decompress_dev", "rsn_lzss_compress_dev", "rsn_lzss_decompress_dev",
    "rsn_prof_enable", "rsn_prof_reset", "rsn_prof_get", "rsn_huffman_table",
    "rsn_huffman_plan", "rsn_huffman_parse_header", "rsn_huffman_slice_cuts",
    "rsn_layers_compress", "rsn_layers_decompress", "rsn_layers_compress_dev", "rsn_layers_decompress_dev", "rsn_layers_roundtrip",
    "rsn_prof_copied",
    "rsn_arithmetic_compress_bound", "rsn_arithmetic_compress", "rsn_arithmetic_decompress",
    "rsn_arithmetic_compress_batch", "rsn_arithmetic_decompress_batch", "rsn_arithmetic_compress_dev", "rsn_arithmetic_decompress_dev",
    "rsn_lzss_compress_batch_dev", "rsn_lzss_decompress_batch_dev", "rsn_arithmetic_compress_batch_dev", "rsn_arithmetic_decompress_batch_dev",
    "rsn_huffman_compress_batch_dev", "rsn_huffman_decompress_batch_dev",
    "rsn_layers_compress_batch", "rsn_layers_decompress_batch", "rsn_layers_compress_batch_dev", "rsn_layers_decompress_batch_dev",
    "rsn_layers_roundtrip_batch", "rsn_layers_roundtrip_batch_dev",
    "rsn_layers_suite_batch", "rsn_layers_suite_batch_dev",
]


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("raisin_amd: %s not found -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C raisin_amd/csrc`; there is no fallback path" % LIB_PATH)
    # librsn is LINKED against the system ROCm runtime (/opt/rocm, libamdhip64.so.7); PyTorch bundles a copy of an older release
    # under the same SONAME.  A process holds ONE library per SONAME: whichever is loaded first serves both, so with torch imported
    # first (below: the tensor helpers and bench.py need it, and torch must initialise its own copy) librsn runs on torch's runtime,
    # not on the one it was linked against (hipRuntimeGetVersion 70051831 against 70226015, r05).  Device memory is shared by
    # address either way; stream / event HANDLES are never exchanged (librsn always runs on its own stream, see the tensor helpers).
    # RSN_NO_TORCH=1 skips the import: the runtime a C / Go host gets.
    if not NO_TORCH:
        try:
            import torch  # noqa: F401
            if torch.cuda.is_available():
                torch.cuda.init()
        except ImportError:
            pass
    L = ctypes.CDLL(LIB_PATH)
    u8p = ctypes.POINTER(ctypes.c_uint8)
    vp, sz, szp = ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)
    L.rsn_last_error.restype = ctypes.c_char_p
    L.rsn_version.restype = ctypes.c_char_p
    L.rsn_trim.argtypes = []
    L.rsn_trim.restype = None
    L.rsn_free.argtypes = [vp]
    L.rsn_free.restype = None
    L.rsn_device_set.argtypes = [ctypes.c_int]
    for name in ("rsn_huffman_compress", "rsn_huffman_decompress", "rsn_lzss_decompress", "rsn_arithmetic_compress", "rsn_arithmetic_decompress"):
        getattr(L, name).argtypes = [ctypes.c_char_p, sz, ctypes.POINTER(u8p), szp]
    L.rsn_lzss_compress.argtypes = [ctypes.c_char_p, sz, ctypes.c_int64, ctypes.POINTER(u8p), szp]
    L.rsn_lzss_compress_legacy.argtypes = [ctypes.c_char_p, sz, ctypes.c_int64, ctypes.POINTER(u8p), szp]
    L.rsn_huffman_compress_bound.argtypes = [sz]
    L.rsn_huffman_compress_bound.restype = sz
    L.rsn_lzss_compress_bound.argtypes = [sz]
    L.rsn_lzss_compress_bound.restype = sz
    L.rsn_arithmetic_compress_bound.argtypes = [sz]
    L.rsn_arithmetic_compress_bound.restype = sz
    for name in ("rsn_huffman_compress_dev", "rsn_huffman_decompress_dev", "rsn_lzss_decompress_dev", "rsn_arithmetic_compress_dev", "rsn_arithmetic_decompress_dev"):
        getattr(L, name).argtypes = [vp, sz, vp, sz, szp, vp]
    L.rsn_lzss_compress_dev.argtypes = [vp, sz, ctypes.c_int64, vp, sz, szp, vp]
    mp = ctypes.POINTER(DevMember)
    L.rsn_lzss_compress_batch_dev.argtypes = [sz, mp, ctypes.c_int64, szp, vp]
    for name in ("rsn_lzss_decompress_batch_dev", "rsn_arithmetic_compress_batch_dev", "rsn_arithmetic_decompress_batch_dev",
                 "rsn_huffman_compress_batch_dev", "rsn_huffman_decompress_batch_dev"):
        getattr(L, name).argtypes = [sz, mp, szp, vp]
    L.rsn_prof_enable.argtypes = [ctypes.c_int]
    L.rsn_prof_enable.restype = None
    L.rsn_prof_reset.restype = None
    L.rsn_prof_get.argtypes = [ctypes.POINTER(ProfEntry), ctypes.c_int]
    L.rsn_huffman_table.argtypes = [ctypes.c_char_p, sz, vp, vp, vp, vp, sz]
    L.rsn_huffman_table.restype = ctypes.c_int64
    L.rsn_huffman_plan.argtypes = [vp, vp, sz, vp, vp, vp, vp, sz, szp]
    L.rsn_huffman_plan.restype = ctypes.c_int64
    L.rsn_huffman_parse_header.argtypes = [ctypes.c_char_p, sz, vp, vp, sz]
    L.rsn_huffman_parse_header.restype = ctypes.c_int64
    L.rsn_huffman_slice_cuts.argtypes = [ctypes.c_char_p, sz, ctypes.c_int, szp, sz]
    L.rsn_huffman_slice_cuts.restype = ctypes.c_int64
    L.rsn_huffman_compress_sharded.argtypes = [ctypes.c_char_p, sz, ctypes.c_int, ctypes.POINTER(u8p), szp]
    L.rsn_huffman_compress_batch.argtypes = [sz, ctypes.POINTER(ctypes.c_char_p), szp, ctypes.POINTER(u8p), szp]
    L.rsn_huffman_decompress_batch.argtypes = [sz, ctypes.POINTER(ctypes.c_char_p), szp, ctypes.POINTER(u8p), szp]
    for name in ("rsn_arithmetic_compress_batch", "rsn_arithmetic_decompress_batch"):
        getattr(L, name).argtypes = [sz, ctypes.POINTER(ctypes.c_char_p), szp, ctypes.POINTER(u8p), szp]
    L.rsn_lzss_compress_batch.argtypes = [sz, ctypes.POINTER(ctypes.c_char_p), szp, ctypes.c_int64, ctypes.POINTER(u8p), szp]
    L.rsn_lzss_decompress_batch.argtypes = [sz, ctypes.POINTER(ctypes.c_char_p), szp, ctypes.POINTER(u8p), szp]
    ip = ctypes.POINTER(ctypes.c_int)
    for name in ("rsn_layers_compress", "rsn_layers_decompress"):
        getattr(L, name).argtypes = [ctypes.c_char_p, sz, ip, sz, ctypes.POINTER(u8p), szp]
    for name in ("rsn_layers_compress_dev", "rsn_layers_decompress_dev"):
        getattr(L, name).argtypes = [vp, sz, ip, sz, vp, sz, szp, vp]
    for name in ("rsn_layers_compress_batch", "rsn_layers_decompress_batch"):
        getattr(L, name).argtypes = [sz, ctypes.POINTER(ctypes.c_char_p), szp, ip, sz, ctypes.POINTER(u8p), szp]
    for name in ("rsn_layers_compress_batch_dev", "rsn_layers_decompress_batch_dev"):
        getattr(L, name).argtypes = [sz, mp, ip, sz, szp, vp]
    L.rsn_layers_roundtrip.argtypes = [ctypes.c_char_p, sz, ip, sz, ctypes.POINTER(RoundTripResult), ctypes.POINTER(u8p), szp]
    rmp, u32p = ctypes.POINTER(RoundTripMember), ctypes.POINTER(ctypes.c_uint32)
    L.rsn_layers_roundtrip_batch.argtypes = [sz, ctypes.POINTER(ctypes.c_char_p), szp, ip, sz, rmp, u32p]
    L.rsn_layers_roundtrip_batch_dev.argtypes = [sz, mp, ip, sz, rmp, u32p, vp]
    llp, i32p = ctypes.POINTER(LayerList), ctypes.POINTER(ctypes.c_int)
    L.rsn_layers_suite_batch.argtypes = [sz, ctypes.POINTER(ctypes.c_char_p), szp, sz, llp, rmp, i32p, u32p, u32p, u32p]
    L.rsn_layers_suite_batch_dev.argtypes = [sz, mp, sz, llp, rmp, i32p, u32p, u32p, u32p, vp]
    L.rsn_prof_copied.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    L.rsn_prof_copied.restype = None
    _lib = L
    return L


def check(rc):
    if rc != RSN_OK:
        raise RsnError(rc, lib().rsn_last_error().decode("utf-8", "replace"))


def call_host(fn, data, *extra):
    """bytes in -> bytes out through a host-buffer entry point."""
    L = lib()
    data = bytes(data)
    out = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_size_t(0)
    check(fn(data, len(data), *extra, ctypes.byref(out), ctypes.byref(n)))
    try:
        return ctypes.string_at(out, n.value)
    finally:
        L.rsn_free(out)


def call_batch(fn, chunks, *extra):
    """list of bytes in -> list of bytes out through a batch entry point (rsn_*_batch: n, ins, lens, [extra,] outs, out_lens)."""
    L = lib()
    chunks = [bytes(c) for c in chunks]
    k = len(chunks)
    ins = (ctypes.c_char_p * max(k, 1))(*chunks)
    lens = (ctypes.c_size_t * max(k, 1))(*[len(c) for c in chunks])
    outs = (ctypes.POINTER(ctypes.c_uint8) * max(k, 1))()
    olens = (ctypes.c_size_t * max(k, 1))()
    check(fn(k, ins, lens, *extra, outs, olens))
    try:
        return [ctypes.string_at(outs[i], olens[i]) for i in range(k)]
    finally:
        for i in range(k):
            L.rsn_free(outs[i])


def call_dev(fn, d_in, n, d_out, cap, stream, *extra):
    """device pointers in/out; returns the produced size.  On RSN_ERR_CAPACITY
    raises RsnError whose .needed holds the capacity that would have sufficed."""
    got = ctypes.c_size_t(0)
    rc = fn(d_in, n, *extra, d_out, cap, ctypes.byref(got), stream)
    if rc != RSN_OK:
        err = RsnError(rc, lib().rsn_last_error().decode("utf-8", "replace"))
        err.needed = got.value
        raise err
    return got.value


def call_batch_dev(fn, members, stream, *extra):
    """(d_in, n, d_out, out_cap) per member -> the list of out_lens through a batch entry point on device buffers (rsn_*_batch_dev: n,
    members, [extra,] out_lens, stream).  On RSN_ERR_CAPACITY raises RsnError whose .out_lens holds the list: out_lens[i] > out_cap marks
    a member that did not fit, the value is a capacity that suffices; every other member is complete."""
    k = len(members)
    arr = (DevMember * max(k, 1))(*[DevMember(a or None, n, b or None, cap) for a, n, b, cap in members])
    olens = (ctypes.c_size_t * max(k, 1))()
    rc = fn(k, arr, *extra, olens, stream)
    got = [int(olens[i]) for i in range(k)]
    if rc != RSN_OK:
        err = RsnError(rc, lib().rsn_last_error().decode("utf-8", "replace"))
        err.out_lens = got
        raise err
    return got


class Writer:
    """The reference's whole-buffer io.WriteCloser: Write compresses the buffer once with `compress` and returns len(compressed)."""

    def __init__(self, w, compress):
        self.w = w
        self._compress = compress

    def Write(self, data):
        compressed = self._compress(data)
        self.w.write(compressed)
        return len(compressed)

    write = Write

    def Close(self):
        return None

    close = Close


class Reader:
    """The reference's io.Reader: the first Read drains the source and decompresses everything with `decompress`."""

    def __init__(self, r, decompress):
        self.r = r
        self._decompress = decompress
        self.decompressed = None
        self.pos = 0

    def Read(self, size=-1):
        if self.decompressed is None:
            self.decompressed = self._decompress(self.r.read())
        if size is None or size < 0:
            size = len(self.decompressed) - self.pos
        chunk = self.decompressed[self.pos:self.pos + size]
        self.pos += len(chunk)
        return chunk

    read = Read


_hip = None


def hip():
    """The HIP runtime this process's librsn runs on, through ctypes (the SONAME librsn links: already loaded, so this is the same
    library object) -- device memory without torch: the torch-free mode's way to the device-pointer entry points."""
    global _hip
    if _hip is None:
        lib()
        H = ctypes.CDLL("libamdhip64.so.7")
        H.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        H.hipFree.argtypes = [ctypes.c_void_p]
        H.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        H.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
        H.hipRuntimeGetVersion.argtypes = [ctypes.POINTER(ctypes.c_int)]
        _hip = H
    return _hip


def runtime_info():
    """(hipRuntimeGetVersion, path of the libamdhip64 mapped into this process) -- which of the two runtimes librsn is running on."""
    v = ctypes.c_int(0)
    hip().hipRuntimeGetVersion(ctypes.byref(v))
    paths = sorted({ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln})
    return v.value, paths


def dev_codec(fn, data, cap, *extra):
    """bytes -> device buffer -> a device-pointer entry point (`fn`: rsn_*_dev) -> bytes, without torch: hipMalloc / hipMemcpy of the
    runtime librsn runs on.  The general path for inputs the host-buffer entry points would route to the small-input codec."""
    H, L = hip(), lib()
    data = bytes(data)
    n = len(data)
    check(L.rsn_device_set(0))
    d_in, d_out = ctypes.c_void_p(), ctypes.c_void_p()

    def ok(e):
        if e != 0:
            raise RuntimeError("HIP error %d" % e)
    ok(H.hipMalloc(ctypes.byref(d_in), n + 64))
    try:
        ok(H.hipMemset(d_in, 0, n + 64))
        ok(H.hipMemcpy(d_in, data, n, 1))
        for attempt in range(2):
            ok(H.hipMalloc(ctypes.byref(d_out), cap + 64))
            try:
                got = call_dev(fn, d_in, n, d_out, cap, None, *extra)
                buf = ctypes.create_string_buffer(max(got, 1))
                ok(H.hipMemcpy(buf, d_out, got, 2))
                return buf.raw[:got]
            except RsnError as e:
                if e.code != RSN_ERR_CAPACITY or attempt:
                    raise
                cap = e.needed
            finally:
                H.hipFree(d_out)
    finally:
        H.hipFree(d_in)


def prof_enable(on=True):
    lib().rsn_prof_enable(1 if on else 0)


def prof_reset():
    lib().rsn_prof_reset()


def prof_get():
    L = lib()
    arr = (ProfEntry * 64)()
    k = L.rsn_prof_get(arr, 64)
    return {arr[i].name.decode(): (int(arr[i].launches), float(arr[i].total_ms)) for i in range(min(k, 64))}


def prof_copied():
    """(host-to-device, device-to-host) bytes queued on copy commands since prof_reset(), process-wide (rsn_prof_copied)."""
    up, down = ctypes.c_uint64(0), ctypes.c_uint64(0)
    lib().rsn_prof_copied(ctypes.byref(up), ctypes.byref(down))
    return int(up.value), int(down.value)


def dev_tensor(fn, src, out, stream, guess, *extra, retry=True, floor=0):
    """`fn` (rsn_*_dev) over the uint8 CUDA tensor src -> a view of `out` when it was large enough, otherwise (RSN_ERR_CAPACITY: .needed is
    a size that suffices) a view of a fresh tensor of that size, at least `floor` bytes; retry=False raises instead.  Without `out`: a
    tensor of `guess` bytes, or with guess None the size query first (d_out NULL) -- a guess of the expansion would be a buffer of many
    times the input, held by the view returned."""
    import torch
    n = src.numel()
    st = own_stream(src, stream)

    def run(to):
        if to is None:
            return call_dev(fn, src.data_ptr(), n, None, 0, st, *extra)
        return call_dev(fn, src.data_ptr(), n, to.data_ptr(), to.numel(), st, *extra)

    def fresh(size):
        return torch.empty(size, dtype=torch.uint8, device=src.device)

    if out is None and guess is not None:
        out = fresh(guess)
    if out is None:
        try:
            need = run(None)
        except RsnError as e:
            if e.code != RSN_ERR_CAPACITY:
                raise
            need = e.needed
        out = fresh(max(need, 16))
    try:
        got = run(out)
    except RsnError as e:
        if e.code != RSN_ERR_CAPACITY or not retry:
            raise
        out = fresh(max(e.needed, floor))
        got = run(out)
    return out[:got]


def _ru16(x):
    return (x + 15) // 16 * 16


def dev_tensors(fn, srcs, outs, stream, guess, *extra, retry=True):
    """`fn` (rsn_*_batch_dev) over a list of 1-D uint8 CUDA tensors -> a list of tensors trimmed to the result sizes.  Every tensor's
    data_ptr must be 16-byte aligned (slices of one allocation at 16-byte offsets are).  Without `outs` the results are views of ONE
    allocation, member i's slot guess(n_i) bytes; a member whose slot or `out` turns out too small (RSN_ERR_CAPACITY: out_lens[i] is a size
    that suffices) is run once more, alone with the others of its kind, into a fresh allocation -- the way dev_tensor treats a single;
    retry=False raises instead."""
    import torch
    srcs = list(srcs)
    if not srcs:
        return []
    st = own_stream(srcs[0], stream)
    dev = srcs[0].device

    def slots(sizes):
        offs, at = [], 0
        for b in sizes:
            offs.append(at)
            at += _ru16(max(b, 16))
        whole = torch.empty(at, dtype=torch.uint8, device=dev)
        return [whole[o:o + b] for o, b in zip(offs, sizes)]

    def run(which, to):
        return call_batch_dev(fn, [(srcs[i].data_ptr() if srcs[i].numel() else None, srcs[i].numel(),
                                    to[i].data_ptr() if to[i].numel() else None, to[i].numel()) for i in which], st, *extra)

    if outs is None:
        outs = slots([guess(t.numel()) for t in srcs])
    outs = list(outs)
    every = list(range(len(srcs)))
    try:
        got = run(every, outs)
    except RsnError as e:
        if e.code != RSN_ERR_CAPACITY or not retry:
            raise
        got = e.out_lens
        again = [i for i in every if got[i] > outs[i].numel()]
        for i, t in zip(again, slots([got[i] for i in again])):
            outs[i] = t
        for i, v in zip(again, run(again, outs)):
            got[i] = v
    return [outs[i][:got[i]] for i in every]


def own_stream(tensor, stream=None):
    """Orders a librsn call after the work already queued on the tensor's torch
    stream and returns the stream argument for the C ABI.  `stream` must be a
    hipStream_t created by the SAME HIP runtime librsn links (never a torch
    stream handle: PyTorch carries its own runtime copy); None = librsn's own
    per-thread stream."""
    import torch
    torch.cuda.current_stream(tensor.device).synchronize()
    lib().rsn_device_set(tensor.device.index or 0)
    return stream
