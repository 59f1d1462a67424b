"""Mirror of /root/reference/engine (engine.go, util.go) for the codecs on the
accelerated path.  The engine is the CALLER of the hot path: layering, file
I/O, ratio / lossless / entropy reporting stay on the host exactly as the
reference does them; every byte of codec work goes through librsn."""
import io
import math
import os
import time
from dataclasses import dataclass

from . import _lib, huffman, layers as _layers, lz

# engine.go:32 lists 11 engines; the MI355X build carries the two this path names
# (the others -- arithmetic, dmc, mcc, stdlib bindings -- are out of scope).
Engines = ["lzss", "huffman"]
Suites = {"all": list(Engines), "suite": list(Engines)}

# engine.go:48-58 / :101-111
Readers = {"lzss": lz.NewReader, "huffman": huffman.NewReader}
Writers = {"lzss": lz.NewWriter, "huffman": huffman.NewWriter}


class CompressedFile:
    """engine.go:39-45,60-139"""

    def __init__(self, CompressionEngine="", Compressed=b"", MaxSearchBufferLength=4096):
        self.CompressionEngine = CompressionEngine
        self.Compressed = bytes(Compressed)
        self.Decompressed = None
        self.pos = 0
        self.MaxSearchBufferLength = MaxSearchBufferLength  # never read by the reference either (engine.go:445)

    def Write(self, content):
        newWriter = Writers[self.CompressionEngine]        # unknown engine: KeyError (reference: nil type assertion panics)
        b = io.BytesIO()
        w = newWriter(b)
        w.Write(content)                                   # ONE write of the whole buffer (engine.go:133)
        w.Close()
        compressed = b.getvalue()
        self.Compressed += compressed
        return len(compressed)

    def Read(self, size):
        """engine.go:60-98: first call decompresses everything, then serves `size` bytes; returns (chunk, eof)."""
        if self.Decompressed is None:
            r = Readers[self.CompressionEngine](io.BytesIO(self.Compressed))
            self.Decompressed = r.Read(-1)
        chunk = self.Decompressed[self.pos:self.pos + size]
        eof = len(self.Decompressed) - self.pos <= size
        if not eof:
            self.pos += size
        return chunk, eof


def _on_device(algorithms):
    """every layer is one the layered calls carry (rsn_layers_*: the stream stays on the device between the layers)"""
    return all(a in _layers.IDS for a in algorithms)


def compress(content, algorithms):
    """engine.go:443-452: layers applied in order.  Two or more layers of lzss / huffman go through the layered call, in runs of at
    most RSN_LAYERS_MAX."""
    algorithms = list(algorithms)
    if len(algorithms) >= 2 and _on_device(algorithms):
        for i in range(0, len(algorithms), _layers.LAYERS_MAX):
            content = _layers.Compress(content, algorithms[i:i + _layers.LAYERS_MAX])
        return content
    for algorithm in algorithms:
        f = CompressedFile(MaxSearchBufferLength=4096)
        f.CompressionEngine = algorithm
        f.Write(content)
        content = f.Compressed
    return content


def decompress(content, algorithms):
    """engine.go:454-479: layers undone in reverse order, read through a 512-byte buffer (the layered call for two or more layers of
    lzss / huffman, the runs of compress() last to first)."""
    algorithms = list(algorithms)
    if len(algorithms) >= 2 and _on_device(algorithms):
        runs = [algorithms[i:i + _layers.LAYERS_MAX] for i in range(0, len(algorithms), _layers.LAYERS_MAX)]
        for run in reversed(runs):
            content = _layers.Decompress(content, run)
        return content
    for algorithm in reversed(algorithms):
        f = CompressedFile(CompressionEngine=algorithm, Compressed=content)
        while True:
            _, eof = f.Read(512)
            if eof:
                break
        content = f.Decompressed
    return content


def CompressFile(algorithms, path, output):
    """engine.go:157-172"""
    data = open(path, "rb").read()
    print("Compressing...")
    out = compress(data, algorithms)
    open(output, "wb").write(out)
    print("Original bytes: %d" % len(data))
    print("Compressed bytes: %d" % len(out))
    print("Compression ratio: %.2f%%" % (len(out) / len(data) * 100 if data else float("nan")))
    return out


BATCH_BYTES = 4 << 30        # files are read and batched in groups of at most this many bytes: N x 1 GiB inputs never all sit in memory


# one-layer lists that go through a batch call: compress (huffman: rsn_huffman_compress_batch; lzss: rsn_lzss_compress_batch, small files many
# to a launch) and decompress (rsn_lzss_decompress_batch / rsn_huffman_decompress_batch)
_COMPRESS_BATCH = {"huffman": huffman.CompressBatch, "lzss": lambda datas: lz.CompressAsyncBatch(datas, lz.DefaultWindowSize)}
_DECOMPRESS_BATCH = {"huffman": huffman.DecompressBatch, "lzss": lz.DecompressBatch}


def _layered(algorithms, files):
    """a multi-file list under two or more layers, every one lzss or huffman (the CLI's default lzss,huffman): each group of files goes
    through the layers' batch calls in turn"""
    return len(files) > 1 and len(algorithms) > 1 and all(a in _COMPRESS_BATCH for a in algorithms)


def _batch_layers(batches, datas):
    """datas through the batch calls in turn, each layer's outputs the next one's inputs; None when a call fails (the loop's turn)"""
    try:
        for call in batches:
            datas = call(datas)
    except Exception:                                           # noqa: BLE001 -- the loop finds the file that fails, after writing the ones before it
        return None
    return datas


def _groups(files, take_empty):
    """The files in groups of at most BATCH_BYTES, read in order: yields (group, datas, bad) -- bad: files[i] right behind the group is
    empty (when the batch does not take empty files) or cannot be read, and is the per-file loop's to meet, in order, after the group."""
    i = 0
    while i < len(files):
        group, datas, size = [], [], 0
        bad = None
        while i < len(files):
            try:
                fsize = os.path.getsize(files[i])
                if (fsize == 0 and not take_empty) or (group and size + fsize > BATCH_BYTES):
                    bad = files[i] if fsize == 0 and not take_empty else None
                    break
                d = open(files[i], "rb").read()
            except OSError:                                  # (a file that cannot be read ends the group -- the ones before it are
                bad = files[i]                               #  done and written first, as the reference's loop would have, engine.go:150-154)
                break
            group.append(files[i]); datas.append(d); size += len(d); i += 1
        yield group, datas, bad
        if bad is not None:
            i += 1


def CompressFiles(algorithms, files, extension):
    """engine.go:150-154: one .rsn per input, file after file.  Several files under one Huffman or one LZSS layer go through the batch call
    (small files many to a launch; larger Huffman inputs: upload / encode / download overlapped on the device), and under several such
    layers (lzss,huffman) through each layer's batch call in turn, in GROUPS of at most BATCH_BYTES, in
    the loop's order and with the loop's semantics: a file's lines are printed and its .rsn is written before the next group is read, and a
    file the batch cannot take (empty under Huffman: the reference panics in heap.Pop, huffman.go:102) or a group that fails falls back to
    the per-file loop, which stops at the failing file with every earlier .rsn already on disk -- exactly where the reference's loop would stop."""
    files = list(files)
    if _layered(algorithms, files):
        # several layers: the same groups through each layer's batch call in order; an empty file ends a group when a layer is Huffman
        for group, datas, bad in _groups(files, take_empty="huffman" not in algorithms):
            outs = _batch_layers([_COMPRESS_BATCH[a] for a in algorithms], datas) if len(group) > 1 else None
            if outs is None:
                for f in group:
                    CompressFile(algorithms, f, f + extension)
            else:
                for f, data, out in zip(group, datas, outs):
                    print("Compressing...")
                    open(f + extension, "wb").write(out)
                    print("Original bytes: %d" % len(data))
                    print("Compressed bytes: %d" % len(out))
                    print("Compression ratio: %.2f%%" % (len(out) / len(data) * 100 if data else float("nan")))
            if bad is not None:
                CompressFile(algorithms, bad, bad + extension)   # raises like the reference panics; the earlier files are written
        return
    if len(files) > 1 and list(algorithms) == ["lzss"]:
        for group, datas, bad in _groups(files, take_empty=True):
            outs = None
            if len(group) > 1:
                try:
                    outs = _COMPRESS_BATCH["lzss"](datas)
                except Exception:                               # noqa: BLE001 -- the loop finds the file that fails, after writing the ones before it
                    outs = None
            if outs is None:
                for f in group:
                    CompressFile(algorithms, f, f + extension)
            else:
                for f, data, out in zip(group, datas, outs):
                    print("Compressing...")
                    open(f + extension, "wb").write(out)
                    print("Original bytes: %d" % len(data))
                    print("Compressed bytes: %d" % len(out))
                    print("Compression ratio: %.2f%%" % (len(out) / len(data) * 100 if data else float("nan")))
            if bad is not None:
                CompressFile(algorithms, bad, bad + extension)   # raises like the reference panics; the earlier files are written
        return
    if len(files) > 1 and list(algorithms) == ["huffman"]:
        i = 0
        while i < len(files):
            group, datas, size = [], [], 0
            bad = False                                          # files[i] is empty, missing or unreadable: the per-file call below meets it in order
            while i < len(files):
                try:
                    fsize = os.path.getsize(files[i])
                    if fsize == 0 or (group and size + fsize > BATCH_BYTES):
                        bad = fsize == 0
                        break
                    d = open(files[i], "rb").read()
                except OSError:                                  # (a file that cannot be read ends the group -- the ones before it are
                    bad = True                                   #  compressed and written first, as the reference's loop would have, engine.go:150-154)
                    break
                group.append(files[i]); datas.append(d); size += len(d); i += 1
            outs = None
            if len(group) > 1:
                try:
                    outs = huffman.CompressBatch(datas)
                except Exception:                               # noqa: BLE001 -- the loop finds the file that fails, after writing the ones before it
                    outs = None
            if outs is None:
                for f in group:
                    CompressFile(algorithms, f, f + extension)
            else:
                for f, data, out in zip(group, datas, outs):
                    print("Compressing...")
                    open(f + extension, "wb").write(out)
                    print("Original bytes: %d" % len(data))
                    print("Compressed bytes: %d" % len(out))
                    print("Compression ratio: %.2f%%" % (len(out) / len(data) * 100 if data else float("nan")))
            if bad:
                CompressFile(algorithms, files[i], files[i] + extension)   # raises like the reference panics; the earlier files are written
                i += 1
        return
    for f in files:
        CompressFile(algorithms, f, f + extension)


def DecompressFile(algorithms, path, output):
    """engine.go:187-199"""
    data = open(path, "rb").read()
    print("Decompressing...")
    out = decompress(data, algorithms)
    with open(output, "wb") as fh:                                 # check(err) after WriteFile (engine.go:196-197): raises before any caller deletes the input
        fh.write(out)
    return out


def DecompressFiles(algorithms, files, extension):
    """engine.go:175-185: file after file.  Several files under ONE layer (lzss or huffman) go through that codec's batch call (under several
    such layers: each layer's, the last layer first) in groups of
    at most BATCH_BYTES, with the loop's semantics: outputs in order, a group written before the next is read, and a group that fails is
    done again by the loop, which stops at the failing file with everything before it written and nothing after it."""
    files = list(files)

    def out_path(f):
        path = f + extension
        if extension.strip() in ("", "."):
            path = os.path.splitext(f)[0]
        return path

    algorithms = list(algorithms)
    if _layered(algorithms, files):
        # several layers: each group through the layers' batch calls, the last layer first
        for group, datas, bad in _groups(files, take_empty="huffman" not in algorithms):
            outs = _batch_layers([_DECOMPRESS_BATCH[a] for a in reversed(algorithms)], datas) if len(group) > 1 else None
            if outs is None:
                for f in group:
                    DecompressFile(algorithms, f, out_path(f))
            else:
                for f, out in zip(group, outs):
                    print("Decompressing...")
                    with open(out_path(f), "wb") as fh:
                        fh.write(out)
            if bad is not None:
                DecompressFile(algorithms, bad, out_path(bad))   # raises where the loop would
        return
    if len(files) > 1 and len(algorithms) == 1 and algorithms[0] in _DECOMPRESS_BATCH:
        for group, datas, bad in _groups(files, take_empty=True):
            outs = None
            if len(group) > 1:
                try:
                    outs = _DECOMPRESS_BATCH[algorithms[0]](datas)
                except Exception:                               # noqa: BLE001 -- the loop finds the file that fails, after writing the ones before it
                    outs = None
            if outs is None:
                for f in group:
                    DecompressFile(algorithms, f, out_path(f))
            else:
                for f, out in zip(group, outs):
                    print("Decompressing...")
                    with open(out_path(f), "wb") as fh:
                        fh.write(out)
            if bad is not None:
                DecompressFile(algorithms, bad, out_path(bad))   # raises where the loop would
        return
    for f in files:
        DecompressFile(algorithms, f, out_path(f))


@dataclass
class Result:
    """engine.go:201-209"""
    CompressionEngine: str
    TimeTaken: str
    Ratio: float
    ActualEntropy: float
    Entropy: float
    Lossless: bool
    Failed: bool


def _entropy(counts, total):
    """goent discrete.Entropy(p, math.Log): -sum p ln p (natural log, engine.go:410)."""
    h = 0.0
    for c in counts:
        if c:
            p = c / total
            h -= p * math.log(p)
    return h


def _byte_counts(b):
    import numpy as np
    return np.bincount(np.frombuffer(b, dtype=np.uint8), minlength=256).tolist() if b else []


def BenchmarkFile(algorithms, fileString, PrintStats=False):
    """engine.go:357-441: ONE timer around compress+decompress, ratio%, lossless by
    byte equality, and the entropy columns -- including the quirk at :412-423 that
    the 'compressed' entropy is computed over the DECOMPRESSED bytes divided by the
    compressed length."""
    data = open(fileString, "rb").read()
    name = ",".join(algorithms)
    algorithms = list(algorithms)
    if 1 <= len(algorithms) <= _layers.LAYERS_MAX and _on_device(algorithms):
        # one call: upload once, both directions, the comparison and both byte counts on the device; the entropies from the 256 counts here
        start = time.perf_counter()
        rt, _ = _layers.RoundTrip(data, algorithms)
        dur = time.perf_counter() - start
        n_compressed, n_decompressed, lossless = int(rt.compressed_n), int(rt.decompressed_n), bool(rt.lossless)
        entropy = _entropy(list(rt.hist_original), len(data)) if data else 0.0
        actual = _entropy(list(rt.hist_decompressed), n_compressed) if n_compressed else 0.0
    else:
        entropy = _entropy(_byte_counts(data), len(data)) if data else 0.0
        start = time.perf_counter()
        compressed = compress(data, algorithms)
        decompressed = decompress(compressed, algorithms)
        dur = time.perf_counter() - start
        lossless = decompressed == data
        n_compressed, n_decompressed = len(compressed), len(decompressed)
        actual = _entropy(_byte_counts(decompressed), n_compressed) if compressed else 0.0
    ratio = n_compressed / len(data) * 100 if data else float("nan")
    res = Result(name, _time_taken(dur), ratio, actual, entropy, lossless, False)
    if PrintStats:
        print("Lossless: %s" % str(lossless).lower())
        print("Original bytes: %d" % len(data))
        print("Compressed bytes: %d" % n_compressed)
        if not lossless:
            print("Decompressed bytes: %d" % n_decompressed)
        print("Compression ratio: %.2f%%" % ratio)
        print("Time taken: %s" % res.TimeTaken)
    return res


def AsyncBenchmarkFile(algorithms, fileString):
    """engine.go:310-355: a panic in a codec becomes a 'failed' row."""
    try:
        return BenchmarkFile(algorithms, fileString)
    except Exception:  # noqa: BLE001 -- mirrors recover()
        return Result(",".join(algorithms), "failed", 0.0, 0.0, 0.0, False, True)


def BenchmarkFiles(algorithms, files):
    """The benchmark loop for ONE layer list over many files (ai/helpers/compressor.py:89-108 over engine.BenchmarkFile): one Result per
    file, in order, with BenchmarkFile's Ratio, Entropy, ActualEntropy (the quirk included, from the same counts) and Lossless.  The files
    are taken in groups of at most BATCH_BYTES; a group of two or more files under layers that are all on the device is ONE call
    (layers.RoundTripBatch: compressed, undone, compared and counted on the device, only the answers come down).  There is one timer around
    a group's call: TimeTaken is that wall time divided by the group's file count.  A group whose call fails in the library -- one empty
    file under Huffman -- is done again file by file through AsyncBenchmarkFile, so that file becomes a `failed` row and the others get
    theirs; anything else that is raised is the caller's to see."""
    algorithms, files = list(algorithms), list(files)
    name = ",".join(algorithms)
    batched = 1 <= len(algorithms) <= _layers.LAYERS_MAX and _on_device(algorithms)
    results = []
    for group, datas, bad in _groups(files, take_empty=True):
        rows = None
        if batched and len(group) > 1:
            try:
                start = time.perf_counter()
                rows = _layers.RoundTripBatch(datas, algorithms)
                dur = (time.perf_counter() - start) / len(group)
            except _lib.RsnError:                               # a member's failure ends the call: the per-file loop finds the file
                rows = None
        if rows is None:
            results.extend(AsyncBenchmarkFile(algorithms, f) for f in group)
        else:
            for data, rt in zip(datas, rows):
                entropy = _entropy(rt.hist_original, len(data)) if data else 0.0
                actual = _entropy(rt.hist_decompressed, rt.compressed_n) if rt.compressed_n else 0.0
                ratio = rt.compressed_n / len(data) * 100 if data else float("nan")
                results.append(Result(name, _time_taken(dur), ratio, actual, entropy, rt.lossless, False))
        if bad is not None:
            results.append(AsyncBenchmarkFile(algorithms, bad))  # a file that cannot be read: a failed row, in order
    return results


def _best_result(results):
    """ai/helpers/files.py:67-78 (best="ratio"): the first result unless a later one's Ratio is strictly smaller, `Lossless` not looked at;
    the reference's loop never appends a result that raised (compressor.py:96-100), so `failed` rows do not take part.  None without one."""
    best = None
    for r in results:
        if not r.Failed and (best is None or r.Ratio < best.Ratio):
            best = r
    return best


def BenchmarkFilesSuite(files, algorithms):
    """The benchmark loop of files x layer lists (benchmark_files, ai/helpers/compressor.py:89-108, with best_result of files.py:67-78):
    returns, per file in order, (the list of Results in the order of `algorithms`, the best of them).  BenchmarkFiles' groups (_groups,
    BATCH_BYTES) and its Ratio / Entropy / ActualEntropy arithmetic, the quirk included; a group of two or more files goes through ONE call
    for all the lists that are on the device (layers.SuiteBatch: every shared prefix compressed once, the files uploaded and their bytes
    counted once), with one timer around it: TimeTaken is that wall time divided by the group's file count and by the lists the call ran.
    A list that is not on the device, and a list the call reports as failed -- an empty file under Huffman --, goes file by file through
    AsyncBenchmarkFile, as does everything when the call as a whole fails; so do the lists behind the first RSN_SUITE_LISTS_MAX that are
    on the device.  A layer name that neither the layered calls nor the engine's writers know raises ValueError."""
    files = list(files)
    algorithms = [list(a) for a in algorithms]
    names = [",".join(a) for a in algorithms]
    _layers.ids([x for a in algorithms for x in a if x not in Writers])   # a name nobody knows: ValueError, before a file is read
    on_device = [l for l, a in enumerate(algorithms) if 1 <= len(a) <= _layers.LAYERS_MAX and _on_device(a)][:_layers.SUITE_LISTS_MAX]
    out = []
    for group, datas, bad in _groups(files, take_empty=True):
        rows, errors = None, None
        if on_device and len(group) > 1:
            try:
                start = time.perf_counter()
                rows, _, errors = _layers.SuiteBatch(datas, [algorithms[l] for l in on_device])
                dur = (time.perf_counter() - start) / len(group) / max(1, sum(e is None for e in errors))
            except _lib.RsnError:
                rows = None
        slot = {l: k for k, l in enumerate(on_device)} if rows is not None else {}
        for i, (f, data) in enumerate(zip(group, datas)):
            results = []
            for l, a in enumerate(algorithms):
                k = slot.get(l)
                if k is None or errors[k] is not None:
                    results.append(AsyncBenchmarkFile(a, f))
                    continue
                rt = rows[k][i]
                entropy = _entropy(rt.hist_original, len(data)) if data else 0.0
                actual = _entropy(rt.hist_decompressed, rt.compressed_n) if rt.compressed_n else 0.0
                ratio = rt.compressed_n / len(data) * 100 if data else float("nan")
                results.append(Result(names[l], _time_taken(dur), ratio, actual, entropy, rt.lossless, False))
            out.append((results, _best_result(results)))
        if bad is not None:
            results = [AsyncBenchmarkFile(a, bad) for a in algorithms]  # a file that cannot be read: failed rows, in order
            out.append((results, _best_result(results)))
    return out


def _suite_order(results):
    """engine.go:266-276: lossless rows before lossy ones, each group by ascending ratio."""
    return sorted(results, key=lambda r: (not r.Lossless, r.Ratio))


BenchmarkTimeout = 60.0   # engine.go:216 `timeout := 1 * time.Minute`


def _go_duration_ns(ns):
    """time.Duration.String() (Go's published format: the largest unit that leaves a non-zero integer part below a
    second -- "190µs", "1.23ms" --, "XhYmZ.ZZZs" from a second up, fractions without trailing zeros, "0s" for zero)."""
    if ns == 0:
        return "0s"
    sign, u = ("-", -ns) if ns < 0 else ("", ns)

    def frac(v, prec):                       # fmtFrac: v / 10^prec, and the fraction's digits without trailing zeros
        q, r = divmod(v, 10 ** prec)
        digits = ("%0*d" % (prec, r)).rstrip("0") if prec else ""
        return q, ("." + digits) if digits else ""

    if u < 1000000000:
        if u < 1000:
            return "%s%dns" % (sign, u)
        prec, unit = (3, "\u00b5s") if u < 1000000 else (6, "ms")
        q, f = frac(u, prec)
        return "%s%d%s%s" % (sign, q, f, unit)
    sec, f = frac(u, 9)
    out = "%d%ss" % (sec % 60, f)
    mins = sec // 60
    if mins > 0:
        out = "%dm" % (mins % 60) + out
        if mins // 60 > 0:
            out = "%dh" % (mins // 60) + out
    return sign + out


def _go_round_ns(ns, m):
    """time.Duration.Round(m): to the nearest multiple of m, halfway values away from zero."""
    if m <= 0:
        return ns
    r = abs(ns) % m
    v = abs(ns) - r if r + r < m else abs(ns) + m - r
    return -v if ns < 0 else v


def _go_duration(seconds):
    """time.Duration.String() of a duration given in seconds (the timeout row, engine.go:258: ">1m0s")."""
    return _go_duration_ns(int(round(seconds * 1e9)))


def _time_taken(seconds):
    """engine.go:425: duration.Round(10*time.Microsecond).String() -- "190µs", "4.61s"."""
    return _go_duration_ns(_go_round_ns(int(round(seconds * 1e9)), 10000))


def BenchmarkSuite(files, algorithms, out=None, timeout=None):
    """engine.go:213-309 without the HTML report.  As in the reference, every algorithm entry of a
    file runs CONCURRENTLY on its own thread (one goroutine each, :235-244; librsn keeps one device
    context per calling thread), the suite waits at most `timeout` (1 minute, :216,246, util.go:15)
    and every entry that has not delivered by then gets a ">1m0s" DNF row (:256-263) while its
    thread is left running.  Per file one table: header, finished rows in the reference's order,
    failed rows as DNF, the File/Size footer.  Returns the flat list of results.
    An entry that misses the deadline keeps running on its daemon thread -- like the reference's goroutine -- so it goes on
    using the device (and holds its thread's scratch arena) while the next file is timed."""
    import sys
    import threading
    out = out or sys.stdout
    timeout = BenchmarkTimeout if timeout is None else timeout
    all_results = []
    for i, f in enumerate(files):
        print("Compressing file %d/%d - %s" % (i + 1, len(files), f), file=out)
        file_size = os.path.getsize(f)                          # ioutil.ReadFile + check(err) before anything starts (:223-225)
        slots, threads = {}, []
        for layer in algorithms:
            name = ",".join(layer)
            print("Benchmarking", name, file=out)
            box = []
            slots[name] = box                                   # resultChans[algorithmsString] (:240): a repeated entry shares its slot
            t = threading.Thread(target=lambda layer=layer, box=box, f=f: box.append(AsyncBenchmarkFile(layer, f)), daemon=True)
            t.start()
            threads.append(t)
        deadline = time.monotonic() + timeout                   # waitTimeout(&wg, timeout)
        for t in threads:
            t.join(max(0.0, deadline - time.monotonic()))
        done, failed = [], []
        for name, box in slots.items():
            if box:
                r = box[0]
                (failed if r.Failed else done).append(r)
            else:                                               # select default: nothing delivered in time
                failed.append(Result(name, ">" + _go_duration(timeout), 0.0, 0.0, 0.0, False, True))
        rows = [("engine", "time taken", "compression ratio", "actual entropy", "theoretical entropy", "lossless")]
        for r in _suite_order(done):
            rows.append((r.CompressionEngine, r.TimeTaken, "%.2f%%" % r.Ratio, "%.2f" % r.ActualEntropy, "%.2f" % r.Entropy, str(r.Lossless).lower()))
            all_results.append(r)
        for r in failed:
            rows.append((r.CompressionEngine, r.TimeTaken, "DNF", "DNF", "DNF", str(r.Lossless).lower()))
            all_results.append(r)
        rows.append(("File", f, "Size", ByteCountSI(file_size), "", ""))
        width = [max(len(row[c]) for row in rows) for c in range(6)]
        for row in rows:
            print(" | ".join(cell.ljust(w) for cell, w in zip(row, width)).rstrip(), file=out)
    return all_results


def parseAlgorithms(s):
    """cmd/cli.go:203-231: "a,[b,c]" -> [[a],[b,c]]"""
    algorithms, buf, layer, in_layer = [], "", [], False
    for ch in s:
        if ch == ",":
            if in_layer and buf:
                layer.append(buf)
            elif buf:
                algorithms.append([buf])
            buf = ""
        elif ch == "[":
            in_layer = True
        elif ch == "]":
            layer.append(buf)
            buf = ""
            in_layer = False
            algorithms.append(layer)
            layer = []
        else:
            buf += ch
    if buf:
        algorithms.append([buf])
    return algorithms


def ByteCountSI(b):
    """engine/util.go:30-42"""
    unit = 1000
    if b < unit:
        return "%d B" % b
    div, exp = unit, 0
    n = b // unit
    while n >= unit:
        div *= unit
        exp += 1
        n //= unit
    return "%.1f %cB" % (b / div, "kMGTPE"[exp])
