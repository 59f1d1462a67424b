"""The batch calls against a loop of single calls on many SMALL members, host buffer to host buffer.

For K in {16, 256, 4096} members: LZSS compress and decompress of the reference README's 13-byte and 25-byte files and of 1 KiB of text,
Huffman compress of those and of 16 KiB of text, Huffman decompress of those and of 64 KiB of text, and the CLI's default two layers
(lzss,huffman: the two batch calls one after the other against a loop of two single calls per member).  Every time is the median of REPS
runs of the whole list; both sides go through ctypes the same way.  `--single` first prints the single calls' own times per call (the
small-input paths the batch shares its kernels with).  `--only` runs the rows whose call name contains one of its comma-separated words.

`--mid` runs the rows of the mid-size LZSS class instead (csrc/lzss_mid.hip): LZSS compress and decompress of 4, 16 and 64 KiB of text and
lzss,huffman of 4 and 16 KiB, for K in {2, 4, 16, 64, 256, 4096} (64 KiB: 1024 in place of 4096 -- result blocks of 256 MiB are a host
cost of their own); with `--single` also the single calls at those sizes.  `--parent LIB` first runs the same rows in a child process on
another build of the library (RSN_LIB_PATH: the parent commit's), so that one job on one box gives the three legs the cutoffs rest on:
the parent's batch call and loop, this build's loop, this build's batch call.
`--huff-mid` runs the rows of the mid-size Huffman class (csrc/huff_mid.hip) the same way: Huffman compress and decompress of 20, 32 and
64 KiB of text and lzss,huffman of 64 KiB, for K in {2, 4, 16, 64, 256} and 1024 at 64 KiB; with `--single` also the single calls.
Usage: python scripts/batch_small_bench.py [--single] [--mid | --huff-mid] [--parent LIB] [--reps R] [--k 16,256,4096] [--only huffman compress,lzss,huffman]"""
import argparse
import ctypes
import os
import random
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raisin_amd import _lib, huffman, lz  # noqa: E402

README = [b"Hello world!\n", b"abcabcabcabcabcabcabcabc\n"]
WORDS = [b"the", b"quick", b"brown", b"fox", b"jumps", b"over", b"lazy", b"dog", b"compression", b"a", b"I", b"Sam", b"ham"]


def text(seed, n):
    rng = random.Random(seed)
    t = bytearray()
    while len(t) < n:
        t += rng.choice(WORDS) + rng.choice([b" ", b"\n", b", ", b". "])
    return bytes(t[:n])


def members(kind, k):
    if kind == "13B":
        return [README[0]] * k
    if kind == "25B":
        return [README[1]] * k
    distinct = [text(i, {"1KiB": 1024, "4KiB": 4 << 10, "16KiB": 16 << 10, "20KiB": 20 << 10, "32KiB": 32 << 10, "64KiB": 64 << 10}[kind]) for i in range(min(k, 64))]
    return [distinct[i % len(distinct)] for i in range(k)]


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def batch_fn(L, name, bufs, extra):
    k = len(bufs)
    ins = (ctypes.c_char_p * k)(*bufs)
    lens = (ctypes.c_size_t * k)(*[len(b) for b in bufs])
    outs = (ctypes.POINTER(ctypes.c_uint8) * k)()
    olens = (ctypes.c_size_t * k)()
    fn = getattr(L, name)

    def run():
        _lib.check(fn(k, ins, lens, *extra, outs, olens))
        for i in range(k):
            L.rsn_free(outs[i])
    return run


def loop_fn(L, name, bufs, extra):
    fn = getattr(L, name)
    out, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t()
    lens = [len(b) for b in bufs]

    def run():
        for b, m in zip(bufs, lens):
            _lib.check(fn(b, m, *extra, ctypes.byref(out), ctypes.byref(n)))
            L.rsn_free(out)
    return run


def layered_fns(L, bufs):
    """lzss,huffman: both batch calls in turn / both single calls per member"""
    def batch():
        k = len(bufs)
        mid = _lib.call_batch(L.rsn_lzss_compress_batch, bufs, 4096)
        outs = _lib.call_batch(L.rsn_huffman_compress_batch, mid)
        assert len(outs) == k

    def loop():
        for b in bufs:
            huffman.Compress(lz.CompressAsync(b, False, 4096))
    return batch, loop


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--single", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", default="16,256,4096")
    ap.add_argument("--only", default="")
    ap.add_argument("--mid", action="store_true")
    ap.add_argument("--huff-mid", action="store_true")
    ap.add_argument("--parent", default="")
    a = ap.parse_args()
    only = [w for w in a.only.split(",") if w]
    if a.parent:                                                          # the same rows on another build, in a process of its own
        argv = [x for i, x in enumerate(sys.argv[1:]) if x != "--parent" and (i == 0 or sys.argv[i] != "--parent")]
        sys.stdout.flush()
        subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, check=True, env=dict(os.environ, RSN_LIB_PATH=os.path.abspath(a.parent)))
    L = _lib.lib()
    print("library: %s" % os.path.basename(_lib.LIB_PATH))
    if a.single:
        print("single calls, median of %d x 200 calls, us per call:" % a.reps)
        cases = [("lzss compress", "rsn_lzss_compress", README[0], (4096,)), ("lzss compress", "rsn_lzss_compress", README[1], (4096,)),
                 ("lzss compress", "rsn_lzss_compress", text(0, 1024), (4096,)),
                 ("lzss decompress", "rsn_lzss_decompress", lz.CompressAsync(README[0]), ()),
                 ("lzss decompress", "rsn_lzss_decompress", lz.CompressAsync(README[1]), ()),
                 ("lzss decompress", "rsn_lzss_decompress", lz.CompressAsync(text(0, 1024)), ()),
                 ("huffman compress", "rsn_huffman_compress", README[0], ()), ("huffman compress", "rsn_huffman_compress", README[1], ()),
                 ("huffman compress", "rsn_huffman_compress", text(0, 1024), ()), ("huffman compress", "rsn_huffman_compress", text(0, 64 << 10), ()),
                 ("huffman decompress", "rsn_huffman_decompress", huffman.Compress(text(0, 16 << 10)), ()),
                 ("huffman decompress", "rsn_huffman_decompress", huffman.Compress(text(0, 64 << 10)), ())]
        if a.mid:
            cases = [("lzss compress", "rsn_lzss_compress", text(0, n << 10), (4096,)) for n in (4, 16, 64)]
            cases += [("lzss decompress", "rsn_lzss_decompress", lz.CompressAsync(text(0, n << 10)), ()) for n in (4, 16, 64)]
        if a.huff_mid:
            cases = [("huffman compress", "rsn_huffman_compress", text(0, n << 10), ()) for n in (20, 32, 64)]
            cases += [("huffman decompress", "rsn_huffman_decompress", huffman.Compress(text(0, n << 10)), ()) for n in (20, 32, 64)]
        for label, name, data, extra in cases:
            run = loop_fn(L, name, [data] * 200, extra)
            run()
            print("  %-20s %6d B in: %7.1f us" % (label, len(data), timed(run, a.reps) / 200 * 1e6))
    print("%-20s %6s %5s %10s %10s %8s" % ("call", "member", "K", "batch ms", "loop ms", "loop/batch"))
    plan = [("lzss compress", "rsn_lzss_compress_batch", "rsn_lzss_compress", ("13B", "25B", "1KiB"), (4096,)),
            ("lzss decompress", "rsn_lzss_decompress_batch", "rsn_lzss_decompress", ("13B", "25B", "1KiB"), ()),
            ("huffman decompress", "rsn_huffman_decompress_batch", "rsn_huffman_decompress", ("13B", "25B", "1KiB", "16KiB", "64KiB"), ()),
            ("huffman compress", "rsn_huffman_compress_batch", "rsn_huffman_compress", ("13B", "25B", "1KiB", "16KiB"), ()),
            ("lzss,huffman", None, None, ("13B", "25B", "1KiB"), ())]
    ks = [int(x) for x in a.k.split(",")]
    if a.mid:
        plan = [("lzss compress", "rsn_lzss_compress_batch", "rsn_lzss_compress", ("4KiB", "16KiB", "64KiB"), (4096,)),
                ("lzss decompress", "rsn_lzss_decompress_batch", "rsn_lzss_decompress", ("4KiB", "16KiB", "64KiB"), ()),
                ("lzss,huffman", None, None, ("4KiB", "16KiB"), ())]
        if a.k == ap.get_default("k"):
            ks = [2, 4, 16, 64, 256, 4096]
    if a.huff_mid:
        plan = [("huffman compress", "rsn_huffman_compress_batch", "rsn_huffman_compress", ("20KiB", "32KiB", "64KiB"), ()),
                ("huffman decompress", "rsn_huffman_decompress_batch", "rsn_huffman_decompress", ("20KiB", "32KiB", "64KiB"), ()),
                ("lzss,huffman", None, None, ("64KiB",), ())]
        if a.k == ap.get_default("k"):
            ks = [2, 4, 16, 64, 256, 1024]
    for label, bname, sname, kinds, extra in plan:
        if only and not any(w == label or w in label.replace(",", " ").split() for w in only):
            continue
        for kind in kinds:
            for k in ks:
                if kind == "64KiB" and k > 1024:
                    k = 1024
                if a.huff_mid and kind != "64KiB" and k > 256:
                    continue
                src = members(kind, k)
                if label == "lzss decompress":
                    bufs = lz.CompressAsyncBatch(src)
                elif label == "huffman decompress":
                    bufs = [huffman.Compress(s) for s in src]
                else:
                    bufs = src
                if bname is None:
                    b, lp = layered_fns(L, bufs)
                else:
                    b, lp = batch_fn(L, bname, bufs, extra), loop_fn(L, sname, bufs, extra)
                b(), lp()
                tb, tl = timed(b, a.reps), timed(lp, a.reps)
                print("%-20s %6s %5d %10.3f %10.3f %8.1fx" % (label, kind, k, tb * 1e3, tl * 1e3, tl / tb), flush=True)


if __name__ == "__main__":
    main()
