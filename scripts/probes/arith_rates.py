"""Rates of the arithmetic codec (README): the batch calls against a loop of single calls, one stream's encode and
decode rate at several sizes, and the longest a hostile stream can hold the decoder.  Nothing here is gated; the size limit of one
member (RSN_ARITH_MAX_BYTES) is derived from the single-stream figures this writes.

    python scripts/probes/arith_rates.py [out_file]          (default profiles/arith_rates.txt)

Host wall clock around calls that synchronise before they return; a warm-up of every shape, then the median of the repeats.  The
kernel columns are the library's own launch profile (rsn_prof_*: device events around every launch), taken in a pass of their own."""
import os
import platform
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from raisin_amd import RsnError, _lib, arithmetic as A  # noqa: E402


def text(n, seed):
    rng = np.random.default_rng(seed)
    return rng.choice(np.frombuffer(b"eeeeeeeetttttaaaaoooiinnsshhrrdlu \n", dtype=np.uint8), size=n).tobytes()


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts), min(ts)


def kernel_ms(fn, names):
    _lib.prof_enable(True)
    _lib.prof_reset()
    fn()
    got = _lib.prof_get()
    _lib.prof_enable(False)
    return sum(ms for k, (_, ms) in got.items() if k in names), sum(n for k, (n, _) in got.items() if k in names)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "arith_rates.txt")
    import torch
    _lib.check(_lib.lib().rsn_device_set(0))
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say("arithmetic codec rates -- %s, host %s, %s" % (torch.cuda.get_device_name(0), platform.node(), time.strftime("%Y-%m-%d")))
    say("HIP runtime %s; host wall clock around synchronising calls, median (min) of the repeats after a warm-up" % (_lib.runtime_info()[0],))
    say()
    say("batch of 4096 members against a loop of 4096 single calls")
    say("%-10s %-10s %14s %14s %8s" % ("member", "direction", "batch ms", "loop ms", "ratio"))
    for size in (13, 25, 1024):
        files = [text(size, 1000 * size + i) for i in range(4096)]
        streams = A.CompressBatch(files)
        assert A.DecompressBatch(streams) == files
        for name, batch, single, items in (("compress", A.CompressBatch, A.Compress, files), ("decompress", A.DecompressBatch, A.Decompress, streams)):
            b_med, b_min = timed(lambda: batch(items), 7, 2)
            l_med, l_min = timed(lambda: [single(x) for x in items], 3, 1)
            say("%-10s %-10s %7.2f (%5.2f) %7.1f (%5.1f) %7.0fx" % ("%d B" % size, name, b_med * 1e3, b_min * 1e3, l_med * 1e3, l_min * 1e3, l_med / b_med))
    say()
    say("one stream (one wavefront): call = host call with its copies; kernels = device time of k_arith_enc (+ k_arith_pack) / k_arith_dec")
    say("%-12s %-10s %10s %10s %12s %10s %9s" % ("input", "direction", "call ms", "MB/s", "kernels ms", "MB/s", "launches"))
    for label, n in (("16000 B *", 16000), ("64 KiB", 64 << 10), ("1 MiB", 1 << 20), ("16 MiB", 16 << 20)):
        data = text(n, n)
        enc = A.Compress(data)
        assert A.Decompress(enc) == data
        reps = 3 if n >= (1 << 20) else 7
        for name, fn, names in (("compress", lambda: A.Compress(data), ("k_arith_enc", "k_arith_pack")), ("decompress", lambda: A.Decompress(enc), ("k_arith_dec",))):
            med, mn = timed(fn, reps, 1)
            k_ms, k_n = kernel_ms(fn, names)
            say("%-12s %-10s %10.2f %10.2f %12.2f %10.2f %9d" % (label, name, med * 1e3, n / med / 1e6, k_ms, n / (k_ms / 1e3) / 1e6 if k_ms else 0.0, k_n))
    say("* never reaches the freeze (16126 updates): the loop with the table update; the larger sizes run frozen for all but their first 16126 symbols")
    say("  (MB = 10^6 bytes of the ORIGINAL, in both directions; the text compresses to %.1f %%)" % (100.0 * len(enc) / len(data)))
    say()
    say("the worst a hostile stream does per byte: a frozen table with one dominant symbol, then zeros -- refused by the tail rule, or by the size limit when it decodes that far")
    for n_zero, reps, warm in ((4000, 5, 1), (1 << 20, 1, 0)):
        good = A.Compress(bytes(20000))
        bad = good[:-40] + bytes(n_zero)

        code = [None]

        def refuse():
            try:
                A.Decompress(bad)
            except RsnError as e:
                assert e.code in (-3, -6), e
                code[0] = "tail rule" if e.code == -3 else "size limit"
                return
            raise AssertionError("a stream of zeros decoded")
        med, mn = timed(refuse, reps, warm)
        say("%8d zero bytes behind a frozen table of zeros: refused (%s) after %.2f ms (min %.2f)" % (n_zero, code[0], med * 1e3, mn * 1e3))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
