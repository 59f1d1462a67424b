"""Rates of the batch suite (README): the standard suite {[huffman], [lzss], [lzss, huffman]} over the same members, one job on
one box, two ways in the same process:

    (loop)  three calls of rsn_layers_roundtrip_batch in turn, one per list      the route before: unchanged by the suite
    (suite) one call of rsn_layers_suite_batch                                     members up once, originals counted once, LZSS encoded once

each in the host form and in the device form (the members already on the device: rsn_layers_roundtrip_batch_dev against
rsn_layers_suite_batch_dev).

    timeout -k 10 900 python scripts/probes/suite_batch_rates.py [out_file]     (default profiles/suite_batch_rates.txt)

Host wall clock around calls that synchronise before they return; every leg is warmed up once, then five repeats: the median with the
least and the greatest beside it.  All legs go through ctypes with their argument arrays built beforehand.  The suite's rows and
histograms are compared with the loop's once.  No threshold: the last column says whether the suite's median is below the loop's FASTEST
repeat, and the exit status is 0 either way."""
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from batch_dev_rates import Packed, five, text  # noqa: E402
from raisin_amd import _lib, layers  # noqa: E402

LISTS = [["huffman"], ["lzss"], ["lzss", "huffman"]]


def legs(datas):
    """-> (loop host, suite host, loop dev, suite dev), each (median, min, max) in ms"""
    L = _lib.lib()
    n, k = len(datas), len(LISTS)
    keep = [layers.ids(a) for a in LISTS]
    arr = (_lib.LayerList * k)(*[_lib.LayerList(ctypes.cast(a, ctypes.POINTER(ctypes.c_int)), c) for a, c in keep])
    ins = (ctypes.c_char_p * n)(*datas)
    lens = (ctypes.c_size_t * n)(*[len(d) for d in datas])
    p = Packed(datas, [0] * n)
    mem = (_lib.DevMember * n)(*[_lib.DevMember(m[0], m[1], None, 0) for m in p.members])
    u32p = ctypes.POINTER(ctypes.c_uint32)
    res1 = (_lib.RoundTripMember * (k * n))()
    counts1 = np.zeros(512 * k * n, dtype=np.uint32)
    res = (_lib.RoundTripMember * (k * n))()
    codes = (ctypes.c_int * k)()
    best = np.zeros(n, dtype=np.uint32)
    ho, hd = np.zeros(256 * n, dtype=np.uint32), np.zeros(256 * k * n, dtype=np.uint32)

    def loop(dev):
        for l, (a, c) in enumerate(keep):
            r = ctypes.cast(ctypes.addressof(res1) + l * n * ctypes.sizeof(_lib.RoundTripMember), ctypes.POINTER(_lib.RoundTripMember))
            h = counts1[512 * l * n:].ctypes.data_as(u32p)
            rc = L.rsn_layers_roundtrip_batch_dev(n, mem, a, c, r, h, None) if dev else L.rsn_layers_roundtrip_batch(n, ins, lens, a, c, r, h)
            assert rc == 0, L.rsn_last_error()

    def suite(dev):
        tail = (k, arr, res, codes, ho.ctypes.data_as(u32p), hd.ctypes.data_as(u32p), best.ctypes.data_as(u32p))
        rc = L.rsn_layers_suite_batch_dev(n, mem, *tail, None) if dev else L.rsn_layers_suite_batch(n, ins, lens, *tail)
        assert rc == 0, L.rsn_last_error()

    def same():
        for j in range(k * n):
            a, b = res1[j], res[j]
            assert (a.original_n, a.compressed_n, a.decompressed_n, a.first_difference, a.lossless) == (b.original_n, b.compressed_n, b.decompressed_n, b.first_difference, b.lossless), j
        both = counts1.reshape(k, n, 512)
        assert all(np.array_equal(both[l, :, :256], ho.reshape(n, 256)) for l in range(k)) and np.array_equal(both[:, :, 256:], hd.reshape(k, n, 256))
    out = []
    for dev in (False, True):
        loop(dev)
        ho[:] = 0
        hd[:] = 0
        suite(dev)
        same()
        out += [five(lambda: loop(dev)), five(lambda: suite(dev))]
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "suite_batch_rates.txt")
    import torch
    L = _lib.lib()
    _lib.check(L.rsn_device_set(0))
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say("batch suite, {[huffman], [lzss], [lzss, huffman]} -- %s, %s" % (torch.cuda.get_device_name(0), time.strftime("%Y-%m-%d")))
    say("HIP runtime %s; ms of host wall clock around synchronising calls: median (min .. max) of five repeats after a warm-up" % (_lib.runtime_info()[0],))
    say("loop: three rsn_layers_roundtrip_batch(_dev) calls in turn   suite: one rsn_layers_suite_batch(_dev) call   x: loop median / suite median")
    say("below: is the suite's median below the loop's fastest repeat")
    say()
    fmt = "%8.2f (%7.2f .. %7.2f)"
    say("%-14s %26s %26s %6s %6s   %26s %26s %6s %6s" % ("members", "host loop ms", "host suite ms", "x", "below", "dev loop ms", "dev suite ms", "x", "below"))
    for count, size in ((4096, 25), (4096, 1024), (256, 16 << 10), (256, 64 << 10)):
        datas = [text(size, 1000 * size + i) for i in range(count)]
        hl, hs, dl, ds = legs(datas)
        say("%-14s %s %s %5.2fx %6s   %s %s %5.2fx %6s" % ("%d x %d B" % (count, size), fmt % hl, fmt % hs, hl[0] / hs[0], "yes" if hs[0] < hl[1] else "NO",
                                                       fmt % dl, fmt % ds, dl[0] / ds[0], "yes" if ds[0] < dl[1] else "NO"))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
