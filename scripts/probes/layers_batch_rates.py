"""Rates of the layered batch calls (README): five ways to run the same members under [lzss, huffman], one job on one box.

    (a) the loop of single rsn_layers_*_dev calls      what a caller with device-resident members had before these calls
    (b) the two host-buffer batch calls in turn        the engine's route: every intermediate comes down and goes up again
    (c) the two rsn_*_batch_dev calls in turn          the caller makes the intermediate buffers and the second member table
    (d) rsn_layers_*_batch_dev                         the new device form
    (e) rsn_layers_*_batch                             the new host form, host memory to host memory

    python scripts/probes/layers_batch_rates.py [out_file]     (default profiles/layers_batch_rates.txt)

Host wall clock around calls that synchronise before they return; every leg is warmed up once, then the median of five runs, with the
five runs' least and greatest beside it.  All legs go through ctypes with their argument arrays built beforehand (leg (c) copies the
first call's sizes into the second table with one numpy assignment), so what is timed is the library.  The condition the calls were
built under: at the shapes of 4096 members (d) beats (a) by more than the spread (max - min) of (a)'s five runs; the column says
whether it holds, and the exit status is 1 when it does not.  (d) against (c) -- the same work -- and (e) against (b) are reported."""
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from batch_dev_rates import Packed, five, ru16, text  # noqa: E402
from raisin_amd import _lib, huffman as H, layers, lz  # noqa: E402

U8P = ctypes.POINTER(ctypes.c_uint8)
NAMES = ["lzss", "huffman"]


def legs(enc, datas, mids, want):
    """enc: datas -lzss-> mids -huffman-> want; otherwise datas -huffman-> mids -lzss-> want.  -> the five legs' (median, min, max) in ms;
    every leg's results are compared with `want` once"""
    import torch
    L = _lib.lib()
    k = len(datas)
    ids, n_ids = layers.ids(NAMES)
    if enc:
        caps1, caps2 = [L.rsn_lzss_compress_bound(len(d)) for d in datas], [L.rsn_huffman_compress_bound(len(m)) for m in mids]
        single, dev_l = L.rsn_layers_compress_dev, L.rsn_layers_compress_batch_dev
        host1, x1, host2, x2 = L.rsn_lzss_compress_batch, (4096,), L.rsn_huffman_compress_batch, ()
        dev1, dev2, host_l = L.rsn_lzss_compress_batch_dev, L.rsn_huffman_compress_batch_dev, L.rsn_layers_compress_batch
    else:
        caps1, caps2 = [len(m) for m in mids], [len(w) for w in want]
        single, dev_l = L.rsn_layers_decompress_dev, L.rsn_layers_decompress_batch_dev
        host1, x1, host2, x2 = L.rsn_huffman_decompress_batch, (), L.rsn_lzss_decompress_batch, ()
        dev1, dev2, host_l = L.rsn_huffman_decompress_batch_dev, L.rsn_lzss_decompress_batch_dev, L.rsn_layers_decompress_batch
    p = Packed(datas, caps2)                                              # the members, and the slots of the final results
    mid = Packed([b""] * k, caps1)                                        # the caller-made intermediate slots of leg (c)
    got = ctypes.c_size_t(0)

    def leg_a():
        for d_in, n, d_out, cap in p.members:
            rc = single(d_in, n, ids, n_ids, d_out, cap, ctypes.byref(got), None)
            assert rc == 0, L.rsn_last_error()
    ins = (ctypes.c_char_p * k)(*datas)
    lens = (ctypes.c_size_t * k)(*[len(d) for d in datas])
    outs1, outs2 = (U8P * k)(), (U8P * k)()
    olens1, olens2 = (ctypes.c_size_t * k)(), (ctypes.c_size_t * k)()
    as_ins = ctypes.cast(outs1, ctypes.POINTER(ctypes.c_char_p))

    def free(outs):
        for i in range(k):
            L.rsn_free(outs[i])

    def leg_b(keep=False):
        rc = host1(k, ins, lens, *x1, outs1, olens1)
        assert rc == 0, L.rsn_last_error()
        rc = host2(k, as_ins, olens1, *x2, outs2, olens2)
        assert rc == 0, L.rsn_last_error()
        res = [ctypes.string_at(outs2[i], olens2[i]) for i in range(k)] if keep else None
        free(outs1)
        free(outs2)
        return res
    arr = (_lib.DevMember * k)(*[_lib.DevMember(*m) for m in p.members])
    arr1 = (_lib.DevMember * k)(*[_lib.DevMember(m[0], m[1], s[2], s[3]) for m, s in zip(p.members, mid.members)])
    arr2 = (_lib.DevMember * k)(*[_lib.DevMember(s[2], 0, m[2], m[3]) for m, s in zip(p.members, mid.members)])
    n2 = np.frombuffer(arr2, dtype=np.uint64).reshape(k, 4)[:, 1]         # the second table's lengths, written from the first call's answers
    dlens1, dlens = (ctypes.c_size_t * k)(), (ctypes.c_size_t * k)()
    n1 = np.frombuffer(dlens1, dtype=np.uint64)

    def leg_c():
        rc = dev1(k, arr1, *x1, dlens1, None)
        assert rc == 0, L.rsn_last_error()
        n2[:] = n1
        rc = dev2(k, arr2, *x2, dlens, None)
        assert rc == 0, L.rsn_last_error()

    def leg_d():
        rc = dev_l(k, arr, ids, n_ids, dlens, None)
        assert rc == 0, L.rsn_last_error()

    def leg_e(keep=False):
        rc = host_l(k, ins, lens, ids, n_ids, outs2, olens2)
        assert rc == 0, L.rsn_last_error()
        res = [ctypes.string_at(outs2[i], olens2[i]) for i in range(k)] if keep else None
        free(outs2)
        return res
    for leg in (leg_d, leg_c):
        leg()
        assert [p.result(i, dlens[i]) for i in range(k)] == want
        p.o.zero_()
        torch.cuda.synchronize()
    leg_a()
    assert [p.result(i, len(w)) for i, w in enumerate(want)] == want
    assert leg_b(keep=True) == want and leg_e(keep=True) == want
    return five(leg_a), five(leg_b), five(leg_c), five(leg_d), five(leg_e)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "layers_batch_rates.txt")
    import torch
    L = _lib.lib()
    _lib.check(L.rsn_device_set(0))
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say("layered batch calls, [lzss, huffman] -- %s, %s" % (torch.cuda.get_device_name(0), time.strftime("%Y-%m-%d")))
    say("HIP runtime %s; ms of host wall clock around synchronising calls: median (min .. max) of five runs after a warm-up" % (_lib.runtime_info()[0],))
    say("(a) loop of rsn_layers_*_dev   (b) the two host batch calls in turn   (c) the two rsn_*_batch_dev calls in turn   (d) rsn_layers_*_batch_dev   (e) rsn_layers_*_batch")
    say()
    fmt = "%8.2f (%7.2f .. %7.2f)"
    say("%-14s %-10s %26s %26s %26s %26s %26s %7s %6s %6s  %s" % ("members", "direction", "(a) ms", "(b) ms", "(c) ms", "(d) ms", "(e) ms", "a/d", "c/d", "b/e", "d < a - spread(a)"))
    ok = True
    for count, size in ((4096, 25), (4096, 1024), (256, 16 << 10), (256, 64 << 10)):
        datas = [text(size, 1000 * size + i) for i in range(count)]
        mids = lz.CompressAsyncBatch(datas, 4096)
        streams = H.CompressBatch(mids)
        assert lz.DecompressBatch(H.DecompressBatch(streams)) == datas
        for name, enc, ins, want in (("compress", True, datas, streams), ("decompress", False, streams, datas)):
            a, b, c, d, e = legs(enc, ins, mids, want)
            holds = d[0] < a[0] - (a[2] - a[1])
            if count == 4096 and not holds:
                ok = False
            say("%-14s %-10s %s %s %s %s %s %6.1fx %5.2fx %5.2fx  %s" % ("%d x %d B" % (count, size), name, fmt % a, fmt % b, fmt % c, fmt % d, fmt % e,
                                                                       a[0] / d[0], c[0] / d[0], b[0] / e[0], "holds" if holds else "DOES NOT HOLD"))
    say()
    say("the condition (4096-member shapes): %s" % ("holds at every shape" if ok else "DOES NOT HOLD at a shape above"))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
