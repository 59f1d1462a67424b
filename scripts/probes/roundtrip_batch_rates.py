"""Rates of the batch round trip (README): four ways to get the benchmark's answer -- sizes, lossless or not, the first
difference and both byte histograms -- for the same members under [lzss, huffman], one job on one box.

    (a) the loop of rsn_layers_roundtrip               the only one-call route before the batch round trip
    (b) rsn_layers_compress_batch + rsn_layers_decompress_batch, then the comparison and numpy.bincount on the host
                                                       the engine's route before: every stream and every file comes down
    (c) rsn_layers_roundtrip_batch                     the new host form
    (d) rsn_layers_roundtrip_batch_dev                 the new device form, the members already on the device

    timeout -k 10 900 python scripts/probes/roundtrip_batch_rates.py [out_file]     (default profiles/roundtrip_batch_rates.txt)

One process.  Host wall clock around calls that synchronise before they return; every leg is warmed up once, then the median of five
runs, with the five runs' least and greatest beside it.  All legs go through ctypes with their argument arrays built beforehand, so what
is timed is the library (and, in (b), the host's comparison and counting, which are that route's work).  The condition the calls were
built under: at the shapes of 4096 members (c) and (d) each beat (a) by more than the spread (max - min) of (a)'s five runs; the column
says whether it holds, and the exit status is 1 when it does not.  Reported beside it: (c) against (b), and k_members_verify's own time
from the library's profile (summed over the call's runs) against k_members_move's over the same members -- the mover reads and writes each byte once, the verify
kernel reads two buffers of that size and counts every byte, so it is not expected to match a copy; the column says how far off it is."""
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

U8P = ctypes.POINTER(ctypes.c_uint8)
NAMES = ["lzss", "huffman"]


def legs(datas):
    """-> the four legs' (median, min, max) in ms, and (members_verify ms, members_move ms) of one launch each; every leg's answers are
    compared with leg (b)'s -- host arithmetic over the bytes the batch calls returned -- once"""
    L = _lib.lib()
    k = len(datas)
    ids, n_ids = layers.ids(NAMES)
    ins = (ctypes.c_char_p * k)(*datas)
    lens = (ctypes.c_size_t * k)(*[len(d) for d in datas])
    one = _lib.RoundTripResult()

    def leg_a(keep=False):
        rows = []
        for d in datas:
            rc = L.rsn_layers_roundtrip(d, len(d), ids, n_ids, ctypes.byref(one), None, None)
            assert rc == 0, L.rsn_last_error()
            if keep:
                rows.append(((one.original_n, one.compressed_n, one.decompressed_n, one.first_difference, one.lossless), list(one.hist_original) + list(one.hist_decompressed)))
        return rows
    outs1, outs2 = (U8P * k)(), (U8P * k)()
    olens1, olens2 = (ctypes.c_size_t * k)(), (ctypes.c_size_t * k)()
    as_ins = ctypes.cast(outs1, ctypes.POINTER(ctypes.c_char_p))

    def leg_b():
        rc = L.rsn_layers_compress_batch(k, ins, lens, ids, n_ids, outs1, olens1)
        assert rc == 0, L.rsn_last_error()
        rc = L.rsn_layers_decompress_batch(k, as_ins, olens1, ids, n_ids, outs2, olens2)
        assert rc == 0, L.rsn_last_error()
        rows = []
        for i, d in enumerate(datas):
            a = np.frombuffer(d, dtype=np.uint8)
            b = np.ctypeslib.as_array(outs2[i], shape=(olens2[i],)) if olens2[i] else a[:0]
            m = min(len(a), len(b))
            differ = np.flatnonzero(a[:m] != b[:m])
            first = int(differ[0]) if len(differ) else ((1 << 64) - 1 if len(a) == len(b) else m)
            counts = np.bincount(a, minlength=256).tolist() + np.bincount(b, minlength=256).tolist()
            rows.append(((len(d), olens1[i], olens2[i], first, int(first == (1 << 64) - 1)), counts))
        for i in range(k):
            L.rsn_free(outs1[i])
            L.rsn_free(outs2[i])
        return rows
    res = (_lib.RoundTripMember * k)()
    counts = np.zeros(512 * k, dtype=np.uint32)
    counts_p = counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))

    def rows_of():
        return [((res[i].original_n, res[i].compressed_n, res[i].decompressed_n, res[i].first_difference, res[i].lossless), counts[512 * i:512 * i + 512].tolist()) for i in range(k)]

    def leg_c():
        rc = L.rsn_layers_roundtrip_batch(k, ins, lens, ids, n_ids, res, counts_p)
        assert rc == 0, L.rsn_last_error()
    p = Packed(datas, [len(d) for d in datas])                            # the members on the device; the slots are the mover's in the last measurement
    arr = (_lib.DevMember * k)(*[_lib.DevMember(m[0], m[1], None, 0) for m in p.members])

    def leg_d():
        rc = L.rsn_layers_roundtrip_batch_dev(k, arr, ids, n_ids, res, counts_p, None)
        assert rc == 0, L.rsn_last_error()
    want = leg_b()
    assert leg_a(keep=True) == want
    leg_c()
    assert rows_of() == want
    counts[:] = 0
    leg_d()
    assert rows_of() == want
    times = five(leg_a), five(leg_b), five(leg_c), five(leg_d)
    # the verify kernel's own time, and the mover's over the same members (the device form without layers is k_members_move alone)
    move = (_lib.DevMember * k)(*[_lib.DevMember(*m) for m in p.members])
    dlens = (ctypes.c_size_t * k)()
    none, n_none = layers.ids([])
    _lib.prof_enable(True)
    try:
        kernels = []
        for name, call in (("members_verify", leg_d), ("members_move", lambda: L.rsn_layers_compress_batch_dev(k, move, none, n_none, dlens, None))):
            call()
            ms = []
            for _ in range(5):
                _lib.prof_reset()
                call()
                ms.append(_lib.prof_get()[name][1])                        # (the sum over the call's runs: a launch a run)
            kernels.append(sorted(ms)[2])
    finally:
        _lib.prof_enable(False)
    return times, kernels


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "roundtrip_batch_rates.txt")
    import torch
    L = _lib.lib()
    _lib.check(L.rsn_device_set(0))
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say("batch round trip, [lzss, huffman] -- %s, %s" % (torch.cuda.get_device_name(0), time.strftime("%Y-%m-%d")))
    say("HIP runtime %s; ms of host wall clock around synchronising calls: median (min .. max) of five runs after a warm-up" % (_lib.runtime_info()[0],))
    say("(a) loop of rsn_layers_roundtrip   (b) rsn_layers_compress_batch + rsn_layers_decompress_batch + host compare and bincount   "
        "(c) rsn_layers_roundtrip_batch   (d) rsn_layers_roundtrip_batch_dev")
    say("verify / move: k_members_verify's and k_members_move's own time over the same members, summed over a call's launches (median of five, from the profile)")
    say()
    fmt = "%8.2f (%7.2f .. %7.2f)"
    say("%-14s %26s %26s %26s %26s %7s %7s %6s %10s %9s %7s  %s" % ("members", "(a) ms", "(b) ms", "(c) ms", "(d) ms", "a/c", "a/d", "b/c", "verify ms", "move ms", "v/m", "c, d < a - spread(a)"))
    ok = True
    for count, size in ((4096, 25), (4096, 1024), (256, 16 << 10), (256, 64 << 10)):
        datas = [text(size, 1000 * size + i) for i in range(count)]
        (a, b, c, d), (verify, move) = legs(datas)
        holds = max(c[0], d[0]) < a[0] - (a[2] - a[1])
        if count == 4096 and not holds:
            ok = False
        say("%-14s %s %s %s %s %6.1fx %6.1fx %5.2fx %10.4f %9.4f %6.2fx  %s" % ("%d x %d B" % (count, size), fmt % a, fmt % b, fmt % c, fmt % d, a[0] / c[0], a[0] / d[0], b[0] / c[0],
                                                                            verify, move, verify / move, "holds" if holds else "DOES NOT HOLD"))
    say()
    say("the condition (4096-member shapes): %s" % ("holds at every shape" if ok else "DOES NOT HOLD at a shape above"))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
