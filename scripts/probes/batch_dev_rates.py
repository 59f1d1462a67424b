"""Rates of the batch calls on device buffers (README): three ways to run the same members, one job on one box.

    (a) the loop of single *_dev calls        what a caller with device-resident members had before these calls
    (b) the host-buffer batch call            the same members starting from, and ending in, host memory
    (c) the batch call on device buffers      rsn_*_batch_dev

    python scripts/probes/batch_dev_rates.py [out_file [codec ...]]     (default profiles/batch_dev_rates.txt, every codec)

With codecs named (lzss, arithmetic, huffman) only their rows are run, and they are APPENDED to the file under a heading of their own.

Host wall clock around calls that synchronise before they return; every leg is warmed up once, then the median of five runs, with the
five runs' least and greatest beside it.  All three legs go through ctypes with their argument arrays built beforehand, so what is
timed is the library.  The condition the calls were built under: at the shapes of 4096 members (c) beats (a) by more than the spread
(max - min) of (a)'s five runs; the last column says whether it holds, and the exit status is 1 when it does not."""
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from raisin_amd import _lib, arithmetic as A, huffman as H, lz  # noqa: E402

U8P = ctypes.POINTER(ctypes.c_uint8)
VOCAB = None


def text(n, seed):
    """words of a small vocabulary: compresses like prose in both codecs"""
    global VOCAB
    rng = np.random.default_rng(seed)
    if VOCAB is None:
        v = np.random.default_rng(1)
        VOCAB = [bytes(v.choice(np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8), size=int(v.integers(2, 10)))) for _ in range(300)]
    out = bytearray()
    while len(out) < n:
        out += VOCAB[int(rng.integers(0, len(VOCAB)))] + b" "
    return bytes(out[:n])


def ru16(x):
    return (x + 15) // 16 * 16


def five(fn):
    fn()
    ts = []
    for _ in range(5):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


class Packed:
    """members back to back in one device allocation at 16-byte offsets, and output slots of `caps` bytes in another"""

    def __init__(self, datas, caps):
        import torch
        buf, self.offs = bytearray(), []
        for d in datas:
            self.offs.append(len(buf))
            buf += d + bytes(ru16(len(d)) - len(d))
        buf += bytes(64)
        self.t = torch.frombuffer(buf, dtype=torch.uint8).cuda()
        self.out_offs, at = [], 0
        for c in caps:
            self.out_offs.append(at)
            at += ru16(c) + 16
        self.o = torch.zeros(at + 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.members = [(self.t.data_ptr() + a, len(d), self.o.data_ptr() + b, c) for a, d, b, c in zip(self.offs, datas, self.out_offs, caps)]

    def result(self, i, k):
        b = self.out_offs[i]
        return bytes(self.o[b:b + k].cpu().numpy())


def legs(single, host_batch, dev_batch, extra, datas, caps, want):
    """-> the three legs' (median, min, max) in ms; every leg's results are compared with `want` once"""
    import torch
    L = _lib.lib()
    k = len(datas)
    p = Packed(datas, caps)
    got = ctypes.c_size_t(0)

    def leg_a():
        for d_in, n, d_out, cap in p.members:
            rc = single(d_in, n, *extra, d_out, cap, ctypes.byref(got), None)
            assert rc == 0, L.rsn_last_error()
    ins = (ctypes.c_char_p * k)(*datas)
    lens = (ctypes.c_size_t * k)(*[len(d) for d in datas])
    outs = (U8P * k)()
    olens = (ctypes.c_size_t * k)()

    def leg_b(keep=False):
        rc = host_batch(k, ins, lens, *extra, outs, olens)
        assert rc == 0, L.rsn_last_error()
        res = [ctypes.string_at(outs[i], olens[i]) for i in range(k)] if keep else None
        for i in range(k):
            L.rsn_free(outs[i])
        return res
    arr = (_lib.DevMember * k)(*[_lib.DevMember(*m) for m in p.members])
    dlens = (ctypes.c_size_t * k)()

    def leg_c():
        rc = dev_batch(k, arr, *extra, dlens, None)
        assert rc == 0, L.rsn_last_error()
    leg_c()
    assert [p.result(i, dlens[i]) for i in range(k)] == want
    p.o.zero_()
    torch.cuda.synchronize()
    leg_a()
    assert [p.result(i, len(w)) for i, w in enumerate(want)] == want
    assert leg_b(keep=True) == want
    return five(leg_a), five(leg_b), five(leg_c)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "batch_dev_rates.txt")
    import torch
    L = _lib.lib()
    _lib.check(L.rsn_device_set(0))
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say("batch calls on device buffers -- %s, %s" % (torch.cuda.get_device_name(0), time.strftime("%Y-%m-%d")))
    say("HIP runtime %s; ms of host wall clock around synchronising calls: median (min .. max) of five runs after a warm-up" % (_lib.runtime_info()[0],))
    say("(a) loop of single *_dev calls   (b) host-buffer batch call, host memory to host memory   (c) rsn_*_batch_dev")
    say()
    say("%-11s %-14s %-10s %26s %26s %26s %7s %7s  %s" % ("codec", "members", "direction", "(a) ms", "(b) ms", "(c) ms", "a/c", "b/c", "c < a - spread(a)"))
    ok = True
    shapes = [("lzss", 4096, 25), ("lzss", 4096, 1024), ("lzss", 256, 16 << 10), ("lzss", 256, 64 << 10), ("arithmetic", 4096, 25), ("arithmetic", 4096, 1024),
              ("huffman", 4096, 25), ("huffman", 4096, 1024), ("huffman", 256, 16 << 10), ("huffman", 256, 64 << 10)]
    only = sys.argv[2:]
    for codec, count, size in shapes:
        if only and codec not in only:
            continue
        datas = [text(size, 1000 * size + i) for i in range(count)]
        if codec == "huffman":
            streams = H.CompressBatch(datas)
            assert H.DecompressBatch(streams) == datas
            bound = L.rsn_huffman_compress_bound
            rows = (("compress", L.rsn_huffman_compress_dev, L.rsn_huffman_compress_batch, L.rsn_huffman_compress_batch_dev, (), datas, streams),
                    ("decompress", L.rsn_huffman_decompress_dev, L.rsn_huffman_decompress_batch, L.rsn_huffman_decompress_batch_dev, (), streams, datas))
        elif codec == "lzss":
            streams = lz.CompressAsyncBatch(datas, 4096)
            assert lz.DecompressBatch(streams) == datas
            bound = L.rsn_lzss_compress_bound
            rows = (("compress", L.rsn_lzss_compress_dev, L.rsn_lzss_compress_batch, L.rsn_lzss_compress_batch_dev, (4096,), datas, streams),
                    ("decompress", L.rsn_lzss_decompress_dev, L.rsn_lzss_decompress_batch, L.rsn_lzss_decompress_batch_dev, (), streams, datas))
        else:
            streams = A.CompressBatch(datas)
            assert A.DecompressBatch(streams) == datas
            bound = L.rsn_arithmetic_compress_bound
            rows = (("compress", L.rsn_arithmetic_compress_dev, L.rsn_arithmetic_compress_batch, L.rsn_arithmetic_compress_batch_dev, (), datas, streams),
                    ("decompress", L.rsn_arithmetic_decompress_dev, L.rsn_arithmetic_decompress_batch, L.rsn_arithmetic_decompress_batch_dev, (), streams, datas))
        for name, single, host_batch, dev_batch, extra, ins, want in rows:
            caps = [bound(len(d)) for d in ins] if name == "compress" else [len(w) for w in want]
            a, b, c = legs(single, host_batch, dev_batch, extra, ins, caps, want)
            holds = c[0] < a[0] - (a[2] - a[1])
            if count == 4096 and not holds:
                ok = False
            fmt = "%8.2f (%7.2f .. %7.2f)"
            say("%-11s %-14s %-10s %s %s %s %6.1fx %6.2fx  %s" % (codec, "%d x %d B" % (count, size), name, fmt % a, fmt % b, fmt % c, a[0] / c[0], b[0] / c[0],
                                                                 "holds" if holds else "DOES NOT HOLD"))
    say()
    say("the condition (4096-member shapes): %s" % ("holds at every shape" if ok else "DOES NOT HOLD at a shape above"))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a" if only else "w") as f:
        f.write(("\n" if only else "") + "\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
