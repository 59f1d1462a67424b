"""k_byte_hist256 and k_bytes_differ at 1 GiB, through rsn_layers_roundtrip with the library's own events around every
launch: uniform 7-bit bytes under [huffman] and one repeated byte under [lzss] -- in both the decoded buffer is a second gigabyte equal
to the input, so the comparison reads both to the end -- next to torch's read-only pass over the same gigabyte (bench.py --full's
yardstick).  RSN_HIST256_COPIES=16 selects the histogram's other shape (one process per shape: the switch is read once).
Under rocprofv3 --kernel-trace --stats the same run gives the kernels' own durations."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import workloads as W
from raisin_amd import _lib, layers

GIB = 1 << 30


def read_only_ms(t, reps=10):
    for _ in range(3):
        t.view(torch.int64).sum()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        t.view(torch.int64).sum()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    n = (int(sys.argv[1]) << 20) if len(sys.argv) > 1 else GIB
    src = W.config_input("2a", n, "cuda")
    ro = read_only_ms(src)
    print("copies %s | read-only pass (torch int64 sum) %.4f ms per %d MiB = %.0f GB/s" % (os.environ.get("RSN_HIST256_COPIES", "32"), ro, n >> 20, n / ro / 1e6))
    cases = [("uniform 0x00-0x7F", bytes(src.cpu().numpy()), ["huffman"]), ("one byte", b"z" * n, ["lzss"])]
    del src
    torch.cuda.empty_cache()
    for name, data, ls in cases:
        layers.RoundTrip(data, ls)                                       # warm-up: arenas, code objects
        for rep in range(3):
            _lib.prof_enable(True)
            _lib.prof_reset()
            res, _ = layers.RoundTrip(data, ls)
            p = _lib.prof_get()
            _lib.prof_enable(False)
            assert res.lossless and sum(res.hist_original) == n
            h, d = p["byte_hist256"], p["bytes_differ"]
            hm, dm = h[1] / h[0], d[1] / d[0]
            print("%-18s | byte_hist256 %.4f ms per launch (%d launches; %.2f of the read-only pass' rate) | bytes_differ %.4f ms for 2 x %d MiB (%.2f of that rate)"
                  % (name, hm, h[0], ro / hm, dm, n >> 20, 2 * ro / dm), flush=True)


if __name__ == "__main__":
    main()
