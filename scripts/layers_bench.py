"""Host buffer to host buffer timings of the layered calls: [lzss, huffman] compress, decompress and round trip on
25 B, 64 KiB, 16 MiB and 1 GiB of text, median of five after a warm-up, in three legs that alternate in ONE job on one box:
  (a) the chain of single host calls on ANOTHER build of librsn (--parent-lib: the parent commit's), in a child process
  (b) the same chain on this build
  (c) the layered calls of this build
The round trip of the chained legs is what engine.BenchmarkFile did: both chains, two byte histograms and a comparison on the host.
Plain ctypes (a parent build has no layered symbols for raisin_amd._lib to bind).

  python scripts/layers_bench.py --parent-lib scripts/ab/librsn_parent.so [--rounds 2] [--max-mib 1024]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LAYERS = (ctypes.c_int * 2)(1, 2)
u8p = ctypes.POINTER(ctypes.c_uint8)


class RoundTrip(ctypes.Structure):
    _fields_ = [("original_n", ctypes.c_uint64), ("compressed_n", ctypes.c_uint64), ("decompressed_n", ctypes.c_uint64),
                ("lossless", ctypes.c_int), ("first_difference", ctypes.c_uint64),
                ("hist_original", ctypes.c_uint64 * 256), ("hist_decompressed", ctypes.c_uint64 * 256),
                ("compress_ms", ctypes.c_double), ("decompress_ms", ctypes.c_double)]


def inputs(max_mib):
    import torch
    import workloads as W
    n = min(max_mib, 1024) << 20
    text = W.config_input("4", n, "cuda").cpu().numpy()
    torch.cuda.synchronize()
    out = [("25 B", __import__("numpy").frombuffer(b"abcabcabcabcabcabcabcabc\n", dtype="uint8").copy())]
    for label, size in (("64 KiB", 64 << 10), ("16 MiB", 16 << 20), ("1 GiB", 1 << 30)):
        if size <= n:
            out.append((label, text[:size].copy() if size < n else text))
    return out


def child(leg, max_mib):
    import numpy as np
    import torch  # noqa: F401 -- first, as raisin_amd._lib does: every leg runs on the same HIP runtime
    L = ctypes.CDLL(os.environ.get("RSN_LIB_PATH") or os.path.join(ROOT, "raisin_amd", "librsn.so"))
    L.rsn_last_error.restype = ctypes.c_char_p
    L.rsn_free.argtypes = [ctypes.c_void_p]

    def call(fn, buf, *extra):
        out, n = u8p(), ctypes.c_size_t(0)
        rc = fn(ctypes.c_void_p(buf.ctypes.data), ctypes.c_size_t(buf.size), *extra, ctypes.byref(out), ctypes.byref(n))
        if rc != 0:
            raise RuntimeError(L.rsn_last_error().decode())
        res = np.ctypeslib.as_array(out, shape=(max(n.value, 1),))[:n.value].copy()
        L.rsn_free(out)
        return res

    win = ctypes.c_int64(4096)
    if leg == "layered":
        comp = lambda x: call(L.rsn_layers_compress, x, LAYERS, ctypes.c_size_t(2))          # noqa: E731
        dec = lambda x: call(L.rsn_layers_decompress, x, LAYERS, ctypes.c_size_t(2))         # noqa: E731

        def trip(x):
            r = RoundTrip()
            rc = L.rsn_layers_roundtrip(ctypes.c_void_p(x.ctypes.data), ctypes.c_size_t(x.size), LAYERS, ctypes.c_size_t(2), ctypes.byref(r), None, None)
            assert rc == 0 and r.lossless, L.rsn_last_error()
    else:
        comp = lambda x: call(L.rsn_huffman_compress, call(L.rsn_lzss_compress, x, win))     # noqa: E731
        dec = lambda x: call(L.rsn_lzss_decompress, call(L.rsn_huffman_decompress, x))       # noqa: E731

        def trip(x):                                                                         # engine.go:357-441 on the host
            h0 = np.bincount(x, minlength=256)
            d = dec(comp(x))
            h1 = np.bincount(d, minlength=256)
            assert np.array_equal(d, x) and h0.sum() == h1.sum()

    def timed(fn, x):
        fn(x)
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            fn(x)
            ts.append((time.perf_counter() - t0) * 1e3)
        return [round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)]

    res = {}
    for label, x in inputs(max_mib):
        c = comp(x)
        res[label] = {"compress": timed(comp, x), "decompress": timed(dec, c), "round trip": timed(trip, x), "C2": int(c.size)}
        if leg != "layered":
            res[label]["C1"] = int(call(L.rsn_lzss_compress, x, win).size)
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "scripts", "ab", "librsn_parent.so"))
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--max-mib", type=int, default=1024)
    ap.add_argument("--leg")
    a = ap.parse_args()
    if a.leg:
        return child(a.leg, a.max_mib)
    legs = [("(a) parent, chained", "chained", a.parent_lib), ("(b) this build, chained", "chained", None), ("(c) this build, layered", "layered", None)]
    for rnd in range(a.rounds):
        for name, leg, lib in legs:
            env = dict(os.environ)
            env.pop("RSN_LIB_PATH", None)
            if lib:
                env["RSN_LIB_PATH"] = os.path.abspath(lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--max-mib", str(a.max_mib)], env=env, capture_output=True, text=True, timeout=900)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print("round %d %s: FAILED rc=%d %s" % (rnd, name, p.returncode, p.stderr[-600:]))
                return 1
            for label, r in json.loads(line[0][7:]).items():
                print("round %d | %-24s | %-7s | compress %s | decompress %s | round trip %s ms (median, min, max of 5) | C1 %s C2 %s"
                      % (rnd, name, label, r["compress"], r["decompress"], r["round trip"], r.get("C1", "-"), r["C2"]), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
