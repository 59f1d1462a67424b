"""LZSS batch decompress of streams that no workgroup holds (csrc/lzss_tile_dec.hip; DESIGN 4.7: LZSS_TILE_DEC_GROUP_MIN, LZSS_TILE_DEC_IN_MAX,
LZSS_TILE_DEC_OUT_MAX): the batch call against the loop of single calls on this build and against the same batch call on the PARENT
commit's build, same box.

    python scripts/probes/lzss_tile_dec_batch.py --parent PARENT_LIBRSN [--wide WIDE_LIBRSN] [--out FILE] [--k 4,8,16,32,64,256]
                                                                                  (default profiles/lzss_tile_dec_batch.txt)

PARENT_LIBRSN is the parent commit's build of librsn.so, WIDE_LIBRSN this commit's PROBE build (raisin_amd/csrc/Makefile: the class's
minimum lowered to 2, so that every row of at least 2 candidates takes the tiled route whatever the constant is in this build); each is
loaded through RSN_LIB_PATH in a child process of its own, this build runs in a third.  A child times every shape -- K streams of the
text of 16 KiB and 64 KiB (below the mid class's minimum they took the single call, and take the tiled class from
LZSS_TILE_DEC_GROUP_MIN on) and of 96 KiB, 128 KiB and 256 KiB (huff_big_batch.py's generator, compressed
by this library at the window of 4096) -- through rsn_lzss_decompress_batch (host) and rsn_lzss_decompress_batch_dev (device), and this
build's child through the loop of rsn_lzss_decompress / rsn_lzss_decompress_dev over the same streams as well.  Host wall clock around
calls that synchronise before they return; a warm-up, then five runs; a row is the median and the least and greatest of the five.  The
builds' results are compared by digest.  In the parent every such stream takes the single call inside the batch (K >= 64 streams of
16 KiB: the mid class, in both builds).

LZSS_TILE_DEC_GROUP_MIN by its rule: the smallest measured K from which on the batch call's median lies below the loop's by
more than the spread of the loop's five runs, at every measured size, in both forms.  The script prints it and says whether this build
carries it.  The batch column is the probe build's when --wide is given, else this build's, where a K below the minimum shows the single
calls inside the batch, not the class."""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from huff_big_batch import five, ru16, text   # noqa: E402

SIZES = (("16KiB", 16 << 10), ("64KiB", 64 << 10), ("96KiB", 96 << 10), ("128KiB", 128 << 10), ("256KiB", 256 << 10))
WINDOW = 4096


def child(ks, loops):
    """every shape once in this process's build -> one JSON line {key: {"ms": [five], "digest": ...}}"""
    import torch

    from raisin_amd import _lib, lz
    L = _lib.lib()
    _lib.check(L.rsn_device_set(0))
    U8P = ctypes.POINTER(ctypes.c_uint8)
    out = {}
    distinct = {}
    for name, size in SIZES:
        for i in range(8):
            d = text(7919 * i + size, size)
            distinct[size, i] = (d, lz.CompressAsync(d, False, WINDOW))
    for name, size in SIZES:
        for k in ks:
            datas = [distinct[size, i % 8][0] for i in range(k)]
            streams = [distinct[size, i % 8][1] for i in range(k)]
            sizes = [len(s) for s in streams]
            ins = (ctypes.c_char_p * k)(*streams)
            lens = (ctypes.c_size_t * k)(*sizes)
            outs = (U8P * k)()
            olens = (ctypes.c_size_t * k)()
            one, one_n = U8P(), ctypes.c_size_t()

            def host(keep=False):
                rc = L.rsn_lzss_decompress_batch(k, ins, lens, outs, olens)
                assert rc == 0, L.rsn_last_error()
                res = [ctypes.string_at(outs[i], olens[i]) for i in range(k)] if keep else None
                for i in range(k):
                    L.rsn_free(outs[i])
                return res

            def host_loop():
                for s, n in zip(streams, sizes):
                    rc = L.rsn_lzss_decompress(s, n, ctypes.byref(one), ctypes.byref(one_n))
                    assert rc == 0, L.rsn_last_error()
                    L.rsn_free(one)
            assert host(keep=True) == datas
            in_at, out_at, a, b = [], [], 0, 0
            for n in sizes:
                in_at.append(a); out_at.append(b)
                a += ru16(n); b += ru16(size) + 16
            src = torch.frombuffer(bytearray(b"".join(s + bytes(ru16(len(s)) - len(s)) for s in streams) + bytes(64)), dtype=torch.uint8).cuda()
            dst = torch.zeros(b + 16, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            arr = (_lib.DevMember * k)(*[_lib.DevMember(src.data_ptr() + in_at[i], sizes[i], dst.data_ptr() + out_at[i], size) for i in range(k)])
            dlens = (ctypes.c_size_t * k)()

            def dev():
                rc = L.rsn_lzss_decompress_batch_dev(k, arr, dlens, None)
                assert rc == 0, L.rsn_last_error()

            def dev_loop():
                for i in range(k):
                    rc = L.rsn_lzss_decompress_dev(src.data_ptr() + in_at[i], sizes[i], dst.data_ptr() + out_at[i], size, ctypes.byref(one_n), None)
                    assert rc == 0, L.rsn_last_error()
            dev()
            h = dst.cpu().numpy()
            assert [bytes(h[out_at[i]:out_at[i] + dlens[i]]) for i in range(k)] == datas
            digest = hashlib.sha256(b"".join(datas)).hexdigest()[:16]
            for form, fn, loop in (("host", host, host_loop), ("dev", dev, dev_loop)):
                out["%s %d %s batch" % (name, k, form)] = {"ms": five(fn), "digest": digest, "stream": sum(sizes) // k}
                if loops:
                    out["%s %d %s loop" % (name, k, form)] = {"ms": five(loop), "digest": digest}
            del src, dst
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="")
    ap.add_argument("--wide", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lzss_tile_dec_batch.txt"))
    ap.add_argument("--k", default="4,8,16,32,64,256")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--loops", action="store_true")
    a = ap.parse_args()
    ks = [int(x) for x in a.k.split(",")]
    if a.child:
        return child(ks, a.loops)
    if not a.parent:
        ap.error("--parent PARENT_LIBRSN is needed: the third column is the parent build's batch call")
    runs = {}
    # every step a process of its own under its own time limit, the next one only when it ended well: a fault ends the run
    for build, lib in (("parent", a.parent), ("this", ""), ("wide", a.wide)):
        if build == "wide" and not lib:
            continue
        env = dict(os.environ)
        env.pop("RSN_LIB_PATH", None)
        if lib:
            env["RSN_LIB_PATH"] = os.path.abspath(lib)
        cmd = ["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--child", "--k", a.k] + (["--loops"] if build == "this" else [])
        p = subprocess.run(cmd, env=env, capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write("the %s build's child ended with %d\n" % (build, p.returncode) + p.stdout[-2000:] + p.stderr[-4000:])
            return 1
        runs[build] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print("%s build: done" % build, flush=True)
    from raisin_amd import lz
    this = runs["this"]
    tiled = runs.get("wide", this)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say("LZSS batch decompress, streams of text compressed at window %d: this build's batch call, the loop of single calls, the parent commit's batch call -- %s" % (WINDOW, time.strftime("%Y-%m-%d")))
    say("ms of host wall clock around synchronising calls: median (min .. max) of five runs after a warm-up, a process a build")
    say("this build: LZSS_TILE_DEC_IN_MAX = %d, LZSS_TILE_DEC_OUT_MAX = %d, LZSS_TILE_POS = %d, LZSS_TILE_DEC_GROUP_MIN = %d, groups of %d MiB"
        % (lz.TILE_DEC_IN_MAX, lz.TILE_DEC_OUT_MAX, lz.TILE_POS, lz.TILE_DEC_GROUP_MIN, lz.TILE_GROUP_BYTES >> 20))
    say("batch call: " + ("the probe build of this commit (the class from 2 candidates on)" if "wide" in runs else "this build: a row with K below LZSS_TILE_DEC_GROUP_MIN is the single calls inside the batch"))
    say("16 KiB and 64 KiB with K >= %d: the mid class, in both builds" % lz.MID_GROUP_MIN)
    say()
    say("%-8s %7s %4s %-4s %28s %28s %28s %8s %8s" % ("member", "stream", "K", "form", "batch call ms", "loop of single calls ms", "parent's call ms", "loop/bat", "par/bat"))
    fmt = "%9.3f (%8.3f .. %8.3f)"
    med = statistics.median
    beats = {}
    for name, size in SIZES:
        for k in ks:
            for form in ("host", "dev"):
                key = "%s %d %s batch" % (name, k, form)
                t, lp, par = tiled[key]["ms"], this[key.replace(" batch", " loop")]["ms"], runs["parent"][key]["ms"]
                for r in runs.values():
                    assert r[key]["digest"] == runs["parent"][key]["digest"], "the builds' results differ: " + key
                say("%-8s %7d %4d %-4s %s %s %s %7.1fx %7.1fx" % (name, this[key]["stream"], k, form, fmt % (med(t), min(t), max(t)), fmt % (med(lp), min(lp), max(lp)),
                                                                  fmt % (med(par), min(par), max(par)), med(lp) / med(t), med(par) / med(t)))
                beats[name, k, form] = med(t) < med(lp) - (max(lp) - min(lp))
    say()
    group_min = None
    for k in sorted(ks, reverse=True):
        if all(beats[name, k, form] for name, _ in SIZES for form in ("host", "dev")):
            group_min = k
        else:
            break
    say("LZSS_TILE_DEC_GROUP_MIN by its rule: %s; this build: %d"
        % (group_min if group_min else "none", lz.TILE_DEC_GROUP_MIN))
    top = max(ks)
    slower = [form for form in ("host", "dev") if not beats["256KiB", top, form]]
    say("256 KiB at K = %d against the loop: %s" % (top, "slower in " + ", ".join(slower) + " -- the class must end below it" if slower else "faster in both forms: the class keeps its limits"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
