"""LZSS batch compress of members above 64 KiB (csrc/lzss_tile.hip; DESIGN 4.7: LZSS_TILE_IN_MAX, LZSS_TILE_GROUP_MIN): the grouped call
against the loop of single calls on this build and against the same batch call on the PARENT commit's build, same box.

    python scripts/probes/lzss_tile_batch.py --parent PARENT_LIBRSN [--wide WIDE_LIBRSN] [--out FILE] [--k 4,8,16,32,64,256]
                                                                                             (default profiles/lzss_tile_batch.txt)

PARENT_LIBRSN is the parent commit's build of librsn.so, WIDE_LIBRSN this commit's PROBE build (raisin_amd/csrc/Makefile: the class widened
to 1 MiB and its minimum lowered to 2, so that every row below takes the tiled route whatever the two constants are in this build); each is
loaded through RSN_LIB_PATH in a child process of its own, this build runs in a third.  A child times every shape -- K members of 96 KiB,
128 KiB, 256 KiB, 512 KiB and 1 MiB of text (huff_big_batch.py's generator), K = 64 the most from 512 KiB on -- through rsn_lzss_compress_batch
(host) and rsn_lzss_compress_batch_dev (device) at the window of 4096, and this build's child through the loop of rsn_lzss_compress /
rsn_lzss_compress_dev over the same members as well.  Host wall clock around calls that synchronise before they return; a warm-up, then
five runs; a row is the median and the least and greatest of the five.  The builds' results are compared by digest.  In the parent every
member above 64 KiB takes the single call inside the batch.

The two constants by their rules, from the tiled column -- the probe build's when --wide is given, else this build's:
  LZSS_TILE_IN_MAX     the largest of 128 KiB, 256 KiB, 512 KiB and 1 MiB at which, and at every measured size below which, the tiled call
                       at K = 256 (K = 64 from 512 KiB) is at least twice as fast as the parent's call and as the loop, in both forms;
  LZSS_TILE_GROUP_MIN  the smallest measured K from which on the tiled call's median lies below the loop's by more than the spread of the
                       loop's five runs, at every measured size in the class, in both forms.
The script prints both and says whether this build carries them."""
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

SIZES = (("96KiB", 96 << 10), ("128KiB", 128 << 10), ("256KiB", 256 << 10), ("512KiB", 512 << 10), ("1MiB", 1 << 20))
CANDIDATES = ("128KiB", "256KiB", "512KiB", "1MiB")     # what LZSS_TILE_IN_MAX may be
K_MOST_BIG = 64                                          # the largest K from 512 KiB on
WINDOW = 4096


def shapes(ks):
    return [(name, k, size) for name, size in SIZES for k in ks if k <= K_MOST_BIG or size < (512 << 10)]


def child(ks, loops):
    """every shape once in this process's build -> one JSON line {key: {"ms": [five], "digest": ...}}"""
    import torch

    from raisin_amd import _lib
    L = _lib.lib()
    _lib.check(L.rsn_device_set(0))
    U8P = ctypes.POINTER(ctypes.c_uint8)
    out = {}
    distinct = {}
    for name, k, size in shapes(ks):
        datas = []
        for i in range(k):
            key = (size, i % 8)
            if key not in distinct:
                distinct[key] = text(7919 * (i % 8) + size, size)
            datas.append(distinct[key])
        sizes = [size] * k
        ins = (ctypes.c_char_p * k)(*datas)
        lens = (ctypes.c_size_t * k)(*sizes)
        outs = (U8P * k)()
        olens = (ctypes.c_size_t * k)()
        one, one_n = U8P(), ctypes.c_size_t()

        def host(keep=False):
            rc = L.rsn_lzss_compress_batch(k, ins, lens, WINDOW, outs, olens)
            assert rc == 0, L.rsn_last_error()
            res = [ctypes.string_at(outs[i], olens[i]) for i in range(k)] if keep else None
            for i in range(k):
                L.rsn_free(outs[i])
            return res

        def host_loop():
            for d, n in zip(datas, sizes):
                rc = L.rsn_lzss_compress(d, n, WINDOW, ctypes.byref(one), ctypes.byref(one_n))
                assert rc == 0, L.rsn_last_error()
                L.rsn_free(one)
        want = host(keep=True)
        caps = [int(L.rsn_lzss_compress_bound(n)) for n in sizes]
        in_at, out_at, a, b = [], [], 0, 0
        for n, c in zip(sizes, caps):
            in_at.append(a); out_at.append(b)
            a += ru16(n); b += ru16(c) + 16
        src = torch.frombuffer(bytearray(b"".join(d + bytes(ru16(len(d)) - len(d)) for d in datas) + bytes(64)), dtype=torch.uint8).cuda()
        dst = torch.zeros(b + 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        arr = (_lib.DevMember * k)(*[_lib.DevMember(src.data_ptr() + in_at[i], sizes[i], dst.data_ptr() + out_at[i], caps[i]) for i in range(k)])
        dlens = (ctypes.c_size_t * k)()

        def dev():
            rc = L.rsn_lzss_compress_batch_dev(k, arr, WINDOW, dlens, None)
            assert rc == 0, L.rsn_last_error()

        def dev_loop():
            for i in range(k):
                rc = L.rsn_lzss_compress_dev(src.data_ptr() + in_at[i], sizes[i], WINDOW, dst.data_ptr() + out_at[i], caps[i], ctypes.byref(one_n), None)
                assert rc == 0, L.rsn_last_error()
        dev()
        h = dst.cpu().numpy()
        assert [bytes(h[out_at[i]:out_at[i] + dlens[i]]) for i in range(k)] == want
        digest = hashlib.sha256(b"".join(want)).hexdigest()[:16]
        for form, fn, loop in (("host", host, host_loop), ("dev", dev, dev_loop)):
            out["%s %d %s batch" % (name, k, form)] = {"ms": five(fn), "digest": digest}
            if loops:
                out["%s %d %s loop" % (name, k, form)] = {"ms": five(loop), "digest": digest}
        del src, dst
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="")
    ap.add_argument("--wide", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lzss_tile_batch.txt"))
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
    tiled = runs.get("wide", runs["this"])
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say("LZSS batch compress, members above 64 KiB, window %d: the tiled call, the loop of single calls, the parent commit's batch call -- %s" % (WINDOW, time.strftime("%Y-%m-%d")))
    say("ms of host wall clock around synchronising calls: median (min .. max) of five runs after a warm-up, a process a build")
    say("this build: LZSS_TILE_IN_MAX = %d, LZSS_TILE_POS = %d, LZSS_TILE_GROUP_MIN = %d, groups of %d MiB; parent: every such member takes the single call inside the batch"
        % (lz.TILE_IN_MAX, lz.TILE_POS, lz.TILE_GROUP_MIN, lz.TILE_GROUP_BYTES >> 20))
    say("tiled call: " + ("the probe build of this commit (the class up to 1 MiB, from 2 members on): every row takes the tiled route" if "wide" in runs
                          else "this build: a row outside the class or below its minimum takes the single call"))
    say()
    say("%-8s %4s %-4s %28s %28s %28s %8s %8s %28s" % ("member", "K", "form", "tiled call ms", "loop of single calls ms", "parent's call ms", "loop/til", "par/til", "this build's call ms"))
    fmt = "%9.3f (%8.3f .. %8.3f)"
    med = statistics.median
    twice, beats = {}, {}
    for name, k, size in shapes(ks):
        for form in ("host", "dev"):
            key = "%s %d %s batch" % (name, k, form)
            t, lp, par, own = tiled[key]["ms"], runs["this"][key.replace(" batch", " loop")]["ms"], runs["parent"][key]["ms"], runs["this"][key]["ms"]
            for r in runs.values():
                assert r[key]["digest"] == runs["parent"][key]["digest"], "the builds' results differ: " + key
            say("%-8s %4d %-4s %s %s %s %7.1fx %7.1fx %s" % (name, k, form, fmt % (med(t), min(t), max(t)), fmt % (med(lp), min(lp), max(lp)), fmt % (med(par), min(par), max(par)),
                                                          med(lp) / med(t), med(par) / med(t), fmt % (med(own), min(own), max(own))))
            twice[name, k, form] = med(par) >= 2 * med(t) and med(lp) >= 2 * med(t)
            beats[name, k, form] = med(t) < med(lp) - (max(lp) - min(lp))
    say()
    in_max, holds = None, True
    for name, size in SIZES:                                                  # (96 KiB: a measured size below every candidate)
        k = max(x for x in ks if x <= K_MOST_BIG or size < (512 << 10))
        holds = holds and all(twice[name, k, form] for form in ("host", "dev"))
        say("%-8s K = %3d: twice as fast as the parent's call and as the loop, both forms: %s" % (name, k, "yes" if twice[name, k, "host"] and twice[name, k, "dev"] else "NO"))
        if holds and name in CANDIDATES:
            in_max = size
    say("LZSS_TILE_IN_MAX by its rule: %s; this build: %d" % (in_max if in_max else "none -- the class is not ready", lz.TILE_IN_MAX))
    group_min = None
    inside = [name for name, size in SIZES if in_max and size <= in_max]
    for k in sorted(ks, reverse=True):
        if inside and all(beats[name, k, form] for name in inside for form in ("host", "dev") if (name, k, form) in beats):
            group_min = k
        else:
            break
    say("LZSS_TILE_GROUP_MIN by its rule (the sizes up to LZSS_TILE_IN_MAX): %s; this build: %d" % (group_min if group_min else "none", lz.TILE_GROUP_MIN))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
