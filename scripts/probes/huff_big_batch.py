"""Huffman batch compress of members above 64 KiB (csrc/huff_big.hip; DESIGN 4.7: HUFF_BIG_IN_MAX, HUFF_BIG_GROUP_MIN): the grouped call
against the loop of single calls on this build and against the same batch call on the PARENT commit's build, same box.

    python scripts/probes/huff_big_batch.py --parent PARENT_LIBRSN [--out FILE] [--k 4,16,64,256]     (default profiles/huff_big_batch.txt)

PARENT_LIBRSN is the parent commit's build of librsn.so (raisin_amd/csrc/Makefile: make BUILD=build_parent OUT=...), loaded through
RSN_LIB_PATH in a child process; this build runs in a child of its own.  A child times every shape -- K members of 128 KiB, 256 KiB and
1 MiB of text (and of 384 and 512 KiB, to place the break-even), and one list of the eleven Canterbury file sizes (text of those sizes: six of them lie in the class, two in the mid class,
three below) -- through rsn_huffman_compress_batch (host) and rsn_huffman_compress_batch_dev (device), and through the loop of
rsn_huffman_compress / rsn_huffman_compress_dev over the same members.  Host wall clock around calls that synchronise before they
return; a warm-up, then five runs; a row is the median and the least and greatest of the five.  The builds' results are compared by digest.
In the parent every member above 64 KiB takes the single call inside the batch.  The class holds where, at every size and every
K >= HUFF_BIG_GROUP_MIN, this build's batch call is faster than both others by more than the spread of their runs: the script says so,
or names the rows where it is not."""
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

SIZES = (("128KiB", 128 << 10), ("256KiB", 256 << 10), ("384KiB", 384 << 10), ("512KiB", 512 << 10), ("1MiB", 1 << 20))   # (384 and 512 KiB: to place the break-even)
CANTERBURY = (152089, 125179, 24603, 11150, 3721, 1029744, 426754, 481861, 513216, 38240, 4227)   # alice29.txt ... xargs.1
WORDS = [b"the", b"quick", b"brown", b"fox", b"jumps", b"over", b"lazy", b"dog", b"compression", b"a", b"I", b"Sam", b"ham", b"green", b"eggs"]


def text(seed, n):
    import numpy as np
    rng = np.random.default_rng(seed)
    words = np.array(WORDS, dtype=object)
    seps = np.array([b" ", b" ", b"\n", b", ", b". "], dtype=object)
    k = n // 2 + 8
    parts = np.empty(2 * k, dtype=object)
    parts[0::2] = words[rng.integers(0, len(words), k)]
    parts[1::2] = seps[rng.integers(0, len(seps), k)]
    return b"".join(parts)[:n]


def ru16(x):
    return (x + 15) // 16 * 16


def five(fn):
    fn()
    ts = []
    for _ in range(5):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return ts


def child(ks):
    """every shape once in this process's build -> one JSON line {key: {"ms": [five], "digest": ...}}"""
    import torch

    from raisin_amd import _lib
    L = _lib.lib()
    _lib.check(L.rsn_device_set(0))
    U8P = ctypes.POINTER(ctypes.c_uint8)
    out = {}
    shapes = [(name, k, [size] * k) for name, size in SIZES for k in ks] + [("canterbury", len(CANTERBURY), list(CANTERBURY))]
    for name, k, sizes in shapes:
        distinct = {}
        datas = []
        for i, n in enumerate(sizes):
            key = (n, i % 8)
            if key not in distinct:
                distinct[key] = text(7919 * (i % 8) + n, n)
            datas.append(distinct[key])
        ins = (ctypes.c_char_p * k)(*datas)
        lens = (ctypes.c_size_t * k)(*sizes)
        outs = (U8P * k)()
        olens = (ctypes.c_size_t * k)()
        one, one_n = U8P(), ctypes.c_size_t()

        def host(keep=False):
            rc = L.rsn_huffman_compress_batch(k, ins, lens, outs, olens)
            assert rc == 0, L.rsn_last_error()
            res = [ctypes.string_at(outs[i], olens[i]) for i in range(k)] if keep else None
            for i in range(k):
                L.rsn_free(outs[i])
            return res

        def host_loop():
            for d, n in zip(datas, sizes):
                rc = L.rsn_huffman_compress(d, n, ctypes.byref(one), ctypes.byref(one_n))
                assert rc == 0, L.rsn_last_error()
                L.rsn_free(one)
        want = host(keep=True)
        caps = [int(L.rsn_huffman_compress_bound(n)) for n in sizes]
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
            rc = L.rsn_huffman_compress_batch_dev(k, arr, dlens, None)
            assert rc == 0, L.rsn_last_error()

        def dev_loop():
            for i in range(k):
                rc = L.rsn_huffman_compress_dev(src.data_ptr() + in_at[i], sizes[i], dst.data_ptr() + out_at[i], caps[i], ctypes.byref(one_n), None)
                assert rc == 0, L.rsn_last_error()
        dev()
        h = dst.cpu().numpy()
        assert [bytes(h[out_at[i]:out_at[i] + dlens[i]]) for i in range(k)] == want
        digest = hashlib.sha256(b"".join(want)).hexdigest()[:16]
        for form, fn, loop in (("host", host, host_loop), ("dev", dev, dev_loop)):
            out["%s %d %s batch" % (name, k, form)] = {"ms": five(fn), "digest": digest}
            out["%s %d %s loop" % (name, k, form)] = {"ms": five(loop), "digest": digest}
        del src, dst
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "huff_big_batch.txt"))
    ap.add_argument("--k", default="4,16,64,256")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    ks = [int(x) for x in a.k.split(",")]
    if a.child:
        return child(ks)
    if not a.parent:
        ap.error("--parent PARENT_LIBRSN is needed: the third column is the parent build's batch call")
    runs = {}
    for build in ("parent", "this"):
        env = dict(os.environ)
        env.pop("RSN_LIB_PATH", None)
        if build == "parent":
            env["RSN_LIB_PATH"] = os.path.abspath(a.parent)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--k", a.k], env=env, capture_output=True, text=True, timeout=1100)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            return 1
        runs[build] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print("%s build: done" % build, flush=True)
    from raisin_amd import huffman
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say("Huffman batch compress, members above 64 KiB: the grouped call, the loop of single calls, the parent commit's batch call -- %s" % time.strftime("%Y-%m-%d"))
    say("ms of host wall clock around synchronising calls: median (min .. max) of five runs after a warm-up, a process a build")
    say("this build: HUFF_BIG_IN_MAX = %d, HUFF_BIG_TILE = %d, HUFF_BIG_GROUP_MIN = %d, groups of %d MiB; parent: every such member takes the single call inside the batch"
        % (huffman.BIG_IN_MAX, huffman.BIG_TILE, huffman.BIG_GROUP_MIN, huffman.BIG_GROUP_BYTES >> 20))
    say()
    say("%-10s %4s %-4s %28s %28s %28s %8s %8s" % ("member", "K", "form", "this call ms", "loop of single calls ms", "parent's call ms", "loop/this", "par/this"))
    fmt = "%9.3f (%8.3f .. %8.3f)"
    med = statistics.median
    not_faster, moved, outside = [], [], set()
    for key in runs["this"]:
        name, k, form, what = key.split()
        if what != "batch":
            continue
        t, lp, par = runs["this"][key]["ms"], runs["this"][key.replace(" batch", " loop")]["ms"], runs["parent"][key]["ms"]
        assert runs["this"][key]["digest"] == runs["parent"][key]["digest"], "the two builds' results differ: " + key
        say("%-10s %4s %-4s %s %s %s %7.1fx %7.1fx" % (name, k, form, fmt % (med(t), min(t), max(t)), fmt % (med(lp), min(lp), max(lp)), fmt % (med(par), min(par), max(par)),
                                                    med(lp) / med(t), med(par) / med(t)))
        if name == "canterbury":
            grouped = sum(1 for n in CANTERBURY if huffman.MID_IN_MAX < n <= huffman.BIG_IN_MAX) >= huffman.BIG_GROUP_MIN
        else:
            grouped = int(k) >= huffman.BIG_GROUP_MIN and dict(SIZES)[name] <= huffman.BIG_IN_MAX
        if not grouped:
            outside.add(name)
        elif not (max(t) < min(lp) and max(t) < min(par)):
            not_faster.append("%s x %s %s" % (k, name, form))
    say()
    say("the single calls, this build against the parent's (the loops above): median ms, this / parent")
    for key in runs["this"]:
        name, k, form, what = key.split()
        if what != "loop":
            continue
        t, par = runs["this"][key]["ms"], runs["parent"][key]["ms"]
        say("%-10s %4s %-4s %9.3f %9.3f %6.2fx   (parent's runs %8.3f .. %8.3f)" % (name, k, form, med(t), med(par), med(t) / med(par), min(par), max(par)))
        if not min(par) * 0.9 <= med(t) <= max(par) * 1.1:
            moved.append("%s x %s %s" % (k, name, form))
    say()
    if outside:
        say("not grouped in this build (above HUFF_BIG_IN_MAX, or fewer members of the class than its minimum): " + ", ".join(sorted(outside)))
    if not_faster:
        say("NOT faster than both others by more than the runs' spread (this call's slowest run against their fastest): " + "; ".join(not_faster))
    else:
        say("at every size and every K >= %d the grouped call's slowest run is faster than the fastest run of the loop and of the parent's call" % huffman.BIG_GROUP_MIN)
    say("single calls outside 0.9 x min .. 1.1 x max of the parent's five runs: " + ("; ".join(moved) if moved else "none"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
