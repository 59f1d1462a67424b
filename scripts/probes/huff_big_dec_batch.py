"""Huffman batch decompress of streams that promise more than 64 KiB (csrc/huff_big_dec.hip; DESIGN 4.7: HUFF_BIG_OUT_MAX,
HUFF_BIG_DEC_GROUP_MIN): the grouped call against the loop of single calls on this build and against the same batch call on the PARENT
commit's build, same box.

    python scripts/probes/huff_big_dec_batch.py --parent PARENT_LIBRSN [--out FILE] [--k 2,4,16,64,256]     (default profiles/huff_big_dec_batch.txt)

PARENT_LIBRSN is the parent commit's build of librsn.so (raisin_amd/csrc/Makefile: make BUILD=build_parent OUT=...), loaded through
RSN_LIB_PATH in a child process; this build runs in a child of its own.  A child times every shape -- K streams of 96 KiB, 128 KiB and
256 KiB of text -- through rsn_huffman_decompress_batch (host) and rsn_huffman_decompress_batch_dev (device), and through the loop of
rsn_huffman_decompress / rsn_huffman_decompress_dev over the same streams; then 200 single calls of rsn_huffman_decompress at 64, 128 and
256 KiB, which this change must not have moved.  Host wall clock around calls that synchronise before they return; a warm-up, then five
runs; a row is the median and the least and greatest of the five.  The builds' results are compared by digest.  Every child runs with
glibc's malloc thresholds pinned at their defaults (MALLOC_MMAP_THRESHOLD_ = MALLOC_TRIM_THRESHOLD_ = 128 KiB), so that a cell does not
depend on what earlier cells freed: unpinned, glibc raises both after the first large free, and the 256 results of 256 KiB that a batch
call returns (64 MiB, the caller's to free) are then trimmed off the heap's top by the frees and faulted in again by every call -- 39 ms
a call instead of 19, in whichever build.  In the parent every
such stream takes the single call inside the batch.  The script reports the smallest K from which on, at every size and in both forms,
this build's slowest run beats the fastest run of both the loop and the parent's call -- the rule HUFF_BIG_DEC_GROUP_MIN is set by --
and names the rows where a K at or above the minimum in force does not."""
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

SIZES = (("96KiB", 96 << 10), ("128KiB", 128 << 10), ("256KiB", 256 << 10))
SINGLE = (("64KiB", 64 << 10), ("128KiB", 128 << 10), ("256KiB", 256 << 10))
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
    one, one_n = U8P(), ctypes.c_size_t()

    def compress(d):
        rc = L.rsn_huffman_compress(d, len(d), ctypes.byref(one), ctypes.byref(one_n))
        assert rc == 0, L.rsn_last_error()
        s = ctypes.string_at(one, one_n.value)
        L.rsn_free(one)
        return s
    for name, size in SIZES:
        distinct = [text(7919 * i + size, size) for i in range(8)]
        coded = [compress(d) for d in distinct]
        for k in ks:
            datas = [distinct[i % 8] for i in range(k)]
            streams = [coded[i % 8] for i in range(k)]
            lens_in = [len(s) for s in streams]
            ins = (ctypes.c_char_p * k)(*streams)
            lens = (ctypes.c_size_t * k)(*lens_in)
            outs = (U8P * k)()
            olens = (ctypes.c_size_t * k)()

            def host(keep=False):
                rc = L.rsn_huffman_decompress_batch(k, ins, lens, outs, olens)
                assert rc == 0, L.rsn_last_error()
                res = [ctypes.string_at(outs[i], olens[i]) for i in range(k)] if keep else None
                for i in range(k):
                    L.rsn_free(outs[i])
                return res

            def host_loop():
                for s, n in zip(streams, lens_in):
                    rc = L.rsn_huffman_decompress(s, n, ctypes.byref(one), ctypes.byref(one_n))
                    assert rc == 0, L.rsn_last_error()
                    L.rsn_free(one)
            assert host(keep=True) == datas
            caps = [ru16(size) + 16] * k
            in_at, out_at, a, b = [], [], 0, 0
            for n, c in zip(lens_in, caps):
                in_at.append(a); out_at.append(b)
                a += ru16(n); b += ru16(c) + 16
            src = torch.frombuffer(bytearray(b"".join(s + bytes(ru16(len(s)) - len(s)) for s in streams) + bytes(64)), dtype=torch.uint8).cuda()
            dst = torch.zeros(b + 16, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            arr = (_lib.DevMember * k)(*[_lib.DevMember(src.data_ptr() + in_at[i], lens_in[i], dst.data_ptr() + out_at[i], caps[i]) for i in range(k)])
            dlens = (ctypes.c_size_t * k)()

            def dev():
                rc = L.rsn_huffman_decompress_batch_dev(k, arr, dlens, None)
                assert rc == 0, L.rsn_last_error()

            def dev_loop():
                for i in range(k):
                    rc = L.rsn_huffman_decompress_dev(src.data_ptr() + in_at[i], lens_in[i], dst.data_ptr() + out_at[i], caps[i], ctypes.byref(one_n), None)
                    assert rc == 0, L.rsn_last_error()
            dev()
            h = dst.cpu().numpy()
            assert [bytes(h[out_at[i]:out_at[i] + dlens[i]]) for i in range(k)] == datas
            digest = hashlib.sha256(b"".join(datas)).hexdigest()[:16]
            for form, fn, loop in (("host", host, host_loop), ("dev", dev, dev_loop)):
                out["%s %d %s batch" % (name, k, form)] = {"ms": five(fn), "digest": digest}
                out["%s %d %s loop" % (name, k, form)] = {"ms": five(loop), "digest": digest}
            del src, dst
    for name, size in SINGLE:                                                 # the single call, 200 times: five runs of it
        s = compress(text(31 + size, size))

        def calls():
            for _ in range(200):
                rc = L.rsn_huffman_decompress(s, len(s), ctypes.byref(one), ctypes.byref(one_n))
                assert rc == 0, L.rsn_last_error()
                L.rsn_free(one)
        out["%s 200 host single" % name] = {"ms": five(calls), "digest": hashlib.sha256(s).hexdigest()[:16]}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "huff_big_dec_batch.txt"))
    ap.add_argument("--k", default="2,4,16,64,256")
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
        env.update(MALLOC_MMAP_THRESHOLD_="131072", MALLOC_TRIM_THRESHOLD_="131072")    # (set: glibc stops adjusting them)
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
    say("Huffman batch decompress, streams that promise more than 64 KiB: the grouped call, the loop of single calls, the parent commit's batch call -- %s" % time.strftime("%Y-%m-%d"))
    say("ms of host wall clock around synchronising calls: median (min .. max) of five runs after a warm-up, a process a build")
    say("this build: HUFF_BIG_OUT_MAX = %d, tiles of %d lanes of %d bits, HUFF_BIG_DEC_GROUP_MIN = %d, groups of %d MiB; parent: every such stream takes the single call inside the batch"
        % (huffman.BIG_OUT_MAX, huffman.BIG_DEC_LANES, huffman.BIG_DEC_LANE_BITS, huffman.BIG_DEC_GROUP_MIN, huffman.BIG_GROUP_BYTES >> 20))
    say()
    say("%-10s %4s %-4s %28s %28s %28s %8s %8s" % ("member", "K", "form", "this call ms", "loop of single calls ms", "parent's call ms", "loop/this", "par/this"))
    fmt = "%9.3f (%8.3f .. %8.3f)"
    med = statistics.median
    wins, not_faster, moved = {}, [], []
    for key in runs["this"]:
        name, k, form, what = key.split()
        if what != "batch":
            continue
        t, lp, par = runs["this"][key]["ms"], runs["this"][key.replace(" batch", " loop")]["ms"], runs["parent"][key]["ms"]
        assert runs["this"][key]["digest"] == runs["parent"][key]["digest"], "the two builds' results differ: " + key
        say("%-10s %4s %-4s %s %s %s %7.1fx %7.1fx" % (name, k, form, fmt % (med(t), min(t), max(t)), fmt % (med(lp), min(lp), max(lp)), fmt % (med(par), min(par), max(par)),
                                                    med(lp) / med(t), med(par) / med(t)))
        won = max(t) < min(lp) and max(t) < min(par)
        wins.setdefault(int(k), []).append(won)
        if int(k) >= huffman.BIG_DEC_GROUP_MIN and dict(SIZES)[name] <= huffman.BIG_OUT_MAX and not won:
            not_faster.append("%s x %s %s" % (k, name, form))
    say()
    say("the single call, 200 times: median ms of five runs, this build against the parent's")
    for key in runs["this"]:
        name, k, form, what = key.split()
        if what != "single":
            continue
        t, par = runs["this"][key]["ms"], runs["parent"][key]["ms"]
        say("%-10s %4s %-4s %9.3f %9.3f %6.2fx   (parent's runs %8.3f .. %8.3f)" % (name, k, form, med(t), med(par), med(t) / med(par), min(par), max(par)))
        if not min(par) <= med(t) <= max(par):
            moved.append("%s (%.3f against %.3f .. %.3f)" % (name, med(t), min(par), max(par)))
    say()
    floor = None                                                              # the smallest measured K from which on every row wins
    for k in sorted(wins, reverse=True):
        if not all(wins[k]):
            break
        floor = k
    say("smallest measured K from which on this call's slowest run beats the fastest run of the loop and of the parent's call, at every size, in both forms: %s"
        % (floor if floor is not None else "none"))
    if huffman.BIG_DEC_GROUP_MIN > min(ks):
        say("(below HUFF_BIG_DEC_GROUP_MIN = %d this build's call IS the single calls: those rows compare like with like)" % huffman.BIG_DEC_GROUP_MIN)
    if not_faster:
        say("NOT faster than both others by more than the runs' spread at K >= %d: %s" % (huffman.BIG_DEC_GROUP_MIN, "; ".join(not_faster)))
    else:
        say("at every size and every K >= %d the grouped call's slowest run is faster than the fastest run of the loop and of the parent's call" % huffman.BIG_DEC_GROUP_MIN)
    say("single calls whose median lies outside the parent's own min .. max of five runs: " + ("; ".join(moved) if moved else "none"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
