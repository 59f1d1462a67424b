"""Huffman batch decompress of rune streams that promise 16 to 64 KiB: this build against the PARENT commit's, same call, same box
(HUFF_RUNE_MID_DEC_GROUP_MIN).

    python scripts/probes/huff_rune_mid_dec_rates.py PARENT_LIBRSN [out_file [rounds]]     (default profiles/huff_rune_mid_dec_batch.txt, 2 rounds)

PARENT_LIBRSN is the parent commit's build of librsn.so (raisin_amd/csrc/Makefile: make BUILD=build_parent OUT=...), loaded through
RSN_LIB_PATH.  The two builds alternate, a process each, `rounds` times (A B A B), every process under its own time limit, and the first
that fails ends the job.  A process times every shape -- the streams of UTF-8 text of 20, 32 and 64 KiB (one accented letter in twenty),
K = 4, 8, 16, 64 and 256 of them, through rsn_huffman_decompress_batch (host) and rsn_huffman_decompress_batch_dev (device) -- and, as rows
that must not move, 256 rune streams of 16 KiB (k_huff_batch_rune_dec, whose unit this build recompiles) and 256 ASCII streams of 64 KiB
(k_huff_mid_dec).  Host wall clock around calls that synchronise before they return, a warm-up and ten runs a process; a row is the median,
least and greatest of a build's runs over all rounds (two rounds: twenty runs), and both builds' results are compared by digest.  In the
parent every such stream takes the single call inside the batch; in this build a call with at least HUFF_RUNE_MID_DEC_GROUP_MIN of them
runs k_huff_mid_rune_dec.  bench.py runs once on each build at the end."""
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

SIZES = (20 << 10, 32 << 10, 64 << 10)
COUNTS = (4, 8, 16, 64, 256)
STILL = (("utf8", 256, 16 << 10), ("ascii", 256, 64 << 10))
RUNS = 10
WORDS = "the quick brown fox jumps over lazy dog naïve café a I Sam déjà vu green eggs and señor would not could in box with house mouse here there über 12 € anywhere compression".split()


def text(n, seed, ascii_only=False):
    """n bytes of words (cut between characters, padded with dots)"""
    import random
    rng = random.Random(seed)
    words = [w for w in WORDS if w.isascii()] if ascii_only else WORDS
    out = [b"%d " % seed]
    size = len(out[0])
    while True:
        w = (rng.choice(words) + rng.choice([" ", " ", " ", "\n", ", ", ". "])).encode()
        if size + len(w) > n:
            return b"".join(out) + b"." * (n - size)
        out.append(w)
        size += len(w)


def ru16(x):
    return (x + 15) // 16 * 16


def timed(fn):
    fn()
    ts = []
    for _ in range(RUNS):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return ts


def child():
    """every shape once in this process's build -> one JSON line {key: {"ms": [...], "digest": ...}}"""
    import torch

    from raisin_amd import _lib
    L = _lib.lib()
    _lib.check(L.rsn_device_set(0))
    U8P = ctypes.POINTER(ctypes.c_uint8)
    out = {}
    for kind, k, size in [("utf8", c, s) for s in SIZES for c in COUNTS] + list(STILL):
        datas = [text(size, 7919 * size + i, kind == "ascii") for i in range(k)]
        assert kind == "ascii" or all(max(d) >= 0x80 for d in datas)
        ins = (ctypes.c_char_p * k)(*datas)
        lens = (ctypes.c_size_t * k)(*[size] * k)
        outs = (U8P * k)()
        olens = (ctypes.c_size_t * k)()
        rc = L.rsn_huffman_compress_batch(k, ins, lens, outs, olens)      # the streams: this process's build writes them, the digests compare them
        assert rc == 0, L.rsn_last_error()
        streams = [ctypes.string_at(outs[i], olens[i]) for i in range(k)]
        for i in range(k):
            L.rsn_free(outs[i])
        ins = (ctypes.c_char_p * k)(*streams)
        lens = (ctypes.c_size_t * k)(*map(len, streams))
        slot = ru16(max(map(len, streams)))

        def host(keep=False):
            rc = L.rsn_huffman_decompress_batch(k, ins, lens, outs, olens)
            assert rc == 0, L.rsn_last_error()
            res = [ctypes.string_at(outs[i], olens[i]) for i in range(k)] if keep else None
            for i in range(k):
                L.rsn_free(outs[i])
            return res
        want = host(keep=True)
        assert want == datas
        cap = ru16(size) + 16                                             # (what the single call asks for)
        src = torch.frombuffer(bytearray(b"".join(d + bytes(slot - len(d)) for d in streams) + bytes(64)), dtype=torch.uint8).cuda()
        dst = torch.zeros(k * (ru16(cap) + 16) + 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        arr = (_lib.DevMember * k)(*[_lib.DevMember(src.data_ptr() + i * slot, len(streams[i]), dst.data_ptr() + i * (ru16(cap) + 16), cap) for i in range(k)])
        dlens = (ctypes.c_size_t * k)()

        def dev():
            rc = L.rsn_huffman_decompress_batch_dev(k, arr, dlens, None)
            assert rc == 0, L.rsn_last_error()
        dev()
        h = dst.cpu().numpy()
        assert [bytes(h[i * (ru16(cap) + 16):][:dlens[i]]) for i in range(k)] == want
        digest = hashlib.sha256(b"".join(streams) + b"".join(want)).hexdigest()[:16]
        out["%s %d %d host" % (kind, k, size)] = {"ms": timed(host), "digest": digest}
        out["%s %d %d dev" % (kind, k, size)] = {"ms": timed(dev), "digest": digest}
        del src, dst
    print("RESULT " + json.dumps(out), flush=True)


def main():
    if sys.argv[1] == "--child":
        return child()
    parent_lib = os.path.abspath(sys.argv[1])
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "huff_rune_mid_dec_batch.txt")
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    runs = {"parent": {}, "this": {}}

    def env_of(build):
        env = dict(os.environ)
        env.pop("RSN_LIB_PATH", None)
        if build == "parent":
            env["RSN_LIB_PATH"] = parent_lib
        return env
    for r in range(rounds):
        for build in ("parent", "this"):
            p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child"], env=env_of(build), capture_output=True, text=True)
            if p.returncode != 0:                                         # (a failure, a fault or the time limit: nothing more is started)
                sys.stderr.write("round %d, %s build: exit %d\n" % (r, build, p.returncode) + p.stdout[-2000:] + p.stderr[-4000:])
                return 1
            res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            for key, v in res.items():
                e = runs[build].setdefault(key, {"ms": [], "digest": v["digest"]})
                e["ms"] += v["ms"]
            print("round %d, %s build: done" % (r, build), flush=True)
    from raisin_amd import huffman
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say("Huffman batch decompress, rune streams that promise 16 to 64 KiB: this build against the parent commit's -- %s" % time.strftime("%Y-%m-%d"))
    say("ms of host wall clock around synchronising calls: median (min .. max) of %d runs a build, %d alternating processes of %d runs each" % (RUNS * rounds, rounds, RUNS))
    say("this build: HUFF_RUNE_MID_DEC_GROUP_MIN = %d, so K >= that runs k_huff_mid_rune_dec; parent: every such stream takes the single call inside the batch" % huffman.RUNE_MID_DEC_GROUP_MIN)
    say()
    say("%-6s %-16s %-5s %28s %28s %9s" % ("kind", "members", "form", "parent ms", "this build ms", "parent/this"))
    fmt = "%9.3f (%8.3f .. %8.3f)"
    notes = []
    still = {(kind, k, size) for kind, k, size in STILL}
    for key in runs["this"]:
        kind, k, size, form = key.split()
        a, b = runs["parent"][key], runs["this"][key]
        assert a["digest"] == b["digest"], "the two builds' results differ: " + key
        ma, mb = statistics.median(a["ms"]), statistics.median(b["ms"])
        say("%-6s %-16s %-5s %s %s %8.2fx" % (kind, "%s x %s B" % (k, size), form, fmt % (ma, min(a["ms"]), max(a["ms"])), fmt % (mb, min(b["ms"]), max(b["ms"])), ma / mb))
        inside = min(a["ms"]) <= mb <= max(a["ms"]) and min(b["ms"]) <= ma <= max(b["ms"])
        spread = max(a["ms"]) - min(a["ms"])
        if (kind, int(k), int(size)) in still:
            notes.append("must not move, %s: each build's median %s the other's min .. max" % (key, "inside" if inside else "NOT inside"))
        elif int(k) < huffman.RUNE_MID_DEC_GROUP_MIN:
            notes.append("below the minimum, %s: the medians differ by %.3f ms, the parent's spread is %.3f ms -- %s" % (key, abs(ma - mb), spread, "within" if abs(ma - mb) <= spread else "NOT within"))
        elif int(k) == 16:
            notes.append("at 16, %s: this build wins by %.3f ms, the parent's spread is %.3f ms -- %s" % (key, ma - mb, spread, "more than the spread" if ma - mb > spread else "NOT more than the spread"))
    say()
    for s in notes:
        say(s)
    say()
    for build in ("parent", "this"):                                      # the flagship benchmark, once on each build: no flat kernel changes
        p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3"], env=env_of(build), capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write("bench.py, %s build: exit %d\n" % (build, p.returncode) + p.stdout[-2000:] + p.stderr[-4000:])
            return 1
        say("bench.py --gpus 1 --steps 20 --warmup 3, %s build: %s" % (build, p.stdout.strip().splitlines()[-1]))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
