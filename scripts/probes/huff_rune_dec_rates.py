"""Huffman batch decompress of rune streams: this build against the PARENT commit's, same call, same box (HUFF_RUNE_DEC_GROUP_MIN).

    python scripts/probes/huff_rune_dec_rates.py PARENT_LIBRSN [out_file [rounds [controls]]]     (default profiles/huff_rune_dec_batch.txt, 2 rounds)

PARENT_LIBRSN is the parent commit's build of librsn.so (raisin_amd/csrc/Makefile: make BUILD=build_parent OUT=...), loaded through
RSN_LIB_PATH.  The two builds alternate, a process each, `rounds` times (A B A B): a process times every shape -- the streams of members
of 25 B, 1 KiB and 16 KiB of UTF-8 text, 16, 32, 64, 256 and 4096 of them, through rsn_huffman_decompress_batch (host) and
rsn_huffman_decompress_batch_dev (device) -- and, as controls, the streams of ASCII-only members through the same two calls
(4096 x 1 KiB, 256 x 16 KiB), whose route this build does not change.  Host wall clock around calls that synchronise before they return,
a warm-up and five runs a process; a row is the median, least and greatest of a build's runs over all rounds (two rounds: the median of
ten), and both builds' results are compared by digest.  In the parent every rune stream takes the single call inside the batch; in this
build a call with at least HUFF_RUNE_DEC_GROUP_MIN of them runs k_huff_batch_rune_dec.  The chosen minimum is the smallest count tried
from which this build's median is no greater than the parent's at every size and in both forms; it is never below 16, and counts below
the smallest tried stay not measured.  A fourth argument "controls" times the ASCII rows alone (with more rounds: what a control that
left the other build's range is looked at with)."""
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

SIZES = (25, 1024, 16384)
COUNTS = (16, 32, 64, 256, 4096)
ASCII = ((4096, 1024), (256, 16384))
WORDS = "naïve café déjà vu señor über straße crème brûlée façade jalapeño piñata smörgåsbord the of and to in is that for it as with was on be € — « » “quoted” ’s résumé coöperate Zoë 12 °C".split()


def utf8_text(n, seed, ascii_only=False):
    """n bytes of words (cut between characters, padded with dots)"""
    import random
    rng = random.Random(seed)
    words = [w for w in WORDS if w.isascii()] if ascii_only else WORDS
    out = b""
    while True:
        w = (rng.choice(words) + rng.choice([" ", " ", ", ", ". ", "\n"])).encode()
        if len(out) + len(w) > n:
            return out + b"." * (n - len(out))
        out += w


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


def child(controls=False):
    """every shape once in this process's build -> one JSON line {key: {"ms": [five], "digest": ...}}"""
    import torch

    from raisin_amd import _lib
    L = _lib.lib()
    _lib.check(L.rsn_device_set(0))
    U8P = ctypes.POINTER(ctypes.c_uint8)
    out = {}
    shapes = ([] if controls else [("utf8", c, s) for s in SIZES for c in COUNTS]) + [("ascii", c, s) for c, s in ASCII]
    for kind, k, size in shapes:
        datas = [utf8_text(size, 7919 * size + i, kind == "ascii") for i in range(k)]
        if kind == "utf8":
            assert all(max(d) >= 0x80 for d in datas[:16])
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
        out["%s %d %d host" % (kind, k, size)] = {"ms": five(host), "digest": digest}
        out["%s %d %d dev" % (kind, k, size)] = {"ms": five(dev), "digest": digest}
        del src, dst
    print("RESULT " + json.dumps(out), flush=True)


def main():
    if sys.argv[1] in ("--child", "--child-controls"):
        return child(sys.argv[1] == "--child-controls")
    parent_lib = os.path.abspath(sys.argv[1])
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "huff_rune_dec_batch.txt")
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    controls = len(sys.argv) > 4 and sys.argv[4] == "controls"
    runs = {"parent": {}, "this": {}}
    for r in range(rounds):
        for build in ("parent", "this"):
            env = dict(os.environ)
            env.pop("RSN_LIB_PATH", None)
            if build == "parent":
                env["RSN_LIB_PATH"] = parent_lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-controls" if controls else "--child"], env=env, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
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
    say("Huffman batch decompress, streams of UTF-8 members: this build against the parent commit's -- %s" % time.strftime("%Y-%m-%d"))
    say("ms of host wall clock around synchronising calls: median (min .. max) of %d runs a build, %d alternating processes of five runs each" % (5 * rounds, rounds))
    say("this build: HUFF_RUNE_DEC_GROUP_MIN = %d, so every count below runs k_huff_batch_rune_dec; parent: every rune stream takes the single call inside the batch" % huffman.RUNE_DEC_GROUP_MIN)
    say()
    say("%-6s %-16s %-5s %28s %28s %9s" % ("kind", "members", "form", "parent ms", "this build ms", "parent/this"))
    fmt = "%9.3f (%8.3f .. %8.3f)"
    slower = {}
    for key in runs["this"]:
        kind, k, size, form = key.split()
        a, b = runs["parent"][key], runs["this"][key]
        assert a["digest"] == b["digest"], "the two builds' results differ: " + key
        ma, mb = statistics.median(a["ms"]), statistics.median(b["ms"])
        say("%-6s %-16s %-5s %s %s %8.2fx" % (kind, "%s x %s B" % (k, size), form, fmt % (ma, min(a["ms"]), max(a["ms"])), fmt % (mb, min(b["ms"]), max(b["ms"])), ma / mb))
        if kind == "utf8" and mb > ma:
            slower[int(k)] = slower.get(int(k), []) + ["%s B %s" % (size, form)]
    say()
    ok_from = [c for c in COUNTS if all(d not in slower for d in COUNTS if d >= c)]
    if ok_from:
        say("smallest count tried from which this build is no slower at every size and in both forms: %d" % ok_from[0])
    else:
        say("this build is slower than the parent at the largest count tried: %s" % slower)
    for c in sorted(slower):
        say("slower at %d members: %s" % (c, ", ".join(slower[c])))
    say("ASCII rows: controls -- the byte decoders' route is unchanged (their body gained two template parameters); parent/this is to be read against the rows' own min .. max")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
