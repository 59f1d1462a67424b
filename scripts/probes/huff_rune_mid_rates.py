"""Huffman batch compress of UTF-8 members of 20 to 64 KiB: this build against the PARENT commit's, same call, same box (DESIGN 4.7:
HUFF_RUNE_MID_GROUP_MIN, HUFF_RUNE_MID_IN_MAX).

    python scripts/probes/huff_rune_mid_rates.py PARENT_LIBRSN [out_file [rounds [bench]]]   (default profiles/huff_rune_mid_batch.txt, 2 rounds)

PARENT_LIBRSN is the parent commit's build of librsn.so (raisin_amd/csrc/Makefile: make BUILD=build_parent OUT=...), loaded through
RSN_LIB_PATH.  The two builds alternate, a process each, `rounds` times (A B A B): a process times every shape -- 4, 8, 16, 64 and 256
members of 20, 32 and 64 KiB of UTF-8 text (ASCII words, one letter in twenty accented), through rsn_huffman_compress_batch (host) and
rsn_huffman_compress_batch_dev (device) -- and, for what must not have moved, ASCII-only members through the same two calls (256 x 16 KiB,
256 x 64 KiB: no kernel they run was edited).  Host wall clock around calls that synchronise before they return, a warm-up and ten runs a
process; a row is the median, least and greatest of a build's runs over all rounds, and both builds' results are compared by digest.  In
the parent every such UTF-8 member takes the single call inside the batch; in this build a call with at least HUFF_RUNE_MID_GROUP_MIN of
them runs k_huff_mid_rune_enc.  A shape is WON when this build's median lies below the parent's by more than the parent's own spread
(max - min) at that shape; the minimum to choose is the smallest count tried, not below 16, that wins at all three sizes in both forms.
With a fourth argument `bench` the flagship benchmark (bench.py --gpus 1 --steps 20 --warmup 3) runs once on each build too, alternating,
for the record.  Every child process has a time limit of its own, and the first that fails ends the probe."""
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
ASCII = ((256, 16 << 10), (256, 64 << 10))
RUNS = 10
WORDS = "the of and to in is that for it as with was on be at by this have from or one had not but what all were when we there can an your which their said if will each about how up out them then she many some so these would other into has more her two like him see time could no make than first been its who now people my made over did down only way find use may water long little very after words called just where most know".split()
ACCENTS = {"a": "à", "e": "é", "i": "ï", "o": "ö", "u": "ü", "n": "ñ", "c": "ç"}


def text(n, seed, ascii_only=False):
    """n bytes of words; but for ascii_only, one letter in twenty that has an accented form takes it (cut between characters, padded with dots)"""
    import random
    rng = random.Random(seed)
    out, size = [], 0
    while size < n + 8:
        w = rng.choice(WORDS) + rng.choice([" ", " ", " ", ", ", ". ", "\n"])
        out.append(w)
        size += len(w)
    s = "".join(out)
    if not ascii_only:
        s = "".join(ACCENTS[ch] if ch in ACCENTS and rng.random() < 0.16 else ch for ch in s)      # (a third of the letters have a form: one in twenty of all)
    b = s.encode()[:n]
    while b and (b[-1] & 0xC0) == 0x80:
        b = b[:-1]
    if b and b[-1] >= 0xC0:
        b = b[:-1]
    return b + b"." * (n - len(b))


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
    """every shape once in this process's build -> one JSON line {key: {"ms": [RUNS], "digest": ...}}"""
    import torch

    from raisin_amd import _lib
    L = _lib.lib()
    _lib.check(L.rsn_device_set(0))
    U8P = ctypes.POINTER(ctypes.c_uint8)
    out = {}
    pool = {}
    shapes = [("utf8", c, s) for s in SIZES for c in COUNTS] + [("ascii", c, s) for c, s in ASCII]
    for kind, k, size in shapes:
        datas = []
        for i in range(k):
            key = (kind, size, i % 16)                                   # sixteen texts a size, told apart by the member's number in front
            if key not in pool:
                pool[key] = text(size - 7, 7919 * size + i % 16, kind == "ascii")
            datas.append(b"%06d " % i + pool[key])
        assert all(len(d) == size and (max(d) >= 0x80) == (kind == "utf8") for d in datas)
        ins = (ctypes.c_char_p * k)(*datas)
        lens = (ctypes.c_size_t * k)(*[size] * k)
        outs = (U8P * k)()
        olens = (ctypes.c_size_t * k)()

        def host(keep=False):
            rc = L.rsn_huffman_compress_batch(k, ins, lens, outs, olens)
            assert rc == 0, L.rsn_last_error()
            res = [ctypes.string_at(outs[i], olens[i]) for i in range(k)] if keep else None
            for i in range(k):
                L.rsn_free(outs[i])
            return res
        want = host(keep=True)
        cap = int(L.rsn_huffman_compress_bound(size))
        src = torch.frombuffer(bytearray(b"".join(d + bytes(ru16(size) - size) for d in datas) + bytes(64)), dtype=torch.uint8).cuda()
        dst = torch.zeros(k * (ru16(cap) + 16) + 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        arr = (_lib.DevMember * k)(*[_lib.DevMember(src.data_ptr() + i * ru16(size), size, dst.data_ptr() + i * (ru16(cap) + 16), cap) for i in range(k)])
        dlens = (ctypes.c_size_t * k)()

        def dev():
            rc = L.rsn_huffman_compress_batch_dev(k, arr, dlens, None)
            assert rc == 0, L.rsn_last_error()
        dev()
        h = dst.cpu().numpy()
        assert [bytes(h[i * (ru16(cap) + 16):][:dlens[i]]) for i in range(k)] == want
        digest = hashlib.sha256(b"".join(want)).hexdigest()[:16]
        out["%s %d %d host" % (kind, k, size)] = {"ms": timed(host), "digest": digest}
        out["%s %d %d dev" % (kind, k, size)] = {"ms": timed(dev), "digest": digest}
        del src, dst
    print("RESULT " + json.dumps(out), flush=True)


def run_child(cmd, env, limit):
    """a child process under its own time limit -> its stdout, or None (what it said goes to stderr)"""
    try:
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=limit, cwd=ROOT)
    except subprocess.TimeoutExpired:
        sys.stderr.write("timed out after %d s: %s\n" % (limit, " ".join(cmd)))
        return None
    if p.returncode != 0:
        sys.stderr.write("exit status %d: %s\n" % (p.returncode, " ".join(cmd)) + p.stdout[-2000:] + p.stderr[-4000:])
        return None
    return p.stdout


def main():
    if sys.argv[1] == "--child":
        return child()
    parent_lib = os.path.abspath(sys.argv[1])
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "huff_rune_mid_batch.txt")
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    bench = len(sys.argv) > 4 and sys.argv[4] == "bench"

    def env_of(build):
        env = dict(os.environ)
        env.pop("RSN_LIB_PATH", None)
        if build == "parent":
            env["RSN_LIB_PATH"] = parent_lib
        return env
    runs = {"parent": {}, "this": {}}
    benches = {"parent": [], "this": []}
    for r in range(rounds):
        for build in ("parent", "this"):
            so = run_child([sys.executable, os.path.abspath(__file__), "--child"], env_of(build), 420)
            if so is None:
                return 1                                                  # (nothing more is started on the device)
            res = json.loads([ln for ln in so.splitlines() if ln.startswith("RESULT ")][-1][7:])
            for key, v in res.items():
                e = runs[build].setdefault(key, {"ms": [], "digest": v["digest"]})
                e["ms"] += v["ms"]
            print("round %d, %s build: done" % (r, build), flush=True)
    if bench:
        for build in ("parent", "this"):
            so = run_child([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3"], env_of(build), 300)
            if so is None:
                return 1
            benches[build].append([ln for ln in so.splitlines() if ln.startswith("{")][-1])
            print("bench, %s build: done" % build, flush=True)
    from raisin_amd import huffman
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say("Huffman batch compress, UTF-8 members of 20 to 64 KiB: this build against the parent commit's -- %s" % time.strftime("%Y-%m-%d"))
    say("ms of host wall clock around synchronising calls: median (min .. max) of %d runs a build, %d alternating processes of %d runs each" % (RUNS * rounds, rounds, RUNS))
    say("this build: HUFF_RUNE_MID_GROUP_MIN = %d, HUFF_RUNE_MID_IN_MAX = %d: a call of at least that many runs k_huff_mid_rune_enc; parent: every member takes the single call inside the batch"
        % (huffman.RUNE_MID_GROUP_MIN, huffman.RUNE_MID_IN_MAX))
    say()
    say("%-6s %-16s %-5s %28s %28s %11s %s" % ("kind", "members", "form", "parent ms", "this build ms", "parent/this", "won"))
    fmt = "%9.3f (%8.3f .. %8.3f)"
    lost = {}
    for key in runs["this"]:
        kind, k, size, form = key.split()
        a, b = runs["parent"][key], runs["this"][key]
        assert a["digest"] == b["digest"], "the two builds' results differ: " + key
        ma, mb = statistics.median(a["ms"]), statistics.median(b["ms"])
        won = ma - mb > max(a["ms"]) - min(a["ms"])
        say("%-6s %-16s %-5s %s %s %10.2fx %s" % (kind, "%s x %s B" % (k, size), form, fmt % (ma, min(a["ms"]), max(a["ms"])), fmt % (mb, min(b["ms"]), max(b["ms"])), ma / mb,
                                                 ("yes" if won else "no") if kind == "utf8" and int(k) >= huffman.RUNE_MID_GROUP_MIN else "-"))
        if kind == "utf8" and int(k) >= 16 and not won:
            lost[int(k)] = lost.get(int(k), []) + ["%s B %s" % (size, form)]
    say()
    wins_from = [c for c in COUNTS if c >= 16 and all(d not in lost for d in COUNTS if d >= c)]
    if wins_from:
        say("smallest count tried, not below 16, from which this build wins at every size and in both forms: %d" % wins_from[0])
    else:
        say("this build does not win at the largest count tried: %s" % lost)
    for c in sorted(lost):
        say("not won at %d members: %s" % (c, ", ".join(lost[c])))
    say("counts below HUFF_RUNE_MID_GROUP_MIN and the ASCII rows run the same kernels in both builds: parent/this is to be read against the rows' own min .. max")
    for build in ("parent", "this"):
        for ln in benches[build]:
            say("bench.py --gpus 1 --steps 20 --warmup 3, %s build: %s" % (build, ln))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
