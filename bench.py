#!/usr/bin/env python3
"""bench.py -- headline benchmark: BASELINE.json configs[1] (config 5's per-GPU chunk when --gpus > 1).

  python bench.py --gpus N --steps K --warmup W          (N > 1 without a launcher: bench.py starts its N ranks itself)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

Timed workload (per GPU): `-algorithm=huffman` on a 1 GiB uniform-random buffer (config "2a": bytes uniform
over 0x00..0x7F so that the reference's rune-level Huffman is lossless; splitmix64 seed 0x5EED0002, rank r
uses 0x5EED0050+r when N > 1 -- workloads.py).  A step is what the reference's BenchmarkFile times
(engine/engine.go:379-406): compress, then decompress, of one buffer, input already resident in HBM.
value = uncompressed MB (1e6 B) through encode+decode per second, whole job.

A plain run sets up, warms up, times --steps steps and prints the line (with the per-kernel times that librsn's events
record inside the timed steps).  `--dump-outputs DIR` then also writes what the last timed step returned -- the compressed
stream and the decoded buffer -- as float32 .npy files: the first MiB of each, 2^22 bytes at seeded positions and the
length (DIR/<output>_head.npy, _sample.npy, _size.npy), so that two builds can be compared output for output.

Everything else runs with `--full` only.  After the timed region: the HBM calibration (torch copy and read passes);
for N > 1 configs[4]'s eight chunks dealt over the ranks and the segment gather; for N = 1 the headline's CPU
baseline, and every other BASELINE config runs at the same size and is reported under
`other_configs`: 2b (uniform 0x00..0xFF: the rune path, lossy exactly like the reference), `skewed` (unequal code
lengths: the general Huffman kernels), 3 (`lzss`, 4096-periodic), 4 (`lzss,huffman` on Zipf text) -- each with
encode/decode ms, ratio, lossless, a bit-exact check against the oracle on a sample, the dominant kernel, the
algorithmic-byte fractions of the HBM peak and its own threaded CPU baseline -- and config 1, the host-buffer
rates, the general Huffman path on 2a and the CLI's cold start.

Kernel timings come from HIP events recorded by librsn on its own launch stream (rsn_prof_*), live inside the
timed region.  The CPU baseline is oracle/cpu_baseline.c -- the C restatement of the reference (the reference is
Go and cannot run here: kind "port") on all host cores, on a bounded sample, on rank 0.
"""
import argparse
import statistics
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

OTHER_PASSES = 5           # timed passes per entry of other_configs (after one warm-up pass)
HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec peak (guides/MI355X_MICROARCH.md)


# librsn's profiling names of the headline (flat-code) kernels -> the kernel's name in a rocprofv3 trace
TRACE_NAME = {"huff_emit": "k_emit_flat", "huff_dec_flat": "k_dec_flat", "huff_byte_hist": "k_byte_hist"}


def load_traffic(prof_name):
    """HBM bytes per launch of one headline kernel from the newest committed PMC summary of the HEADLINE workload
    (profiles/<tag>_pmc_headline.json: scripts/profile.sh <tag> headline + summarize_prof.py -- FETCH_SIZE doubled per the gfx950
    note + WRITE_SIZE, separate passes, the kernel's largest launch): a constant of that profile, not a measurement of this run;
    the file's name is reported next to it."""
    import glob
    want = TRACE_NAME.get(prof_name)
    best = None
    for p in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_headline.json"))):
        try:
            d = json.load(open(p))
        except Exception:
            continue
        for k, v in d.items():
            if want and k.startswith(want) and isinstance(v, dict) and v.get("hbm_max"):
                best = (v["hbm_max"], os.path.basename(p))
    if best is None:                                     # the older summaries (r01/r02: one mean per kernel name)
        for p in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc.json"))):
            try:
                d = json.load(open(p))
            except Exception:
                continue
            for k, v in d.items():
                if want and k.startswith(want):
                    best = (v, os.path.basename(p))
    return best


# librsn profiling name -> candidate kernel names in a rocprofv3 trace (the first one the workload's PMC summary holds is used)
TRACE_CANDIDATES = {
    "huff_emit": ["k_emit_flat", "k_emit_ascii32", "k_emit<"], "huff_emit_rune": ["k_emit<"], "huff_emit_wide": ["k_emit<"],
    "huff_byte_hist": ["k_byte_hist"], "huff_rune_hist": ["k_rune_hist"], "huff_tile_bits_rune": ["k_tile_bits_rune"],
    "huff_dec_flat": ["k_dec_flat"], "huff_dec_emit": ["k_dec_emit"], "huff_dec_sync": ["k_dec_sync"], "huff_dec_fused": ["k_dec_fused"],
    "lzss_match_chain": ["k_match_chain"], "lzss_match_hash": ["k_match_hash"], "lzss_match": ["k_match2", "k_match"],
    "lzss_tok_emit": ["k_tok_emit"], "lzss_esc_write": ["k_esc_try", "k_esc_write"], "lzss_esc_check": ["k_esc_try"], "lzss_tile_periodic": ["k_tile_periodic"],
    "lzss_chain_tail": ["k_chain_serial", "k_chain_tail"], "lzss_dec_resolve": ["k_lzd_resolve"], "lzss_dec_emit": ["k_lzd_emit"],
    "lzss_dec_count": ["k_lzd_count2", "k_lzd_count"], "lzss_dec_compose": ["k_lzd_compose"], "lzss_dec_runs": ["k_lzd_runs"],
    "lzss_dec_lit": ["k_lzd_lit"], "lzss_dec_patch": ["k_lzd_patch"], "lzss_dec_run_fill": ["k_lzd_run_fill"], "lzss_periodic_tail": ["k_periodic_tail"],
}
PMC_LABEL = {"2b": "2b", "skewed": "skewed", "3": "config3", "4": "config4", "5": "5", "headline": "headline"}


def workload_traffic(workload, prof_name):
    """HBM bytes (FETCH_SIZE doubled + WRITE_SIZE, the kernel's largest launch) of one kernel in ONE workload's newest committed
    PMC summary, profiles/<tag>_pmc_<label>.json (scripts/profile.sh <tag> <label>): (bytes, file) or None."""
    import glob
    label = PMC_LABEL.get(workload, workload)
    for p in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_%s.json" % label)), reverse=True):
        try:
            d = json.load(open(p))
        except Exception:
            continue
        for cand in TRACE_CANDIDATES.get(prof_name, ["k_" + prof_name.split("_", 1)[-1]]):
            hits = [v for k, v in d.items() if k.startswith(cand) and isinstance(v, dict) and v.get("hbm_max")]
            if hits:
                return max(h["hbm_max"] for h in hits), os.path.basename(p)
    return None


VALU_BOUND_FROM = 0.6     # a kernel whose vector instructions alone account for this share of its duration is priced as issue-bound


def valu_issue(workload, prof_name):
    """Vector-issue share of one kernel in the workload's newest committed SQ-counter summary (profiles/<tag>_valu_<label>.txt,
    scripts/pmc_valu.sh: SQ_INSTS_VALU of the kernel's largest launch x 3.5 cycles / 1024 SIMDs / its duration; a wave64 integer
    VALU instruction holds its SIMD 3.4-5.0 cycles, scripts/valu_probe.cpp): (share, file) or None.  A constant of that profile."""
    import glob
    label = PMC_LABEL.get(workload, workload)
    for p in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_valu_%s.txt" % label)), reverse=True):
        try:
            rows = open(p).read().splitlines()[1:]
        except Exception:
            continue
        for cand in TRACE_CANDIDATES.get(prof_name, ["k_" + prof_name.split("_", 1)[-1]]):
            for row in rows:
                if row.startswith(cand):
                    try:
                        return float(row.split()[-1]), os.path.basename(p)
                    except ValueError:
                        pass
    return None


def roofline_of(workload, prof_name, alg_bytes, ms):
    """The bench line's roofline object for one kernel of one workload: achieved = ALGORITHMIC bytes / the kernel's average launch
    duration (HIP events on librsn's stream, this run); traffic = that kernel's PMC bytes in the workload's committed profile.
    SURVEY 8(d): LZSS encode is VALU / LDS-compare-bound -- a kernel whose committed SQ counters say vector issue fills its time is
    labelled "valu", with that share, and keeps its fraction of the HBM peak beside it."""
    tr = workload_traffic(workload, prof_name)
    vi = valu_issue(workload, prof_name)
    ach = alg_bytes / ms / 1e6 if ms > 0 else 0.0
    out = {"kernel": prof_name, "bound": "valu" if vi and vi[0] >= VALU_BOUND_FROM else "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
           "frac": round(ach / HBM_PEAK_GBPS, 5), "traffic": tr[0] if tr else None,
           "traffic_source": ("profiles/" + tr[1]) if tr else None, "algorithmic_bytes": int(alg_bytes)}
    if vi:
        out["valu_issue_frac"] = vi[0]
        out["valu_source"] = "profiles/" + vi[1]
        if out["bound"] == "valu":
            out["note"] = "vector-issue-bound: `frac` is the algorithmic bytes against the HBM peak, which is not what limits this kernel"
    return out


# ---------------------------------------------------------------------------------------------- CPU baselines
def _timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t0


def _grow(run, sizes_mib, target_s):
    """Runs `run(mib)` on growing samples until one takes long enough to be a measurement (or the list ends)."""
    res = None
    for mib in sizes_mib:
        res = run(mib)
        if res["seconds"] >= target_s / 4:
            break
    return res


def cpu_huffman(make_sample, cores, target_s=10.0):
    """Threaded oracle: encode + decode of one buffer (engine.go:379-406 times both together)."""
    from oracle import oracle as O

    def run(mib):
        s = make_sample(mib << 20)
        c, te = _timed(lambda: O.huffman_compress_mt(s, cores))
        d, td = _timed(lambda: O.huffman_decompress_mt(c, cores))
        return {"value": round(len(s) / 1e6 / (te + td), 2), "unit": "MB/s", "cores": cores, "kind": "port",
                "sample": "%d MiB prefix of the same buffer: oracle/cpu_baseline.c on %d threads, encode %.2f s + decode %.2f s"
                          % (mib, cores, te, td),
                "encode_MBps": round(len(s) / 1e6 / te, 2), "decode_MBps": round(len(s) / 1e6 / td, 2),
                "seconds": te + td, "_c": c, "_s": s}
    return _grow(run, (32, 128, 512), target_s)


def cpu_lzss(make_sample, cores, window=4096, target_s=10.0, sizes=(2, 8, 32, 128)):
    """Threaded oracle in the reference's own shape (a Reference for every position in parallel, serial compaction,
    lzss.go:117-151), serial decode (lzss.go:323-364); plus the lazy single-thread form for context."""
    from oracle import oracle as O

    def run(mib):
        s = make_sample(mib << 20)
        c, te = _timed(lambda: O.lzss_compress_mt(s, window, cores, 4096))
        d, td = _timed(lambda: O.lzss_decompress(c))
        return {"value": round(len(s) / 1e6 / (te + td), 2), "unit": "MB/s", "cores": cores, "kind": "port",
                "sample": "%d MiB prefix of the same buffer: every-position match table on %d threads + serial compaction "
                          "%.2f s, serial decode %.2f s" % (mib, cores, te, td),
                "encode_MBps": round(len(s) / 1e6 / te, 2), "decode_MBps": round(len(s) / 1e6 / td, 2),
                "seconds": te + td, "_c": c, "_s": s}
    return _grow(run, sizes, target_s)


def cpu_lzss_per_position(make_sample, cores, mib=1):
    """The reference's goroutine-per-byte shape taken literally: one task per position (lzss.go:117-130)."""
    from oracle import oracle as O
    s = make_sample(mib << 20)
    _, t = _timed(lambda: O.lzss_compress_mt(s, 4096, cores, 1))
    _, tl = _timed(lambda: O.lzss_compress(s, 4096))
    return {"one_task_per_position_MBps": round(len(s) / 1e6 / t, 2), "lazy_single_thread_MBps": round(len(s) / 1e6 / tl, 2),
            "sample_MiB": mib, "cores": cores}


def _public(d):
    return {k: v for k, v in d.items() if not k.startswith("_") and k != "seconds"}


# ---------------------------------------------------------------------------------------------- other configs
ALG_NOTE = "algorithmic HBM bytes (SURVEY.md 8d): huffman encode 2N+C, decode C+N_out; lzss encode N+C, decode C+N"


def run_other_configs(torch, device, n, cores, with_cpu, names):
    import workloads as W
    from oracle import oracle as O
    from raisin_amd import _lib, huffman, lz
    out = {}

    def gpu_bytes(t):
        return bytes(t.cpu().numpy())

    def one(name):
        src = W.config_input(name, n, device)
        layers = {"2a": ["huffman"], "2b": ["huffman"], "skewed": ["huffman"], "3": ["lzss"], "4": ["lzss", "huffman"]}[name]
        enc = {"huffman": huffman.compress_tensor, "lzss": lz.compress_tensor}
        dec = {"huffman": huffman.decompress_tensor, "lzss": lz.decompress_tensor}

        ebuf, dbuf = {}, {}                                 # output buffers, sized by the warm-up pass and reused by the timed passes

        def compress(x, bufs=None):                         # engine.go:443-452: layers in order
            sizes = []
            for i, a in enumerate(layers):
                x = enc[a](x, out=bufs.get(i) if bufs else None)
                sizes.append(int(x.numel()))
            return x, sizes

        def decompress(x, bufs=None):                       # engine.go:454-479: layers in reverse
            outs = []
            for i, a in enumerate(reversed(layers)):
                x = dec[a](x, out=bufs.get(i) if bufs else None)
                outs.append(int(x.numel()))
            return x, outs

        c, wsz = compress(src)                              # warm-up: scratch arenas grow here, not in the timed pass
        d, dsz = decompress(c)
        del c, d
        for i, m in enumerate(wsz):
            ebuf[i] = torch.empty(m + (1 << 16), dtype=torch.uint8, device=device)
        for i, m in enumerate(dsz):
            dbuf[i] = torch.empty(m + (1 << 16), dtype=torch.uint8, device=device)
        torch.cuda.synchronize(device)
        reps = OTHER_PASSES
        tes, tds = [], []
        for _ in range(reps):                               # the timed passes: no events around the launches (r05: with them a call of a
            (c, sizes), t = _timed(lambda: compress(src, ebuf))   # dozen launches read 0.1-0.2 ms long -- config 3: 1.05 against 0.88 ms);
            tes.append(t * 1e3)                                   # the C ABI calls return after their stream has been synchronised
            (d, _), t = _timed(lambda: decompress(c, dbuf))
            tds.append(t * 1e3)
        _lib.prof_enable(True)                              # ... then one pass each way under the library's events, for the kernels' share
        _lib.prof_reset()
        compress(src, ebuf)
        prof_e = _lib.prof_get()
        _lib.prof_reset()
        decompress(c, dbuf)
        prof_d = _lib.prof_get()
        _lib.prof_enable(False)
        te, td = statistics.median(tes), statistics.median(tds)     # (the entry's times are the MEDIANS; min and the passes ride along)
        C, n_out = int(c.numel()), int(d.numel())
        lossless = bool(n_out == n and torch.equal(d, src))
        # algorithmic bytes of the whole call(s)
        if name == "4":
            l1 = sizes[0]
            alg_e, alg_d = (n + l1) + (2 * l1 + C), (C + l1) + (l1 + n)
        elif layers == ["lzss"]:
            alg_e, alg_d = n + C, C + n
        else:
            alg_e, alg_d = 2 * n + C, C + n_out
        ent = {
            "algorithm": ",".join(layers), "bytes": n, "encode_ms": round(te, 3), "decode_ms": round(td, 3),
            "round_trip_MBps": round(n / 1e6 / ((te + td) / 1e3), 1), "ratio_pct": round(100.0 * C / n, 3), "lossless": lossless,
            "decoded_bytes": n_out,
            "passes": reps, "encode_ms_min": round(min(tes), 3), "decode_ms_min": round(min(tds), 3),
            "encode_ms_all": [round(x, 3) for x in tes], "decode_ms_all": [round(x, 3) for x in tds],
            "encode_frac_of_hbm_peak": round(alg_e / (te / 1e3) / 1e9 / HBM_PEAK_GBPS, 5),
            "decode_frac_of_hbm_peak": round(alg_d / (td / 1e3) / 1e9 / HBM_PEAK_GBPS, 5),
            "kernels_encode_ms": {k: round(v[1], 3) for k, v in sorted(prof_e.items())},
            "kernels_decode_ms": {k: round(v[1], 3) for k, v in sorted(prof_d.items())},
        }
        # the split VERDICT r5 #8 asks for (2b: most of a call is the host's Go-exact tree, not the kernels): kernel time under the library's
        # events in a pass of its own, and what is left of the timed passes' median -- host work, launches, round trips
        ke, kd = sum(v[1] for v in prof_e.values()), sum(v[1] for v in prof_d.values())
        ent["encode_kernels_ms"], ent["decode_kernels_ms"] = round(ke, 3), round(kd, 3)
        ent["encode_host_and_launch_ms"], ent["decode_host_and_launch_ms"] = round(max(te - ke, 0.0), 3), round(max(td - kd, 0.0), 3)
        if name == "4":
            ent["layer_sizes"] = sizes
        allk = {**{k: v[1] for k, v in prof_e.items()}, **{k: v[1] for k, v in prof_d.items()}}
        dom = max(allk, key=allk.get)
        kalg = {"huff_byte_hist": n, "huff_rune_hist": n, "huff_tile_bits_rune": n, "huff_emit": n + C, "huff_emit_rune": n + C,
                "huff_dec_sync": C, "huff_dec_emit": C + n_out, "huff_dec_flat": C + n_out}
        if name in ("3", "4"):
            kalg.update({"lzss_match_chain": n, "lzss_match_hash": n, "lzss_match": n})   # reads the (escaped) stream once
        ent["dominant_kernel"] = {"name": dom, "ms": round(allk[dom], 3)}
        if name == "4":                                     # layered: the Huffman layer's kernels work on the LZSS stream (l1 bytes)
            kalg.update({"huff_byte_hist": l1, "huff_rune_hist": l1, "huff_tile_bits_rune": l1, "huff_emit": l1 + C, "huff_emit_rune": l1 + C,
                         "huff_dec_sync": C, "huff_dec_emit": C + l1, "huff_dec_flat": C + l1})
        if name in ("3", "4"):
            lc = sizes[0]                                   # the LZSS stream
            kalg.update({"lzss_tok_emit": n + lc, "lzss_esc_write": n, "lzss_esc_check": n, "lzss_tile_periodic": n, "lzss_dec_resolve": lc + n, "lzss_dec_emit": lc + n,
                         "lzss_dec_count": lc, "lzss_dec_lit": lc + n, "lzss_dec_patch": n, "lzss_dec_run_fill": lc + n})
        launches = {**{k: v[0] for k, v in prof_e.items()}, **{k: v[0] for k, v in prof_d.items()}}
        if dom in kalg:
            # allk holds the kernel's TOTAL ms in the last timed pass; a kernel launched several times in a call (second looks over
            # a handful of tiles) is priced at the whole call's time for the whole call's algorithmic bytes
            ent["dominant_kernel"]["algorithmic_bytes"] = kalg[dom]
            ent["dominant_kernel"]["launches"] = launches.get(dom)
            ent["dominant_kernel"]["frac_of_hbm_peak"] = round(kalg[dom] / (allk[dom] / 1e3) / 1e9 / HBM_PEAK_GBPS, 5)
            ent["roofline"] = roofline_of(name, dom, kalg[dom], allk[dom])
        else:
            ent["roofline"] = {"kernel": dom, "bound": "hbm", "achieved": None, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": None,
                               "traffic": (workload_traffic(name, dom) or [None])[0]}
        # bit-exact against the oracle on a sample (prefix of the same buffer), through the same layers
        smp = {"2a": 32 << 20, "2b": 32 << 20, "skewed": 32 << 20, "3": 2 << 20, "4": 8 << 20}[name]
        smp = min(smp, n)
        pre = src[:smp].contiguous()
        got, _ = compress(pre)
        ref = gpu_bytes(pre)
        for a in layers:
            ref = O.huffman_compress(ref) if a == "huffman" else O.lzss_compress(ref, 4096)
        ent["bit_exact_vs_oracle_on_sample"] = bool(gpu_bytes(got) == ref)
        ent["oracle_sample_MiB"] = smp >> 20
        if with_cpu:
            def make(k, src=src):
                return gpu_bytes(src[:min(k, n)])
            if layers == ["huffman"]:
                ent["cpu_baseline"] = _public(cpu_huffman(make, cores, target_s=6.0))
            elif layers == ["lzss"]:
                ent["cpu_baseline"] = _public(cpu_lzss(make, cores, sizes=(1, 4, 16), target_s=6.0))
            else:                                          # layered: lzss on the sample, huffman on ITS output, both timed
                r1 = cpu_lzss(make, cores, target_s=6.0)
                l1c = r1["_c"]
                c2, t2e = _timed(lambda: O.huffman_compress_mt(l1c, cores))
                _, t2d = _timed(lambda: O.huffman_decompress_mt(c2, cores))
                tot = r1["seconds"] + t2e + t2d
                ent["cpu_baseline"] = {"value": round(len(r1["_s"]) / 1e6 / tot, 2), "unit": "MB/s", "cores": cores, "kind": "port",
                                       "sample": r1["sample"] + "; huffman layer on its output: encode %.2f s + decode %.2f s" % (t2e, t2d),
                                       "lzss_layer_MBps": r1["value"]}
                ent["cpu_lzss_shape"] = cpu_lzss_per_position(make, cores)
        out[name] = ent
        del src, c, d, ebuf, dbuf
        torch.cuda.empty_cache()

    def chunks_on_one_gpu(k=8):
        """Config 5 as one GPU sees it: k independent chunks (seeds 0x5EED0050 + i), one complete .rsn segment each, encoded one
        after the other (engine.CompressFiles' loop, engine.go:150-154); the multi-GPU form is `bench.py --gpus N`.
        Inputs and outputs are ONE allocation each, touched by two warm-up passes (r02: 16 separate 1 GiB blocks from torch's
        caching allocator gave 5.6 ms on one box and 7.9 on the driver's); every chunk's time is reported."""
        cap = n + n // 8 + (1 << 20)
        cap = (cap + 255) & ~255
        src_all = torch.empty(k * n, dtype=torch.uint8, device=device)
        out_all = torch.empty(k * cap, dtype=torch.uint8, device=device)
        srcs = [src_all[i * n:(i + 1) * n] for i in range(k)]
        outs = [out_all[i * cap:(i + 1) * cap] for i in range(k)]
        for i in range(k):
            srcs[i].copy_(W.config_input("5", n, device, chunk=i))
        for _ in range(2):
            for i in range(k):
                huffman.compress_tensor(srcs[i], out=outs[i])
        torch.cuda.synchronize(device)
        reps, te = 3, 0.0
        per_chunk = [0.0] * k
        passes = []
        _lib.prof_enable(True)
        _lib.prof_reset()
        for _ in range(reps):
            t_pass = 0.0
            segs = []
            for i in range(k):
                seg, t = _timed(lambda i=i: huffman.compress_tensor(srcs[i], out=outs[i]))
                segs.append(seg)
                per_chunk[i] += t
                t_pass += t
            passes.append(t_pass * 1e3)
            te += t_pass
        prof5 = _lib.prof_get()
        _lib.prof_enable(False)
        te = te / reps * 1e3
        dec = torch.empty(n + (1 << 20), dtype=torch.uint8, device=device)
        ok = all(bool(torch.equal(huffman.decompress_tensor(segs[i], out=dec), srcs[i])) for i in range(k))   # every segment decodes on its own
        C = sum(int(x.numel()) for x in segs)
        out["5"] = {"algorithm": "huffman", "chunks": k, "bytes": k * n, "encode_ms": round(te, 3), "encode_MBps": round(k * n / 1e6 / (te / 1e3), 1),
                    "ratio_pct": round(100.0 * C / (k * n), 3), "lossless": ok,
                    "encode_frac_of_hbm_peak": round((2 * k * n + C) / (te / 1e3) / 1e9 / HBM_PEAK_GBPS, 5),
                    "per_chunk_ms": [round(x / reps * 1e3, 4) for x in per_chunk], "pass_ms": [round(x, 3) for x in passes],
                    "kernels_ms_per_chunk": {kk: round(v[1] / (reps * k), 4) for kk, v in sorted(prof5.items())},
                    "roofline": roofline_of("headline", "huff_emit", n + C // k, prof5["huff_emit"][1] / prof5["huff_emit"][0]) if "huff_emit" in prof5 else None,
                    "note": "one GPU, chunks one after the other, wall time per call; one allocation for the 8 inputs and one for the 8 outputs, "
                            "two warm-up passes; the sharded form with its gather is the --gpus N run"}
        del srcs, outs, segs, dec, src_all, out_all
        torch.cuda.empty_cache()

    for name in names:
        try:
            if name == "5":
                chunks_on_one_gpu()
            else:
                one(name)
        except Exception as e:          # noqa: BLE001 -- reported in the line, the other configs still run
            out[name] = {"error": "%s: %s" % (type(e).__name__, e)}
            torch.cuda.empty_cache()
    return out


def _host_call(fn, buf, *extra):
    """One host-buffer C-ABI call on a numpy array (pageable memory in, library-owned block out, PCIe both ways): (result, ms)."""
    import ctypes

    import numpy as np
    from raisin_amd import _lib
    out = ctypes.POINTER(ctypes.c_uint8)()
    got = ctypes.c_size_t(0)
    t0 = time.perf_counter()
    _lib.check(fn(buf.ctypes.data_as(ctypes.c_char_p), buf.size, *extra, ctypes.byref(out), ctypes.byref(got)))
    ms = (time.perf_counter() - t0) * 1e3
    res = np.ctypeslib.as_array(out, shape=(got.value,)).copy() if got.value else np.empty(0, np.uint8)
    _lib.lib().rsn_free(out)
    return res, ms


def config1_and_host_api(torch, device, n, with_host_gib):
    """SURVEY 8(d) config 1 and the host-buffer rates, both PCIe-INCLUSIVE and therefore never `value`:
      "1": `huffman` on 64 KiB of text (samIAm tiled and cut to 65 536 B; enwik8 is not available) through rsn_huffman_compress /
           _decompress exactly as the cgo shim calls them, next to the single-thread oracle on the same bytes -- the one size at which
           the reference's own regime applies, and where a GPU call's fixed cost (launches + two PCIe round trips) is expected to lose;
      "host_api": ms per call at the bench size for Huffman (2a) and LZSS (config 4's text), host buffer in, host buffer out."""
    import numpy as np
    import workloads as W
    from oracle import oracle as O
    from raisin_amd import _lib
    L = _lib.lib()
    out = {}
    sam = open(os.path.join(ROOT, "tests", "golden", "samiam.txt"), "rb").read()
    data = (sam * (65536 // len(sam) + 1))[:65536]
    arr = np.frombuffer(data, dtype=np.uint8)
    enc, dec = [], []
    for _ in range(25):
        c, te = _host_call(L.rsn_huffman_compress, arr)
        d, td = _host_call(L.rsn_huffman_decompress, c)
        enc.append(te)
        dec.append(td)
    enc, dec = sorted(enc)[len(enc) // 2], sorted(dec)[len(dec) // 2]
    oe, od = [], []
    for _ in range(5):
        rc, t = _timed(lambda: O.huffman_compress(data))
        oe.append(t * 1e3)
        rd, t = _timed(lambda: O.huffman_decompress(rc))
        od.append(t * 1e3)
    oe, od = sorted(oe)[2], sorted(od)[2]
    out["1"] = {"algorithm": "huffman", "bytes": len(data), "api": "host buffers (rsn_huffman_compress / _decompress), PCIe included",
                "encode_ms": round(enc, 4), "decode_ms": round(dec, 4), "round_trip_MBps": round(len(data) / 1e6 / ((enc + dec) / 1e3), 2),
                "ratio_pct": round(100.0 * c.size / len(data), 3), "lossless": bool(d.tobytes() == data),
                "bit_exact_vs_oracle": bool(c.tobytes() == rc), "compressed_bytes": int(c.size),
                "cpu_baseline": {"value": round(len(data) / 1e6 / ((oe + od) / 1e3), 2), "unit": "MB/s", "cores": 1, "kind": "port",
                                 "sample": "the whole 64 KiB, single-thread oracle: encode %.3f ms + decode %.3f ms (median of 5)" % (oe, od)},
                "gpu_faster_than_one_cpu_core": bool(enc + dec < oe + od),
                "note": "median of 25 calls; the small-input path (huff_small.hip): compress = 2 launches, decompress = 1, no copy command, "
                        "the host polls flags in pinned memory instead of waiting for the stream (r04: ~10 launches, 0.087 / 0.128 ms)"}
    # the reference's own table is files of 13-25 bytes (README.md:153-167): its two strings, and 2 KiB of samiam.txt, through both codecs'
    # host-buffer entry points (the small-input paths: lzss_small.hip one launch each way up to 1 KiB / 2 KiB, huff_small.hip two / one
    # from 2 bytes up), next to the single-thread oracle
    for alg, comp, decomp, extra, ocomp, odecomp in (
            ("lzss", L.rsn_lzss_compress, L.rsn_lzss_decompress, (4096,), lambda d: O.lzss_compress(d, 4096), O.lzss_decompress),
            ("huffman", L.rsn_huffman_compress, L.rsn_huffman_decompress, (), O.huffman_compress, O.huffman_decompress)):
        try:
            rows = {}
            for label, dat in (("README_25B", b"abcabcabcabcabcabcabcabc\n"), ("README_13B", b"Hello world!\n"), ("samiam_2KiB", sam[:2048])):
                a = np.frombuffer(dat, dtype=np.uint8)
                es, ds = [], []
                for _ in range(25):
                    cc, te = _host_call(comp, a, *extra)
                    dd, td = _host_call(decomp, cc)
                    es.append(te)
                    ds.append(td)
                oes, ods = [], []
                for _ in range(5):
                    rcc, t = _timed(lambda: ocomp(dat))
                    oes.append(t * 1e3)
                    _, t = _timed(lambda: odecomp(rcc))
                    ods.append(t * 1e3)
                rows[label] = {"bytes": len(dat), "encode_ms": round(sorted(es)[12], 4), "decode_ms": round(sorted(ds)[12], 4), "compressed_bytes": int(cc.size),
                               "lossless": bool(dd.tobytes() == dat), "bit_exact_vs_oracle": bool(cc.tobytes() == rcc),
                               "oracle_1_thread_ms": [round(sorted(oes)[2], 4), round(sorted(ods)[2], 4)]}
            out["1_" + alg + "_readme_files"] = {"algorithm": alg, "api": "host buffers, PCIe included", "files": rows,
                                                 "note": "median of 25 calls each (r05: the general paths, 0.1-0.2 ms)"}
        except Exception as e:                              # noqa: BLE001
            out["1_" + alg + "_readme_files"] = {"error": "%s: %s" % (type(e).__name__, e)}
    if with_host_gib:
        # Host buffer in, library-owned host buffer out (what the cgo shim binds).  The figures are a plain C++ PROCESS's (what a cgo caller
        # is like; scripts/probes/host_call_probe.cpp on the same bytes, best of three warm calls), pipelined and with RSN_HOST_SERIAL=1;
        # `python_process` is the same call through ctypes from this process, which has imported torch and therefore runs librsn on
        # the HIP runtime torch bundles (7.0.2 under the system runtime's SONAME): a download does not start there while an upload
        # runs (scripts/probes/py_decode_torch_order.py).
        import subprocess
        ha = {"bytes": n, "note": "host buffer in, library-owned host buffer out, warm calls (pages mapped, arenas grown); PCIe included, never `value`; "
                                  "encode_ms / decode_ms: the second ctypes call in THIS process, as in r01-r04 (torch imported: its bundled HIP runtime); "
                                  "c_process.pipelined / .serial: a freshly compiled C process (scripts/probes/host_call_probe.cpp, the runtime a cgo host "
                                  "gets), best of three warm calls, the second with RSN_HOST_SERIAL=1 (r05 reported the C process under encode_ms / decode_ms)"}
        exe = "/tmp/rsn_host_call_probe_%d" % os.getpid()
        try:
            subprocess.check_call(["g++", "-O2", "-o", exe, os.path.join(ROOT, "scripts", "probes", "host_call_probe.cpp"),
                                   "-L" + os.path.join(ROOT, "raisin_amd"), "-lrsn", "-Wl,-rpath," + os.path.join(ROOT, "raisin_amd")])
        except Exception as e:                              # noqa: BLE001
            exe = None
            ha["c_process_error"] = "%s: %s" % (type(e).__name__, e)
        for key, cfg, kind, comp, decomp, extra in (("huffman_2a", "2a", "h@", L.rsn_huffman_compress, L.rsn_huffman_decompress, ()),
                                                    ("lzss_text", "4", "@", L.rsn_lzss_compress, L.rsn_lzss_decompress, (4096,))):
            src = W.config_input(cfg, n, device).cpu().numpy()
            for rep in range(2):
                c, te = _host_call(comp, src, *extra)
                d, td = _host_call(decomp, c)
            py = {"encode_ms": round(te, 2), "decode_ms": round(td, 2), "lossless": bool(np.array_equal(d, src))}
            del c, d
            entry = {}
            if exe:
                data_file = "/tmp/rsn_bench_%s_%d.bin" % (cfg, os.getpid())
                try:
                    src.tofile(data_file)
                    for label, env in (("pipelined", {}), ("serial", {"RSN_HOST_SERIAL": "1"})):
                        r = subprocess.run([exe, str(n >> 20), kind + data_file], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
                        line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
                        res = json.loads(line[-1][7:]) if line else {"error": (r.stderr or r.stdout)[-300:]}
                        if "compress_ms" in res:
                            res = {"encode_ms": res["compress_ms"], "decode_ms": res["decompress_ms"], "lossless": res["lossless"],
                                   "compressed_bytes": res["compressed"],
                                   "encode_GBps": round(n / res["compress_ms"] / 1e6, 2), "decode_GBps": round(n / res["decompress_ms"] / 1e6, 2)}
                        entry.setdefault("c_process", {"method": "best of three warm calls in a C process"})[label] = res
                except Exception as e:                      # noqa: BLE001
                    entry["c_process_error"] = "%s: %s" % (type(e).__name__, e)
                finally:
                    if os.path.exists(data_file):
                        os.remove(data_file)
            entry.update(py)
            ha[key] = entry
            del src
        if exe and os.path.exists(exe):
            os.remove(exe)
        out["host_api"] = ha
        L.rsn_trim()
    return out


def config5_dealt(torch, dist, device, n, rank, world, backend, k=8):
    """BASELINE configs[4] in SURVEY 8(d)'s form: EIGHT independent chunks (seeds 0x5EED0050+i) dealt over the ranks, chunk i -> rank
    i mod world (raisin_amd/shard.py), every rank encodes its chunks one after the other, time = the slowest rank's; then the finished
    segments go to rank 0 (all_gather of sizes + grouped send/recv; RCCL over xGMI under nccl), timed on its own.  Total work is
    fixed as N grows: this object is the STRONG-scaling view next to the line's weak-scaling `value`."""
    import workloads as W
    from raisin_amd import huffman
    from raisin_amd import shard as _shard
    mine = _shard.chunks_for_rank(k, rank, world)
    cap = (n + n // 8 + (1 << 20) + 255) & ~255
    srcs = [W.config_input("5", n, device, chunk=i) for i in mine]
    outs = [torch.empty(cap, dtype=torch.uint8, device=device) for _ in mine]

    def fence():
        torch.cuda.synchronize(device)
        dist.barrier()
        torch.cuda.synchronize(device)

    for j in range(len(mine)):
        huffman.compress_tensor(srcs[j], out=outs[j])
    fence()
    t0 = time.perf_counter()
    segs = [huffman.compress_tensor(srcs[j], out=outs[j]) for j in range(len(mine))]
    torch.cuda.synchronize(device)
    mine_s = time.perf_counter() - t0
    fence()
    cpu = torch.device("cpu")
    t_max = _shard.max_over_ranks(dist, mine_s, device if backend == "nccl" else cpu)
    dec = torch.empty(n + (1 << 20), dtype=torch.uint8, device=device)
    ok = all(bool(torch.equal(huffman.decompress_tensor(segs[j], out=dec), srcs[j])) for j in range(len(mine)))
    ok_all = torch.tensor([1 if ok else 0], dtype=torch.int64, device=device if backend == "nccl" else cpu)
    dist.all_reduce(ok_all, op=dist.ReduceOp.MIN)
    # gather: round j moves every rank's j-th segment (ranks with fewer chunks send an empty one); an untimed 1-byte round first --
    # RCCL's lazy channel set-up must not be what gather_ms measures (shard.warm_gather)
    fence()
    n_rounds = (k + world - 1) // world
    rounds = [segs[j] if j < len(segs) else torch.empty(0, dtype=torch.uint8, device=device) for j in range(n_rounds)]
    if backend != "nccl":
        rounds = [x.cpu() for x in rounds]
    g = _shard.timed_gather(dist, rounds, device if backend == "nccl" else cpu, 0, sync=lambda: torch.cuda.synchronize(device))
    total = g["gathered_bytes"]
    g.pop("segments")
    C_mine = sum(int(x.numel()) for x in segs)
    ranks = _shard.per_rank(dist, [mine_s * 1e3, len(mine), (2 * len(mine) * n + C_mine) / max(mine_s, 1e-9) / 1e9 / HBM_PEAK_GBPS],
                            device if backend == "nccl" else cpu)
    return {"chunks": k, "chunks_per_rank": [len(_shard.chunks_for_rank(k, r, world)) for r in range(world)], "bytes": k * n,
            "encode_ms": round(t_max * 1e3, 3), "encode_MBps": round(k * n / 1e6 / t_max, 1), "scaling": "strong",
            "encode_frac_of_hbm_peak": round((2 * k * n + total) / t_max / 1e9 / (world * HBM_PEAK_GBPS), 5) if total else None,
            "per_rank": {"encode_ms": [round(r[0], 3) for r in ranks], "chunks": [int(r[1]) for r in ranks],
                         "encode_frac_of_hbm_peak": [round(r[2], 5) for r in ranks]},
            "gather_ms": round(g["gather_ms"], 3), "gather_warmup_ms": round(g["gather_warmup_ms"], 3),
            "gather_GBps": round(total / 1e6 / g["gather_ms"], 2) if g["gather_ms"] > 0 else None,
            "gathered_bytes": total, "lossless": bool(int(ok_all.item()) == 1),
            "note": "8 x %d MiB chunks, chunk i -> rank i mod %d; encode only (what CompressFiles does per file); time = max over ranks" % (n >> 20, world)}


def general_path_2a(mib):
    """The headline input through the GENERAL Huffman kernels: 2a's 128 equiprobable symbols all get 7-bit codes, so the timed step runs
    the flat specialisations (k_emit_flat<7> / k_dec_flat<7>); RSN_NO_FLAT=1 -- read once per process, hence a child process -- sends the
    same bytes through k_emit_ascii32 / k_dec_sync + k_dec_emit, the kernels any other code takes."""
    import subprocess
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--profile-only", "2a", "--mib", str(mib)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, RSN_NO_FLAT="1"))
    if r.returncode != 0:
        return {"error": (r.stderr or r.stdout)[-400:]}
    ent = json.loads(r.stdout.strip().splitlines()[-1])["profile_only"]["2a"]
    keep = ("encode_ms", "decode_ms", "encode_ms_min", "decode_ms_min", "passes", "round_trip_MBps", "ratio_pct", "lossless", "encode_frac_of_hbm_peak",
            "decode_frac_of_hbm_peak", "kernels_encode_ms", "kernels_decode_ms", "dominant_kernel", "bit_exact_vs_oracle_on_sample")
    out = {k: ent[k] for k in keep if k in ent}
    out["switch"] = "RSN_NO_FLAT=1 (child process)"
    return out


def cold_start(torch, n):
    """What a CLI user pays: `raisin_amd/host/rsn -compress <file> -algorithm=huffman` as a fresh process -- HIP initialisation, code-object
    load, file read, PCIe both ways, file write -- on a 64 KiB text file and on the bench buffer (2a), wall time from process start, next
    to the oracle's Compress on the same bytes in this process (the reference's own table is small files, whole process: README.md:153-167)."""
    import subprocess
    import tempfile
    import workloads as W
    from oracle import oracle as O
    root = os.path.dirname(os.path.abspath(__file__))
    exe = os.path.join(root, "raisin_amd", "host", "rsn")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe)])
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for label, data in (("64KiB_text", bytes(W.config_input("4", 64 << 10).numpy())), ("bench_buffer_2a", bytes(W.config_input("2a", n).numpy()))):
            path = os.path.join(td, label + ".bin")
            with open(path, "wb") as f:
                f.write(data)
            walls = []
            for _ in range(3):                              # (the first run also pages the binary and the library in)
                t0 = time.perf_counter()
                r = subprocess.run([exe, "-compress", path, "-algorithm=huffman", "-out=" + path + ".rsn"], capture_output=True, text=True, timeout=600)
                walls.append((time.perf_counter() - t0) * 1e3)
                if r.returncode != 0:
                    out[label] = {"error": (r.stderr or r.stdout)[-300:]}
                    break
            else:
                same = open(path + ".rsn", "rb").read()
                cores = O.host_cores()
                if len(data) <= (4 << 20):
                    ref, t_or = _timed(lambda: O.huffman_compress(data))
                    kind = "oracle, 1 thread"
                else:
                    ref, t_or = _timed(lambda: O.huffman_compress_mt(data, cores))
                    kind = "oracle, %d threads" % cores
                out[label] = {"bytes": len(data), "wall_ms": [round(w, 2) for w in walls], "wall_ms_best_of_3": round(min(walls), 2), "oracle_compress_ms": round(t_or * 1e3, 2),
                              "oracle": kind, "same_bytes_as_oracle": bool(same == ref)}
            for q in (path, path + ".rsn"):
                if os.path.exists(q):
                    os.remove(q)
    out["note"] = "whole process: HIP init + code-object load + file read + PCIe + file write; the oracle's time is the Compress call alone"
    return out


DUMP_HEAD = 1 << 20        # leading bytes of each output written whole (the compressed stream's header and table are at its start)
DUMP_SAMPLE = 1 << 22      # bytes of each output at seeded positions: 2 outputs x (1 + 4) Mi float32 = 40 MiB in all
DUMP_SEED = 0x5EED00D0


def dump_outputs(torch, outdir, outputs):
    """--dump-outputs: `outputs` = {name: 1-D uint8 device tensor}, what the last timed step returned.  Per output, as float32:
    <name>_head.npy (the first DUMP_HEAD bytes), <name>_sample.npy (DUMP_SAMPLE bytes at sorted positions drawn from a fixed
    seed and the output's length; the whole output when it is no longer), and <name>_size.npy (its length, float64)."""
    import numpy as np
    os.makedirs(outdir, exist_ok=True)
    for name, t in outputs.items():
        m = int(t.numel())
        np.save(os.path.join(outdir, name + "_size.npy"), np.array([m], dtype=np.float64))
        np.save(os.path.join(outdir, name + "_head.npy"), t[:DUMP_HEAD].cpu().numpy().astype(np.float32))
        if m <= DUMP_SAMPLE:
            smp = t.cpu().numpy()
        else:
            pos = np.sort(np.random.default_rng(DUMP_SEED).integers(0, m, size=DUMP_SAMPLE, dtype=np.int64))
            smp = t[torch.from_numpy(pos).to(t.device)].cpu().numpy()
        np.save(os.path.join(outdir, name + "_sample.npy"), smp.astype(np.float32))



def self_launch(n_ranks):
    """`python bench.py --gpus N` without a launcher: this process becomes the launcher's parent -- it starts
    `python -m torch.distributed.run --nproc-per-node N bench.py <same flags>` as a CHILD (one rank per GPU over RCCL), lets the
    child's stdout (rank 0's JSON line) through and returns its exit code.  Nothing here imports torch or touches the GPU: a process
    that has initialised the GPU must never be replaced or re-exec'ed on this pool."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC: what RCCL needs on this host driver
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_ranks),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mib", type=int, default=1024, help="buffer size per GPU (default: the 1 GiB of BASELINE.json)")
    ap.add_argument("--full", action="store_true", help="after the timed steps, also measure everything else: the HBM calibration, "
                    "the CPU baselines, the other BASELINE configs (N = 1), config 5's dealt chunks and the segment gather (N > 1)")
    ap.add_argument("--dump-outputs", metavar="DIR", default="", help="write what the last timed step returned to DIR/*.npy "
                    "(float32: the head and a seeded sample of the compressed stream and of the decoded buffer, and their lengths)")
    ap.add_argument("--no-cpu", action="store_true", help="--full: skip the CPU baselines")
    ap.add_argument("--no-others", action="store_true", help="--full: skip the other BASELINE configs after the timed region")
    ap.add_argument("--others", default="1,2b,skewed,3,4,5", help="1 = config 1 (64 KiB, host-buffer API) + the host-API rates at the bench size")
    ap.add_argument("--no-dealt", action="store_true", help="--full, N > 1: skip config 5's eight dealt chunks (the strong-scaling view)")
    ap.add_argument("--profile-only", default="", help="run ONLY these other configs (no headline step, no CPU baselines) and print their entries: "
                    "what scripts/profile.sh puts under rocprofv3, so that a workload's counters hold that workload's launches and nothing else")
    ap.add_argument("--gather-hang-ok", action="store_true", help="exit 0 even when the segment gather is still pending after 120 s")
    ap.add_argument("--dist-backend", default="nccl", help="nccl (= RCCL, one GPU per rank) or gloo (control-flow test: all ranks share GPU 0)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args.gpus))            # plain `python bench.py --gpus N`: start the N ranks ourselves (nothing has touched the GPU yet)

    import torch
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world:
        print("bench.py: --gpus %d but the launcher started %d rank(s) (WORLD_SIZE)" % (args.gpus, world), file=sys.stderr)
        sys.exit(2)
    dist = None
    if world > 1:
        import torch.distributed as dist
        if args.dist_backend == "gloo":
            local_rank = 0                       # test mode: every rank drives GPU 0, collectives run on host tensors
            dist.init_process_group("gloo")
        else:
            if local_rank >= torch.cuda.device_count():
                print("bench.py: rank %d has no GPU of its own (%d visible): one rank per GPU; `--dist-backend gloo` shares GPU 0 "
                      "for a control-flow check" % (local_rank, torch.cuda.device_count()), file=sys.stderr)
                sys.exit(2)
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)

    import workloads as W
    from raisin_amd import _lib, huffman
    from raisin_amd import shard as _shard
    _lib.check(_lib.lib().rsn_device_set(local_rank))

    n = args.mib << 20
    if args.profile_only:
        from oracle import oracle as O
        O.build()
        names = [x for x in args.profile_only.split(",") if x]
        print(json.dumps({"profile_only": run_other_configs(torch, device, n, O.host_cores(), False, names)}), flush=True)
        return
    seed = _shard.chunk_seed(rank, world)
    src = W.uniform_bytes(n, seed, 128, device)
    comp_buf = torch.empty(n + n // 8 + (1 << 20), dtype=torch.uint8, device=device)
    dec_buf = torch.empty(n + (1 << 20), dtype=torch.uint8, device=device)

    def step():
        c = huffman.compress_tensor(src, out=comp_buf)
        d = huffman.decompress_tensor(c, out=dec_buf)
        return c, d

    def fence():
        torch.cuda.synchronize(device)
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize(device)

    for _ in range(args.warmup):
        step()
    _lib.prof_enable(True)
    _lib.prof_reset()
    fence()
    t0 = time.perf_counter()
    t_enc = 0.0
    for _ in range(args.steps):
        a = time.perf_counter()
        c = huffman.compress_tensor(src, out=comp_buf)
        b = time.perf_counter()
        d = huffman.decompress_tensor(c, out=dec_buf)
        t_enc += b - a
    fence()
    elapsed = time.perf_counter() - t0
    prof = _lib.prof_get()
    _lib.prof_enable(False)

    t_max = elapsed
    ranks = None
    if dist is not None:
        cdev = device if args.dist_backend == "nccl" else torch.device("cpu")
        t_max = _shard.max_over_ranks(dist, elapsed, cdev)
        # every rank's own figures (north_star: MB/s AND fraction of the HBM peak at 1/2/4/8 GPUs); the line's `value` is the whole job's
        K_ = max(args.steps, 1)
        e_ms, d_ms = t_enc / K_ * 1e3, (elapsed - t_enc) / K_ * 1e3
        C_ = int(c.numel())
        ranks = _shard.per_rank(dist, [elapsed / K_ * 1e3, e_ms, d_ms, (2 * n + C_) / (e_ms / 1e3) / 1e9 / HBM_PEAK_GBPS,
                                       (C_ + n) / (d_ms / 1e3) / 1e9 / HBM_PEAK_GBPS, n / (e_ms / 1e3) / 1e9 / HBM_PEAK_GBPS], cdev)

    if args.dump_outputs and rank == 0:
        dump_outputs(torch, args.dump_outputs, {"compressed": c, "decompressed": d})
    lossless = bool(d.numel() == n and torch.equal(d, src))   # checked BEFORE anything else touches dec_buf
    comp_n = int(c.numel())

    # --full: context for the roofline: what a plain device-to-device copy and a read-only pass reach on THIS GPU
    # (torch kernels, timed with torch events on torch's stream; not part of the timed region above)
    def _rate(fn, nbytes, reps=10):
        for _ in range(3):
            fn()
        torch.cuda.synchronize(device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize(device)
        return nbytes / (e0.elapsed_time(e1) / reps) / 1e6
    if args.full:
        copy_gbps = _rate(lambda: dec_buf[:n].copy_(src), 2 * n)
        read_gbps = _rate(lambda: src.view(torch.int64).sum(), n)

    gather_ms = None
    gather_stuck = False
    dealt = None
    if dist is not None and args.full and not args.no_dealt:
        del dec_buf
        torch.cuda.empty_cache()
        try:
            dealt = config5_dealt(torch, dist, device, n, rank, world, args.dist_backend)
        except Exception as e:                              # noqa: BLE001 -- extra information: reported, never instead of the line
            dealt = {"error": "%s: %s" % (type(e).__name__, e)}
    if dist is not None and args.full:
        # config 5: compressed segments to rank 0 over RCCL, timed on its own (not part of `value`)
        seg = c.clone() if args.dist_backend == "nccl" else c.cpu()
        fence()
        # The gather is extra information: it runs under a watchdog so that a stuck collective can
        # never cost the job its throughput line (value does not depend on it).
        import threading
        box = {}

        def _gather():
            torch.cuda.set_device(device)
            g = _shard.timed_gather(dist, [seg], seg.device, 0, sync=lambda: torch.cuda.synchronize(device))   # (an untimed 1-byte round first)
            box["ms"], box["warm_ms"], box["bytes"] = g["gather_ms"], g["gather_warmup_ms"], g["gathered_bytes"]
            got = g["segments"][0] if rank == 0 else None
            box["ok"] = rank != 0 or (len(got) == world and got[0].numel() == comp_n)

        th = threading.Thread(target=_gather, daemon=True)
        th.start()
        th.join(120.0)
        gather_stuck = th.is_alive()
        if not gather_stuck and box.get("ok"):
            gather_ms = box["ms"]

    if rank == 0:
        K = args.steps
        per = {k: v[1] / v[0] for k, v in prof.items()}      # avg ms per launch
        cnt = {k: v[0] / K for k, v in prof.items()}         # launches per step
        C = comp_n
        alg = {  # ALGORITHMIC HBM bytes per launch (DESIGN.md "kernels")
            "huff_byte_hist": n, "huff_emit": n + C, "huff_dec_sync": C, "huff_dec_emit": C + n, "huff_dec_flat": C + n,
        }
        kernels = {}
        for k, ms in per.items():
            ent = {"ms": round(ms, 4), "launches_per_step": round(cnt[k], 2)}
            if k in alg:
                ent["algorithmic_bytes"] = alg[k]
                ent["GBps"] = round(alg[k] / ms / 1e6, 1)
                ent["frac_of_hbm_peak"] = round(alg[k] / ms / 1e6 / HBM_PEAK_GBPS, 4)
            kernels[k] = ent
        dom = max((k for k in per if k in alg), key=lambda k: per[k] * cnt[k])
        traffic = load_traffic(dom)
        roofline = {
            "kernel": dom, "bound": "hbm", "achieved": round(alg[dom] / per[dom] / 1e6, 1), "peak": HBM_PEAK_GBPS,
            "unit": "GB/s", "frac": round(alg[dom] / per[dom] / 1e6 / HBM_PEAK_GBPS, 4), "traffic": traffic[0] if traffic else None,
            "traffic_source": ("profiles/" + traffic[1]) if traffic else None, "algorithmic_bytes": alg[dom],
        }
        enc_ms = t_enc / K * 1e3
        dec_ms = (elapsed - t_enc) / K * 1e3
        gpu_enc_ms = sum(per[k] * cnt[k] for k in per if k.startswith("huff_") and "dec" not in k)
        out = {
            "metric": "encode+decode MB/s", "value": round(world * K * n / 1e6 / t_max, 1), "unit": "MB/s",
            "n_gpus": world, "steps": K, "warmup": args.warmup, "ms_per_step": round(t_max / K * 1e3, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
            "config": {"workload": ("huffman encode+decode, %d MiB uniform-random bytes 0x00-0x7F (BASELINE configs[1]), splitmix64 seed 0x%X" % (args.mib, seed))
                       if world == 1 else
                       ("WEAK scaling: one %d MiB chunk per GPU (BASELINE configs[4]'s chunks, seeds 0x5EED0050+rank), huffman encode+decode of it "
                        "on every rank, no data-path collective; configs[4]'s fixed eight chunks dealt over the ranks are under config5_dealt" % args.mib),
                       "algorithm": "huffman", "bytes_per_gpu": n, "chunks": world},
            "encode_MBps": round(n / 1e6 / (enc_ms / 1e3), 1), "decode_MBps": round(n / 1e6 / (dec_ms / 1e3), 1),
            "encode_ms": round(enc_ms, 4), "decode_ms": round(dec_ms, 4),
            "encode_kernel_ms": round(gpu_enc_ms, 4),
            "encode_frac_of_hbm_peak_2N_plus_C": round((2 * n + C) / (enc_ms / 1e3) / 1e9 / HBM_PEAK_GBPS, 4),
            "encode_input_read_frac_of_hbm_peak": round(n / (enc_ms / 1e3) / 1e9 / HBM_PEAK_GBPS, 4),
            "ratio_pct": round(100.0 * C / n, 3), "lossless": lossless,
            "roofline": roofline, "kernels": kernels,
        }
        if args.full:
            out["hbm_calibration_GBps"] = {"torch_copy_read_plus_write": round(copy_gbps, 1), "torch_read_only_sum": round(read_gbps, 1)}
        if ranks is not None:
            out["per_rank"] = {"ms_per_step": [round(r[0], 4) for r in ranks], "encode_ms": [round(r[1], 4) for r in ranks],
                               "decode_ms": [round(r[2], 4) for r in ranks],
                               "encode_frac_of_hbm_peak_2N_plus_C": [round(r[3], 4) for r in ranks],
                               "decode_frac_of_hbm_peak_C_plus_N": [round(r[4], 4) for r in ranks],
                               "encode_input_read_frac_of_hbm_peak": [round(r[5], 4) for r in ranks]}
            # the whole job against N GPUs' peak: algorithmic bytes of all ranks' steps / the slowest rank's time / (N x 8 TB/s)
            out["frac_of_hbm_peak_all_gpus"] = round(world * K * ((2 * n + C) + (C + n)) / t_max / 1e9 / (world * HBM_PEAK_GBPS), 4)
        if gather_ms is not None:
            out["gather_ms"] = round(gather_ms, 3)
            out["gather_warmup_ms"] = round(box.get("warm_ms", 0.0), 3)
            out["gather_GBps"] = round(box.get("bytes", 0) / 1e6 / gather_ms, 2) if gather_ms > 0 else None
            out["gather_note"] = ("one untimed 1-byte round first (RCCL sets peer-to-peer channels up on first use: gather_warmup_ms), then "
                                  "all_gather of sizes + grouped send/recv of one segment per rank to rank 0")
        if dealt is not None:
            out["config5_dealt"] = dealt
        if dist is not None and args.full and gather_ms is None:
            out["gather_ms"] = None
            out["gather_note"] = "segment gather did not complete within 120 s" if gather_stuck else "segment gather failed its size check"
        if world == 1 and args.full:
            from oracle import oracle as O
            O.build()
            cores = O.host_cores()
            # (everything below is extra information: whatever goes wrong there is reported in the line, never instead of it)
            if not args.no_cpu:
                try:
                    def make(k):
                        return bytes(src[:min(k, n)].cpu().numpy())
                    cb = cpu_huffman(make, cores)
                    smp = cb["_s"]
                    pre = min(len(smp), 32 << 20)          # the threaded baseline's bytes on the whole sample, the plain oracle's on a prefix
                    ok = bytes(huffman.compress_tensor(src[:len(smp)].contiguous()).cpu().numpy()) == cb["_c"]
                    ok = ok and bytes(huffman.compress_tensor(src[:pre].contiguous()).cpu().numpy()) == O.huffman_compress(smp[:pre])
                    out["bit_exact_vs_oracle_on_sample"] = bool(ok)
                    out["cpu_baseline"] = _public(cb)
                except Exception as e:                      # noqa: BLE001
                    out["cpu_baseline_error"] = "%s: %s" % (type(e).__name__, e)
            del comp_buf, dec_buf
            torch.cuda.empty_cache()
            if not args.no_others:
                names = [x for x in args.others.split(",") if x]
                try:
                    first = {}
                    if "1" in names:
                        names.remove("1")
                        try:
                            first = config1_and_host_api(torch, device, n, with_host_gib=True)
                        except Exception as e:              # noqa: BLE001
                            first = {"1": {"error": "%s: %s" % (type(e).__name__, e)}}
                    out["other_configs"] = {**first, **run_other_configs(torch, device, n, cores, not args.no_cpu, names)}
                    out["other_configs_note"] = ALG_NOTE + "; one warm-up pass, then %d timed passes per config: encode_ms / decode_ms are the medians" % OTHER_PASSES
                except Exception as e:                      # noqa: BLE001
                    out["other_configs_error"] = "%s: %s" % (type(e).__name__, e)
                for key, fn in (("general_path_2a", lambda: general_path_2a(args.mib)), ("cold_start", lambda: cold_start(torch, n))):
                    try:
                        out[key] = fn()
                    except Exception as e:                  # noqa: BLE001
                        out[key] = {"error": "%s: %s" % (type(e).__name__, e)}
        print(json.dumps(out), flush=True)
    if dist is not None:
        if gather_stuck:
            # a collective is still pending: leave without waiting for it.  The throughput line is already out (and says so:
            # gather_ms null + gather_note), so a failing exit code cannot lose it -- and a hung RCCL collective must not read as
            # success.  --gather-hang-ok restores exit 0 for a driver that insists on it.
            sys.stdout.flush()
            os._exit(0 if args.gather_hang_ok else 3)
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
