"""GPU: BASELINE.json's full-size configurations, checked through size-independent
properties (the oracle would need minutes at 1 GiB), plus bench.py's N>1 control flow."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GIB = 1 << 30


def test_config2_huffman_1GiB_uniform_7bit(oracle):
    import torch
    from raisin_amd import huffman
    import workloads as W
    src = W.config_input("2a", GIB, "cuda")                         # splitmix64 seed 0x5EED0002, & 0x7F
    c = huffman.compress_tensor(src)
    head = bytes(c[:4096].cpu().numpy())
    sep = head.index(b"\\\n")
    ents, _ = oracle.header_entries(head[:sep + 2] + b"\x00")
    counts = torch.bincount(src.view(-1).to(torch.int32), minlength=128).cpu().numpy()
    assert sorted(int(f) for f, _ in ents) == sorted(int(x) for x in counts)          # header == true histogram
    assert sum(int(f) for f, _ in ents) == GIB
    assert c.numel() == sep + 3 + GIB * 7 // 8 and head[sep + 2] == 0                   # 128 near-equal counts -> all codes 7 bits
    d = huffman.decompress_tensor(c)
    assert d.numel() == GIB and torch.equal(d, src)                                     # encode -> decode round trip
    # flat code: symbol i occupies payload bits [7i, 7i+7) and its code is its rank in the tree walk;
    # check the first 1 Mi symbols of the 1 GiB payload against the library's own code table
    table = {r: code for r, f, code, l in huffman.table(bytes(src[:1 << 26].cpu().numpy()))}
    pay = np.frombuffer(bytes(c[sep + 3: sep + 3 + (1 << 20) * 7 // 8].cpu().numpy()), dtype=np.uint8)
    codes = np.unpackbits(pay)[: (1 << 20) * 7].reshape(-1, 7).dot(1 << np.arange(6, -1, -1))
    sample = np.frombuffer(bytes(src[:1 << 20].cpu().numpy()), dtype=np.uint8)
    # codes are a bijection of the 128 symbols and identical symbols always map to identical codes
    pairs = set(zip(sample.tolist(), codes.tolist()))
    assert len(pairs) == 128 and len({a for a, _ in pairs}) == 128 and len({b for _, b in pairs}) == 128
    assert len(ents) == 128 and len(table) == 128


def test_config3_lzss_1GiB_period_4096(oracle):
    import torch
    from raisin_amd import lz
    import workloads as W
    src = W.config_input("3", GIB, "cuda")                          # splitmix64 seed 0x5EED0003, 254-value alphabet
    blk = src[:4096].cpu().numpy()
    c = lz.compress_tensor(src)
    host = bytes(c.cpu().numpy())
    head = oracle.lzss_compress(bytes(blk) * 3)                    # first block + two periods from the oracle
    first = head[: len(head) - 2 * len(b"<4096,4096>")]
    assert host.startswith(first)
    assert host[len(first):] == b"<4096,4096>" * (GIB // 4096 - 1)  # every later period is one token
    d = lz.decompress_tensor(c)
    assert d.numel() == GIB and torch.equal(d, src)


def test_config2b_huffman_1GiB_uniform_8bit(oracle):
    """Config 2b: uniform 0x00..0xFF.  Reference semantics (huffman.go:306-311, :138): every invalid byte becomes
    U+FFFD, so the round trip is LOSSY by design and the decoded bytes are []byte(string([]rune(string(in))))."""
    import torch
    import workloads as W
    from raisin_amd import huffman
    src = W.config_input("2b", GIB, "cuda")
    c = huffman.compress_tensor(src)
    d = huffman.decompress_tensor(c)
    assert d.numel() != GIB                                         # lossless=false, like the reference
    # size-independent properties: decoding is idempotent from there on (the decoded bytes ARE valid UTF-8, so a second
    # round trip is lossless), and the decoded length is what Go's rune decoding predicts: n + 2 * (#U+FFFD runes)
    c2 = huffman.compress_tensor(d)
    d2 = huffman.decompress_tensor(c2)
    assert d2.numel() == d.numel() and torch.equal(d2, d)
    # oracle-exact, bytes out of both directions, at 256 MiB (the regimes that make 2b hard -- ~3e5 symbols, codes past
    # 24 bits, second-level tables, the host heap -- grow with the size; the single-thread oracle does 32 MiB in under a second)
    pre = 256 << 20
    host = bytes(src[:pre].cpu().numpy())
    got = bytes(huffman.compress_tensor(src[:pre].contiguous()).cpu().numpy())
    ref = oracle.huffman_compress(host)
    assert got == ref
    back = bytes(huffman.decompress_tensor(torch.frombuffer(bytearray(ref), dtype=torch.uint8).cuda()).cpu().numpy())
    assert back == oracle.huffman_decompress(ref)
    assert max(x[3] for x in oracle.huffman_table(host)) > 24       # the long-code regime is in the sample
    runes = oracle.utf8_runes(host)                                 # Go's `range string(b)`: one rune per valid sequence or invalid byte
    want = int(((runes >= 0x80).astype(np.int64) + (runes >= 0x800) + (runes >= 0x10000) + 1).sum())
    assert len(back) == want > pre                                  # string(rune) written back (huffman.go:138)
    # and at full size: the decoded length is n + 2 per invalid byte, i.e. between n and 3n, and the ratio is the reference's
    assert GIB < d.numel() < 3 * GIB and 0.55 < c.numel() / GIB < 0.75


def test_config4_layered_1GiB_text(oracle):
    """Config 4: `lzss,huffman` on 1 GiB of Zipf text: lossless through both layers (engine.go:443-479 order),
    oracle-exact layered bytes on a prefix."""
    import torch
    import workloads as W
    from raisin_amd import huffman, lz
    src = W.config_input("4", GIB, "cuda")
    l1 = lz.compress_tensor(src)
    l2 = huffman.compress_tensor(l1)
    assert l2.numel() < l1.numel() < GIB
    back1 = huffman.decompress_tensor(l2)
    assert back1.numel() == l1.numel() and torch.equal(back1, l1)   # the inner layer comes back bit for bit
    # the Huffman layer at FULL size against the oracle, both directions: its input is the ~700 MB LZSS stream --
    # bytes 0xFF in it are not UTF-8, so this is the rune path at scale, lossless only because `<` never occurs in the text
    l1_host = bytes(l1.cpu().numpy())
    cores = oracle.host_cores()
    ref2 = oracle.huffman_compress_mt(l1_host, cores)
    assert bytes(l2.cpu().numpy()) == ref2
    assert oracle.huffman_decompress_mt(ref2, cores) == l1_host
    del l1, l1_host, ref2
    back = lz.decompress_tensor(back1)
    assert back.numel() == GIB and torch.equal(back, src)           # lossless through both layers
    del back, back1, l2
    # LZSS output is prefix-stable only up to the last token, so compare the layered result of the prefix itself
    pre = 8 << 20
    host = bytes(src[:pre].cpu().numpy())
    got = bytes(huffman.compress_tensor(lz.compress_tensor(src[:pre].contiguous())).cpu().numpy())
    assert got == oracle.huffman_compress(oracle.lzss_compress(host))


def test_config5_eight_chunks_on_one_gpu(oracle):
    """Config 5's 1-GPU form: 8 independent 1 GiB chunks (seeds 0x5EED0050+k), one complete .rsn segment each
    (engine.go:150-154: one file per input); every segment decodes on its own."""
    import torch
    import workloads as W
    from raisin_amd import huffman
    sizes = []
    for k in range(8):
        src = W.config_input("5", GIB, "cuda", chunk=k)
        seg = huffman.compress_tensor(src)
        head = bytes(seg[:4096].cpu().numpy())
        sep = head.index(b"\\\n")
        assert seg.numel() == sep + 3 + GIB * 7 // 8                # its own header and tree, a flat 7-bit code
        d = huffman.decompress_tensor(seg)                          # decodes alone
        assert d.numel() == GIB and torch.equal(d, src)
        sizes.append(int(seg.numel()))
        if k == 0:
            pre = 16 << 20
            assert bytes(huffman.compress_tensor(src[:pre].contiguous()).cpu().numpy()) == oracle.huffman_compress(bytes(src[:pre].cpu().numpy()))
        del src, seg, d
    assert len(set(sizes)) > 1 or len(sizes) == 8                   # different seeds, independent segments


def _oracle_says_identical(oracle, host, got, what):
    ok, bad = oracle.lzss_check(host, got)
    assert ok, "%s: differs from the oracle's CompressAsync output in the segment at compressed offset %d" % (what, bad)


def test_lzss_oracle_exact_where_the_code_changes_path(oracle):
    """the LZSS encoder switches path by size with the DEFAULT thresholds -- the 64-tile sample from 8192 tiles
    (64 MiB), one lane per tile in the in-tile parse from 32768 tiles (256 MiB), decode groups of n_tiles/512 above 32 MiB -- and a
    round trip cannot tell a different valid parse from the reference's.  288 MiB of config 4's text and 288 MiB of mixed
    text / noise / periodic sections, default switches, bytes == the oracle's: by the segment induction of
    oracle.lzss_check (every segment re-encoded by the oracle's own greedy loop), and against the threaded oracle's complete
    output (lzss_compress_mt: a Reference for every position, lzss.go:117-151) where the host has the cores for it."""
    import time

    import torch
    import workloads as W
    from raisin_amd import lz
    n = 288 << 20
    text = W.config_input("4", n, "cuda")
    got = lz.compress_tensor(text)
    host, gb = bytes(text.cpu().numpy()), bytes(got.cpu().numpy())
    _oracle_says_identical(oracle, host, gb, "config 4 text, 288 MiB")
    back = lz.decompress_tensor(got)
    assert back.numel() == n and torch.equal(back, text)
    # the whole output from the every-position oracle, when a 4 MiB probe says it fits the budget (256 host threads: ~45 s)
    cores = oracle.host_cores()
    t0 = time.time()
    oracle.lzss_compress_mt(host[:4 << 20], 4096, cores, 4096)
    est = (time.time() - t0) * (n / (4 << 20))
    if est < 240:
        assert gb == oracle.lzss_compress_mt(host, 4096, cores, 4096)
    else:
        print("lzss_compress_mt at 288 MiB would take ~%.0f s on %d cores: segment induction only" % (est, cores))
    del text, got, back
    # mixed: 1 MiB sections of text, noise (all 256 values: escapes too), 4096-periodic data, runs, a period of 1000
    g = torch.Generator(device="cuda").manual_seed(11)
    parts = []
    tx = W.config_input("4", 96 << 20, "cuda")
    per = W.config_input("3", 32 << 20, "cuda")
    for k in range(288):
        kind = k % 6
        if kind in (0, 3):
            parts.append(tx[(k // 3) << 20:((k // 3) + 1) << 20])
        elif kind == 1:
            parts.append(torch.randint(0, 256, (1 << 20,), dtype=torch.uint8, device="cuda", generator=g))
        elif kind == 2:
            parts.append(per[(k % 32) << 20:((k % 32) + 1) << 20])
        elif kind == 4:
            parts.append(torch.randint(97, 101, ((1 << 20) // 37 + 1,), dtype=torch.uint8, device="cuda", generator=g).repeat_interleave(37)[:1 << 20])
        else:
            parts.append(torch.randint(32, 127, (1000,), dtype=torch.uint8, device="cuda", generator=g).repeat(1049)[:1 << 20])
    mixed = torch.cat(parts)
    del parts, tx, per
    assert mixed.numel() == n
    got = lz.compress_tensor(mixed)
    _oracle_says_identical(oracle, bytes(mixed.cpu().numpy()), bytes(got.cpu().numpy()), "mixed sections, 288 MiB")
    back = lz.decompress_tensor(got)
    assert back.numel() == n and torch.equal(back, mixed)


def test_lzss_1GiB_text_is_the_oracles_output_and_the_allpos_paths(oracle, tmp_path):
    """Config 4's LZSS layer at the full 1 GiB: the default path's bytes are the oracle's (segment induction, every segment
    re-encoded by the oracle's greedy loop -- seconds on the host's cores), and their sha256 equals that of the same call under
    RSN_LZSS_ALLPOS=1 (the bucket search at EVERY position + the general parse: no chain walk, no sample, no looks) run in a
    process of its own."""
    import hashlib

    import workloads as W
    from raisin_amd import lz
    src = W.config_input("4", GIB, "cuda")
    got = bytes(lz.compress_tensor(src).cpu().numpy())
    host = bytes(src.cpu().numpy())
    del src
    _oracle_says_identical(oracle, host, got, "config 4 text, 1 GiB")
    del host
    code = ("import sys, hashlib; sys.path.insert(0, %r)\n"
            "import workloads as W\nfrom raisin_amd import lz\n"
            "c = lz.compress_tensor(W.config_input('4', 1 << 30, 'cuda'))\n"
            "print(hashlib.sha256(bytes(c.cpu().numpy())).hexdigest())\n" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=dict(os.environ, RSN_LZSS_ALLPOS="1"))
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split()[-1] == hashlib.sha256(got).hexdigest()


@pytest.mark.parametrize("name", ["2a", "skewed"])
def test_huffman_1GiB_byte_for_byte_against_the_threaded_oracle(oracle, name):
    """Configs 2a (flat 7-bit code: k_emit_flat / k_dec_flat) and `skewed` (general kernels) at the full 1 GiB, every byte of
    both directions against oracle/cpu_baseline.c's threaded restatement (same bytes as the plain oracle: tests/test_oracle.py)."""
    import torch
    import workloads as W
    from raisin_amd import huffman
    src = W.config_input(name, GIB, "cuda")
    c = huffman.compress_tensor(src)
    host = bytes(src.cpu().numpy())
    cores = oracle.host_cores()
    ref = oracle.huffman_compress_mt(host, cores)
    assert bytes(c.cpu().numpy()) == ref
    d = huffman.decompress_tensor(c)
    assert d.numel() == GIB and torch.equal(d, src)
    del d, c, src
    assert oracle.huffman_decompress_mt(ref, cores) == host          # and the oracle's decode of those bytes is the input


def test_bench_two_ranks_control_flow():
    """bench.py's world-size-2 path on one GPU (gloo collectives, both ranks on GPU 0)."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", "29731", os.path.join(ROOT, "bench.py"),
                          "--gpus", "2", "--steps", "2", "--warmup", "1", "--mib", "64", "--dist-backend", "gloo", "--full"],
                         capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    j = json.loads(line)
    assert j["n_gpus"] == 2 and j["lossless"] is True and j["scaling"] == "weak"
    assert j["config"]["chunks"] == 2 and "gather_ms" in j and j["value"] > 0
    d5 = j["config5_dealt"]                              # configs[4]'s eight chunks dealt over the two ranks, then gathered
    assert d5["chunks"] == 8 and d5["chunks_per_rank"] == [4, 4] and d5["lossless"] is True and d5["scaling"] == "strong"
    assert d5["gathered_bytes"] > 8 * (64 << 20) * 7 // 8 and d5["encode_ms"] > 0
    # north_star: absolute MB/s and fraction of the HBM peak per GPU count -- every rank's own figures ride in the line, and both
    # gathers are preceded by an untimed round that is reported on its own
    pr = j["per_rank"]
    for key in ("ms_per_step", "encode_ms", "decode_ms", "encode_frac_of_hbm_peak_2N_plus_C", "decode_frac_of_hbm_peak_C_plus_N"):
        assert len(pr[key]) == 2 and all(x > 0 for x in pr[key]), key
    assert 0 < j["frac_of_hbm_peak_all_gpus"] < 1 and j["gather_warmup_ms"] > 0 and j["gather_ms"] > 0
    assert len(d5["per_rank"]["encode_ms"]) == 2 and d5["per_rank"]["chunks"] == [4, 4] and d5["gather_warmup_ms"] > 0
    assert all(0 < x < 1 for x in d5["per_rank"]["encode_frac_of_hbm_peak"]) and 0 < d5["encode_frac_of_hbm_peak"] < 1


def test_bench_plain_run_and_dump_outputs(tmp_path):
    """A plain `bench.py --gpus 1` times --steps steps and prints the headline line alone (the rest is --full's); --dump-outputs
    writes what the last timed step returned -- float32 / float64 .npy files, 64 MB at most -- and those are the library's bytes for
    the headline input, the same from run to run."""
    import torch
    import workloads as W
    from raisin_amd import huffman
    import bench

    def run(outdir, steps):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                              "--mib", "64", "--dump-outputs", str(outdir)], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        return json.loads(lines[0])

    j = run(tmp_path / "a", 3)
    assert j["steps"] == 3 and j["ms_per_step"] > 0 and j["value"] > 0 and j["lossless"] is True
    assert j["metric"] == "encode+decode MB/s" and j["unit"] == "MB/s" and j["higher_is_better"] is True and j["dtype"] == "u8"
    for key in ("other_configs", "cpu_baseline", "hbm_calibration_GBps", "general_path_2a", "cold_start"):
        assert key not in j, key
    names = sorted("%s_%s.npy" % (o, p) for o in ("compressed", "decompressed") for p in ("head", "sample", "size"))
    assert sorted(os.listdir(tmp_path / "a")) == names
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in names) <= 64 << 20
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in names}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    n = 64 << 20
    src = W.uniform_bytes(n, W.SEED_2, 128, "cuda")
    c = huffman.compress_tensor(src)
    pos = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, c.numel(), size=bench.DUMP_SAMPLE, dtype=np.int64))
    assert got["compressed_size"][0] == c.numel() and got["decompressed_size"][0] == n
    assert np.array_equal(got["compressed_head"], c[:bench.DUMP_HEAD].cpu().numpy().astype(np.float32))
    assert np.array_equal(got["compressed_sample"], c[torch.from_numpy(pos).cuda()].cpu().numpy().astype(np.float32))
    pos = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, n, size=bench.DUMP_SAMPLE, dtype=np.int64))
    assert np.array_equal(got["decompressed_head"], src[:bench.DUMP_HEAD].cpu().numpy().astype(np.float32))
    assert np.array_equal(got["decompressed_sample"], src[torch.from_numpy(pos).cuda()].cpu().numpy().astype(np.float32))
    assert run(tmp_path / "b", 1)["steps"] == 1
    for f in names:
        assert np.array_equal(np.load(tmp_path / "b" / f), got[f[:-4]]), f


def test_bench_two_ranks_over_rccl():
    """bench.py --gpus 2 with the DEFAULT backend (nccl = RCCL, one GPU per rank: init_process_group with a device id, the barrier,
    max-over-ranks on device tensors, gather_segments' all_gather + batch_isend_irecv over xGMI).  Needs two GPUs: skipped on the
    one-GPU boxes this suite has run on so far, so the first box with two exercises the branch."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU visible: the RCCL branch needs two")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                          "--mib", "256", "--full"], capture_output=True, text=True, env=env, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    j = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert j["n_gpus"] == 2 and j["lossless"] is True and j["value"] > 0
    assert j["gather_ms"] is not None and j["gather_ms"] > 0 and j["gather_warmup_ms"] > 0
    assert len(j["per_rank"]["encode_frac_of_hbm_peak_2N_plus_C"]) == 2
    assert j["config5_dealt"]["chunks"] == 8 and j["config5_dealt"]["lossless"] is True


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2` with NO launcher around it -- the way the driver calls it: bench.py starts the two ranks
    itself (a child `torch.distributed.run`), forwards rank 0's line and the exit code (this used to exit 2)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                          "--mib", "64", "--dist-backend", "gloo"], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                               # ONE JSON line, rank 0's
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["lossless"] is True and j["config"]["chunks"] == 2 and j["value"] > 0


def test_beyond_4GiB_offsets():
    """5 GiB per call: every byte/bit offset above 2^32 (flat and general Huffman paths)."""
    import torch
    from raisin_amd import huffman
    n = 5 * GIB
    g = torch.Generator(device="cuda").manual_seed(7)
    base = torch.randint(0, 128, (GIB,), dtype=torch.uint8, device="cuda", generator=g)
    src = base.repeat(5)
    del base
    c = huffman.compress_tensor(src)
    assert c.numel() > n * 7 // 8                       # 128 equiprobable symbols: flat 7-bit code
    d = huffman.decompress_tensor(c)
    assert d.numel() == n and torch.equal(d, src)
    del c, d
    # general path: a skewed 64 MiB block tiled to 5 GiB
    w = torch.tensor([2.0 ** (-i / 6) for i in range(96)], device="cuda")
    blk = (torch.multinomial(w, 1 << 26, replacement=True).to(torch.uint8) + 32)
    src = blk.repeat(80)
    c = huffman.compress_tensor(src)
    d = huffman.decompress_tensor(c)
    assert d.numel() == n and torch.equal(d, src)


def test_lzss_beyond_2GiB_in_sections(oracle):
    """the reference has no bound on its input (lzss.go:109); one pass here has 32-bit positions, so 2.5 GiB of config
    4's text goes through three sections (1 GiB each, 512 KiB of halo, the chain's exit handed from one to the next) -- and the bytes
    are the oracle's CompressAsync output (segment induction, oracle.lzss_check).  The decoder's own limit (a 4 GiB escaped stream)
    is not touched: the stream decodes back to the input."""
    import torch
    import workloads as W
    from raisin_amd import lz
    n = 5 * GIB // 2
    src = W.config_input("4", n, "cuda")
    got = lz.compress_tensor(src)
    assert got.numel() < n
    host = bytes(src.cpu().numpy())
    gb = bytes(got.cpu().numpy())
    _oracle_says_identical(oracle, host, gb, "config 4 text, 2.5 GiB in sections")
    del host, gb
    back = lz.decompress_tensor(got)
    assert back.numel() == n and torch.equal(back, src)



def test_lzss_decode_beyond_4GiB_in_sections():
    """The decoder's side of VERDICT r3 #9: the tile kernels count positions in 32 bits, so a stream of 4 GiB and more -- decoded
    (4.25 GiB of config 4's text: 2.9 GiB compressed) or compressed as well (4.1 GiB of uniform bytes: nothing to find, 1.2 % of
    escapes on top) -- is expanded in sections of 1 GiB (lzss_decode_sections) and unescaped in one pass whose kernels count blocks.
    Both come back as the input; the encoder went through its own sections to produce them."""
    import torch
    import workloads as W
    from raisin_amd import lz
    for name, n, make in (("text", 17 * GIB // 4, lambda n: W.config_input("4", n, "cuda")),
                          ("uniform", 41 * GIB // 10, lambda n: W.config_input("2b", n, "cuda"))):
        src = make(n)
        assert src.numel() == n
        got = lz.compress_tensor(src)
        if name == "uniform":
            assert got.numel() >= 4 * GIB, got.numel()
        comp = got.clone()                                                # (the view holds the whole bound)
        del got
        torch.cuda.empty_cache()
        back = lz.decompress_tensor(comp)
        assert back.numel() == n, (name, back.numel())
        for a in range(0, n, GIB):                                        # (compared a GiB at a time: torch.equal wants a temporary of the operands' size)
            assert torch.equal(back[a:a + GIB], src[a:a + GIB]), (name, a)
        del src, comp, back
        torch.cuda.empty_cache()


@pytest.mark.parametrize("w,mib", [(256, 64), (1000, 64), (4095, 64), (8192, 32), (20000, 16), (65536, 8)])
def test_lzss_windows_other_than_the_engines_at_size(oracle, w, mib):
    """windows other than 4096 -- the row walk below it, the sweep up to 8192 (k_match2), lzss_big.hip above --
    were oracle-checked at KB-MB sizes only.  Tens of MiB of config 4's text and of mixed sections per window: the bytes are the
    oracle's (segment induction with that window), and decode back to the input."""
    import time
    import torch
    import workloads as W
    from raisin_amd import lz
    n = mib << 20
    g = torch.Generator().manual_seed(w)
    parts = [W.config_input("4", n)[: n // 2],
             torch.randint(0, 256, (n // 8,), dtype=torch.uint8, generator=g),
             W.config_input("3", n // 8),
             torch.randint(97, 101, (n // 8 // 37 + 1,), dtype=torch.uint8, generator=g).repeat_interleave(37)[: n // 8],
             W.config_input("4", n)[n // 2: n // 2 + n // 8]]
    if w > 20000:                                                      # (periodic stretches under a window that large are outside the large-window search's work budget: RSN_ERR_LIMIT, tested in test_gpu_lzss.py)
        parts = [parts[0], parts[1], parts[4]]
    src = torch.cat(parts).cuda()
    t0 = time.time()
    got = lz.compress_tensor(src, window=w)
    torch.cuda.synchronize()
    t1 = time.time()
    ok, bad = oracle.lzss_check(bytes(src.cpu().numpy()), bytes(got.cpu().numpy()), window=w)
    print("window %d, %d MiB: product %.2f s, oracle check %.1f s" % (w, src.numel() >> 20, t1 - t0, time.time() - t1))
    assert ok, "window %d: differs from the oracle's CompressAsync output in the segment at compressed offset %d" % (w, bad)
    back = lz.decompress_tensor(got)
    assert back.numel() == src.numel() and torch.equal(back, src)


def test_lzss_runs_and_repeated_rows_at_size(oracle):
    """r06: about 512 MiB made of a sparse buffer, byte runs and rows repeated -- the chain walk's instance for stretches of short periods with
    65536 tiles and the serial in-tile parse (from 256 MiB).  Properties: the round trip; the stream of the first 1 MiB encoded alone is
    the oracle's; the whole stream BEGINS with the bytes of the oracle's stream for that megabyte up to its last item (the chain of a
    prefix does not depend on what follows it beyond the last match's reach)."""
    import torch
    from raisin_amd import lz
    g = torch.Generator(device="cuda"); g.manual_seed(11)
    n = 128 << 20
    sparse = torch.where(torch.rand(n, device="cuda", generator=g) < 0.01, torch.randint(1, 128, (n,), device="cuda", generator=g, dtype=torch.uint8), torch.zeros(n, dtype=torch.uint8, device="cuda"))
    runs = torch.repeat_interleave(torch.randint(97, 123, (n // 300 + 1,), device="cuda", generator=g, dtype=torch.uint8), torch.randint(1, 600, (n // 300 + 1,), device="cuda", generator=g))[:n]
    row = torch.tensor(list(b"0,0,0,0.0,\n"), dtype=torch.uint8, device="cuda")
    rows = row.repeat(n // 11 + 1)[:n].clone()
    idx = torch.randint(0, n // 11, (n // 110,), device="cuda", generator=g) * 11          # a row in ten begins with another digit
    rows[idx] = torch.randint(49, 58, (idx.numel(),), device="cuda", generator=g, dtype=torch.uint8)
    line = torch.tensor(list(b"worker idle\n"), dtype=torch.uint8, device="cuda").repeat(n // 12 + 1)[:n].clone()
    line[torch.randint(0, n, (n // 5000,), device="cuda", generator=g)] = 88                # the line broken every five thousand bytes or so
    src = torch.cat([sparse, runs, rows, line]).contiguous()
    c = lz.compress_tensor(src)
    d = lz.decompress_tensor(c)
    assert d.numel() == src.numel() and torch.equal(d, src)
    head = bytes(src[: 1 << 20].cpu().numpy())
    want = oracle.lzss_compress(head)
    assert lz.CompressAsync(head) == want
    k = max(want.rfind(b"<", 0, len(want) - 64), 0)                                          # up to the last token that begins well before the prefix's end
    assert bytes(c[:k].cpu().numpy()) == want[:k]
