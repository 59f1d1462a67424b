"""GPU: the layered calls (rsn_layers_*, include/rsn.h) against the chain of single calls on the same build and against the oracle --
bytes, the one-layer delegation, the round trip's counts and comparison, the copy counters, errors, threads, and 1 GiB of config 4."""
import ctypes
import math
import os
import random
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLACK = 64 << 10          # tables, headers and size words (the issue's figure)

LISTS = [["lzss"], ["huffman"], ["lzss", "huffman"], ["huffman", "lzss"], ["lzss", "lzss"], ["huffman", "huffman", "lzss"], []]


def _text(seed, n):
    rng = random.Random(seed)
    words = ["".join(rng.choice("etaoinshrdlucmfwypvbgkqjxz") for _ in range(rng.randint(1, 9))) for _ in range(300)]
    out, size = [], 0
    while size < n:
        w = rng.choice(words) + rng.choice([" ", " ", " ", ", ", ".\n"])
        out.append(w)
        size += len(w)
    return "".join(out).encode()[:n]


def _inputs():
    rng = np.random.default_rng(0x1A7E)
    sam = open(os.path.join(ROOT, "tests", "golden", "samiam.txt"), "rb").read()
    period = rng.integers(97, 123, size=4096, dtype=np.uint8).tobytes()
    return [("13 bytes", b"Hello world!\n"), ("25 bytes", b"abcabcabcabcabcabcabcabc\n"), ("samiam", sam),
            ("text 64 KiB", _text(1, 65536)), ("text 1 MiB", _text(2, 1 << 20)),
            ("specials", (b"a<b\\c\xffd<<\\\\\xff\xff" + _text(3, 200)) * 700),
            ("runes", "héllo wörld ✓ 𝄞 naïve café\n".encode() * 5000),
            ("invalid utf-8", bytes(range(256)) * 300),
            ("4096-periodic", period * 40)]


def _single(direction, name):
    from raisin_amd import huffman, lz
    if direction == "c":
        return (lambda d: lz.CompressAsync(d, False, 4096)) if name == "lzss" else huffman.Compress
    return lz.Decompress if name == "lzss" else huffman.Decompress


def _chain_compress(data, layers):
    for a in layers:
        data = _single("c", a)(data)
    return data


def _chain_decompress(data, layers):
    for a in reversed(layers):
        data = _single("d", a)(data)
    return data


def _oracle_compress(O, data, layers):
    for a in layers:
        data = O.lzss_compress(data, 4096) if a == "lzss" else O.huffman_compress(data)
    return data


def _oracle_decompress(O, data, layers):
    for a in reversed(layers):
        data = O.lzss_decompress(data) if a == "lzss" else O.huffman_decompress(data)
    return data


def _decompress_like_the_chain(LY, stream, layers):
    """rsn_layers_decompress against the chain of single decompress calls: the same bytes, or -- where a layer of the chain fails, as a
    Huffman layer does over bytes an outer Huffman layer has changed (the codec is lossy on bytes that are not UTF-8) -- the same code
    and the single call's message behind "layer <k> (<name>): ".  Returns the bytes, or None when both fail."""
    from raisin_amd import RsnError
    data = stream
    for k in reversed(range(len(layers))):
        try:
            data = _single("d", layers[k])(data)
        except RsnError as single:
            with pytest.raises(RsnError) as e:
                LY.Decompress(stream, layers)
            assert e.value.code == single.code
            assert str(e.value) == str(single).replace(": ", ": layer %d (%s): " % (k, layers[k]), 1)
            return None
    assert LY.Decompress(stream, layers) == data
    return data


@pytest.mark.parametrize("layers", LISTS, ids=[",".join(x) or "none" for x in LISTS])
def test_bytes_equal_the_chain_of_single_calls_and_the_oracle(oracle, layers):
    from raisin_amd import layers as LY
    for name, data in _inputs():
        want = _chain_compress(data, layers)
        got = LY.Compress(data, layers)
        assert got == want, name
        if len(data) <= (1 << 20):
            assert got == _oracle_compress(oracle, data, layers), name
        back = _decompress_like_the_chain(LY, got, layers)
        if back is None:
            continue
        if len(data) <= (1 << 20) and len(layers) <= 2:
            assert back == _oracle_decompress(oracle, want, layers), name


def test_sixteen_mib_and_one_byte_and_the_longest_list(oracle):
    from raisin_amd import layers as LY
    big = _text(5, (16 << 20) + 1)
    for layers in (["lzss", "huffman"], ["huffman", "lzss"]):
        want = _chain_compress(big, layers)
        got = LY.Compress(big, layers)
        assert got == want
        assert LY.Decompress(got, layers) == big
    run = b"z" * (1 << 20)                                               # one distinct byte: behind an lzss first layer only
    for layers in (["lzss"], ["lzss", "huffman"], ["lzss", "lzss"]):
        got = LY.Compress(run, layers)
        assert got == _chain_compress(run, layers) == _oracle_compress(oracle, run, layers)
        assert LY.Decompress(got, layers) == run
    short = _text(6, 3000)
    eight = ["lzss", "huffman"] * 4
    got = LY.Compress(short, eight)
    assert got == _chain_compress(short, eight) == _oracle_compress(oracle, short, eight)
    # (a Huffman layer's output holds bytes >= 0x80, which the next Huffman layer does not give back: from the fourth layer on the
    #  round trip is lossy or fails, in the chain and in the call alike)
    _decompress_like_the_chain(LY, got, eight)
    big8 = _text(7, 200000)                                              # the same list above the host-chain cutoff: on the device
    got = LY.Compress(big8, eight)
    assert got == _chain_compress(big8, eight)
    _decompress_like_the_chain(LY, got, eight)
    four = ["lzss", "huffman", "lzss", "lzss"]                           # one Huffman layer: lossless through all of them, both paths
    for data in (short, big8):
        assert _decompress_like_the_chain(LY, LY.Compress(data, four), four) == data


def test_device_forms_give_the_same_bytes(oracle):
    import torch
    from raisin_amd import RsnError, _lib, layers as LY
    L = _lib.lib()
    H = _lib.hip()
    for layers in (["lzss", "huffman"], ["huffman", "lzss"], ["lzss"], ["huffman"], [], ["huffman", "huffman", "lzss"]):
        for data in (_text(8, 300000), bytes(range(256)) * 300, _text(9, 4096)):
            want = _chain_compress(data, layers)
            src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
            c = LY.compress_tensor(src, layers)
            assert bytes(c.cpu().numpy()) == want
            arr, k = LY.ids(layers)
            calls = [(L.rsn_layers_compress_dev, src, want)]
            try:
                back = _chain_decompress(want, layers)
            except RsnError:                                             # (two Huffman layers over bytes the first one changed: nothing to compare)
                back = None
            if back is not None:
                d = LY.decompress_tensor(c.clone(), layers)
                assert bytes(d.cpu().numpy()) == back
                calls.append((L.rsn_layers_decompress_dev, c.clone(), back))
            # the size query (d_out NULL), then a too-small buffer, then a buffer of the capacity the call asked for
            for fn, x, ref in calls:
                torch.cuda.synchronize()
                with pytest.raises(RsnError) as e:
                    _lib.call_dev(fn, x.data_ptr(), x.numel(), None, 0, None, arr, k)
                assert e.value.code == -7 and e.value.needed >= len(ref)
                need = e.value.needed
                if len(ref) > 64:
                    small = torch.empty(len(ref) - 16, dtype=torch.uint8, device="cuda")
                    with pytest.raises(RsnError) as e2:
                        _lib.call_dev(fn, x.data_ptr(), x.numel(), small.data_ptr(), small.numel(), None, arr, k)
                    assert e2.value.code == -7 and e2.value.needed >= len(ref)
                out = torch.empty(need, dtype=torch.uint8, device="cuda")
                got = _lib.call_dev(fn, x.data_ptr(), x.numel(), out.data_ptr(), out.numel(), None, arr, k)
                assert got == len(ref) and bytes(out[:got].cpu().numpy()) == ref
    # a stream of the caller's own (created by the runtime librsn runs on)
    H.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    H.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    st = ctypes.c_void_p()
    assert H.hipStreamCreate(ctypes.byref(st)) == 0
    try:
        data = _text(10, 500000)
        src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        c = LY.compress_tensor(src, ["lzss", "huffman"], stream=st)
        assert bytes(c.cpu().numpy()) == _chain_compress(data, ["lzss", "huffman"])
        assert bytes(LY.decompress_tensor(c, ["lzss", "huffman"], stream=st).cpu().numpy()) == data
    finally:
        H.hipStreamDestroy(st)


def _launches(fn):
    from raisin_amd import _lib
    _lib.prof_enable(True)
    _lib.prof_reset()
    try:
        out = fn()
        return out, {k: v[0] for k, v in _lib.prof_get().items() if v[0]}
    finally:
        _lib.prof_enable(False)


def test_one_layer_is_the_single_call():
    from raisin_amd import huffman, layers as LY
    rng = random.Random(7)                                               # the 64 KiB of tests/test_gpu_huffman_small.py's launch test
    words = ["".join(rng.choice("etaoinshrdlucmfwypvbgkqjxz") for _ in range(rng.randint(1, 9))) for _ in range(300)]
    out, size = [], 0
    while size < 65536:
        w = rng.choice(words) + rng.choice([" ", " ", " ", ", ", ".\n", "\\ "])
        out.append(w)
        size += len(w)
    data = "".join(out).encode()[:65536]
    LY.Decompress(LY.Compress(data, ["huffman"]), ["huffman"])
    assert _launches(lambda: huffman.Compress(data))[1] == {"huff_small_hist": 1, "huff_small_emit": 1}   # (the single call, for reference)
    c, enc = _launches(lambda: LY.Compress(data, ["huffman"]))
    back, dec = _launches(lambda: LY.Decompress(c, ["huffman"]))
    assert back == data
    assert enc == {"huff_small_hist": 1, "huff_small_emit": 1} and dec == {"huff_small_dec": 1}
    small = b"abcabcabcabcabcabcabcabc\n"
    c, enc = _launches(lambda: LY.Compress(small, ["lzss"]))
    back, dec = _launches(lambda: LY.Decompress(c, ["lzss"]))
    assert back == small and enc == {"lzss_small_enc": 1} and dec == {"lzss_small_dec": 1}


def _expect_roundtrip(data, layers):
    comp = _chain_compress(data, layers)
    back = _chain_decompress(comp, layers)
    a, b = np.frombuffer(data, dtype=np.uint8), np.frombuffer(back, dtype=np.uint8)
    m = min(len(a), len(b))
    diff = np.nonzero(a[:m] != b[:m])[0]
    first = int(diff[0]) if len(diff) else (m if len(a) != len(b) else (1 << 64) - 1)
    return comp, back, first, np.bincount(a, minlength=256), np.bincount(b, minlength=256)


def test_round_trip_counts_and_comparison():
    from raisin_amd import layers as LY
    text = _text(11, 3 << 20)
    cases = [(text, ["lzss", "huffman"]),                                            # lossless
             (text[:-1] + b"\xff", ["lzss", "huffman"]),                             # a difference in the LAST byte (U+FFFD comes back: longer, too)
             (text[: 1 << 20] + b"\xc3", ["huffman"]),                               # a lead byte without its continuation, one layer
             (bytes(range(256)) * 5000, ["huffman", "lzss"]),                        # lossy all over, another length
             (_text(12, 200000) + b"\xe2\x82", ["huffman"]),                         # a truncated rune at the end
             (_text(13, 5000), ["lzss", "huffman"]), (b"", ["lzss"]), (_text(14, 100000), [])]
    for data, layers in cases:
        comp, back, first, h0, h1 = _expect_roundtrip(data, layers)
        res, got_c = LY.RoundTrip(data, layers, keep_compressed=True)
        assert got_c == comp
        assert (res.original_n, res.compressed_n, res.decompressed_n) == (len(data), len(comp), len(back))
        assert bool(res.lossless) == (back == data) and res.first_difference == first
        assert list(res.hist_original) == h0.tolist() and list(res.hist_decompressed) == h1.tolist()
        assert res.compress_ms >= 0 and res.decompress_ms >= 0
        res2, none = LY.RoundTrip(data, layers)
        assert none is None and res2.first_difference == first and res2.compressed_n == len(comp)


def test_round_trip_prefix_and_last_byte_on_the_device():
    """The two comparison cases the kernel must get right, through the C ABI's own pieces: the decoded buffer a strict prefix of the
    original cannot come out of a codec, so k_bytes_differ / the length rule are also driven through a lossy last byte."""
    from raisin_amd import layers as LY
    base = _text(15, (2 << 20) + 5)
    data = base + b"\xff"                                                 # Huffman decodes the last byte as EF BF BD: differs AT the last offset
    res, _ = LY.RoundTrip(data, ["huffman"])
    assert not res.lossless and res.first_difference == len(data) - 1 and res.decompressed_n == len(data) + 2
    data = base + b"\xef"                                                 # ... as EF BF BD again: the original is a STRICT PREFIX of what comes back
    res, _ = LY.RoundTrip(data, ["huffman"])
    assert not res.lossless and res.first_difference == len(data) and res.decompressed_n == len(data) + 2
    res, _ = LY.RoundTrip(b"ab" * 500 + b"\xef", ["huffman"])             # the same below the cutoff (the host's comparison)
    assert not res.lossless and res.first_difference == 1001 and res.decompressed_n == 1003
    data = base + b"\xef\xbf\xbd"                                          # valid U+FFFD: comes back as it went
    res, _ = LY.RoundTrip(data, ["huffman"])
    assert res.lossless and res.first_difference == (1 << 64) - 1


def test_benchmark_file_equals_the_host_side_formulae(tmp_path):
    from raisin_amd import engine
    for k, (data, layers) in enumerate([(_text(16, 300000), ["lzss", "huffman"]), (bytes(range(256)) * 2000, ["huffman"]),
                                        (_text(17, 2000), ["huffman", "lzss"]), (_text(18, 150000), ["lzss"])]):
        p = tmp_path / ("f%d" % k)
        p.write_bytes(data)
        r = engine.BenchmarkFile(layers, str(p))
        comp, back, _, h0, h1 = _expect_roundtrip(data, layers)

        def ent(counts, total):
            return -sum(c / total * math.log(c / total) for c in counts.tolist() if c)
        want = engine.Result(",".join(layers), r.TimeTaken, len(comp) / len(data) * 100, ent(h1, len(comp)), ent(h0, len(data)), back == data, False)
        assert r == want


def test_the_stream_stays_on_the_device():
    from raisin_amd import _lib, layers as LY
    data = _text(19, 16 << 20)
    layers = ["lzss", "huffman"]
    LY.Compress(data, layers)
    _lib.prof_enable(True)
    try:
        _lib.prof_reset()
        c2 = LY.Compress(data, layers)
        up, down = _lib.prof_copied()
        print("layered compress: h2d %d (n %d), d2h %d (C2 %d)" % (up, len(data), down, len(c2)))
        assert up <= len(data) + SLACK and down <= len(c2) + SLACK
        _lib.prof_reset()
        c1 = _single("c", "lzss")(data)
        assert _single("c", "huffman")(c1) == c2
        up_chain, down_chain = _lib.prof_copied()
        print("chained compress: h2d %d (n + C1 %d), d2h %d" % (up_chain, len(data) + len(c1), down_chain))
        assert up_chain >= len(data) + len(c1)
        _lib.prof_reset()
        res, none = LY.RoundTrip(data, layers)
        up, down = _lib.prof_copied()
        print("round trip without the compressed stream: h2d %d, d2h %d" % (up, down))
        assert res.lossless and none is None and down < SLACK and up <= len(data) + SLACK
    finally:
        _lib.prof_enable(False)


def test_errors_name_the_layer(oracle):
    from raisin_amd import RsnError, huffman, layers as LY, lz
    both = ["lzss", "huffman"]
    with pytest.raises(RsnError) as e:
        LY.Compress(b"", both)
    assert e.value.code == -2 and "layer 1 (huffman): " in str(e.value)
    bad = b"1|a1|b\\\n\x09\x80"                                          # a damaged Huffman stream: the pad exceeds the payload
    with pytest.raises(RsnError) as single:
        huffman.Decompress(bad)
    with pytest.raises(RsnError) as e:
        LY.Decompress(bad, both)
    assert e.value.code == single.value.code == -3
    assert str(e.value) == str(single.value).replace(": ", ": layer 1 (huffman): ", 1)
    for n in (1000, 400000):                                             # a back-pointer in front of the data, under a sound Huffman layer: both paths
        ptr = huffman.Compress(b"abcdefgh<9999,4>" + _text(21, n))
        with pytest.raises(RsnError) as single:
            lz.Decompress(huffman.Decompress(ptr))
        with pytest.raises(RsnError) as e:
            LY.Decompress(ptr, both)
        assert e.value.code == single.value.code == -3
        assert str(e.value) == str(single.value).replace(": ", ": layer 0 (lzss): ", 1)
    for n in (3000, 200000):                                             # a successful call on the same thread directly afterwards, both paths
        data = _text(22, n)
        assert LY.Decompress(LY.Compress(data, both), both) == data
    L = __import__("raisin_amd")._lib.lib()
    out = ctypes.POINTER(ctypes.c_uint8)()
    k = ctypes.c_size_t(9)
    arr, cnt = LY.ids(both)
    assert L.rsn_layers_decompress(bad, len(bad), arr, cnt, ctypes.byref(out), ctypes.byref(k)) != 0 and not out and k.value == 0


def test_ten_threads_of_round_trips():
    from raisin_amd import layers as LY
    both = ["lzss", "huffman"]
    inputs = [_text(30 + i, 400000 + 37777 * i) for i in range(8)]
    shared = _text(40, 3 << 20)
    serial = [LY.RoundTrip(x, both, keep_compressed=True) for x in inputs + [shared]]
    want = [(bytes(c), r.compressed_n, r.decompressed_n, bool(r.lossless), list(r.hist_decompressed)) for r, c in serial]
    errors = []

    def work(i, data):
        try:
            for _ in range(3):
                r, c = LY.RoundTrip(data, both, keep_compressed=True)
                if (bytes(c), r.compressed_n, r.decompressed_n, bool(r.lossless), list(r.hist_decompressed)) != want[i]:
                    errors.append(("differs", i))
                if LY.Decompress(LY.Compress(data, both), both) != data:
                    errors.append(("chain", i))
        except Exception as e:                                           # noqa: BLE001
            errors.append((i, repr(e)))
    ts = [threading.Thread(target=work, args=(i, inputs[i])) for i in range(8)] + [threading.Thread(target=work, args=(8, shared)) for _ in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


def test_one_gib_of_config_4():
    import torch
    import workloads as W
    from raisin_amd import huffman, layers as LY, lz
    free, _ = torch.cuda.mem_get_info()
    if free < (8 << 30):
        pytest.skip("less than 8 GiB of free device memory")
    both = ["lzss", "huffman"]
    src = W.config_input("4", 1 << 30, "cuda")
    want = huffman.compress_tensor(lz.compress_tensor(src))
    got = LY.compress_tensor(src, both)
    assert got.numel() == want.numel() and torch.equal(got, want)
    del want
    back = LY.decompress_tensor(got, both)
    assert back.numel() == src.numel() and torch.equal(back, src)
    del back, got
    counts = torch.bincount(src.view(-1).to(torch.int32), minlength=256).cpu().tolist()
    host = bytes(src.cpu().numpy())
    del src
    torch.cuda.empty_cache()
    res, _ = LY.RoundTrip(host, both)
    assert res.lossless and res.original_n == res.decompressed_n == (1 << 30)
    assert list(res.hist_original) == counts == list(res.hist_decompressed)
