"""GPU: the batch forms of Huffman decompress and LZSS compress / decompress (rsn.h).  Every member equals the single call
(and the CPU oracle); small members go many to ONE launch of the grouped kernels; a failing member fails the whole batch the documented
way; the engine and the C++ host route one-layer file lists through the batch calls with the per-file loop's results and semantics."""
import concurrent.futures
import os
import random
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
README = [b"Hello world!\n", b"abcabcabcabcabcabcabcabc\n"]        # the reference README's two files (13 and 25 bytes)
WORDS = [b"the", b"quick", b"brown", b"fox", b"jumps", b"over", b"lazy", b"dog", b"compression", b"a", b"I", b"Sam", b"ham"]


def _text(seed, n):
    rng = random.Random(seed)
    t = bytearray()
    while len(t) < n:
        t += rng.choice(WORDS) + rng.choice([b" ", b"\n", b", ", b". "])
    return bytes(t[:n])


@pytest.fixture(scope="module")
def mods():
    from raisin_amd import _lib, huffman, lz
    return _lib, huffman, lz


@pytest.fixture(scope="module")
def plain(samiam):
    rng = np.random.default_rng(7)
    out = list(README) + [samiam, _text(1, 1024), bytes(range(256)), b"<" * 40 + b"\\" * 40 + b"\xff" * 40 + _text(2, 200),
                          bytes(rng.choice(np.frombuffer(b"<\\\xffab", dtype=np.uint8), size=900)), b"q" * 1024]
    return out


def _prof(_lib, fn):
    _lib.prof_enable(True)
    _lib.prof_reset()
    try:
        res = fn()
        return res, {k: v[0] for k, v in _lib.prof_get().items() if v[0]}
    finally:
        _lib.prof_enable(False)


# ---------------------------------------------------------------- bytes
def test_lzss_compress_batch_bytes(mods, oracle, plain):
    _, _, lz = mods
    big = [_text(3, 3 << 20), np.random.default_rng(3).integers(0, 256, size=8 << 20, dtype=np.uint8).tobytes()]
    for window in (4096, 16, 0):
        members = plain + [b"", plain[0], plain[3]] + (big if window == 4096 else [])
        got = lz.CompressAsyncBatch(members, window)
        assert len(got) == len(members)
        for d, g in zip(members, got):
            assert g == lz.CompressAsync(d, False, window), (window, len(d))
            if len(d) <= 65536:
                assert g == oracle.lzss_compress(d, window), (window, len(d))
        if window == 4096:
            assert lz.DecompressBatch(got) == members


def test_lzss_decompress_batch_bytes(mods, oracle, plain):
    _, _, lz = mods
    streams = [oracle.lzss_compress(d, w) for d in plain for w in (4096, 16)]
    streams += [b"", b"plain text without tokens", oracle.lzss_compress(_text(4, 8000)), streams[0],
                oracle.lzss_compress(_text(5, 3 << 20)), oracle.lzss_compress(_text(6, 8 << 20))]
    got = lz.DecompressBatch(streams)
    for s, g in zip(streams, got):
        assert g == lz.Decompress(s)
        assert g == oracle.lzss_decompress(s)


def test_huffman_decompress_batch_bytes(mods, oracle, plain, samiam):
    _, huffman, _ = mods
    rng = np.random.default_rng(11)
    datas = [d for d in plain if len(set(d)) > 1]
    datas += ["rune stream: ÄÖÜ äöü ß € 漢字 ".encode() * 40,            # runes: the general decoder
              rng.integers(65, 97, size=20000, dtype=np.uint8).tobytes(),  # uniform over 32 symbols: five phases
              rng.integers(65, 98, size=12000, dtype=np.uint8).tobytes(),  # 33 symbols: lengths 5 and 6, slow to synchronise
              (samiam * 200)[:30000],                                      # periodic text
              _text(8, 16 << 10), _text(9, 64 << 10), _text(10, 3 << 20), _text(11, 8 << 20)]
    streams = [oracle.huffman_compress(d) for d in datas]
    streams.append(streams[0])                                              # the same buffer twice
    got = huffman.DecompressBatch(streams)
    for s, g in zip(streams, got):
        assert g == huffman.Decompress(s)
        assert g == oracle.huffman_decompress(s)


# ---------------------------------------------------------------- one launch
def test_a_thousand_small_members_are_one_launch(mods, oracle):
    _lib, huffman, lz = mods
    datas = [_text(100 + i, 20 + (i * 37) % 1000) for i in range(1000)]
    comp, p = _prof(_lib, lambda: lz.CompressAsyncBatch(datas))
    assert p == {"lzss_batch_enc": 1}, p
    assert comp[:20] == [oracle.lzss_compress(d) for d in datas[:20]]
    dec, p = _prof(_lib, lambda: lz.DecompressBatch(comp))
    assert p == {"lzss_batch_dec": 1}, p
    assert dec == datas
    hstreams = [oracle.huffman_compress(_text(5000 + i, 200 + (i * 53) % 3000)) for i in range(1000)]
    hdec, p = _prof(_lib, lambda: huffman.DecompressBatch(hstreams))
    assert p == {"huff_batch_dec": 1}, p
    assert hdec[:50] == [oracle.huffman_decompress(s) for s in hstreams[:50]]


def test_small_lzss_decoder_group_ends_on_the_byte_limit(mods, oracle):
    """The small LZSS decoder's output slot is the full 8 KiB + 16 whatever the stream's length, so a stream of at most 16 bytes takes
    16 (entry) + 16 + 32 (input) + 8192 + 16 (output) + 16 (status) = 8288 bytes of a group's 16 MiB of staging: 2024 such members are
    one launch, and the 2025th starts the next."""
    _lib, _, lz = mods
    stream = oracle.lzss_compress(README[0])
    assert len(stream) <= 16
    need = 16 + 16 + 32 + 8192 + 16 + 16
    assert (need, (16 << 20) // need) == (8288, 2024)
    want = oracle.lzss_decompress(stream)
    assert want == README[0]
    for members, launches in ((2024, 1), (2025, 2)):
        dec, p = _prof(_lib, lambda: lz.DecompressBatch([stream] * members))
        assert p == {"lzss_batch_dec": launches}, p
        assert dec == [want] * members


def _payload(stream):
    return len(stream) - stream.index(b"\\\n") - 3


def test_huffman_one_workgroup_cutoff(mods, oracle):
    """A stream with exactly BATCH_GROUP_PAYLOAD_MAX payload bytes is one workgroup of the grouped kernel; one byte more is the single
    call's; both equal the single call."""
    _lib, huffman, _ = mods
    src = np.random.default_rng(12).integers(48, 88, size=40000, dtype=np.uint8).tobytes()   # 40 symbols: ~5.3 bits each
    lo, hi = 1000, len(src)                                    # the longest prefix whose payload is <= the cutoff
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if _payload(oracle.huffman_compress(src[:mid])) <= huffman.BATCH_GROUP_PAYLOAD_MAX:
            lo = mid
        else:
            hi = mid - 1
    inside = oracle.huffman_compress(src[:lo])
    k = lo + 1
    while _payload(oracle.huffman_compress(src[:k])) <= huffman.BATCH_GROUP_PAYLOAD_MAX:
        k += 1
    outside = oracle.huffman_compress(src[:k])
    assert _payload(inside) == huffman.BATCH_GROUP_PAYLOAD_MAX and _payload(outside) == huffman.BATCH_GROUP_PAYLOAD_MAX + 1
    assert lo <= huffman.BATCH_GROUP_OUTPUT_MAX
    got, p = _prof(_lib, lambda: huffman.DecompressBatch([inside, inside]))
    assert p == {"huff_batch_dec": 1}, p
    assert got == [huffman.Decompress(inside)] * 2 == [oracle.huffman_decompress(inside)] * 2
    got, p = _prof(_lib, lambda: huffman.DecompressBatch([outside, outside]))
    assert "huff_batch_dec" not in p and p, p
    assert got == [huffman.Decompress(outside)] * 2 == [oracle.huffman_decompress(outside)] * 2


# ---------------------------------------------------------------- errors
def test_a_failing_member_fails_the_batch(mods, oracle):
    _lib, huffman, lz = mods
    from raisin_amd import RsnError
    good_h = [oracle.huffman_compress(_text(i, 300)) for i in range(10)]
    bad_h = b"1|a1|b\\\n\x09\x80"                                    # the pad exceeds the payload
    with pytest.raises(RsnError) as single:
        huffman.Decompress(bad_h)
    good_l = [oracle.lzss_compress(_text(i, 300)) for i in range(10)]
    bad_l = b"ab<5,3>cd"                                                # a back-pointer before the data
    with pytest.raises(RsnError) as single_l:
        lz.Decompress(bad_l)
    for fn, good, bad, ref in ((huffman.DecompressBatch, good_h, bad_h, single.value),
                               (lz.DecompressBatch, good_l, bad_l, single_l.value)):
        members = list(good)
        members[5] = bad
        members[8] = bad                                                # a later failure does not change the answer
        with pytest.raises(RsnError) as e:
            fn(members)
        assert e.value.code == ref.code == -3
        msg = _lib.lib().rsn_last_error().decode()
        assert msg.startswith("member 5: "), msg
        assert msg[len("member 5: "):] == str(ref).split(": ", 1)[1]
        assert len(fn(good)) == 10                                      # the thread goes on
    assert ref.code == -3


def test_outs_are_null_after_a_failure(mods, oracle):
    import ctypes
    _lib, _, _ = mods
    L = _lib.lib()
    bufs = [oracle.lzss_compress(_text(i, 200)) for i in range(4)] + [b"<9,9>"]
    k = len(bufs)
    ins = (ctypes.c_char_p * k)(*bufs)
    lens = (ctypes.c_size_t * k)(*[len(b) for b in bufs])
    outs = (ctypes.POINTER(ctypes.c_uint8) * k)()
    olens = (ctypes.c_size_t * k)()
    assert L.rsn_lzss_decompress_batch(k, ins, lens, outs, olens) == -3
    assert all(not outs[i] for i in range(k)) and all(olens[i] == 0 for i in range(k))
    assert L.rsn_last_error().startswith(b"member 4: ")


# ---------------------------------------------------------------- concurrency
def _mixed(oracle):
    datas = README + [_text(i, 50 + 37 * i) for i in range(40)] + [_text(99, 300000), b"r" * 1024]
    return datas, [oracle.lzss_compress(d) for d in datas], [oracle.huffman_compress(d) for d in datas]


def test_four_threads_share_inputs(mods, oracle):
    _, huffman, lz = mods
    datas, lstreams, hstreams = _mixed(oracle)
    want = (lz.CompressAsyncBatch(datas), lz.DecompressBatch(lstreams), huffman.DecompressBatch(hstreams))
    assert want[1] == datas and want[2] == [huffman.Decompress(s) for s in hstreams]      # (a one-symbol file: lossy, as the reference)

    def run(_):
        out = []
        for _ in range(3):
            out.append((lz.CompressAsyncBatch(datas), lz.DecompressBatch(lstreams), huffman.DecompressBatch(hstreams)))
        return out

    with concurrent.futures.ThreadPoolExecutor(4) as ex:
        for res in ex.map(run, range(4)):
            for r in res:
                assert r == want


def test_batch_workers_give_the_same_bytes(mods, oracle, tmp_path):
    _, huffman, lz = mods
    datas, lstreams, hstreams = _mixed(oracle)
    want = lz.CompressAsyncBatch(datas) + lz.DecompressBatch(lstreams) + huffman.DecompressBatch(hstreams)
    import pickle
    inp = tmp_path / "in.pkl"
    outp = tmp_path / "out.pkl"
    inp.write_bytes(pickle.dumps((datas, lstreams, hstreams)))
    script = ("import pickle, sys\n"
              "sys.path.insert(0, %r)\n"
              "from raisin_amd import huffman, lz\n"
              "d, l, h = pickle.load(open(%r, 'rb'))\n"
              "pickle.dump(lz.CompressAsyncBatch(d) + lz.DecompressBatch(l) + huffman.DecompressBatch(h), open(%r, 'wb'))\n"
              % (ROOT, str(inp), str(outp)))
    subprocess.run([sys.executable, "-c", script], check=True, timeout=300, env=dict(os.environ, RSN_BATCH_WORKERS="3"))
    assert pickle.loads(outp.read_bytes()) == want


# ---------------------------------------------------------------- the engine and the C++ host
def _files(tmp_path, stem, datas):
    paths = []
    for i, d in enumerate(datas):
        p = tmp_path / ("%s%d.txt" % (stem, i))
        p.write_bytes(d)
        paths.append(str(p))
    return paths


@pytest.fixture(scope="module")
def exe():
    e = os.path.join(ROOT, "raisin_amd", "host", "rsn")
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(e)])
    return e


def test_hosts_route_one_layer_lists_through_the_batch(mods, oracle, samiam, tmp_path, exe):
    from raisin_amd import engine
    datas = README + [samiam, _text(20, 1024), b"", b"w" * 1024, _text(21, 200000)]
    paths = _files(tmp_path, "f", datas)
    engine.CompressFiles(["lzss"], paths, ".pyl")
    out = subprocess.check_output([exe, "-compress", ",".join(paths), "-algorithm=lzss", "-outext=cl"]).decode()
    assert out.count("Compressing...") == len(datas)
    for p, d in zip(paths, datas):
        assert open(p + ".pyl", "rb").read() == oracle.lzss_compress(d)
        assert open(p + ".cl", "rb").read() == oracle.lzss_compress(d)
    for layer, codec, decode in (("lzss", oracle.lzss_compress, oracle.lzss_decompress),
                                 ("huffman", oracle.huffman_compress, oracle.huffman_decompress)):
        keep = [d for d in datas if layer == "lzss" or d]
        src = _files(tmp_path, "s" + layer, keep)
        comp = []
        for p, d in zip(src, keep):
            open(p + ".z", "wb").write(codec(d))
            comp.append(p + ".z")
        engine.DecompressFiles([layer], comp, ".py")
        out = subprocess.check_output([exe, "-decompress", ",".join(comp), "-algorithm=" + layer, "-outext=cc", "-delete=false"]).decode()
        assert out.count("Decompressing...") == len(keep)
        want = [decode(codec(d)) for d in keep]                        # (the per-file loop's: a one-symbol Huffman file is lossy, as the reference)
        for c, w in zip(comp, want):
            assert open(c + ".py", "rb").read() == w
            assert open(c + ".cc", "rb").read() == w
            assert os.path.exists(c)
        subprocess.check_call([exe, "-decompress", ",".join(comp), "-algorithm=" + layer, "-outext=dd"])   # -delete defaults to true
        for c, w in zip(comp, want):
            assert open(c + ".dd", "rb").read() == w and not os.path.exists(c)


def test_hosts_keep_the_loops_semantics_when_the_third_file_fails(mods, oracle, samiam, tmp_path, exe):
    from raisin_amd import RsnError, engine
    datas = [samiam, _text(30, 900), b"", _text(31, 700)]
    for layer, codec, bad in (("lzss", oracle.lzss_compress, b"ab<7,2>"), ("huffman", oracle.huffman_compress, b"1|a1|b")):
        src = _files(tmp_path, "t" + layer, datas)
        comp = []
        for i, (p, d) in enumerate(zip(src, datas)):
            open(p + ".z", "wb").write(bad if i == 2 else codec(d if d else b"ok"))
            comp.append(p + ".z")
        with pytest.raises(RsnError):
            engine.DecompressFiles([layer], comp, ".py")
        r = subprocess.run([exe, "-decompress", ",".join(comp), "-algorithm=" + layer, "-outext=cc"], capture_output=True, text=True)
        assert r.returncode != 0
        for ext in (".py", ".cc"):
            for k in (0, 1):
                assert open(comp[k] + ext, "rb").read() == datas[k]
            assert not os.path.exists(comp[3] + ext)
        assert all(os.path.exists(c) for c in comp)                   # nothing deleted: not every output was written
    # lzss compress: a third file that cannot be read
    paths = _files(tmp_path, "u", [samiam, _text(32, 500), b"x", _text(33, 400)])
    missing = [paths[0], paths[1], str(tmp_path / "not_there.txt"), paths[3]]
    with pytest.raises(OSError):
        engine.CompressFiles(["lzss"], missing, ".pyl")
    r = subprocess.run([exe, "-compress", ",".join(missing), "-algorithm=lzss", "-outext=cl"], capture_output=True, text=True)
    assert r.returncode != 0 and r.stdout.count("Compressing...") == 2
    for ext in (".pyl", ".cl"):
        for k in (0, 1):
            assert open(missing[k] + ext, "rb").read() == oracle.lzss_compress(open(missing[k], "rb").read())
        assert not os.path.exists(paths[3] + ext)
