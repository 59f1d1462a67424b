"""GPU: rsn_huffman_compress_batch with its grouped members (k_huff_batch_enc: one launch per group, a workgroup per member that builds
its own Go-exact tree).  Every output equals Compress(member) and the CPU oracle; members the kernel does not take keep the
pipeline, in index order; a round trip through the grouped encoder and decoder is one launch each way."""
import concurrent.futures
import os
import pickle
import random
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
README = [b"Hello world!\n", b"abcabcabcabcabcabcabcabc\n"]        # the reference README's two files (13 and 25 bytes)
WORDS = [b"the", b"quick", b"brown", b"fox", b"jumps", b"over", b"lazy", b"dog", b"compression", b"a", b"I", b"Sam", b"ham"]
GENERAL = ("huff_byte_hist", "huff_rune", "huff_tile_bits", "huff_emit")   # name fragments of the general encoder's launches


def _text(seed, n):
    rng = random.Random(seed)
    t = bytearray()
    while len(t) < n:
        t += rng.choice(WORDS) + rng.choice([b" ", b"\n", b", ", b". "])
    return bytes(t[:n])


def _ascii(seed, n):
    return np.random.default_rng(seed).integers(0, 128, size=n, dtype=np.uint8).tobytes()


def _with_counts(seed, table):
    """bytes whose counts are `table` ({byte: count}), shuffled"""
    b = bytearray()
    for sym, cnt in table.items():
        b += bytes([sym]) * cnt
    rng = random.Random(seed)
    lst = list(b)
    rng.shuffle(lst)
    return bytes(lst)


def _tie_tables():
    fib, f0, f1 = {}, 1, 1
    for k in range(19):                                            # 1, 1, 2, 3, 5, ... 4181: the deepest codes (10945 bytes)
        fib[48 + k] = f0
        f0, f1 = f1, f0 + f1
    return [
        {b: 100 for b in range(128)},                              # every count equal, 128 symbols
        {b: 7 for b in range(32, 40)},
        {65 + k: 1 << k for k in range(14)},                       # powers of two (16383 bytes)
        fib,
        {b: 3 + (b % 3) for b in range(10, 100)},                  # many duplicate counts, newline among them
        {0x41: 5, 0x42: 5, 0x5C: 9},                               # '\\' the highest byte: its entry goes first
        {0x0A: 12, 0x5C: 12},
        {0: 1, 127: 16382},                                        # two symbols, 16 KiB
    ]


@pytest.fixture(scope="module")
def mods():
    from raisin_amd import _lib, huffman
    return _lib, huffman


def _prof(_lib, fn):
    _lib.prof_enable(True)
    _lib.prof_reset()
    try:
        res = fn()
        return res, {k: v[0] for k, v in _lib.prof_get().items() if v[0]}
    finally:
        _lib.prof_enable(False)


def _members(samiam):
    out = list(README) + [samiam, _text(1, 1024)]
    out += [_ascii(2, 2), _ascii(3, 16383), _ascii(4, 16384), _ascii(5, 16385)]
    out += [b"ab" * 9, b"abc" * 7, bytes(range(1, 128)) * 3, bytes(range(128)) * 2]
    out += [_with_counts(k, t) for k, t in enumerate(_tie_tables())]
    return out


def test_grouped_bytes_equal_the_single_call_and_the_oracle(mods, oracle, samiam):
    _lib, huffman = mods
    members = _members(samiam)
    got, p = _prof(_lib, lambda: huffman.CompressBatch(members))
    assert len(got) == len(members)
    for d, g in zip(members, got):
        assert g == huffman.Compress(d), len(d)
        assert g == oracle.huffman_compress(d), len(d)
    assert p.get("huff_batch_enc") == 1, p                         # (16385 B: over the cutoff, the pipeline's)
    assert huffman.BATCH_COMPRESS_INPUT_MAX == 16384


def test_a_thousand_members_are_one_launch(mods, oracle):
    _lib, huffman = mods
    rng = random.Random(11)
    datas = [_text(k, rng.choice([13, 25, 200, 1024, 4000, 16384])) for k in range(1000)]
    got, p = _prof(_lib, lambda: huffman.CompressBatch(datas))
    assert p == {"huff_batch_enc": 1}, p
    for d, g in zip(datas, got):
        assert g == oracle.huffman_compress(d)
    datas = [README[k % 2] for k in range(4097)]                     # SMALL_GROUP_MAX members a group
    got, p = _prof(_lib, lambda: huffman.CompressBatch(datas))
    assert p == {"huff_batch_enc": 2}, p
    assert got == [oracle.huffman_compress(d) for d in datas]


def test_routing_keeps_index_order(mods, oracle):
    _lib, huffman = mods
    datas = []
    for k in range(12):
        datas += [_text(40 + k, 30 + 50 * k), b"z" * (k + 1), bytes([0xC3, 0xA9]) * (k + 2) + b"abc", _text(60 + k, 20 << 10)]
    got, p = _prof(_lib, lambda: huffman.CompressBatch(datas))
    assert p.get("huff_batch_enc") == 1, p
    for d, g in zip(datas, got):
        assert g == oracle.huffman_compress(d) == huffman.Compress(d), len(d)
    # only the handed-back members (and the 20 KiB ones) take the general path (the pipeline's encoder thread: its launches are counted
    # on that thread's context, not on this one's)
    only_grouped, q = _prof(_lib, lambda: huffman.CompressBatch(datas[0::4]))
    assert q == {"huff_batch_enc": 1}, q
    assert not any(any(g in k for g in GENERAL) for k in q)
    assert only_grouped == got[0::4]
    back, r = _prof(_lib, lambda: huffman.CompressBatch(datas[1::4] + datas[2::4]))
    assert r == {"huff_batch_enc": 1}, r                            # every member handed back, then the pipeline
    assert back == [oracle.huffman_compress(d) for d in datas[1::4] + datas[2::4]]


def test_round_trip_is_one_launch_each_way(mods, samiam):
    _lib, huffman = mods
    datas = [_text(k, 13 + 53 * k) for k in range(300)] + [samiam]
    comp, p = _prof(_lib, lambda: huffman.CompressBatch(datas))
    assert p == {"huff_batch_enc": 1}, p
    dec, q = _prof(_lib, lambda: huffman.DecompressBatch(comp))
    assert q == {"huff_batch_dec": 1}, q
    assert dec == datas


def test_batch_workers_give_the_same_bytes(mods, oracle, tmp_path):
    _, huffman = mods
    datas = README + [_text(k, 40 + 300 * k) for k in range(30)] + [b"y" * 50, _text(77, 100000), bytes([0xE2, 0x82, 0xAC]) * 9]
    want = [oracle.huffman_compress(d) for d in datas]
    assert huffman.CompressBatch(datas) == want
    inp, outp = tmp_path / "in.pkl", tmp_path / "out.pkl"
    inp.write_bytes(pickle.dumps(datas))
    script = ("import pickle, sys\n"
              "sys.path.insert(0, %r)\n"
              "from raisin_amd import huffman\n"
              "pickle.dump(huffman.CompressBatch(pickle.load(open(%r, 'rb'))), open(%r, 'wb'))\n" % (ROOT, str(inp), str(outp)))
    for w in ("1", "2", "8"):
        subprocess.run([sys.executable, "-c", script], check=True, timeout=300, env=dict(os.environ, RSN_BATCH_WORKERS=w))
        assert pickle.loads(outp.read_bytes()) == want, w


def test_four_threads_compress_the_same_inputs(mods, oracle):
    _, huffman = mods
    datas = README + [_text(k, 13 + 211 * k) for k in range(60)] + [b"q" * 9, _text(88, 30000)]
    want = [oracle.huffman_compress(d) for d in datas]

    def run(_):
        return [huffman.CompressBatch(datas) for _ in range(3)]

    with concurrent.futures.ThreadPoolExecutor(4) as ex:
        for res in ex.map(run, range(4)):
            for r in res:
                assert r == want


def test_an_empty_member_still_fails_the_whole_batch(mods):
    from raisin_amd import RsnError
    _, huffman = mods
    with pytest.raises(RsnError):
        huffman.CompressBatch([b"abc", b"", b"de"])
