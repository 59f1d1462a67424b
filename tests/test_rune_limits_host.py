"""The inputs of the rune kernels' limits tests (tests/rune_limits.py), held against the kernels' own hash and plan on a CPU: the Python slot()
against plan_rune_hash, the colliders, the depth builders, and every hand-built stream of test_gpu_huffman_rune_dec_limits.py against
parse_rune_plan_serial (tests/huff_rune_parse_test.cpp's `slots` and `plan` modes, built with the address and undefined-behaviour
sanitizers) and against the oracle.  Runs on any machine."""
import struct
import subprocess

import numpy as np
import pytest

import rune_limits as R
from test_huff_rune_parse_host import parse_test  # noqa: F401  (the fixture: the program, built once for this module)


def _lines(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.split("\n")[:-1]


def _runes_of(oracle, data):
    return [int(x) for x in oracle.utf8_runes(data)]


# ---------------------------------------------------------------- the hash
def test_slot_is_the_kernels_hash(parse_test):  # noqa: F811
    runes = R.all_runes_used() + list(range(0x80)) + [0x10FFFF, 0xD7FF, 0xE000]
    assert len(runes) > 6000 and R.slot(R.FFFD) == R.SLOT_FFFD
    got = []
    for i in range(0, len(runes), 4000):
        got += _lines(parse_test, "slots", *["0x%X" % r for r in runes[i:i + 4000]])
    assert [int(x) for x in got] == [R.slot(r) for r in runes]


def test_colliders():
    c = R.colliders(511, 257)
    assert len(set(c)) == 257 and c == sorted(c) and all(R.slot(r) == 511 and r >= 0x80 and not 0xD800 <= r < 0xE000 for r in c)
    assert [sum(R.width(r) == w for r in c) for w in (2, 3, 4)] == [4, 120, 133]
    assert c[0] == min(r for r in range(0x80, 0x800) if R.slot(r) == 511)             # the FIRST ones: none skipped
    sizes = [len(x) for x in R._by_slot()]
    assert min(sizes) == 2168 and sum(sizes) == 0x110000 - 0x80 - 0x800
    for name in R.CHAINS:
        runes = R.chain_runes(name)
        assert len(set(runes)) == len(runes) and R.FFFD not in runes
    assert {R.slot(r) for r in R.chain_runes("slot 0")} == {0} and {R.slot(r) for r in R.chain_runes("slot of U+FFFD")} == {R.SLOT_FFFD}
    assert sorted({R.slot(r) for r in R.chain_runes("slots 505 to 511")}) == list(range(505, 512))
    assert [len(R.chain_runes(n)) for n in R.CHAINS] == [256, 256, 255, 252]


# ---------------------------------------------------------------- the depth builders
def test_depth_builders():
    for rune in (True, False):
        assert R.depth(R.deep_leaves(57, rune)) == 32 and R.depth(R.deep_leaves(58, rune)) == 33
        assert R.depth(R.deep_leaves(25, rune)) == 24 and R.depth(R.deep_leaves(26, rune)) == 25
        d = [R.depth(R.deep_leaves(z, rune)) for z in range(1, 60)]
        assert d == sorted(d)
        for counts in ((5000, 5001), (20000, 20001)):
            assert [R.depth(R.deep_leaves(z, rune, counts)) for z in (25, 26, 57, 58)] == [24, 25, 32, 33]
    assert len(set(R.ASCII_ZERO)) == len(R.ASCII_ZERO) >= 58 and not set(R.ASCII_ZERO) & set("ab0123456789|\\\n")


# ---------------------------------------------------------------- the decoder's streams
def test_plan_verdicts_of_the_hand_built_streams(parse_test, oracle, tmp_path):  # noqa: F811
    rows = [(v,) + s for v in range(R.COPIES) for s in R.dec_streams(v)]
    path = tmp_path / "streams.bin"
    path.write_bytes(b"".join(struct.pack("<I", len(s)) + s for _, _, s, _, _ in rows))
    lines = _lines(parse_test, "plan", str(path))
    assert len(lines) == len(rows)
    seen = set()
    for (v, name, s, text, taken), line in zip(rows, lines):
        w = line.split()
        verdict, a, deepest, S, T = w[0], int(w[2]), int(w[4]), int(w[6]), int(w[8])
        assert verdict == ("taken" if taken else "refused"), (name, v, line)
        assert oracle.huffman_decompress(s) == text.encode(), (name, v)
        seen.add(name)
        if name.startswith("depth"):
            assert deepest == int(name[6:8]) and a == {24: 27, 25: 28, 32: 59, 33: 60}[deepest] and S == 64, (name, v, line)
            if name.endswith("across lane starts"):
                assert T >= 64, (name, v, line)
        elif name.startswith("a payload"):
            n = int(name.split()[3])
            assert (deepest, S, T) == {18432: (24, 576, 256), 18433: (0, 0, 0), 18436: (0, 0, 0)}[n], (name, v, line)   # (refused by the lanes, before the tree)
        elif name.startswith("256"):
            assert a == 256 and deepest <= 10, (name, v, line)
        else:
            assert (a, deepest) == (0, 0), (name, v, line)                  # 257 colliders: the table refuses the last
    assert len(seen) == 3 + 16 + 3
    # the later entry decides: with the earlier counts the tree would be another
    s, text = R.chain_stream(0, twice=True)
    assert s.startswith(b"40|") and s != R.chain_stream(0)[0] and s[s.index(b"\\\n"):] == R.chain_stream(0)[0][R.chain_stream(0)[0].index(b"\\\n"):]


def test_the_byte_alphabets_streams(parse_test, oracle, tmp_path):  # noqa: F811
    rows = [s for v in range(4) for mid in (False, True) for s in R.byte_streams(v, mid)]
    for name, s, text, taken in rows:
        assert max(s[:s.index(b"\\\n")]) < 0x80 and oracle.huffman_decompress(s) == text.encode(), name
        pay = len(s) - s.index(b"\\\n") - 3
        assert (pay > 4096 and len(text) <= 40001) or (pay < 4096 and len(text) <= 10001), name
    path = tmp_path / "bytes.bin"
    path.write_bytes(b"".join(struct.pack("<I", len(s)) + s for _, s, _, _ in rows))
    assert set(_lines(parse_test, "plan", str(path))) == {"refused a 0 deepest 0 S 0 T 0"}      # no rune >= 0x80: not the rune class's


# ---------------------------------------------------------------- the encoder's members
def test_the_encoder_members_are_what_they_claim(oracle):
    for name in R.CHAINS:
        for v in range(R.COPIES):
            runes = _runes_of(oracle, R.chain_member(name, v))
            want = set(R.chain_runes(name)) | ({R.FFFD} if name == "slot of U+FFFD" else set())
            assert set(runes) == want and len(want) <= 256, (name, v)
            if name == "slot of U+FFFD":
                assert runes.count(R.FFFD) == 8
    assert len({R.chain_member("slot 511", v) for v in range(R.COPIES)}) == R.COPIES
    for name, variant in R.overflow_shapes():
        for v in (0, R.COPIES - 1):
            d = variant(v)
            runes = _runes_of(oracle, d)
            assert len(set(runes)) > 256 and R.FFFD not in runes and len(d) <= 16384, (name, v)
    assert len(R.overflow_shapes()[2][1](3)) == 16383 and len(R.overflow_shapes()[3][1](3)) == 16382
    for name, variant in R.phase_shapes():
        for v in (0, 7):
            d = variant(v)
            runes = _runes_of(oracle, d)
            assert 8192 < len(d) <= 8220 and R.FFFD not in runes and len(set(runes) - {0x61}) == 2, (name, v)
    ends = dict(R.end_shapes())
    for v in range(R.COPIES):
        for name in ("16384 ending on a 3-byte rune", "16384 of 4-byte runes"):
            d = ends[name](v)
            assert len(d) == 16384 and R.FFFD not in _runes_of(oracle, d)
        for c in (1, 2, 3):
            assert _runes_of(oracle, ends["cut %d into a 4-byte rune" % c](v))[-c - 1:] == [0x20] + [R.FFFD] * c
    for name, variant in R.split_shapes():
        f, s, at = bytes.fromhex(name.split()[0]), int(name.split()[2]), int(name.split()[4])
        for v in (0, 9):
            d = variant(v)
            assert d[at - s:at - s + len(f)] == f and at % 16 == 0 and 0 < s < len(f), name
            assert _runes_of(oracle, d).count(R.FFFD) == len(f), name      # invalid in this context: a byte of it, a U+FFFD
    assert len(R.split_shapes()) == 2 * 10


def test_the_fibonacci_members_depth(oracle):
    c = R.fib_counts()
    assert len(c) == 20 and c[:8] == [1, 1, 2, 3, 5, 8, 13, 21] and c[-1] < 6765
    for name, variant in R.fib_shapes():
        for v in (0, 5, R.COPIES - 1):
            d = variant(v)
            table = oracle.huffman_table(d)
            assert len(d) == 16384 and len(table) == 20 and max(t[3] for t in table) == R.FIB_DEPTH == 18, (name, v)
            assert sorted(t[1] for t in table) == sorted(c)
            if name[10:] in R.RUN_AT:
                at, (x, y) = R.RUN_AT[name[10:]], R.fib_symbols(v)[5:7]
                assert d[at:at + 16] == (x + y).encode() * 8, (name, v)
                lens = {t[0]: t[3] for t in table}
                assert (lens[ord(x)], lens[ord(y)]) == (14, 13)
    runs = [t for t in np.frombuffer(R.fib_member("sorted", 0), dtype=np.uint8)[-R.fib_counts()[-1]:]]
    assert len(set(runs)) == 1
