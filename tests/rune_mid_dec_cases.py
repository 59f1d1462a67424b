"""The streams that hold the mid-size grouped rune decoder (k_huff_mid_rune_dec, raisin_amd/csrc/huff_rune_mid_dec.hip) to its
limits, and the verdict of the CPU model of the lane maps (tests/lane_maps.py, unchanged, with this class's SHAPE) on each of them.
tests/test_huff_rune_mid_dec_host.py pins the verdicts on a CPU, tests/test_gpu_huffman_rune_mid_dec.py runs the same members on the GPU.
Nothing here needs a GPU or the library.  Streams come from the CPU oracle or are built by hand with test_gpu_huffman_rune_dec_batch's
_build and _codes (the reference's tree, restated in Python); every member comes in N variants, the class's minimum."""
import random

import lane_maps as M
import rune_limits as R
from oracle import oracle as O
from test_gpu_huffman_rune_batch import _runes
from test_gpu_huffman_rune_dec_batch import _build, _codes, _spread
from test_gpu_huffman_rune_mid import _text

N = 16                                                   # huffman.RUNE_MID_DEC_GROUP_MIN
OUT_MIN, OUT_MAX, PAY_MAX = 16384, 65536, 69120          # HUFF_RUNE_OUT_MAX (the promise lies above it), HUFF_RUNE_MID_OUT_MAX, HUFF_RUNE_MID_PAY_MAX
SHAPE = M.Shape("rune mid", 960, 1, 576, None, PAY_MAX, OUT_MAX, runes=True)
TEXT_SIZES = (16385, 20000, 40001, 65536)
MODEL_SIZES = (16385, 16400, 20000, 32768, 40001, 49152, 65535, 65536)

_ENC = {}


def enc(d):
    if d not in _ENC:
        _ENC[d] = O.huffman_compress(d)
    return _ENC[d]


def payload(s):
    return len(s) - s.index(b"\\\n") - 3


# ---------------------------------------------------------------- the model's verdict
def table_of(leaves):
    """the model's table [(rune, count, code, length)] of a hand-built header's leaves [(count, rune as a string)]"""
    codes = _codes([(c, ord(r)) for c, r in leaves])
    return [(ord(r), c, int(codes[ord(r)], 2), len(codes[ord(r)])) for c, r in leaves]


def verdict(stream, table, expect=None):
    """(taken, reason, S, T) of the stream in the class's lanes; expect: the symbols the header promises (default: the table's counts)"""
    nxt, flat = M.code_ends(stream, table)
    ln = M.Lanes(nxt, flat, SHAPE)
    if not ln.held:
        return False, "lanes", ln.S, ln.T
    took, why, _ = ln.verdict(sum(f for _, f, _, _ in table) if expect is None else expect)
    return took, why, ln.S, ln.T


def verdict_of_member(d):
    """a member the oracle encodes"""
    return verdict(enc(d), O.huffman_table(d))


# ---------------------------------------------------------------- members the class takes (where the model says so)
def text(n, v):
    return _text(81000 + 16 * (n % 977) + v, n)


def two_kinds(v):
    """16384 four-byte runes of two kinds: 2048 bytes of payload that decode to 65536"""
    a, b = chr(0x1D11E + v), chr(0x1F600 + v)
    leaves = [(8192, a), (8192, b)]
    return _build([(c, r, None) for c, r in leaves], _spread({a: 8192, b: 8192}, v)), leaves


def one_bit(v):
    """two runes at one bit each, 64373 bytes"""
    c1 = 10000 + 3 * v
    leaves = [(64373 - 2 * c1, "a"), (c1, "é")]
    return _build([(c, r, None) for c, r in leaves], _spread({r: c for c, r in leaves}, v)), leaves


def counter(v):
    """256 distinct runes ascending, 127 times, and a tail: equal counts give them consecutive 8-bit codes"""
    return (_runes(0x100 + 7 * v, 256) * 127 + _runes(0x100 + 7 * v, 40 + v)).encode()


MIXED = "a b\ncdeé€𝄞ñü—…𝄢𝅘𝅥𝅮😀z"


def mixed_widths(v):
    """runes of width 1 to 4 by a coin each: rune boundaries fall across the threads' runs and the 16-byte store units everywhere"""
    rng = random.Random(500 + v)
    out = "".join(rng.choice(MIXED) for _ in range(17000 + 101 * v)).encode()
    assert OUT_MIN < len(out) <= OUT_MAX
    return out


def lossy_16385(v):
    """16383 bytes that end in a lone lead byte, which comes back as EF BF BD: a member of less than 16 KiB that promises 16385"""
    return (_runes(0xC0 + v, 37) * 222).encode()[:16383]


def _hand_base(v):
    return {"a": 9000 + v, "é": 5000, "€": 1000, " ": 2000 + v % 3}


def zero_count(v):
    base = _hand_base(v)
    leaves = [(c, r) for r, c in sorted(dict(base, ж=0).items())]
    return _build([(c, r, None) for c, r in leaves], _spread(base, v)), leaves


def replaced(v):
    base = _hand_base(v)
    leaves = [(c, r) for r, c in sorted(base.items())]
    return _build([(777, "€", None)] + [(c, r, None) for c, r in leaves], _spread(base, v)), leaves


def promises_more(v):
    """the header counts 3000 + v more of 'a' than the payload holds: the same tree, fewer decoded bytes than promised -- an answer"""
    base = _hand_base(v)
    leaves = [(c + (3000 + v if r == "a" else 0), r) for r, c in sorted(base.items())]
    return _build([(c, r, None) for c, r in leaves], _spread(base, v)), leaves


HAND = (("largest expansion", two_kinds), ("two runes at one bit", one_bit), ("a zero count", zero_count), ("a later entry replaces", replaced),
        ("promises more than it holds", promises_more))
ORACLE = (("256 distinct runes", counter), ("widths 1 to 4 mixed", mixed_widths), ("lossy, promises 16385", lossy_16385))


def shapes(v):
    """[(name, stream, (taken, reason))], variant v"""
    out = []
    for n in TEXT_SIZES:
        d = text(n, v)
        out.append(("text %d" % n, enc(d), verdict_of_member(d)[:2]))
    for name, f in ORACLE:
        d = f(v)
        out.append((name, enc(d), verdict_of_member(d)[:2]))
    for name, f in HAND:
        s, leaves = f(v)
        out.append((name, s, verdict(s, table_of(leaves))[:2]))
    return out


# ---------------------------------------------------------------- the limits: taken
def pay_stream(pay_bytes, v):
    """rune_limits.pay_stream at this class's lanes: 24-bit codes among shallower ones whose code bits are exactly pay_bytes bytes (pad 0).
    The header promises 64384 bytes, the text stays below.  -> (stream, leaves)"""
    leaves = [(0, r) for r in R.ASCII_ZERO[:25]] + [(36384, "a"), (14000, "é")]
    codes = _codes([(c, ord(r)) for c, r in leaves])
    assert max(len(c) for c in codes.values()) == 24
    deep = min(chr(r) for r, c in codes.items() if len(c) == 24)
    rng = random.Random(9500 + v)
    chars = [deep] * 21500 + [rng.choice(R.ASCII_ZERO[:25]) for _ in range(500)]
    bits, want = sum(len(codes[ord(r)]) for r in chars), 8 * pay_bytes
    while want - bits > 64:
        chars.append("aé"[rng.random() < 0.5])
        bits += len(codes[ord(chars[-1])])
    rng.shuffle(chars)
    one = "a" if len(codes[ord("a")]) == 1 else "é"
    t = "".join(chars) + one * (want - bits)
    assert OUT_MIN < len(t.encode()) <= 64384
    s = _build([(c, r, None) for c, r in leaves], t)
    assert payload(s) == pay_bytes and s[s.index(b"\\\n") + 2] == 0
    return s, leaves


def deep_stream(z, v):
    """rune_limits.deep_stream with a promise of 60002 bytes and 4.5 KiB of payload: a comb of DEPTH_OF_Z[z] bits, twenty deep codes in a row"""
    s, _ = R.deep_stream(z, "twenty in a row", v, counts=(20000, 20001), fill_bits=36000)
    return s, R.deep_leaves(z, True, (20000, 20001))


def count_65536(v):
    """one entry counts 65536, the other -- the rune -- nothing: a promise of exactly 65536 bytes, one bit a symbol"""
    leaves = [(65536, "a"), (0, "é")]
    return _build([(c, r, None) for c, r in leaves], _spread({"a": 40000 + v, "é": 9 + v}, v)), leaves


def limits_taken(v):
    out = []
    for name, (s, leaves) in (("a payload of 69120 bytes", pay_stream(PAY_MAX, v)), ("depth 32", deep_stream(57, v)), ("a count of 65536", count_65536(v))):
        out.append((name, s, verdict(s, table_of(leaves))[:2]))
    return out


# ---------------------------------------------------------------- not this class's: the single call's
def not_taken(v):
    """[(name, stream)]"""
    out = [("promises 65537", enc((_runes(0xC0 + v, 37) * 900).encode()[:65535])),
           ("257 distinct runes", enc((_runes(0x100 + 7 * v, 257) * 40).encode())),
           ("one distinct rune", enc("é".encode() * (9000 + v))),
           ("a count of 65537", _build([(65537, "a", None), (5, "é", None)], _spread({"a": 5000 + v, "é": 5}, v))),
           ("a payload of 69121 bytes", pay_stream(PAY_MAX + 1, v)[0]),
           ("depth 33", deep_stream(58, v)[0]),
           ("promises 16384 from more than 18432 bytes", R.pay_stream(R.PAY_MAX + 1, v)[0])]
    return out
