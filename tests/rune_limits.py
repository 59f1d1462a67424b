"""Inputs that hold the grouped rune kernels (k_huff_batch_rune_enc, huff_rune.hip; k_huff_batch_rune_dec, huff_rune_dec.hip) at their limits:
the open-addressing table's probe chains and its wrap from slot 511 to slot 0, runes and invalid forms that a 16-byte unit or a round of
256 units (byte 4096) cuts, the deepest trees (18 bits to encode 16 KiB, 32 bits to decode), and the lane decoder's 576 bits per lane.
tests/test_rune_limits_host.py holds these builders against the kernels' own hash and plan on a CPU, so that the GPU tests
(test_gpu_huffman_rune_limits.py, test_gpu_huffman_rune_dec_limits.py) cannot quietly test something easier.  Nothing here needs a GPU or
the library; streams are built with test_gpu_huffman_rune_dec_batch's _build and _codes (the reference's tree, restated in Python)."""
import random

import numpy as np

from test_gpu_huffman_rune_batch import CLEF, E_ACUTE, INVALID, _prefixed
from test_gpu_huffman_rune_dec_batch import _build, _codes

COPIES = 16                                              # huffman.RUNE_GROUP_MIN and RUNE_DEC_GROUP_MIN: every shape in that many variants
SLOTS = 512                                              # HR_SLOTS, PARSE_RUNE_SLOTS
FFFD = 0xFFFD
SLOT_FFFD = 318                                          # slot(U+FFFD)
FORMS = INVALID + (b"\xf0\x9f\x98",)                     # the invalid forms a unit may split; every byte of one is U+FFFD


# ---------------------------------------------------------------- the hash
def slot(r):
    """plan_rune_hash (huff_plan_rune.h): a rune's first slot"""
    return ((r * 0x9E3779B1) & 0xFFFFFFFF) >> 23


_BY_SLOT = []


def _by_slot():
    """the valid non-surrogate runes >= 0x80 of every slot, ascending"""
    if not _BY_SLOT:
        r = np.arange(0x80, 0x110000, dtype=np.uint64)
        r = r[(r < 0xD800) | (r >= 0xE000)]
        s = ((r * 0x9E3779B1) & 0xFFFFFFFF) >> 23
        order = np.argsort(s, kind="stable")
        r, s = r[order], s[order]
        cuts = np.searchsorted(s, np.arange(SLOTS + 1))
        _BY_SLOT.extend(r[cuts[k]:cuts[k + 1]] for k in range(SLOTS))
    return _BY_SLOT


def colliders(s, k):
    """the first k valid non-surrogate runes >= 0x80 whose slot is s"""
    runes = _by_slot()[s]
    assert len(runes) >= k
    return [int(x) for x in runes[:k]]


def width(r):
    return 1 if r < 0x80 else 2 if r < 0x800 else 3 if r < 0x10000 else 4


# ---------------------------------------------------------------- encoder: collision chains
def _counted(runes, v, extra=()):
    """rune i of `runes` 1 + i % 3 times; variant v rotates which comes first, odd variants are shuffled.  extra: byte strings placed among
    the last quarter of the runes and behind them"""
    cnt = {r: 1 + i % 3 for i, r in enumerate(runes)}
    k = 16 * v % len(runes)
    parts = [chr(r).encode() for r in runes[k:] + runes[:k] for _ in range(cnt[r])]
    if v % 2:
        random.Random(v).shuffle(parts)
    for j, e in enumerate(extra):
        parts.insert(len(parts) - (len(extra) - 1 - j) * 9, e)
    return b"".join(parts)


def chain_runes(name):
    """the alphabets of the chain shapes, 252 to 256 distinct runes"""
    if name == "slot 511":
        return colliders(511, 256)                       # the chain wraps through slots 0 to 254
    if name == "slot 0":
        return colliders(0, 256)
    if name == "slot of U+FFFD":
        return [r for r in colliders(SLOT_FFFD, 257) if r != FFFD][:255]       # U+FFFD itself is the 256th: invalid bytes and a literal EF BF BD
    if name == "slots 505 to 511":
        return [r for s in range(505, 512) for r in colliders(s, 36)]          # seven overlapping chains across the wrap
    raise KeyError(name)


CHAINS = ("slot 511", "slot 0", "slot of U+FFFD", "slots 505 to 511")


def chain_member(name, v):
    extra = ()
    if name == "slot of U+FFFD":
        extra = (b"\xff", b"\xef\xbf\xbd", b"\x80", b"\xef\xbf\xbd", b"\xff", b"\xc0", b"\xef\xbf\xbd", b"\xff")
    return _counted(chain_runes(name), v, extra)


# ---------------------------------------------------------------- encoder: more runes than the class takes
def _many(v):
    """5461 distinct 3-byte runes"""
    return "".join(chr(0x800 + 7 * v + k) for k in range(5461)).encode()


def overflow_shapes():
    """[(name, variant(v) -> bytes)]: handed back.  The last two fill the table's 512 slots while 256 threads insert; with 200 ASCII
    bytes in front the runes are cut to what 16384 bytes leave, the class's largest member"""
    return [("257 colliders of slot 511", lambda v: _counted(colliders(511, 257), v)),
            ("300 distinct runes", lambda v: "".join(chr(0x100 + 7 * v + k) for k in range(300)).encode()),
            ("5461 distinct runes", _many),
            ("200 ASCII bytes, then distinct runes", lambda v: bytes(0x41 + (k + v) % 26 for k in range(200)) + _many(v)[:(16384 - 200) // 3 * 3])]


# ---------------------------------------------------------------- encoder: the classifier at unit and round edges
def _pair(w, v):
    a = (0x4E00 if w == 3 else 0x1F600) + 2 * v
    return chr(a).encode(), chr(a + 1).encode()


def _two_runes(w, k, seed):
    """k runes of width w, each one of two by a coin"""
    rng = random.Random(seed)
    a, b = _pair(w, seed % COPIES)
    return b"".join(a if rng.random() < 0.5 else b for _ in range(k))


def phase_shapes():
    """runes of width 3 and 4 behind 0 to 15 ASCII bytes, past byte 4096 and byte 8192: every phase of a rune against the units and the rounds"""
    return [("width %d at phase %d" % (w, p), (lambda w, p: lambda v: b"a" * p + _two_runes(w, 8200 // w + 1, 1000 * w + 16 * p + v))(w, p)) for w in (3, 4) for p in range(16)]


def end_shapes():
    """members that end on a rune's last byte at 16384, and members cut one, two and three bytes into a last 4-byte rune"""
    out = [("16384 ending on a 3-byte rune", lambda v: b"a" + _two_runes(3, 5461, 5000 + v)),
           ("16384 of 4-byte runes", lambda v: _two_runes(4, 4096, 6000 + v))]
    out += [("cut %d into a 4-byte rune" % c, _prefixed(b"clef " + CLEF + b" and " + E_ACUTE + b" then " + CLEF[:c])) for c in (1, 2, 3)]
    return out


def split_member(f, s, at, v):
    """form f with byte `at` of the member between its bytes s - 1 and s, text around it"""
    letter = bytes([0x41 + v])
    pre = (E_ACUTE + (letter + b"bcdefg ") * (at // 8 + 1))[:at - s]
    return pre + f + b" and more " + E_ACUTE + letter + b" text"


def split_shapes():
    """every form and every split at a unit boundary (byte 64), and at the boundary between two rounds (byte 4096)"""
    return [("%s split %d at %d" % (f.hex(), s, at), (lambda f, s, at: lambda v: split_member(f, s, at, v))(f, s, at))
            for at in (64, 4096) for f in FORMS for s in range(1, len(f))]


# ---------------------------------------------------------------- encoder: the deepest tree and the densest lanes
FIB_SYMS = 20
FIB_DEPTH = 18                                           # the deepest code of fib_counts() by oracle.huffman_table (asserted on a CPU and on the GPU)


def fib_counts():
    """Fibonacci counts of 20 symbols, the two rarest 2-byte runes, the last count cut so that the member is 16384 bytes"""
    c, f0, f1 = [], 1, 1
    while len(c) < FIB_SYMS:
        c.append(f0)
        f0, f1 = f1, f0 + f1
    c[-1] = 16384 - 2 * c[0] - 2 * c[1] - sum(c[2:-1])
    assert c[-1] > c[-3]
    return c


def fib_symbols(v):
    return [chr(0xC0 + 2 * v), chr(0xC1 + 2 * v)] + list("ABCDEFGHIJKLMNOPQRSTUVWXYZ"[v % 8:v % 8 + FIB_SYMS - 2])


RUN_AT = {"aligned to a unit": 1024, "across a unit": 1032, "in the last unit": 16384 - 16, "across byte 4096": 4096 - 8}


def fib_member(order, v):
    """order: 'shuffled', 'sorted' (the rarest first, in runs) or a key of RUN_AT: the two deepest ASCII symbols that occur eight times
    (counts 8 and 13: codes of 14 and 13 bits) alternate through the 16 bytes at that position, everything else shuffled"""
    syms, c = fib_symbols(v), fib_counts()
    if order == "sorted":
        return "".join(s * k for s, k in zip(syms, c)).encode()
    if order == "shuffled":
        chars = [s for s, k in zip(syms, c) for _ in range(k)]
        random.Random(v).shuffle(chars)
        return "".join(chars).encode()
    x, y = syms[5], syms[6]
    assert (c[5], c[6]) == (8, 13)
    rest = [s for s, k in zip(syms[2:], c[2:]) for _ in range(k - (8 if s in (x, y) else 0))]
    random.Random(v).shuffle(rest)
    at = RUN_AT[order] - 4                               # the two runes lie in front: four bytes, and only ASCII behind them
    return "".join(syms[:2] + rest[:at] + [x, y] * 8 + rest[at:]).encode()


def fib_shapes():
    return [("fibonacci " + o, (lambda o: lambda v: fib_member(o, v))(o)) for o in ("shuffled", "sorted") + tuple(RUN_AT)]


# ---------------------------------------------------------------- decoder: collision chains in the header
def chain_stream(v, k=256, twice=False):
    """k colliders of slot 511 as entries in descending order, a text that uses every one.  twice: every fourth has an earlier entry with
    another count in front of those -- the later one must find the slot down the chain, and its count decides the tree"""
    runes = colliders(511, k)
    cnt = {chr(r): 1 + (i + v) % 3 for i, r in enumerate(runes)}
    ents = [(cnt[chr(r)], chr(r), None) for r in reversed(runes)]
    if twice:
        ents = [(40 + i, chr(r), None) for i, r in enumerate(runes) if i % 4 == 0] + ents
    chars = [r for r, c in cnt.items() for _ in range(c)]
    random.Random(v).shuffle(chars)
    text = "".join(chars)
    return _build(ents, text), text


# ---------------------------------------------------------------- decoder: trees of 24, 25, 32 and 33 bits
ASCII_ZERO = "ABCDEFGHIJKLMNOPQRSTUVWXYZcdefghijklmnopqrstuvwxyz!#$%&()*+,-./:;<=>?@"     # (no 'a', no 'b', no digit, '|', '\\' or newline)
DEPTH_OF_Z = {25: 24, 26: 25, 57: 32, 58: 33}           # the deepest code of deep_leaves(z), by _codes


def deep_leaves(z, rune=True, counts=(5, 9)):
    """z zero-count entries -- U+0400 and up, or ASCII -- and two counted ones: [(count, rune as a string)].  Go's heap pops the zeros in
    an order that makes the tree a comb."""
    zero = [chr(0x400 + k) for k in range(z)] if rune else list(ASCII_ZERO[:z])
    return [(0, r) for r in zero] + [(counts[0], "a"), (counts[1], "é" if rune else "b")]


def depth(leaves):
    return max(len(c) for c in _codes([(c, ord(r)) for c, r in leaves]).values())


DEEP_USES = ("first bits", "last bits", "twenty in a row", "across lane starts")


def deep_text(leaves, use, v, fill_bits=0):
    """a text over the two counted symbols that uses the two deepest zero-count symbols: at the payload's first bits, at its last, twenty
    times in a row, or so that a deep code crosses every one of 72 lane starts of 64 bits (1 to 31 bits of it in front of the start).
    fill_bits: that many bits more of the counted symbols, away from the deep codes (the mid class's payloads)"""
    codes = _codes([(c, ord(r)) for c, r in leaves])
    deepest = max(len(c) for c in codes.values())
    d0, d1 = sorted(chr(r) for r, c in codes.items() if len(c) == deepest)
    lo = [r for c, r in leaves if c]
    rng = random.Random(7000 + v)

    def fill(bits):
        out, n = [], 0
        while n < bits:
            out.append(lo[rng.random() < 0.5])
            n += len(codes[ord(out[-1])])
        return out
    if use == "across lane starts":
        one = next(r for r in lo if len(codes[ord(r)]) == 1)
        out, at = [], 0
        for k in range(1, 73):
            start = 64 * k - 1 - (7 * k + v) % 31
            body = fill(max(start - at - 8, 0))
            at += sum(len(codes[ord(r)]) for r in body)
            out += body + [one] * (start - at) + [(d0, d1)[k % 2]]
            at = start + deepest
        return "".join(out + fill(40 + fill_bits))
    body = {"first bits": [d0, d1] + fill(300), "last bits": fill(300) + [d0, d1], "twenty in a row": fill(150) + [d0, d1] * 10 + fill(150)}[use]
    return "".join(fill(fill_bits) + body) if use != "first bits" else "".join(body + fill(fill_bits))


def deep_stream(z, use, v, rune=True, counts=(5000, 5001), fill_bits=0):
    """-> (stream, text): the header promises counts[0] + 2 * counts[1] bytes (rune) or counts[0] + counts[1], the text stays below"""
    leaves = deep_leaves(z, rune, counts)
    text = deep_text(leaves, use, v, fill_bits)
    assert len(text.encode()) <= sum(c * len(r.encode()) for c, r in leaves)
    return _build([(c, r, None) for c, r in leaves], text), text


# ---------------------------------------------------------------- decoder: the payload limit
PAY_MAX = 18432                                          # HUFF_RUNE_PAY_MAX: 256 lanes of 576 bits
PAY_SEED = 0                                             # (no seed has been rejected: see test_gpu_huffman_rune_dec_limits.py)


def pay_stream(pay_bytes, v, seed=PAY_SEED):
    """z = 25 over ASCII zero-count symbols, 'a' and 'é': a pseudo-random mix of the 24-bit symbol and shallower ones whose code bits are
    exactly pay_bytes bytes (pad 0).  The header promises 16384 bytes, the text stays below.  -> (stream, text)"""
    leaves = [(0, r) for r in ASCII_ZERO[:25]] + [(6384, "a"), (5000, "é")]
    codes = _codes([(c, ord(r)) for c, r in leaves])
    assert max(len(c) for c in codes.values()) == 24
    deep = min(chr(r) for r, c in codes.items() if len(c) == 24)
    rng = random.Random(9000 + 100 * seed + v)
    chars = [deep] * 5800 + [rng.choice(ASCII_ZERO[:25]) for _ in range(500)]
    bits, want = sum(len(codes[ord(r)]) for r in chars), 8 * pay_bytes
    while want - bits > 64:
        chars.append("aé"[rng.random() < 0.5])
        bits += len(codes[ord(chars[-1])])
    rng.shuffle(chars)
    one = "a" if len(codes[ord("a")]) == 1 else "é"
    text = "".join(chars) + one * (want - bits)
    assert len(text.encode()) <= 16384
    s = _build([(c, r, None) for c, r in leaves], text)
    assert len(s) - s.index(b"\\\n") - 3 == pay_bytes and s[s.index(b"\\\n") + 2] == 0
    return s, text


# ---------------------------------------------------------------- every hand-built stream of the decoder's tests
def dec_streams(v):
    """[(name, stream, text, taken by the rune class)], variant v"""
    out = [("256 colliders",) + chain_stream(v) + (True,), ("256 colliders, every fourth twice",) + chain_stream(v, twice=True) + (True,),
           ("257 colliders",) + chain_stream(v, 257) + (False,)]
    for z in (25, 26, 57, 58):
        out += [("depth %d, %s" % (DEPTH_OF_Z[z], use),) + deep_stream(z, use, v) + (DEPTH_OF_Z[z] <= 32,) for use in DEEP_USES]
    out += [("a payload of %d bytes" % n,) + pay_stream(n, v) + (n <= PAY_MAX,) for n in (PAY_MAX, PAY_MAX + 1, PAY_MAX + 4)]
    return out


def byte_streams(v, mid):
    """[(name, stream, text, taken by the byte decoder class)]: the depth-32 and depth-33 pair over ASCII, no rune; mid: the header promises
    40001 bytes and the payload is above 4 KiB, which makes the stream the mid class's"""
    kw = dict(rune=False, counts=(20000, 20001), fill_bits=36000) if mid else dict(rune=False)
    return [("depth %d over bytes, %s" % (DEPTH_OF_Z[z], use),) + deep_stream(z, use, v, **kw) + (z == 57,) for z in (57, 58) for use in DEEP_USES]


def all_runes_used():
    """every rune >= 0x80 the GPU tests put into a member or a header (the hash agreement's domain)"""
    runes = {FFFD, 0xE9} | {r for n in CHAINS for r in chain_runes(n)} | set(colliders(511, 257))
    runes |= {0x100 + 7 * v + k for v in range(COPIES) for k in range(300)} | {0x800 + 7 * v + k for v in range(COPIES) for k in range(5461)}
    runes |= {ord(x.decode()) for w in (3, 4) for v in range(COPIES) for x in _pair(w, v)} | {ord(CLEF.decode())}
    runes |= {ord(s) for v in range(COPIES) for s in fib_symbols(v)[:2]} | {0x400 + k for k in range(58)}
    return sorted(runes)
