"""GPU: the grouped Huffman decoder for streams whose header names a rune >= 0x80 (k_huff_batch_rune_dec, raisin_amd/csrc/huff_rune_dec.hip;
DESIGN 4.7): a decompress batch that holds at least huffman.RUNE_DEC_GROUP_MIN such streams runs them one launch per group, in the host
form, the device form (behind one more plan launch, k_huff_dev_rune_plan) and the layered forms.  Every expected byte comes from the CPU
oracle (oracle.huffman_decompress); the streams come from oracle.huffman_compress or are built by hand here (_build), never from the
library.  The instruments are tests/test_gpu_batch_dev.py's -- members back to back in ONE allocation with hostile bytes between and
behind them, outputs with out_cap exactly the result size, the library's launch profile."""
import random

import pytest

from test_gpu_batch_dev import E_CAP, E_FORMAT, OK, Pack, Slots, _batch, _fenced_call, _out_bytes, _prof, _ru16, _single
from test_gpu_huffman_batch_dev import DEC, _run_slots
from test_gpu_huffman_rune_batch import CLEF, E_ACUTE, EURO, INVALID, _prefixed, _runes, _utf8
from test_gpu_lzss_mid import _text

pytestmark = pytest.mark.gpu

GENERAL = ("huff_dec_", "huff_small_dec")                  # name fragments of the single call's launches (huff_decode.hip, huff_small.hip)
RUNE, RUNE_PLAN = "huff_batch_rune_dec", "huff_dev_rune_plan"
LZ, HU = "lzss", "huffman"
FFFD = "\ufffd"


@pytest.fixture(scope="module")
def mods():
    from raisin_amd import _lib, huffman, layers
    _lib.check(_lib.lib().rsn_device_set(0))
    assert huffman.RUNE_DEC_GROUP_MIN >= 16 and huffman.RUNE_OUT_MAX == 16384 and huffman.RUNE_PAY_MAX == 9 * 16384 // 8
    return _lib, huffman, layers


def _general(prof):
    return any(any(f in k for f in GENERAL) for k in prof)


_ENC, _DEC = {}, {}


def _enc(oracle, d):
    if d not in _ENC:
        _ENC[d] = oracle.huffman_compress(d)
    return _ENC[d]


def _dec(oracle, s):
    """the oracle's bytes, computed once per stream"""
    if s not in _DEC:
        _DEC[s] = oracle.huffman_decompress(s)
    return _DEC[s]


# ---------------------------------------------------------------- streams built by hand
def _codes(leaves):
    """{rune: bit string} of the reference's tree over `leaves` [(count, rune)]: leaves by (count, rune), Go's container/heap with Less =
    count strictly less, pop, pop, push; '0' to the left (huffman.go:58-127)"""
    nodes = sorted(leaves)
    heap = list(range(len(nodes)))
    kids = {}

    def less(i, j):
        return nodes[heap[i]][0] < nodes[heap[j]][0]

    def pop():
        n = len(heap) - 1
        heap[0], heap[n] = heap[n], heap[0]
        i = 0
        while True:
            j = 2 * i + 1
            if j >= n:
                break
            if j + 1 < n and less(j + 1, j):
                j += 1
            if not less(j, i):
                break
            heap[i], heap[j] = heap[j], heap[i]
            i = j
        return heap.pop()

    while len(heap) > 1:
        x, y = pop(), pop()
        nodes.append((nodes[x][0] + nodes[y][0], None))
        kids[len(nodes) - 1] = (x, y)
        heap.append(len(nodes) - 1)
        j = len(heap) - 1
        while j:
            i = (j - 1) // 2
            if not less(j, i):
                break
            heap[i], heap[j] = heap[j], heap[i]
            j = i
    out, todo = {}, [(heap[0], "")]
    while todo:
        k, code = todo.pop()
        if k in kids:
            todo += [(kids[k][0], code + "0"), (kids[k][1], code + "1")]
        else:
            out[nodes[k][1]] = code
    return out


def _build(entries, text, between=b"", cut=0):
    """A stream with this header, in this order: entries = [(count, rune, raw)] -- raw: the entry's bytes behind '|' where they are not
    string(rune) (an invalid form that means U+FFFD) -- whose payload codes the runes of `text`.  A later entry for a rune replaces an
    earlier one.  cut: bits dropped from the payload's end (with the pad byte adjusted: whole bytes only)."""
    last = {}
    for count, r, _ in entries:
        last[r] = count or 0
    codes = _codes([(c, ord(r)) for r, c in last.items()])
    bits = "".join(codes[ord(ch)] for ch in text)
    bits = bits[:len(bits) - cut] if cut else bits
    pad = (8 - len(bits) % 8) % 8
    bits = "0" * pad + bits
    hdr = b""
    for count, r, raw in entries:
        hdr += (b"%d|" % count if count is not None else b"|") + (raw if raw is not None else b"\\n" if r == "\n" else r.encode()) + between
    return hdr + b"\\\n" + bytes([pad]) + bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))


def _spread(counts, seed):
    """a text with these counts {rune: count}, shuffled"""
    chars = [r for r, c in counts.items() for _ in range(c)]
    random.Random(seed).shuffle(chars)
    return "".join(chars)


def _hand(v):
    """the hand-built headers the class takes, variant v: [(name, stream)]"""
    base = {"a": 5 + v, "é": 9, "€": 4, "𝄞": 2 + v % 3, " ": 11}
    text = _spread(base, v)
    ents = [(c, r, None) for r, c in sorted(base.items())]
    out = [("descending order", _build(ents[::-1], text))]
    sh = list(ents)
    random.Random(100 + v).shuffle(sh)
    out.append(("shuffled order", _build(sh, text)))
    out.append(("a duplicate entry", _build([(777, "€", None)] + ents, text)))
    out.append(("letters between the entries", _build(ents, text, between=b"xy \t")))
    zero = dict(base, ж=0)
    out.append(("a zero count", _build([(c, r, None) for r, c in sorted(zero.items())], text)))
    out.append(("an empty count", _build([(None, "ж", None)] + ents, text)))
    special = {"\n": 3 + v, "|": 4, "7": 5, "\\": 6, "0": 2, "é": 7}
    out.append(("newline, |, digits and backslash as symbols", _build([(c, r, None) for r, c in sorted(special.items()) if r != "\\"] + [(6, "\\", None), (1, "z", None)],
                                                                      _spread(dict(special, z=1), v))))
    lossy = {"a": 6 + v, FFFD: 5, "b": 3}
    ltext = _spread(lossy, v)
    out.append(("an invalid byte for U+FFFD", _build([(6 + v, "a", None), (3, "b", None), (5, FFFD, b"\xff")], ltext)))
    out.append(("an invalid byte, then a literal EF BF BD", _build([(6 + v, "a", None), (99, FFFD, b"\x80"), (3, "b", None), (5, FFFD, None)], ltext)))
    out.append(("a surrogate's bytes", _build([(6 + v, "a", None), (5, FFFD, b"\xed\xa0\x80"), (3, "b", None)], ltext)))
    out.append(("an over-long form", _build([(6 + v, "a", None), (5, FFFD, b"\xc0\xaf"), (3, "b", None)], ltext)))
    out.append(("a rune the separator cuts", _build([(6 + v, "a", None), (3, "b", None), (5, FFFD, b"\xe2\x82")], ltext)))
    return out


def _largest_expansion(v):
    """two runes of width 4 with 1-bit codes, 4096 symbols: 16384 bytes from 512 bytes of payload"""
    a, b = chr(0x1D11E + v), chr(0x1F600 + v)
    return _build([(2048, a, None), (2048, b, None)], _spread({a: 2048, b: 2048}, v))


def _taken_shapes():
    """[(name, variant(v) -> plain bytes)]: the encoder test's shapes, encoded by the oracle"""
    out = [("width %d" % len(r), _prefixed(b"a" + r)) for r in (E_ACUTE, EURO, CLEF)]
    out.append(("text", _prefixed("héllo wörld, naïve café. ".encode() * 20)))
    out += [("invalid " + f.hex(), _prefixed(b"some text " + f + b" and more of it")) for f in INVALID]
    out.append(("header's special bytes", _prefixed(b"line 1\nline 2 | 3 \\ 4 \\n 5566778899 " + E_ACUTE + b"\n")))
    out.append(("16384 of 2-byte runes", lambda v: (_runes(0xC0 + v, 37) * 222).encode()[:16384]))
    out.append(("256 distinct runes", lambda v: _shuffled("".join(r * (1 + k * k % 11) for k, r in enumerate(_runes(0x100 + 7 * v, 256))), v).encode()))
    return out


def _shuffled(text, seed):
    chars = list(text)
    random.Random(seed).shuffle(chars)
    return "".join(chars)


def _counter(v):
    """256 distinct runes in ASCENDING order, as the encoder's test has them: equal counts give them consecutive codes, so the payload is a
    counter, in which a wrong start stays a consistent parse -- at variants 0 and 10 one lane sees five starts, and more than four phases
    is the lane maps' hand-back (huff_small_body.h).  Which variants the class takes is the verdict of the CPU model of the lane maps
    (tests/lane_maps.py; tests/lane_limit_cases.py: EITHER_WANT pins it): all but 0 and 10."""
    return (_runes(0x100 + 7 * v, 256) + _runes(0x100 + 7 * v, 40 + v)).encode()


def _not_taken(oracle, v):
    """[(name, stream)]: what the class leaves to the single call, which decodes it.  16383 bytes of 2-byte runes end in a lone lead byte,
    which comes back as EF BF BD: the stream promises 16385 bytes, one more than the class holds."""
    out = [("257 distinct runes", _enc(oracle, (_runes(0x100 + 7 * v, 257) + _runes(0x100 + 7 * v, 40 + v)).encode())),
           ("one distinct rune", _enc(oracle, E_ACUTE * (9 + v))),
           ("16383 of 2-byte runes", _enc(oracle, (_runes(0xC0 + v, 37) * 222).encode()[:16383])),
           ("expect 16385", _enc(oracle, b"a" + (_runes(0xC0 + v, 37) * 222).encode()[:16384]))]
    counts = {"b": 10, "a": 30 + v, "é": 50}                        # the header says 25 + v of 'a': the same tree, five bytes fewer than the payload holds
    out.append(("counts that promise fewer bytes", _build([(25 + v, "a", None), (10, "b", None), (50, "é", None)], _spread(counts, v))))
    return out


def _all_shapes(oracle, copies):
    """every shape in `copies` copies with variation: (streams, expected bytes, taken, names)"""
    import lane_limit_cases as C
    streams, taken, names = [], [], []
    for v in range(copies):
        took, why = C.verdict(_counter(v), "rune")                         # the model's: handed back for "phases" at variants 0 and 10
        assert ("rune", took, why) == C.EITHER_WANT["rune counter %d" % v] and why in (None, "phases")
        streams.append(_enc(oracle, _counter(v))); taken.append(took); names.append("256 distinct runes, ascending")
        for name, variant in _taken_shapes():
            streams.append(_enc(oracle, variant(v))); taken.append(True); names.append(name)
        for name, s in _hand(v):
            streams.append(s); taken.append(True); names.append(name)
        streams.append(_largest_expansion(v)); taken.append(True); names.append("largest expansion")
        for name, s in _not_taken(oracle, v):
            streams.append(s); taken.append(False); names.append(name)
    want = [_dec(oracle, s) for s in streams]
    for s, w, n in zip(streams, want, names):
        if n == "largest expansion":
            assert len(w) == 16384 and len(s) - s.index(b"\\\n") - 3 == 512
        if n == "counts that promise fewer bytes":
            assert len(w) == 5 + int(s[:2]) + 10 + 100                    # five bytes more than the header's counts say
        if n in ("an invalid byte for U+FFFD", "a surrogate's bytes", "a rune the separator cuts", "an over-long form", "an invalid byte, then a literal EF BF BD"):
            assert w.count(FFFD.encode()) == 5, n
        if n == "16383 of 2-byte runes":
            assert len(w) == 16385 and w.endswith(FFFD.encode())
        if n == "a zero count":
            assert "ж".encode() not in w and b"0|" in s
    assert max(map(len, want)) == 16385
    return streams, want, taken, names


@pytest.fixture(scope="module")
def shapes(mods, oracle):
    return _all_shapes(oracle, mods[1].RUNE_DEC_GROUP_MIN)


# ---------------------------------------------------------------- 1: shapes, host form and device form
def test_shapes_host_form(mods, oracle, shapes):
    _lib, huffman, _ = mods
    streams, want, taken, names = shapes
    got, prof = _prof(_lib, lambda: huffman.DecompressBatch(streams))[:2]
    for g, w, n in zip(got, want, names):
        assert g == w, n
    assert prof.get(RUNE) == 1, prof
    assert _general(prof)                                                # the shapes listed as not taken took the single call ...
    only, prof = _prof(_lib, lambda: huffman.DecompressBatch([s for s, t in zip(streams, taken) if t]))[:2]
    assert only == [w for w, t in zip(want, taken) if t]
    assert prof == {RUNE: 1}, prof                                       # ... and nothing else did
    for s, w in list(zip(streams, want))[:len(streams) // huffman.RUNE_DEC_GROUP_MIN]:
        assert huffman.Decompress(s) == w


def test_shapes_device_form(mods, oracle, shapes):
    _lib, huffman, _ = mods
    streams, want, taken, names = shapes
    caps = [len(w) if t else _ru16(len(w)) + 16 for w, t in zip(want, taken)]     # exact sizes where the class takes the member
    got, prof, _ = _run_slots(_lib, DEC, streams, caps, behind=lambda i: b"\xac\xbf\x80")
    for g, w, n in zip(got, want, names):
        assert g == w, n
    assert prof.get(RUNE) == 1 and prof.get(RUNE_PLAN) == 1 and prof.get("huff_dev_plan") == 1, prof
    assert _general(prof)
    idx = [i for i, t in enumerate(taken) if t]
    got, prof, _ = _run_slots(_lib, DEC, [streams[i] for i in idx], [len(want[i]) for i in idx])
    assert got == [want[i] for i in idx]
    assert prof == {"huff_dev_plan": 1, RUNE_PLAN: 1, "group_gather": 1, RUNE: 1, "group_scatter": 1}, prof


def test_streams_the_single_call_refuses(mods, oracle):
    """a stream that ends inside a codeword and a header that ends behind '|', among members the class takes: the single call's error"""
    _lib, huffman, _ = mods
    goods = [_enc(oracle, _utf8(k, 40 * k)) for k in range(huffman.RUNE_DEC_GROUP_MIN)]
    counts = {"a": 9, "é": 3, "€": 2}                                 # codes of 1, 2 and 2 bits: nine bits at the end, eight of them cut
    inside = _build([(c, r, None) for r, c in counts.items()], _spread(counts, 1) + "€" + "a" * 7, cut=8)
    behind_bar = b"3|a4|\xc3\xa9" + b"5|" + b"\\\n\x00\x55\x55"
    for bad in (inside, behind_bar):
        with pytest.raises(oracle.OracleError):
            oracle.huffman_decompress(bad)
        with pytest.raises(_lib.RsnError) as single:
            huffman.Decompress(bad)
        streams = goods[:5] + [bad] + goods[5:]
        with pytest.raises(_lib.RsnError) as batch:
            huffman.DecompressBatch(streams)
        assert batch.value.code == single.value.code == E_FORMAT
        assert str(batch.value) == str(single.value).replace(": ", ": member 5: ", 1)
        with pytest.raises(_lib.RsnError) as dev:
            _single(_lib, "rsn_huffman_decompress_dev", bad, 1 << 12)
        pack, slots = Pack(streams), Slots([1 << 12] * len(streams))
        rc, lens, msg = _batch(_lib, DEC, [(pack.ptr(i), len(x), slots.ptr(i), 1 << 12) for i, x in enumerate(streams)])
        assert rc == dev.value.code == E_FORMAT and lens == [0] * len(streams)
        assert "librsn error %d: %s" % (rc, msg) == str(dev.value).replace(": ", ": member 5: ", 1), (msg, str(dev.value))


# ---------------------------------------------------------------- 2: exactly the minimum, and one fewer
def _texts(n):
    """UTF-8 text that repeats nothing: random words, every e with its accent, a few dozen to a few hundred bytes"""
    return [_text(3000 + k, 30 + 41 * k).replace(b"e", E_ACUTE) + ("%d…" % (k * k)).encode() for k in range(n)]


def test_host_form_takes_the_minimum_and_not_one_fewer(mods, oracle):
    _lib, huffman, _ = mods
    n = huffman.RUNE_DEC_GROUP_MIN
    datas = _texts(n)
    streams = [_enc(oracle, d) for d in datas]
    assert [_dec(oracle, s) for s in streams] == datas
    got, prof = _prof(_lib, lambda: huffman.DecompressBatch(streams))[:2]
    assert got == datas
    assert prof == {RUNE: 1}, prof                                       # the rune decoder once, no launch of the general decoder
    got, prof = _prof(_lib, lambda: huffman.DecompressBatch(streams[:n - 1]))[:2]
    assert got == datas[:n - 1]
    assert RUNE not in prof and _general(prof), prof


def test_device_form_takes_the_minimum_and_not_one_fewer(mods, oracle):
    _lib, huffman, _ = mods
    n = huffman.RUNE_DEC_GROUP_MIN
    datas = _texts(n)
    streams = [_enc(oracle, d) for d in datas]
    got, prof, _ = _run_slots(_lib, DEC, streams, [len(d) for d in datas])
    assert got == datas
    assert prof.get(RUNE) == 1 and prof.get(RUNE_PLAN) == 1 and not _general(prof), prof
    got, prof, _ = _run_slots(_lib, DEC, streams[:n - 1], [len(d) for d in datas[:n - 1]])
    assert got == datas[:n - 1]
    assert RUNE not in prof and RUNE_PLAN not in prof and _general(prof), prof


# ---------------------------------------------------------------- 3: more members than a group
def test_more_members_than_a_group(mods, oracle):
    _lib, huffman, _ = mods
    few = [b"%d a" % k + E_ACUTE for k in range(8)]
    datas = [few[(i * 3 + i // 4096) % 8] for i in range(4097)]
    enc = {d: _enc(oracle, d) for d in few}
    assert all(_dec(oracle, enc[d]) == d for d in few)
    streams = [enc[d] for d in datas]
    got, prof = _prof(_lib, lambda: huffman.DecompressBatch(streams))[:2]
    assert got == datas
    assert prof == {RUNE: 2}, prof
    got, prof, _ = _run_slots(_lib, DEC, streams, [len(d) for d in datas])
    assert got == datas
    assert prof == {"huff_dev_plan": 1, RUNE_PLAN: 1, "group_gather": 2, RUNE: 2, "group_scatter": 2}, prof


# ---------------------------------------------------------------- 4: a mixed call in index order
def test_mixed_call_in_index_order(mods, oracle):
    _lib, huffman, _ = mods
    datas = []
    for k in range(huffman.RUNE_DEC_GROUP_MIN + 2):
        datas += [_text(3100 + k, 60 + 90 * k), _utf8(k, 100 * k), _text(3200 + k, 32 << 10), _utf8(k, 300) + b"\xff" * (k + 1)]
    datas.insert(7, _utf8(99, 20 << 10))                                  # a rune stream over the class's size
    streams = [_enc(oracle, d) for d in datas]
    want = [_dec(oracle, s) for s in streams]
    got, prof = _prof(_lib, lambda: huffman.DecompressBatch(streams))[:2]
    assert got == want
    assert prof.get(RUNE) == 1 and prof.get("huff_batch_dec") == 1 and prof.get("huff_batch_mid_dec") == 1 and _general(prof), prof
    got, prof, _ = _run_slots(_lib, DEC, streams, [len(w) if len(w) <= 16384 or max(w) < 0x80 else _ru16(len(w)) + 16 for w in want])
    assert got == want
    assert prof.get(RUNE) == 1 and prof.get(RUNE_PLAN) == 1 and prof.get("huff_batch_dec") == 1 and prof.get("huff_batch_mid_dec") == 1 and _general(prof), prof
    for i in (0, 1, 2, 3, 7):
        assert huffman.Decompress(streams[i]) == want[i]
    # a malformed member among them: the single call's code and words, in both forms
    bad = streams[1][:streams[1].index(b"\\\n")]
    with pytest.raises(_lib.RsnError) as single:
        huffman.Decompress(bad)
    mixed = streams[:9] + [bad] + streams[9:]
    with pytest.raises(_lib.RsnError) as batch:
        huffman.DecompressBatch(mixed)
    assert batch.value.code == single.value.code == E_FORMAT and str(batch.value) == str(single.value).replace(": ", ": member 9: ", 1)


# ---------------------------------------------------------------- 5: capacity
def test_capacity(mods, oracle):
    _lib, huffman, _ = mods
    datas = [_utf8(k, 70 * k + 5) + b"!" * (k % 16) for k in range(huffman.RUNE_DEC_GROUP_MIN + 3)]
    streams = [_enc(oracle, d) for d in datas]
    want = [_dec(oracle, s) for s in streams]
    assert want == datas
    rc, lens, msg, outs = _fenced_call(_lib, DEC, streams, [len(w) for w in want])          # exact capacities, between fences
    assert rc == OK, msg
    assert lens == [len(w) for w in want] and [_out_bytes(o, k) for o, k in zip(outs, lens)] == want
    tight = {2: "one byte short", 5: "null", 11: "one byte short"}
    caps = [len(w) - 1 if i in tight else len(w) for i, w in enumerate(want)]
    rc, lens, msg, outs = _fenced_call(_lib, DEC, streams, caps, null_out=(5,))
    assert rc == E_CAP and msg.startswith("member 2: huffman: output needs %d bytes, buffer holds %d" % (len(want[2]), len(want[2]) - 1)), msg
    for i, w in enumerate(want):
        if i in tight:
            assert lens[i] == _ru16(len(w)) + 16, (i, lens[i])           # the single call's figure
        else:
            assert lens[i] == len(w) and _out_bytes(outs[i], lens[i]) == w, i
    pack, slots = Pack(streams), Slots(caps)                            # sentinels: nothing outside [d_out, d_out + out_cap) is written
    rc, lens2, msg = _batch(_lib, DEC, [(pack.ptr(i), len(s), slots.ptr(i), caps[i]) for i, s in enumerate(streams)])
    assert rc == E_CAP and lens2 == lens
    h = slots.host()
    for i, w in enumerate(want):
        o = slots.offs[i]
        if i in tight:
            assert (h[o:o + _ru16(caps[i]) + 16] == 0xEE).all(), i
        else:
            assert bytes(h[o:o + len(w)]) == w and (h[o + len(w):o + _ru16(caps[i]) + 16] == 0xEE).all(), i
    rc, lens3, msg, outs = _fenced_call(_lib, DEC, streams, [lens[i] if i in tight else caps[i] for i in range(len(want))])   # the reported sizes
    assert rc == OK, msg
    assert lens3 == [len(w) for w in want] and [_out_bytes(o, k) for o, k in zip(outs, lens3)] == want


# ---------------------------------------------------------------- 6: hostile neighbours, device form
def test_hostile_neighbours(mods, oracle):
    _lib, huffman, _ = mods
    n = huffman.RUNE_DEC_GROUP_MIN
    streams = []
    for v in range(n):
        lossy = {"a": 6 + v, FFFD: 5, "b": 3}
        # the header ends in E2 82: what lies behind the stream would complete a euro sign ... were it not behind the separator; the
        # members end on a payload byte, and what follows would add code bits
        streams.append(_build([(6 + v, "a", None), (3, "b", None), (5, FFFD, b"\xe2\x82")], _spread(lossy, v)))
    streams += [_enc(oracle, _utf8(k, 50 + 31 * k)) for k in range(3)]
    want = [_dec(oracle, s) for s in streams]
    got, prof, _ = _run_slots(_lib, DEC, streams, [len(w) for w in want], behind=lambda i: b"\xac\xff\x00\x55")
    assert got == want
    assert prof.get(RUNE) == 1 and prof.get(RUNE_PLAN) == 1 and not _general(prof), prof
    # the last member's allocation ends at n rounded up to 16
    import torch
    last = streams[-1]
    alone = torch.frombuffer(bytearray(last) + bytearray(_ru16(len(last)) - len(last)), dtype=torch.uint8).cuda()
    assert alone.numel() == _ru16(len(last))
    pack, slots = Pack(streams[:-1], lambda i: b"\xac"), Slots([len(w) for w in want])
    members = [(pack.ptr(i), len(x), slots.ptr(i), len(want[i])) for i, x in enumerate(streams[:-1])] + [(alone.data_ptr(), len(last), slots.ptr(len(streams) - 1), len(want[-1]))]
    rc, lens, msg = _batch(_lib, DEC, members)
    assert rc == OK, msg
    h = slots.host()
    assert [bytes(h[o:o + k]) for o, k in zip(slots.offs, lens)] == want


# ---------------------------------------------------------------- 7: layered forms
def test_layered_forms(mods, oracle):
    import torch
    _lib, huffman, layers = mods
    names = [LZ, HU]
    datas = [_utf8(k, 30 + 90 * k) + ("%d “x”" % k).encode() for k in range(huffman.RUNE_DEC_GROUP_MIN)]
    streams = [_enc(oracle, oracle.lzss_compress(d, 4096)) for d in datas]
    want = [oracle.lzss_decompress(_dec(oracle, s)) for s in streams]
    assert want == datas
    got, prof = _prof(_lib, lambda: layers.DecompressBatch(streams, names))[:2]
    assert got == want
    assert prof.get(RUNE) == 1 and not _general(prof), prof
    pack = Pack(streams, lambda i: b"\xac")
    srcs = [pack.t[o:o + n] for o, n in zip(pack.offs, pack.lens)]
    got, prof = _prof(_lib, lambda: [bytes(t.cpu().numpy()) for t in layers.decompress_tensors(srcs, names)])[:2]
    assert got == want
    assert prof.get(RUNE) == 1 and not _general(prof), prof
    rows, prof = _prof(_lib, lambda: layers.RoundTripBatch(datas, names, hists=False))[:2]
    assert prof.get(RUNE) == 1 and not _general(prof), prof
    for d, s, r in zip(datas, streams, rows):
        assert (r.original_n, r.compressed_n, r.decompressed_n, r.lossless) == (len(d), len(s), len(d), True)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 8: round trip through the library's own encoder
def test_round_trip_through_the_library(mods, oracle):
    _lib, huffman, _ = mods
    datas = [_utf8(k, 25 + 400 * k) for k in range(huffman.RUNE_DEC_GROUP_MIN + 8)] + [(_runes(0x400, 200) * 41).encode()[:16384]]
    comp, prof = _prof(_lib, lambda: huffman.CompressBatch(datas))[:2]
    assert comp == [_enc(oracle, d) for d in datas]
    assert prof.get("huff_batch_rune_enc") == 1, prof
    back, prof = _prof(_lib, lambda: huffman.DecompressBatch(comp))[:2]
    assert back == datas
    assert prof == {RUNE: 1}, prof
