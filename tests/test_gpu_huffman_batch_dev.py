"""GPU: the Huffman batch calls on device buffers (include/rsn.h: rsn_huffman_compress_batch_dev, rsn_huffman_decompress_batch_dev; DESIGN
4.10; raisin_amd/csrc/huff_dev.hip).  Expected bytes come from the CPU oracle (oracle.huffman_compress / huffman_decompress), never from the
library; the single *_dev call is held against the same bytes.  The instruments are tests/test_gpu_batch_dev.py's: members packed back to
back in ONE allocation with hostile bytes between them, outputs between the fences of tests/test_gpu_dev_fences.py with out_cap exactly the
result size, the library's launch profile and its count of copied bytes."""
import random

import numpy as np
import pytest

from test_gpu_batch_dev import (E_CAP, E_FORMAT, GROUP_BYTES, GROUP_MEMBERS, OK, SINGLE_WORDS, Pack, Slots, _batch, _fenced_call, _out_bytes,
                                _prof, _ru16, _single)
from test_gpu_lzss_mid import _text

pytestmark = pytest.mark.gpu

ENC, DEC = "rsn_huffman_compress_batch_dev", "rsn_huffman_decompress_batch_dev"
E_EMPTY = -2
HB_PAY_MAX, HB_OUT_MAX = 16384, 32768                  # huff_small_body.h: what k_huff_batch_dec's workgroup holds
PLAN_UP, PLAN_DOWN = 16, 16                            # huff_dev.hip: a candidate's table entry goes up, its summary comes down
DEC_UP, DEC_DOWN = 64, 4                               # ... its group's gather entry goes up, its answer comes down
README = (b"Hello world!\n", b"abcabcabcabcabcabcabcabc\n")


@pytest.fixture(scope="module")
def mods():
    from raisin_amd import _lib, huffman
    _lib.check(_lib.lib().rsn_device_set(0))
    return _lib, huffman


_ENC = {}


def _enc(oracle, d):
    """the oracle's stream, computed once per input"""
    if d not in _ENC:
        _ENC[d] = oracle.huffman_compress(d)
    return _ENC[d]


def _sep(stream):
    return stream.index(b"\\\n")


def _payload(stream):
    return len(stream) - _sep(stream) - 3


def _balanced(seed, n, symbols=128):
    """random bytes below `symbols` whose counts differ by one at most: the code is flat, the payload ceil(n * log2(symbols) / 8) bytes"""
    a = np.resize(np.arange(symbols, dtype=np.uint8), n)
    np.random.default_rng(seed).shuffle(a)
    return a.tobytes()


def _alphabet(seed, n, k):
    """text over k letters (k moves the header's length, and with it the separator)"""
    rng = random.Random(seed)
    return bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz"[:k]) for _ in range(n))


@pytest.fixture(scope="module")
def mid_pad():
    """members that fill a mid class both ways: 20 to 30 KiB of text (their payloads are above k_huff_batch_dec's 16 KiB)"""
    return [_text(2100 + i, 30000 + 2111 * i) for i in range(4)]


def _enc_caps(_lib, huffman, datas, want):
    """exact sizes for the members a grouped encoder takes, the single call's need for the others"""
    L = _lib.lib()
    return [len(w) if 2 <= len(d) <= huffman.MID_IN_MAX and max(d) < 0x80 and len(set(d)) > 1 else L.rsn_huffman_compress_bound(len(d)) for d, w in zip(datas, want)]


def _run_slots(_lib, name, datas, caps, behind=None, loose=()):
    """test_gpu_batch_dev._run_slots: one call over Pack(datas) into Slots(caps) -> (results, prof, copied); asserts RSN_OK and that no byte
    behind a result has changed.  loose: the compress members that take the single call, whose kernels clear whole words up to the need
    they state (rsn.h: the size rounded up to 16, plus 32) -- for those, no byte behind the capacity."""
    pack, slots = Pack(datas, behind), Slots(caps)
    members = [(pack.ptr(i), len(d), slots.ptr(i), caps[i]) for i, d in enumerate(datas)]
    (rc, lens, msg), prof, copied = _prof(_lib, lambda: _batch(_lib, name, members))
    assert rc == OK, msg
    h = slots.host()
    res = []
    for i, c in enumerate(caps):
        o = slots.offs[i]
        assert lens[i] <= c
        res.append(bytes(h[o:o + lens[i]]))
        clean = o + (c if i in loose else lens[i])
        assert (h[clean:o + _ru16(c) + 16] == 0xEE).all(), "member %d of %d bytes: a byte behind its %s changed" % (i, lens[i], "buffer" if i in loose else "result")
    return res, prof, copied


def _singles(caps, want):
    return {i for i, (c, w) in enumerate(zip(caps, want)) if c != len(w)}


# ---------------------------------------------------------------- 1: parity, both directions
def test_parity_lengths_and_cutoffs(mods, oracle, mid_pad):
    _lib, huffman = mods
    K = 1024
    two = _balanced(7, 65536, 2)                                          # 8 KiB of payload that decodes to 64 KiB
    at_small, above_small, at_mid = _balanced(1, 18724), _balanced(2, 18725), _balanced(3, 65536)
    seps = [_alphabet(30 + k, 40 + k, k) for k in range(3, 12)]
    datas = list(README) + [b"ab", _text(2001, K), _text(2002, 16 * K), _text(2003, 16 * K + 1), _text(2004, 64 * K), _text(2005, 64 * K + 1), two,
                            at_small, above_small, at_mid] + seps + mid_pad
    want = [_enc(oracle, d) for d in datas]
    assert [_payload(_enc(oracle, d)) for d in (two, at_small, above_small, at_mid)] == [8192, HB_PAY_MAX, HB_PAY_MAX + 1, huffman.MID_PAY_MAX]
    assert {_sep(w) % 4 for d, w in zip(datas, want) if d in seps} == {0, 1, 2, 3}
    caps = _enc_caps(_lib, huffman, datas, want)
    assert sum(1 for c, w in zip(caps, want) if c != len(w)) == 1        # the member of 64 KiB + 1 takes the single call
    got, prof, _ = _run_slots(_lib, ENC, datas, caps, loose=_singles(caps, want))
    for d, w, g in zip(datas, want, got):
        assert g == w, len(d)
    for d, w in zip(datas[:8], want):
        assert _single(_lib, "rsn_huffman_compress_dev", d, _lib.lib().rsn_huffman_compress_bound(len(d))) == w, len(d)
    assert prof.get("group_gather") == 2 and prof.get("group_scatter") == 2 and prof.get("huff_batch_enc") == 1 and prof.get("huff_batch_mid_enc") == 1, prof
    # ... and back: exact capacities but for the stream that promises 64 KiB + 1, which takes the single call
    caps = [len(d) for d in datas]
    got, prof, _ = _run_slots(_lib, DEC, want, caps)
    for d, s, g in zip(datas, want, got):
        assert g == d == oracle.huffman_decompress(s), len(d)
    for d, s in zip(datas[:9], want):
        assert _single(_lib, "rsn_huffman_decompress_dev", s, len(d)) == d, len(d)
    assert prof.get("huff_dev_plan") == 1 and prof.get("huff_dev_gather") == 2 and prof.get("huff_dev_scatter") == 2, prof
    assert prof.get("huff_batch_dec") == 1 and prof.get("huff_batch_mid_dec") == 1, prof


# ---------------------------------------------------------------- 2: the header shapes that change the parse
def _entries(header):
    """the header's entries as the scan reads them: <digits> '|' <byte>, a newline written as backslash n"""
    out, i = [], 0
    while i < len(header):
        j = header.index(b"|", i)
        k = j + (3 if header[j + 1:j + 3] == b"\\n" else 2)
        out.append(header[i:k])
        i = k
    return out


def _fib_data():
    counts, f0, f1 = [], 1, 1
    while len(counts) < 22:
        counts.append(f0)
        f0, f1 = f1, f0 + f1
    a = np.repeat(np.arange(40, 40 + len(counts), dtype=np.uint8), counts)
    np.random.default_rng(5).shuffle(a)
    return a.tobytes()


def test_header_shapes_decode_as_the_oracle_says(mods, oracle, mid_pad):
    _lib, huffman = mods
    rng = random.Random(77)
    syntax = bytes(rng.choice(b"\n|\\0123456789ab") for _ in range(700))              # the header's own syntax among the symbols
    bs_top = bytes(rng.choice(b"\n019AZ\\") for _ in range(300))                       # '\\' the highest byte: its entry must not come last
    flat = _balanced(9, 4096, 4)
    fib = _fib_data()                                                                  # 21-bit codes: K = DEC_K, the tree walk behind the table
    streams = [_enc(oracle, d) for d in (syntax, bs_top, flat, fib)]
    assert max(bs_top) == 0x5C and not streams[1][:_sep(streams[1])].endswith(b"|\\") and len(fib) > HB_OUT_MAX
    # a foreign header: the entries shuffled ('\\' not last: the reference reads behind the header there), one entry repeated in front
    # with another count -- the later one holds
    text = _text(2200, 900)
    own = _enc(oracle, text)
    ents = _entries(own[:_sep(own)])
    rng.shuffle(ents)
    if ents[-1].endswith(b"|\\"):
        ents[0], ents[-1] = ents[-1], ents[0]
    foreign = b"999|" + ents[5].split(b"|", 1)[1] + b"".join(ents) + own[_sep(own):]
    streams.append(foreign)
    want = [oracle.huffman_decompress(s) for s in streams]
    assert want[:4] == [syntax, bs_top, flat, fib] and want[4] == text
    streams += [_enc(oracle, d) for d in mid_pad]                                      # (the mid class's minimum, for the Fibonacci member)
    want += mid_pad
    got, prof, _ = _run_slots(_lib, DEC, streams, [len(w) for w in want])
    assert got == want
    assert prof.get("huff_dev_plan") == 1 and prof.get("huff_batch_dec") == 1 and prof.get("huff_batch_mid_dec") == 1, prof


# ---------------------------------------------------------------- 3: hostile neighbours
def test_hostile_neighbours(mods, oracle):
    _lib, _ = mods
    text = _text(2300, 600)
    s = _enc(oracle, text)
    sep = _sep(s)
    goods = [_enc(oracle, _text(2301 + i, 300 + 50 * i)) for i in range(3)]
    for cut in (sep, sep + 1):                                            # no separator in the n bytes; the separator cut in two
        bad = s[:cut]
        assert len(bad) >= 8
        with pytest.raises(oracle.OracleError):
            oracle.huffman_decompress(bad)
        with pytest.raises(_lib.RsnError) as single:
            _single(_lib, "rsn_huffman_decompress_dev", bad, 1 << 16)
        streams = goods[:2] + [bad] + goods[2:]

        def behind(i):
            return s[cut:] + b"12|a34|b\\\n\x00" + s[sep + 3:]             # what the stream would go on with: the separator, digits, a valid tail
        pack, slots = Pack(streams, behind), Slots([1 << 16] * len(streams))
        rc, lens, msg = _batch(_lib, DEC, [(pack.ptr(i), len(x), slots.ptr(i), 1 << 16) for i, x in enumerate(streams)])
        assert rc == single.value.code == E_FORMAT
        assert "librsn error %d: %s" % (rc, msg) == str(single.value).replace(": ", ": member 2: ", 1), (msg, str(single.value))
        assert lens == [0] * len(streams)
    # good members followed by the same bytes decode unchanged
    streams = goods + [s]
    want = [oracle.huffman_decompress(x) for x in streams]
    got, prof, _ = _run_slots(_lib, DEC, streams, [len(w) for w in want], behind=lambda i: b"\\\n\x0012|a34|b\\\n\x00" + s[sep + 3:])
    assert got == want and prof.get("huff_batch_dec") == 1, prof
    # ... and inputs followed by more of the same text compress unchanged
    datas = [_text(2310 + i, 100 + 333 * i) for i in range(4)]
    got, _, _ = _run_slots(_lib, ENC, datas, [len(_enc(oracle, d)) for d in datas], behind=lambda i: datas[i][:48])
    assert got == [_enc(oracle, d) for d in datas]


# ---------------------------------------------------------------- 4: a mixed call
def test_mixed_call_in_index_order(mods, oracle, mid_pad):
    _lib, huffman = mods
    runes = _text(2400, 500) + "é".encode() + _text(2401, 500)            # a byte >= 0x80: the encoder hands it back, the plan refuses its header
    big = _text(2402, huffman.MID_IN_MAX + 1000)
    smalls = [_text(2410 + i, 50 + 300 * i) for i in range(4)]
    datas = [smalls[0], mid_pad[0], runes, big, smalls[1], mid_pad[1], b"z" * 100, mid_pad[2], smalls[2], mid_pad[3], smalls[3]]
    want = [_enc(oracle, d) for d in datas]
    caps = _enc_caps(_lib, huffman, datas, want)
    got, prof, _ = _run_slots(_lib, ENC, datas, caps, loose=_singles(caps, want))
    assert got == want
    assert prof.get("huff_batch_enc") == 1 and prof.get("huff_batch_mid_enc") == 1 and len(prof) > 4, prof     # (and the single call's kernels)
    plain = [oracle.huffman_decompress(w) for w in want]                  # (the stream of one distinct byte decodes to ONE byte, in the reference too)
    assert [p == d for p, d in zip(plain, datas)] == [i != 6 for i in range(len(datas))] and plain[6] == b"z"
    back, prof, _ = _run_slots(_lib, DEC, want, [len(d) if len(d) <= huffman.MID_OUT_MAX and max(d) < 0x80 else _ru16(len(d)) + 16 for d in plain])
    assert back == plain
    assert prof.get("huff_dev_plan") == 1 and prof.get("huff_batch_dec") == 1 and prof.get("huff_batch_mid_dec") == 1 and len(prof) > 5, prof
    # two failing members: the lower one's code and words, nothing handed out
    bad = want[0][:_sep(want[0])]
    with pytest.raises(_lib.RsnError) as single:
        _single(_lib, "rsn_huffman_decompress_dev", bad, 1 << 16)
    streams = want[:2] + [bad] + want[2:5] + [b"no header at all"] + want[5:]
    pack, slots = Pack(streams), Slots([1 << 17] * len(streams))
    rc, lens, msg = _batch(_lib, DEC, [(pack.ptr(i), len(x), slots.ptr(i), 1 << 17) for i, x in enumerate(streams)])
    assert rc == single.value.code == E_FORMAT and lens == [0] * len(streams)
    assert "librsn error %d: %s" % (rc, msg) == str(single.value).replace(": ", ": member 2: ", 1), (msg, str(single.value))
    pack = Pack(datas)
    members = [(pack.ptr(i), len(d), slots.ptr(i), 1 << 17) for i, d in enumerate(datas)]
    members[4] = (None, 0, slots.ptr(4), 1 << 17)
    members[7] = (pack.ptr(7), 0, slots.ptr(7), 1 << 17)
    rc, lens, msg = _batch(_lib, ENC, members)
    assert rc == E_EMPTY and msg.startswith("member 4: huffman: empty input") and lens == [0] * len(datas)


# ---------------------------------------------------------------- 5: capacity
@pytest.mark.parametrize("name", (ENC, DEC))
def test_capacity(mods, oracle, mid_pad, name):
    _lib, huffman = mods
    datas = [_text(2500 + i, 40 + 411 * i) for i in range(4)] + mid_pad + [_text(2510, huffman.MID_IN_MAX + 77)]
    encs = [_enc(oracle, d) for d in datas]
    ins, want, slack = (datas, encs, 32) if name == ENC else (encs, datas, 16)
    last = len(datas) - 1                                                 # the single call's member
    figure = [_ru16(len(w)) + slack for w in want]
    # exact sizes: accepted for every grouped member; the single call's member gets what the single call needs
    caps = [len(w) for w in want]
    caps[last] = figure[last] if name == ENC else len(want[last])
    rc, lens, msg, outs = _fenced_call(_lib, name, ins, caps)
    assert rc == OK, msg
    assert lens == [len(w) for w in want] and [_out_bytes(o, k) for o, k in zip(outs, lens)] == want
    if name == ENC:                                                       # ... and not the exact size
        rc, lens, msg, outs = _fenced_call(_lib, name, ins, [len(w) for w in want])
        assert rc == E_CAP and msg.startswith("member %d: huffman: output needs %d bytes, buffer holds %d" % (last, figure[last], len(want[last]))), msg
        assert lens[last] == figure[last] and lens[:last] == [len(w) for w in want[:last]]
    # one byte short, and the size query (a null d_out): the documented figure, every other member complete, the fences untouched
    tight = {1: "one byte short", 2: "null", 5: "one byte short", last: "one byte short"}
    caps = [len(w) - 1 if i in tight else c for i, (w, c) in enumerate(zip(want, caps))]
    rc, lens, msg, outs = _fenced_call(_lib, name, ins, caps, null_out=(2,))
    assert rc == E_CAP and msg.startswith("member 1: huffman: output needs %d bytes, buffer holds %d" % (len(want[1]), len(want[1]) - 1)), msg
    for i, w in enumerate(want):
        if i in tight:
            assert lens[i] == figure[i], (i, lens[i], figure[i])
        else:
            assert lens[i] == len(w) and _out_bytes(outs[i], lens[i]) == w, i
    # a second call with the reported figures
    caps2 = [lens[i] if i in tight else caps[i] for i in range(len(want))]
    rc, lens2, msg, outs = _fenced_call(_lib, name, ins, caps2)
    assert rc == OK, msg
    assert lens2 == [len(w) for w in want] and [_out_bytes(o, k) for o, k in zip(outs, lens2)] == want


# ---------------------------------------------------------------- 6: group edges
def test_the_mid_class_s_minimum(mods, oracle, mid_pad):
    _lib, huffman = mods
    assert huffman.MID_GROUP_MIN == 4 == len(mid_pad)
    for k in (3, 4):
        datas = mid_pad[:k]
        want = [_enc(oracle, d) for d in datas]
        got, prof, _ = _run_slots(_lib, ENC, datas, [_lib.lib().rsn_huffman_compress_bound(len(d)) for d in datas], loose=() if k == 4 else range(k))
        assert got == want and ("huff_batch_mid_enc" in prof) == (k == 4), prof
        back, prof, _ = _run_slots(_lib, DEC, want, [_ru16(len(d)) + 16 for d in datas])
        assert back == datas and ("huff_batch_mid_dec" in prof) == (k == 4) and prof.get("huff_dev_plan") == 1, prof


def test_more_members_than_a_group(mods, oracle):
    _lib, _ = mods
    few = [README[1], b"abcabcabcabcabcabcabcabd\n", b"xyzxyzxyzxyzxyzxyzxyzxyz\n", b"Hello world! Hello, all\n\n"]
    assert all(len(d) == 25 for d in few)
    datas = [few[(i * 7 + i // GROUP_MEMBERS) % 4] for i in range(GROUP_MEMBERS + 1)]
    want = {d: _enc(oracle, d) for d in few}
    got, prof, _ = _run_slots(_lib, ENC, datas, [len(want[d]) for d in datas])
    assert got == [want[d] for d in datas]
    assert prof == {"group_gather": 2, "huff_batch_enc": 2, "group_scatter": 2}, prof
    back, prof, _ = _run_slots(_lib, DEC, got, [25] * len(datas))
    assert back == datas
    assert prof.get("huff_dev_plan") == 1 and prof.get("huff_dev_gather") == 2 and prof.get("huff_batch_dec") == 2 and prof.get("huff_dev_scatter") == 2, prof


@pytest.fixture(scope="module")
def many_large(oracle):
    """270 streams of 64 KiB of text: their promised outputs and their streams pass a group's bytes"""
    three = [_text(2600 + i, 65536) for i in range(3)]
    datas = [three[(i + i // 100) % 3] for i in range(270)]
    return datas, [_enc(oracle, d) for d in datas]


def test_more_bytes_than_a_group_and_nothing_left_over(mods, oracle, many_large):
    _lib, huffman = mods
    datas, streams = many_large
    need = 608 + 64 + _ru16(len(streams[0]) - 4) + 64 + 65536 + 16 + 16                 # (about: group_layout.h's slots of one such member)
    assert 270 * need > GROUP_BYTES
    first, prof, _ = _run_slots(_lib, DEC, streams, [65536] * 270)
    assert first == datas
    assert prof.get("huff_dev_plan") == 1 and prof.get("huff_batch_mid_dec", 0) >= 2 and prof["huff_dev_gather"] == prof["huff_batch_mid_dec"] == prof["huff_dev_scatter"], prof
    # the README's files in the same thread, in the staging and the plan table the large call left
    small = [_enc(oracle, d) for d in README]
    got, _, _ = _run_slots(_lib, DEC, small, [len(d) for d in README])
    assert got == list(README) == [oracle.huffman_decompress(s) for s in small]
    got, _, _ = _run_slots(_lib, ENC, list(README), [len(s) for s in small])
    assert got == small
    again, _, _ = _run_slots(_lib, DEC, streams, [65536] * 270)
    assert again == datas


# ---------------------------------------------------------------- 7: the grouped path is the path
def test_the_grouped_path_is_the_path(mods, oracle):
    _lib, _ = mods
    datas = [_text(2700 + i, 1024) for i in range(256)]
    streams = [_enc(oracle, d) for d in datas]
    assert min(_sep(s) for s in streams) > 100                            # the headers alone are more than the call may copy
    got, prof, copied = _run_slots(_lib, DEC, streams, [1024] * 256)
    assert got == datas
    assert prof == {"huff_dev_plan": 1, "huff_dev_gather": 1, "huff_batch_dec": 1, "huff_dev_scatter": 1}, prof
    assert PLAN_UP + DEC_UP <= 128 and PLAN_DOWN + DEC_DOWN <= 32
    assert copied[0] <= 256 * 128 + SINGLE_WORDS and copied[1] <= 256 * 32 + SINGLE_WORDS and sum(copied) <= 256 * (128 + 32) + SINGLE_WORDS, copied
    got, prof, copied = _run_slots(_lib, ENC, datas, [len(s) for s in streams])
    assert got == streams
    assert prof == {"group_gather": 1, "huff_batch_enc": 1, "group_scatter": 1}, prof
    assert sum(copied) <= 256 * (64 + 4) + SINGLE_WORDS, copied


# ---------------------------------------------------------------- 9: Python
def test_tensor_lists_round_trip(mods, oracle):
    import torch
    _lib, huffman = mods
    datas = [_text(2800 + i, n) for i, n in enumerate((2, 25, 1000, 5000, 20000, 70000, 33, 16))] + [_balanced(11, 65536, 2)]
    pack = Pack(datas)
    srcs = [pack.t[o:o + n] for o, n in zip(pack.offs, pack.lens)]       # slices of one allocation
    comp = huffman.compress_tensors(srcs)
    assert [bytes(t.cpu().numpy()) for t in comp] == [_enc(oracle, d) for d in datas]
    back = huffman.decompress_tensors(comp)
    assert [bytes(t.cpu().numpy()) for t in back] == datas
    # a guess that is too small: the members that did not fit are run once more, the others are kept
    tight = [torch.empty(max(len(d) // (2 if i % 2 else 1), 16), dtype=torch.uint8, device="cuda") for i, d in enumerate(datas)]
    assert [bytes(t.cpu().numpy()) for t in huffman.decompress_tensors(comp, outs=tight)] == datas
    assert huffman.compress_tensors([]) == [] and huffman.decompress_tensors([]) == []
