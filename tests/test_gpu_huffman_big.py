"""GPU: the big class of the Huffman compress batch (csrc/huff_big.hip) -- members above huffman.MID_IN_MAX and up to
huffman.BIG_IN_MAX bytes of a byte alphabet are cut into tiles of huffman.BIG_TILE bytes and a group of them is THREE launches
(huff_batch_big_count, huff_batch_big_plan, huff_batch_big_emit) between k_group_gather and k_group_scatter, in the host form too.  Every
result is compared byte for byte with the CPU oracle AND with the library's single call; what the plan hands back (a byte >= 0x80, one
distinct byte) and the Fibonacci member with a code of 25 bits (317810 bytes: above the class at its measured limit, the plan's refusal
of it is tests/test_huff_big_host.py's) must come out of the single call with the same bytes.  Every list is padded to BIG_GROUP_MIN members of
the class with text of MID_IN_MAX + 1 + 100 i bytes.

With BIG_TILE = 16 KiB some sizes the tile arithmetic suggests (BIG_TILE +- 1, 2 BIG_TILE +- 1, 3 BIG_TILE + 12345) lie below the class:
they stay in the lists -- they are the other classes' or the single call's, and their bytes are pinned all the same -- and the same edges
are taken again at 5 BIG_TILE and 6 BIG_TILE, inside it."""
import numpy as np
import pytest

import long_codes
from test_gpu_batch_dev import E_CAP, OK, SINGLE_WORDS, TABLE_DOWN, TABLE_UP, Pack, Slots, _batch, _fenced_call, _out_bytes, _prof, _ru16

pytestmark = pytest.mark.gpu

ENC = "rsn_huffman_compress_batch_dev"
BIG = ("huff_batch_big_count", "huff_batch_big_plan", "huff_batch_big_emit")
GROUPED = {"group_gather", "group_scatter", "huff_batch_enc", "huff_batch_mid_enc", "huff_batch_rune_enc"} | set(BIG)   # every launch of a grouped encoder
GROUP_MEMBERS = 4096                                    # codecs.h: SMALL_GROUP_MAX
HDR_MAX = 786                                           # huff_big_layout.h: HUFF_BIG_HDR_MAX
LZ, HU = "lzss", "huffman"

_WORDS = np.array([w.encode() for w in ("the", "quick", "brown", "fox", "jumps", "over", "lazy", "dog", "compression", "a", "I", "Sam", "ham", "green",
                                         "eggs", "and", "would", "not", "could", "in", "box", "with", "house", "mouse", "here", "there", "anywhere")], dtype=object)
_SEPS = np.array([b" ", b" ", b" ", b"\n", b", ", b". "], dtype=object)


def _text(seed, n):
    rng = np.random.default_rng(seed)
    k = n // 3 + 8
    parts = np.empty(2 * k, dtype=object)
    parts[0::2] = _WORDS[rng.integers(0, len(_WORDS), k)]
    parts[1::2] = _SEPS[rng.integers(0, len(_SEPS), k)]
    t = b"".join(parts)
    assert len(t) >= n
    return t[:n]


def _with_counts(seed, table, shuffled):
    a = np.concatenate([np.full(c, b, dtype=np.uint8) for b, c in sorted(table.items())])
    if shuffled:
        np.random.default_rng(seed).shuffle(a)
    return a.tobytes()


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


_SINGLE = {}


def _single_call(huffman, d):
    if d not in _SINGLE:
        _SINGLE[d] = huffman.Compress(d)
    return _SINGLE[d]


def _in_class(huffman, d):
    return huffman.MID_IN_MAX < len(d) <= huffman.BIG_IN_MAX


def _taken(huffman, d):
    """a member the three launches complete (the code's depth aside)"""
    return _in_class(huffman, d) and max(d) < 0x80 and len(set(d)) > 1


def _pad(huffman, members, seed=500):
    """at least BIG_GROUP_MIN members of the class: text of MID_IN_MAX + 1 + 100 i bytes behind the ones the test is about"""
    have = sum(1 for d in members if _in_class(huffman, d))
    return list(members) + [_text(seed + i, huffman.MID_IN_MAX + 1 + 100 * i) for i in range(max(0, huffman.BIG_GROUP_MIN - have))]


def _groups(huffman, members):
    """how many groups the class's packing makes of its members (group_layout.h: the table entries, the input slot, the output slot, the status)"""
    groups, k, used = 0, 0, 0
    for d in members:
        n = len(d)
        need = 64 + _ru16(n) + 16 + _ru16(HDR_MAX + (7 * n + 7) // 8) + 16
        if k and (k == GROUP_MEMBERS or used + need > huffman.BIG_GROUP_BYTES):
            groups, k, used = groups + 1, 0, 0
        k, used = k + 1, used + need
    return groups + (1 if k else 0)


def _big_only(huffman, members):
    g = _groups(huffman, members)
    return dict({name: g for name in BIG}, group_gather=g, group_scatter=g)


def _host(mods, oracle, members):
    """the host form -> prof; the bytes against the oracle and the single call"""
    _lib, huffman = mods
    got, prof, copied = _prof(_lib, lambda: huffman.CompressBatch(members))
    assert len(got) == len(members)
    for d, g in zip(members, got):
        assert g == _enc(oracle, d), (len(d), d[:24])
        assert g == _single_call(huffman, d), (len(d), d[:24])
    return prof


def _caps(_lib, huffman, members, want, loose=()):
    """exact sizes for the members the big class completes (a list with at least its minimum of them; not the indexes of `loose`), the
    single call's need for the others"""
    L = _lib.lib()
    grouped = sum(1 for d in members if _in_class(huffman, d)) >= huffman.BIG_GROUP_MIN
    return [len(w) if grouped and _taken(huffman, d) and i not in loose else L.rsn_huffman_compress_bound(len(d)) for i, (d, w) in enumerate(zip(members, want))]


def _dev(mods, oracle, members, loose=()):
    """the device form: members back to back at 16-byte offsets of one allocation, outputs of `caps` bytes in one allocation full of 0xEE
    -> (prof, copied); the bytes against the oracle, nothing behind a result written where the capacity is the exact size (_caps), nothing
    behind the capacity elsewhere"""
    _lib, huffman = mods
    want = [_enc(oracle, d) for d in members]
    caps = _caps(_lib, huffman, members, want, loose)
    pack, slots = Pack(members), Slots(caps)
    (rc, lens, msg), prof, copied = _prof(_lib, lambda: _batch(_lib, ENC, [(pack.ptr(i), len(d), slots.ptr(i), caps[i]) for i, d in enumerate(members)]))
    assert rc == OK, msg
    h = slots.host()
    for i, (w, c) in enumerate(zip(want, caps)):
        o = slots.offs[i]
        assert lens[i] == len(w) and bytes(h[o:o + lens[i]]) == w, (i, len(members[i]))
        clean = o + (lens[i] if c == len(w) else c)
        assert (h[clean:o + _ru16(c) + 16] == 0xEE).all(), "member %d of %d bytes: a byte behind its result changed" % (i, len(members[i]))
    return prof, copied


# ---------------------------------------------------------------- 1: sizes, and one launch set per group
def test_sizes_and_one_launch_set_per_group(mods, oracle):
    _lib, huffman = mods
    T, top = huffman.BIG_TILE, huffman.BIG_IN_MAX
    assert huffman.MID_IN_MAX + 1 == 65537 == 4 * T + 1                       # a last tile of one symbol
    sizes = [65537, T - 1, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 12345, 5 * T - 1, 5 * T, 5 * T + 1, 6 * T + 12345, top, top + 1]
    members = _pad(huffman, [_text(10 + i, n) for i, n in enumerate(sizes)])
    inside = [d for d in members if _in_class(huffman, d)]
    assert len(inside) == 6 and len(inside) >= huffman.BIG_GROUP_MIN
    for run in (_host, lambda m, o, x: _dev(m, o, x)[0]):
        prof = run(mods, oracle, members)
        for name in BIG:
            assert prof.get(name) == _groups(huffman, inside) == 1, prof
        if run is not _host:                                                  # (the host form's single calls run on the batch workers' contexts: this thread's profile does not hold them)
            assert set(prof) - GROUPED, prof                                  # BIG_IN_MAX + 1 is not taken: the single call's kernels
        # a list inside the class: the three launches once a group, and no kernel of a single call
        prof = run(mods, oracle, inside)
        assert prof == _big_only(huffman, inside), prof


def test_more_bytes_than_a_group(mods, oracle):
    _lib, huffman = mods
    three = [_text(40 + i, 131072 + 16 * i) for i in range(3)]
    members = [three[(i + i // 100) % 3] for i in range(300)]
    assert _groups(huffman, members) == 2
    prof, _ = _dev(mods, oracle, members)
    assert prof == _big_only(huffman, members), prof


def test_below_the_minimum_nothing_changes(mods, oracle):
    _lib, huffman = mods
    members = [_text(60 + i, huffman.MID_IN_MAX + 1 + 100 * i) for i in range(huffman.BIG_GROUP_MIN - 1)]
    for prof in (_host(mods, oracle, members), _dev(mods, oracle, members)[0]):
        assert not set(prof) & GROUPED, prof


# ---------------------------------------------------------------- 2: tile edges off the byte grid
def test_tile_edges_off_the_byte_grid(mods, oracle):
    _lib, huffman = mods
    T = huffman.BIG_TILE
    members = []
    for n in (2 * T + 1, 5 * T + 1):                                          # (2 T + 1 lies below the class; 5 T + 1: six tiles, the last of one symbol)
        q = n // 4
        tables = [{0x61: n - 2 * q, 0x62: q, 0x63: q},                        # code lengths 1, 2, 2: a tile's bits end anywhere in a byte
                  {(10 if b == 0 else 31 + b): 1 + (b * b * b) % 997 + (n // 8 if b < 4 else 0) for b in range(96)},
                  {0x61: n // 2, 0x62: n - n // 2}]                           # codes of one bit: the edges lie on the byte grid
        for k, t in enumerate(tables):
            scale = n / sum(t.values())
            t = {b: max(1, int(c * scale)) for b, c in t.items()}
            t[0x61 if 0x61 in t else 32] += n - sum(t.values())
            assert sum(t.values()) == n and min(t.values()) >= 1
            members += [_with_counts(k, t, True), _with_counts(k, t, False)]
    lens = {l for _, _, _, l in oracle.huffman_table(members[6])}
    assert lens == {1, 2}, lens
    inside = [d for d in members if _in_class(huffman, d)]
    assert len(inside) == 6
    assert _host(mods, oracle, inside) == _big_only(huffman, inside)
    prof, _ = _dev(mods, oracle, members)
    assert all(prof.get(name) == 1 for name in BIG), prof


# ---------------------------------------------------------------- 3: hand-backs
def test_hand_backs_take_the_single_call(mods, oracle):
    _lib, huffman = mods
    T = huffman.BIG_TILE
    rune = _text(70, 5 * T + 100) + "é".encode() + _text(71, 50)             # one rune, in the last tile
    one = b"z" * 70000
    fib24 = long_codes.fib_data(25, seed=4)                                   # Fibonacci counts over 25 symbols: a deepest code of 24 bits, taken
    fib25 = long_codes.fib_data(26, seed=3)                                   # ... over 26: 25 bits.  317810 bytes: the plan would hand it back; above BIG_IN_MAX the class does not see it
    assert (len(fib24), len(fib25)) == (196417, 317810) and len(fib24) <= huffman.BIG_IN_MAX
    assert max(l for _, _, _, l in oracle.huffman_table(fib25)) == 25 and max(l for _, _, _, l in oracle.huffman_table(fib24)) == 24
    good = _pad(huffman, [fib24])
    assert _host(mods, oracle, good) == _big_only(huffman, good)              # 24 bits: the whole list grouped
    for bad in (rune, one, fib25):
        members = good[:2] + [bad] + good[2:]
        prof = _host(mods, oracle, members)
        assert all(prof.get(name) == 1 for name in BIG), prof
        prof, _ = _dev(mods, oracle, members, loose=(2,))
        assert all(prof.get(name) == 1 for name in BIG) and set(prof) - GROUPED, prof       # ... and the single call's kernels for the one


# ---------------------------------------------------------------- 4: a mixed call
def test_mixed_call_in_index_order(mods, oracle):
    _lib, huffman = mods
    smalls = [_text(80 + i, 50 + 300 * i) for i in range(4)]
    mids = [_text(90 + i, 30000 + 2111 * i) for i in range(huffman.MID_GROUP_MIN)]
    runes = [_text(100 + i, 200 + 10 * i) + "é".encode() + _text(120 + i, 100) for i in range(huffman.RUNE_GROUP_MIN)]
    bigs = [_text(140 + i, huffman.MID_IN_MAX + 1 + 100 * i) for i in range(huffman.BIG_GROUP_MIN)] + [_text(150, 200000)]
    members = []
    for i in range(max(len(smalls), len(mids), len(runes), len(bigs))):
        members += [x[i] for x in (bigs, smalls, runes, mids) if i < len(x)]
    for prof in (_host(mods, oracle, members), _dev(mods, oracle, members)[0]):
        assert prof.get("huff_batch_enc") == 1 and prof.get("huff_batch_mid_enc") == 1 and prof.get("huff_batch_rune_enc") == 1, prof
        assert all(prof.get(name) == 1 for name in BIG) and not set(prof) - GROUPED, prof


# ---------------------------------------------------------------- 5: the device form's capacities
def test_device_form_capacities_and_copies(mods, oracle):
    _lib, huffman = mods
    T = huffman.BIG_TILE
    members = [_text(160 + i, n) for i, n in enumerate((65537, 5 * T - 1, 5 * T + 7, 100000, 131072, 200001))]
    want = [_enc(oracle, d) for d in members]
    assert len({len(w) % 16 for w in want}) >= 4
    figure = [_ru16(len(w)) + 32 for w in want]                               # rsn.h: what a compress member that does not fit reports
    # exact capacities between fences
    rc, lens, msg, outs = _fenced_call(_lib, ENC, members, [len(w) for w in want])
    assert rc == OK, msg
    assert lens == [len(w) for w in want] and [_out_bytes(o, k) for o, k in zip(outs, lens)] == want
    # one byte short, and the size query: the documented figure, every other member complete, the fences untouched
    tight = {1: "one byte short", 2: "null", 5: "one byte short"}
    caps = [len(w) - 1 if i in tight else len(w) for i, w in enumerate(want)]
    rc, lens, msg, outs = _fenced_call(_lib, ENC, members, caps, null_out=(2,))
    assert rc == E_CAP and msg.startswith("member 1: huffman: output needs %d bytes, buffer holds %d" % (len(want[1]), len(want[1]) - 1)), msg
    for i, w in enumerate(want):
        if i in tight:
            assert lens[i] == figure[i], (i, lens[i], figure[i])
        else:
            assert lens[i] == len(w) and _out_bytes(outs[i], lens[i]) == w, i
    rc, lens2, msg, outs = _fenced_call(_lib, ENC, members, [lens[i] if i in tight else caps[i] for i in range(len(want))])
    assert rc == OK, msg
    assert lens2 == [len(w) for w in want] and [_out_bytes(o, k) for o, k in zip(outs, lens2)] == want
    # members back to back at 16-byte offsets; what crosses to the host is a member's table entries up and its answer down
    prof, copied = _dev(mods, oracle, members)
    assert prof == _big_only(huffman, members), prof
    assert copied[0] <= len(members) * TABLE_UP + SINGLE_WORDS and copied[1] <= len(members) * TABLE_DOWN + SINGLE_WORDS, copied


# ---------------------------------------------------------------- 6: nothing depends on what the scratch held
def test_scratch_independence(mods, oracle):
    _lib, huffman = mods
    T = huffman.BIG_TILE
    sizes = (65537, 5 * T + 1, 100003, 6 * T, 150000)
    first = [_text(170 + i, n) for i, n in enumerate(sizes)]
    other = [_text(180 + i, n + 4001) for i, n in enumerate(sizes)] + [_text(186, 250000)]
    ones = [b"\x7f" * n for n in sizes]                                       # one distinct byte: handed back, the staging's inputs full of 0x7F
    high = [b"\x01" + b"\x7f" * (n - 1) for n in sizes]                        # the frequent byte codes as '1': streams of 0xFF in every output slot
    assert all(_enc(oracle, d)[-40:] == b"\xff" * 40 for d in high)
    for run in (_host, lambda m, o, x: _dev(m, o, x)[0]):
        for between in (other, ones, high):
            assert run(mods, oracle, first) == _big_only(huffman, first)
            run(mods, oracle, between)
        assert run(mods, oracle, first) == _big_only(huffman, first)


# ---------------------------------------------------------------- 7: the layered batch calls
def test_layered_batches(mods, oracle):
    import torch
    _lib, huffman = mods
    from raisin_amd import layers
    members = [_text(190 + i, 200000) for i in range(huffman.BIG_GROUP_MIN)]
    for names in ([HU], [LZ, HU]):
        want = []
        for d in members:
            for a in names:
                d = oracle.lzss_compress(d, 4096) if a == LZ else _enc(oracle, d)
            want.append(d)
        assert [layers.Compress(d, names) for d in members] == want           # the chain of single calls
        got, prof, _ = _prof(_lib, lambda: layers.CompressBatch(members, names))
        assert got == want
        if names == [HU]:
            assert all(prof.get(name) == 1 for name in BIG) and not set(prof) - GROUPED - {"members_move"}, prof
        ts = [torch.frombuffer(bytearray(d) + bytearray(16), dtype=torch.uint8).cuda()[:len(d)] for d in members]
        torch.cuda.synchronize()
        got, prof, _ = _prof(_lib, lambda: [bytes(t.cpu().numpy()) for t in layers.compress_tensors(ts, names)])
        assert got == want
        if names == [HU]:
            assert all(prof.get(name) == 1 for name in BIG) and not set(prof) - GROUPED - {"members_move"}, prof
        res = layers.RoundTripBatch(members, names, hists=False)
        assert [(r.original_n, r.compressed_n, r.decompressed_n, r.lossless) for r in res] == [(len(d), len(w), len(d), True) for d, w in zip(members, want)]
