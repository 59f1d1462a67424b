"""GPU: the tiled class of the LZSS compress batch (csrc/lzss_tile.hip) -- members above lz.MID_IN_MAX and up to lz.TILE_IN_MAX
bytes at a window of 1 to 4096 are cut into tiles of lz.TILE_POS escaped positions and a group of them is the launches lzss_batch_tile_esc,
_search, _chain and _emit between k_group_gather and k_group_scatter, in the host form too.  Every result is compared byte for byte with
the CPU oracle AND with the library's single call; what the kernels hand back (more escaped bytes than the class holds, runs and short
periods) must come out of the single call with the same bytes.  The lists are built from a handful of distinct members, padded to
lz.TILE_GROUP_MIN members of the class with copies of ONE text of 65537 bytes, and the oracle's and the single call's answers are kept
per distinct member."""
import numpy as np
import pytest

from test_gpu_batch_dev import E_CAP, OK, TABLE_DOWN, TABLE_UP, _fenced_call, _out_bytes, _prof, _ru16, _run_slots
from test_gpu_lzss_mid import _alpha, _text

pytestmark = pytest.mark.gpu

ENC = "rsn_lzss_compress_batch_dev"
TILE = ("lzss_batch_tile_esc", "lzss_batch_tile_search", "lzss_batch_tile_chain", "lzss_batch_tile_emit")
ONLY = dict({name: 1 for name in TILE}, group_gather=1, group_scatter=1)     # a list inside the class, one group: every launch once and nothing else
HU_GROUPED = {"huff_batch_enc", "huff_batch_mid_enc", "huff_batch_rune_enc", "huff_batch_big_count", "huff_batch_big_plan", "huff_batch_big_emit"}
LZ, HU = "lzss", "huffman"


@pytest.fixture(scope="module")
def mods():
    from raisin_amd import _lib, lz
    _lib.check(_lib.lib().rsn_device_set(0))
    return _lib, lz


_WANT, _SINGLE = {}, {}
PAD = _text(4000, 65537)                                 # the one short member of the class every list is padded with


def _want(oracle, d, w):
    if (d, w) not in _WANT:
        _WANT[d, w] = oracle.lzss_compress(d, w)
    return _WANT[d, w]


def _single(lz, d, w):
    if (d, w) not in _SINGLE:
        _SINGLE[d, w] = lz.CompressAsync(d, False, w)
    return _SINGLE[d, w]


def _in_class(lz, d):
    return lz.MID_IN_MAX < len(d) <= lz.TILE_IN_MAX


def _escaped(d):
    a = np.frombuffer(d, dtype=np.uint8)
    return len(d) + int(((a == 0x5C) | (a == 0xFF)).sum())


def _pad(lz, members):
    have = sum(1 for d in members if _in_class(lz, d))
    return list(members) + [PAD] * max(0, lz.TILE_GROUP_MIN - have)


def _host(mods, oracle, members, w=4096):
    """the host form -> prof; the bytes against the oracle and the single call"""
    _lib, lz = mods
    got, prof, _ = _prof(_lib, lambda: lz.CompressAsyncBatch(members, w))
    assert len(got) == len(members)
    for i, (d, g) in enumerate(zip(members, got)):
        assert g == _want(oracle, d, w), (i, len(d), w)
        assert g == _single(lz, d, w), (i, len(d), w)
    return prof


def _dev(mods, oracle, members, w=4096, loose=()):
    """the device form: members back to back at 16-byte offsets of one allocation, every output between guard bytes; a capacity is the
    exact size of the result but at the indexes of `loose` (the members the kernels hand back: the single call asks for its bound)
    -> (prof, copied)"""
    _lib, lz = mods
    want = [_want(oracle, d, w) for d in members]
    grouped = sum(1 for d in members if _in_class(lz, d)) >= lz.TILE_GROUP_MIN
    caps = [len(x) if grouped and _in_class(lz, d) and i not in loose else lz.compress_bound(len(d)) for i, (d, x) in enumerate(zip(members, want))]
    got, prof, copied = _run_slots(_lib, ENC, members, caps, w)
    for i, (g, x) in enumerate(zip(got, want)):
        assert g == x, (i, len(members[i]), w)
    return prof, copied


# ---------------------------------------------------------------- 1: the class runs, and only it
@pytest.mark.parametrize("window", [1, 2, 255, 4095, 4096])
def test_the_class_runs_and_only_it(mods, oracle, window):
    _lib, lz = mods
    P, top = lz.TILE_POS, lz.TILE_IN_MAX
    assert lz.MID_IN_MAX + 1 == 65537 and lz.TILE_GROUP_MIN >= 2
    members = _pad(lz, [_text(4001 + i, n) for i, n in enumerate((34 * P - 1, 34 * P, 34 * P + 1, top))])
    assert all(_escaped(d) == len(d) for d in members)                        # (text: a tile edge of the input is one of the escaped stream)
    assert _host(mods, oracle, members, window) == ONLY                       # fails on a build without the class: no such launch
    prof, _ = _dev(mods, oracle, members, window)
    assert prof == ONLY, prof
    # one member fewer than the minimum; members one byte above the class: no launch of the class, the same bytes
    few = members[:lz.TILE_GROUP_MIN - 1]
    above = [_text(4010, top + 1)] * lz.TILE_GROUP_MIN
    for other in (few, above):
        for prof in (_host(mods, oracle, other, window), _dev(mods, oracle, other, window)[0]):
            assert not any(k.startswith("lzss_batch_tile_") for k in prof), prof


# ---------------------------------------------------------------- 2: no match reaches into a neighbour
def test_no_match_reaches_into_a_neighbour(mods, oracle):
    _lib, lz = mods
    k = 4
    blocks = [b"q" + _text(4020 + i, 2999) for i in range(k)]
    members = [blocks[i] + _text(4030 + i, 60000 + 2 * lz.TILE_POS + 77 * i) + blocks[(i + 1) % k] for i in range(k)]
    members = members * ((lz.TILE_GROUP_MIN + k - 1) // k)
    for i, d in enumerate(members):                                           # in the staging and in the caller's allocation they lie back to back
        assert _in_class(lz, d) and d[:3000] == members[i - 1][-3000:] and d[-3000:] == members[(i + 1) % len(members)][:3000]
    for prof in (_host(mods, oracle, members), _dev(mods, oracle, members)[0]):
        assert prof == ONLY, prof
    for d in members[:k]:
        assert _want(oracle, d, 4096)[:1] == b"q"                            # a member's first item is a literal: nothing lies in front of it


# ---------------------------------------------------------------- 3: tile edges of the search
def test_tile_edges_of_the_search(mods, oracle):
    _lib, lz = mods
    block = _alpha(4040, 4096, b"abcdefghijklmnopqrst")                       # 20-letter noise
    members = [(block[:p] * (70000 // p + 1))[:70000] for p in (4096, 2047, 2048, 2049, 4095)]
    # matches of the window's length: the chain steps over whole tiles and enters tiles far from their start, the look-ahead reaches two
    # tiles on, and a position spends 512 extension steps on a candidate 4096 back and 256 on one 2048 back -- two positions a thread stay
    # within the cap of 4096
    w = _want(oracle, members[0], 4096)
    assert b"<4096,4096>" in w and len(w) < 4096 + 70000 // 4096 * 12 + 64
    assert b"<4094,4094>" in _want(oracle, members[1], 4096) and b"<4096,4096>" in _want(oracle, members[2], 4096)
    members = _pad(lz, members)
    for prof in (_host(mods, oracle, members), _dev(mods, oracle, members)[0]):
        assert prof == ONLY, prof                                             # no kernel of a single call: none was handed back


# ---------------------------------------------------------------- 4: escapes at the edges
def _escapes_at(lz, seed, n, edges):
    """text of n bytes with a 5C or an FF (in turn) wherever its pair of escaped bytes straddles a multiple of one of `edges` in the escaped
    stream, and at the raw offsets around the multiples of 16384 and of 16"""
    d = bytearray(_text(seed, n))
    e, turn = 0, 0                                                            # escaped bytes in front of raw byte i
    for i in range(n):
        straddles = any((e + 1) % m == 0 for m in edges) and e > 0
        raw_edge = i % 16384 in (0, 16383) or i % 4099 in (15, 16)
        if (straddles or raw_edge) and i not in (0, n - 1):
            d[i] = (0x5C, 0xFF)[turn % 2]
            turn += 1
            e += 2
        else:
            e += 1
    return bytes(d)


def test_escapes_at_the_edges(mods, oracle):
    _lib, lz = mods
    P, top = lz.TILE_POS, lz.TILE_IN_MAX
    pairs = _escapes_at(lz, 4050, 70001, (P, 1024))
    a = np.frombuffer(pairs, dtype=np.uint8)
    esc = np.cumsum(np.where((a == 0x5C) | (a == 0xFF), 2, 1)) - np.where((a == 0x5C) | (a == 0xFF), 2, 1)   # the escaped offset of every raw byte
    assert sum(1 for i in np.flatnonzero((a == 0x5C) | (a == 0xFF)) if (esc[i] + 1) % P == 0) >= 30         # a pair across every tile edge
    angle = b"<" + _text(4051, 69000) + b"<"
    both = b"<<" + _text(4052, 3 * P - 4) + b"\\<" + _text(4053, 66000) + b"<\xff"
    # E = TILE_E_MAX exactly: the largest member with TILE_IN_MAX / 16 bytes that escape to two; one more of them: handed back
    full = bytearray(_text(4054, top))
    full[7::16] = bytes((0x5C, 0xFF)) * (top // 32)
    full = bytes(full)
    over = bytearray(full)
    over[8] = 0x5C
    over = bytes(over)
    assert _escaped(full) == lz.TILE_E_MAX and _escaped(over) == lz.TILE_E_MAX + 1
    taken = _pad(lz, [pairs, angle, both, full])
    for prof in (_host(mods, oracle, taken), _dev(mods, oracle, taken)[0]):
        assert prof == ONLY, prof
    mixed = taken[:2] + [over] + taken[2:]
    prof = _host(mods, oracle, mixed)
    assert all(prof.get(name) == 1 for name in TILE), prof
    prof, _ = _dev(mods, oracle, mixed, loose=(2,))
    assert all(prof.get(name) == 1 for name in TILE) and set(prof) - set(ONLY), prof    # ... and the single call's kernels for the one
    # a member of which more than half escapes: handed back as well (lzss_tile_layout.h: lzt_e_cap), whatever TILE_E_MAX would hold
    table = bytes((0x5C, 0xFF)[c % 2] if c in b"abcdefghijklmnop " else c for c in range(256))
    dense = _text(4055, 66000).translate(table)
    assert len(dense) + len(dense) // 2 < _escaped(dense) <= lz.TILE_E_MAX
    mixed = taken[:1] + [dense] + taken[1:]
    prof, _ = _dev(mods, oracle, mixed, loose=(1,))
    assert all(prof.get(name) == 1 for name in TILE) and set(prof) - set(ONLY), prof


# ---------------------------------------------------------------- 5: hand-back by the step cap
def test_runs_and_short_periods_take_the_single_call(mods, oracle):
    _lib, lz = mods
    members = _pad(lz, [_text(4060, 70000)])
    members = members[:3] + [b"a" * 100000] + members[3:8] + [b"ab" * 50000] + members[8:]
    prof = _host(mods, oracle, members)
    assert all(prof.get(name) == 1 for name in TILE), prof                    # the text members' launches stay one set a group
    prof, _ = _dev(mods, oracle, members, loose=(3, 9))
    assert all(prof.get(name) == 1 for name in TILE) and set(prof) - set(ONLY), prof    # ... and the single call's kernels for the two


# ---------------------------------------------------------------- 6: nothing left in scratch matters
def test_scratch_independence(mods, oracle):
    _lib, lz = mods
    P = lz.TILE_POS
    first = _pad(lz, [_text(4070 + i, n) for i, n in enumerate((65537, 34 * P + 1, 100003, 40 * P))])
    slashes = [b"\\" * n for n in (66000, 70001, 131072)]                     # escape to twice their length: handed back by the first launch
    angles = [b"<" * n for n in (66001, 69999, 140000)]                       # FF all over the escaped stream and the keys of a run: handed back by the cap
    noise = [np.random.default_rng(4080 + i).integers(0, 256, size=n, dtype=np.uint8).tobytes() for i, n in enumerate((65537 + 4001, 90001, 150001))]
    between = [_pad(lz, x) for x in (slashes, angles, noise)]
    for form in ("host", "dev"):
        run = (lambda x, **kw: _host(mods, oracle, x)) if form == "host" else (lambda x, **kw: _dev(mods, oracle, x, **kw)[0])
        for other in between:
            assert run(first) == ONLY
            run(other, loose=(0, 1, 2))
        assert run(first) == ONLY


# ---------------------------------------------------------------- 7: the device form's capacities and copies
def test_device_form_capacities_and_copies(mods, oracle):
    _lib, lz = mods
    P = lz.TILE_POS
    members = _pad(lz, [_text(4090 + i, n) for i, n in enumerate((65537, 34 * P - 1, 34 * P + 7, 100000, 131072, 200001))])
    want = [_want(oracle, d, 4096) for d in members]
    assert len({len(w) % 16 for w in want}) >= 4
    # exact capacities between fences
    rc, lens, msg, outs = _fenced_call(_lib, ENC, members, [len(w) for w in want], 4096)
    assert rc == OK, msg
    assert lens == [len(w) for w in want] and [_out_bytes(o, k) for o, k in zip(outs, lens)] == want
    # one byte short: the lowest such member is named with its exact need, out_lens is the capacity rsn.h documents for a member that does
    # not fit (the exact size in whole 16-byte units, and 16), every other member complete, the fences untouched -- and with those
    # capacities the call succeeds
    tight = (1, 2, 5)
    caps = [len(w) - 1 if i in tight else len(w) for i, w in enumerate(want)]
    rc, lens, msg, outs = _fenced_call(_lib, ENC, members, caps, 4096)
    assert rc == E_CAP and msg.startswith("member 1: lzss: output needs %d bytes, buffer holds %d" % (len(want[1]), len(want[1]) - 1)), msg
    for i, w in enumerate(want):
        if i in tight:
            assert lens[i] == _ru16(len(w)) + 16, (i, lens[i], len(w))
        else:
            assert lens[i] == len(w) and _out_bytes(outs[i], lens[i]) == w, i
    rc, lens2, msg, outs = _fenced_call(_lib, ENC, members, [lens[i] if i in tight else caps[i] for i in range(len(want))], 4096)
    assert rc == OK, msg
    assert lens2 == [len(w) for w in want] and [_out_bytes(o, k) for o, k in zip(outs, lens2)] == want
    # members back to back at 16-byte offsets; what crosses to the host is a member's table entries up and its answer down
    prof, copied = _dev(mods, oracle, members)
    assert prof == ONLY, prof
    assert copied[0] <= len(members) * TABLE_UP and copied[1] <= len(members) * TABLE_DOWN, copied
    assert (TABLE_UP, TABLE_DOWN) == (64, 4)


# ---------------------------------------------------------------- 8: layered, round trip, suite
def test_layered_round_trip_and_suite(mods, oracle):
    import torch
    _lib, lz = mods
    from raisin_amd import huffman, layers
    k = max(lz.TILE_GROUP_MIN, huffman.BIG_GROUP_MIN)
    three = [_text(4100 + i, 200000) for i in range(3)]
    members = [three[i % 3] for i in range(k)]
    names = [LZ, HU]
    want = [oracle.huffman_compress(_want(oracle, d, 4096)) for d in three]
    assert [layers.Compress(d, names) for d in three] == want                 # the chain of single calls
    want = [want[i % 3] for i in range(k)]
    grouped = set(ONLY) | HU_GROUPED | {"members_move"}
    got, prof, _ = _prof(_lib, lambda: layers.CompressBatch(members, names))
    assert got == want
    assert all(prof.get(name) == 1 for name in TILE) and prof.get("huff_batch_big_emit") == 1 and not set(prof) - grouped, prof
    ts = [torch.frombuffer(bytearray(d) + bytearray(16), dtype=torch.uint8).cuda()[:len(d)] for d in members]
    torch.cuda.synchronize()
    got, prof, _ = _prof(_lib, lambda: [bytes(t.cpu().numpy()) for t in layers.compress_tensors(ts, names)])
    assert got == want
    assert all(prof.get(name) == 1 for name in TILE) and prof.get("huff_batch_big_emit") == 1 and not set(prof) - grouped, prof
    got, prof, _ = _prof(_lib, lambda: [bytes(t.cpu().numpy()) for t in lz.compress_tensors(ts)])
    assert got == [_want(oracle, d, 4096) for d in members] and prof == ONLY, prof
    # the rows of the batch round trip and of the batch suite are the one-member calls' rows
    rows = layers.RoundTripBatch(members, names, hists=False)
    ones = [layers.RoundTripBatch([d], names, hists=False)[0] for d in three]
    assert rows == [ones[i % 3] for i in range(k)]
    assert [(r.original_n, r.compressed_n, r.decompressed_n, r.lossless) for r in rows] == [(len(d), len(w), len(d), True) for d, w in zip(members, want)]
    lists = [[LZ], names]
    suite, best, errors = layers.SuiteBatch(members, lists, hists=False)
    assert errors == [None, None]
    for l, a in enumerate(lists):
        one = [layers.SuiteBatch([d], [a], hists=False)[0][0][0] for d in three]
        assert suite[l] == [one[i % 3] for i in range(k)], a
    assert suite[1] == rows
