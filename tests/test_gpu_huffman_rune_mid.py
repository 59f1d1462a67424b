"""GPU: the grouped Huffman encoder for members of more than 16 KiB and at most 64 KiB with bytes >= 0x80 (k_huff_mid_rune_enc,
raisin_amd/csrc/huff_rune_mid.hip): a call that holds at least huffman.RUNE_MID_GROUP_MIN members which k_huff_mid_enc hands
back because of such a byte runs them one launch per group, in the host form, the device form and the layered forms.  Every expected byte
comes from the CPU oracle (oracle.huffman_compress) AND the library's single call (huffman.Compress), which are held equal once per input,
never from a batch call; the instruments are tests/test_gpu_batch_dev.py's -- members back to back in ONE allocation with hostile bytes
between them, outputs with out_cap exactly the result size, the library's launch profile.

The host form's profile names the byte kernel too: a member reaches this class because k_huff_mid_enc answered GROUP_BACK_RUNES for it, so a
call of such members alone is {"huff_batch_mid_enc": 1, "huff_batch_rune_mid_enc": 1}, as the 16 KiB class's is huff_batch_enc and its own.
The host form deals its single calls over worker threads whose launches the calling thread's profile does not hold: there the exact
profile is the statement that nothing else ran; "the general encoder ran" is asserted of the device form, which runs them on its stream.

The deepest code: a chain of 23 leaves needs counts that sum to at least fib(24) = 46368 when every tie falls towards the chain and
fib(25) - 1 = 75024 when none does (tests/long_codes.py's fib_data); under the reference's heap the smallest such table found is DEEP below,
64074 runes, which fits a member only with its eight frequent symbols as ASCII (65437 bytes)."""
import numpy as np
import pytest

import long_codes
from test_gpu_batch_dev import E_CAP, OK, Pack, Slots, _batch, _prof, _ru16
from test_gpu_huffman_batch_dev import ENC, _run_slots

pytestmark = pytest.mark.gpu

GENERAL = ("huff_byte_hist", "huff_rune", "huff_tile_bits", "huff_emit")   # name fragments of the general encoder's launches (test_gpu_huffman_batch_compress.py)
RUNE, RUNE_MID, MID, SMALL = "huff_batch_rune_enc", "huff_batch_rune_mid_enc", "huff_batch_mid_enc", "huff_batch_enc"
BIG = ("huff_batch_big_count", "huff_batch_big_plan", "huff_batch_big_emit")
HDR_MAX = 256 * 10 + 3                                    # group_layout.h: HUFF_RUNE_HDR_MAX
K16, K64 = 16384, 65536
ROUNDS = (16384, 32768, 49152)                           # where a round of the emit ends: 1024 lanes of 16 bytes
E_ACUTE, EURO, CLEF = "é".encode(), "€".encode(), "𝄞".encode()
# each width of rune, each invalid form, and a lead the member's end (or the ASCII behind it) cuts off
FORMS = (E_ACUTE, EURO, CLEF, b"\x80", b"\xc0\x80", b"\xe0\x80\x80", b"\xed\xa0\x80", b"\xf0\x80\x80\x80", b"\xf5", b"\xe2\x82", b"\xf0\x9f\x8e")
DEEP = (1, 1, 1, 3, 4, 7, 11, 18, 29, 47, 76, 123, 199, 322, 521, 843, 1364, 2207, 3571, 5778, 9348, 15126, 24474)
LZ, HU = "lzss", "huffman"

_WORDS = np.array([w.encode() for w in ("the", "quick", "brown", "fox", "jumps", "over", "lazy", "dog", "naïve", "café", "a", "I", "Sam", "déjà", "vu",
                                         "green", "eggs", "and", "señor", "would", "not", "could", "in", "box", "with", "house", "mouse", "here", "there",
                                         "über", "12", "€", "anywhere", "compression")], dtype=object)
_SEPS = np.array([b" ", b" ", b" ", b"\n", b", ", b". "], dtype=object)


def _text(seed, n):
    """n bytes of UTF-8 text, about one accented letter in twenty; it ends at a rune's end, and `seed` in front keeps members distinct"""
    rng = np.random.default_rng(seed)
    k = n // 3 + 8
    parts = np.empty(2 * k, dtype=object)
    parts[0::2] = _WORDS[rng.integers(0, len(_WORDS), k)]
    parts[1::2] = _SEPS[rng.integers(0, len(_SEPS), k)]
    t = b"%d " % seed + b"".join(parts)
    assert len(t) >= n
    t = bytearray(t[:n])
    for k in (1, 2, 3):                                   # a rune the cut went through: full stops instead
        if k <= n and t[-k] >= 0xC0:
            t[-k:] = b"." * k
            break
        if k <= n and t[-k] < 0x80:
            break
    assert max(t) >= 0x80
    return bytes(t)


def _ascii(seed, n):
    return _text(seed, n + n // 8).decode().encode("ascii", "ignore")[:n]


@pytest.fixture(scope="module")
def mods():
    from raisin_amd import _lib, huffman, layers
    _lib.check(_lib.lib().rsn_device_set(0))
    assert huffman.RUNE_MID_GROUP_MIN >= 16 and huffman.RUNE_MID_IN_MAX == K64 and huffman.BATCH_COMPRESS_INPUT_MAX == K16
    return _lib, huffman, layers


_ENC = {}


@pytest.fixture(scope="module")
def want(mods, oracle):
    """d -> the oracle's stream, which the single call's equals: computed once per input"""
    huffman = mods[1]

    def f(d):
        if d not in _ENC:
            _ENC[d] = oracle.huffman_compress(d)
            assert huffman.Compress(d) == _ENC[d], (len(d), d[:24])
        return _ENC[d]
    return f


def _general(prof):
    return any(any(f in k for f in GENERAL) for k in prof)


def _both_forms(_lib, huffman, want, datas, taken=None, behind=lambda i: b"\xac\xbf\x80"):
    """the list through CompressBatch and through the device form on exact capacities where the class takes the member, poisoned bytes
    behind every member and every output -> (host profile, device profile)"""
    exp = [want(d) for d in datas]
    got, prof = _prof(_lib, lambda: huffman.CompressBatch(datas))[:2]
    assert len(got) == len(datas)
    for d, w, g in zip(datas, exp, got):
        assert g == w, (len(d), d[:24])
    taken = taken or [True] * len(datas)
    bound = _lib.lib().rsn_huffman_compress_bound
    caps = [len(w) if t else bound(len(d)) for d, w, t in zip(datas, exp, taken)]
    got, dprof, _ = _run_slots(_lib, ENC, datas, caps, behind=behind, loose={i for i, t in enumerate(taken) if not t})
    for d, w, g in zip(datas, exp, got):
        assert g == w, (len(d), d[:24])
    return prof, dprof


# ---------------------------------------------------------------- 1: sizes and profiles
SIZES = (16385, 16400, 32767, 32768, 32769, 49151, 49152, 49153, 65535, 65536)


def test_sizes_one_launch_and_no_general_encoder(mods, want):
    _lib, huffman, _ = mods
    n = huffman.RUNE_MID_GROUP_MIN
    datas = [_text(1000 * s + v, size) for s, size in enumerate(SIZES) for v in range(n)]
    assert sorted(set(map(len, datas))) == sorted(SIZES) and len(set(datas)) == len(datas)
    prof, dprof = _both_forms(_lib, huffman, want, datas)
    assert prof == {MID: 1, RUNE_MID: 1}, prof             # the byte kernel that hands them back, and the class: nothing else
    assert dprof.get(RUNE_MID) == 1 and dprof.get(MID) == 1 and RUNE not in dprof and not _general(dprof), dprof


def test_sizes_next_to_the_class_go_where_they_went(mods, want):
    _lib, huffman, _ = mods
    n = huffman.RUNE_MID_GROUP_MIN
    datas, taken = [], []
    for v in range(n):
        datas += [_text(20000 + v, 16384), _text(21000 + v, 16385), _text(22000 + v, 65536), _text(23000 + v, 65537)]
        taken += [True, True, True, False]
    prof, dprof = _both_forms(_lib, huffman, want, datas, taken)
    for p in (prof, dprof):
        assert p.get(RUNE_MID) == 1 and p.get(RUNE) == 1, p                       # 16384: the 16 KiB class
    assert _general(dprof), dprof                                                 # 65537: the single call


def test_exactly_the_minimum_and_one_fewer(mods, want):
    _lib, huffman, _ = mods
    n = huffman.RUNE_MID_GROUP_MIN
    datas = [_text(30000 + v, 16385 + 3000 * v) for v in range(n)]
    assert max(map(len, datas)) <= K64
    prof, dprof = _both_forms(_lib, huffman, want, datas)
    assert prof == {MID: 1, RUNE_MID: 1} and dprof.get(RUNE_MID) == 1 and not _general(dprof), (prof, dprof)
    prof, dprof = _both_forms(_lib, huffman, want, datas[:n - 1], [False] * (n - 1))
    assert prof == {MID: 1}, prof
    assert RUNE_MID not in dprof and RUNE not in dprof and _general(dprof), dprof


# ---------------------------------------------------------------- 2: round boundaries
def _across(form, shift, v):
    """64 KiB of text with `form` starting `shift` bytes before every round's end (shift 0: at the round's first byte; shift > its length:
    it ends before), the same across the 16-byte unit behind each round's end, and as the member's last bytes"""
    t = bytearray(_text(40000 + v, K64))
    for b in ROUNDS:
        for at in (b - shift, b + 16 - shift):
            t[at - 8:at + 8] = b"(boundary here) "                   # ASCII around it, whatever the text held: no rune of the text is cut
            t[at:at + len(form)] = form
    t[-8:] = b" the end"
    t[K64 - len(form):] = form
    return bytes(t)


def test_runes_and_invalid_forms_across_the_rounds(mods, want):
    _lib, huffman, _ = mods
    datas = [_across(f, shift, 10 * k + shift) for k, f in enumerate(FORMS) for shift in range(0, len(f) + 1)]
    assert len(datas) >= huffman.RUNE_MID_GROUP_MIN and all(len(d) == K64 for d in datas)
    d = _across(CLEF, 2, 0)
    assert d[16382:16386] == CLEF and d[16398:16402] == CLEF and d[49150:49154] == CLEF and d.endswith(CLEF)
    prof, dprof = _both_forms(_lib, huffman, want, datas)
    assert prof == {MID: 1, RUNE_MID: 1} and dprof.get(RUNE_MID) == 1 and not _general(dprof), (prof, dprof)


# ---------------------------------------------------------------- 3: the alphabet's limits, the counts, the depth
def _runes(first, count):
    return "".join(chr(first + k) for k in range(count))


def _rare_in(fill, total, rare, v):
    """`total` bytes: `fill` (one ASCII byte) everywhere but for the byte strings `rare`, spread out, at places that vary with v"""
    n_fill = total - sum(map(len, rare))
    cuts = [(k + 1) * n_fill // (len(rare) + 1) + 97 * v for k in range(len(rare))]
    out, at = bytearray(), 0
    for c, r in zip(cuts, rare):
        out += fill * (c - at) + r
        at = c
    out += fill * (n_fill - at)
    assert len(out) == total
    return bytes(out)


def _uniform_256(v):
    """128 ASCII bytes and 128 two-byte runes, as uniform as 65536 bytes allow: 170 of each ASCII byte, 171 of each rune, shuffled"""
    rng = np.random.default_rng(500 + v)
    sym = np.concatenate([np.repeat(np.arange(128), 170), np.repeat(np.arange(128, 256), 171)])
    rng.shuffle(sym)
    hi = (0x100 + v + sym - 128).astype(np.uint32)
    two = np.stack([0xC0 | (hi >> 6), 0x80 | (hi & 0x3F)], axis=1).astype(np.uint8)
    one = np.stack([sym, sym], axis=1).astype(np.uint8)
    keep = np.stack([np.ones(len(sym), bool), sym >= 128], axis=1)
    return np.where((sym >= 128)[:, None], two, one)[keep].tobytes()


def _deep(v):
    """DEEP's counts, shuffled: the fifteen rare symbols two-byte runes, the eight frequent ones ASCII letters"""
    rng = np.random.default_rng(700 + v)
    sym = np.repeat(np.arange(len(DEEP)), DEEP)
    rng.shuffle(sym)
    hi = (0x100 + 7 * sym + v).astype(np.uint32)
    two = np.stack([0xC0 | (hi >> 6), 0x80 | (hi & 0x3F)], axis=1).astype(np.uint8)
    one = np.stack([0x41 + sym, sym], axis=1).astype(np.uint8)
    keep = np.stack([np.ones(len(sym), bool), sym < 15], axis=1)
    return np.where((sym < 15)[:, None], two, one)[keep].tobytes()


def _shapes():
    """[(name, variant(v) -> bytes, taken by the class)]"""
    out = [("256 distinct runes", lambda v: (_runes(0x100 + 7 * v, 256) * 40 + _runes(0x100 + 7 * v, 40 + v)).encode(), True),
           ("257 distinct runes", lambda v: (_runes(0x100 + 7 * v, 257) * 40 + _runes(0x100 + 7 * v, 40 + v)).encode(), False),
           ("one distinct rune", lambda v: E_ACUTE * (9000 + v), False),
           ("the only high byte is the last", lambda v: _ascii(600 + v, 20000 + 16 * v - 1) + b"\xe9", True),
           ("the only high bytes are the last rune", lambda v: _ascii(650 + v, K64 - 3) + EURO, True),
           ("128 ASCII bytes and 128 two-byte runes, uniform", _uniform_256, True),
           ("one rune 65534 times beside two others", lambda v: _rare_in(b"a", K64, [b"b", b"\xff"], v), True),
           ("65535 beside one", lambda v: _rare_in(b"a", K64, [bytes([0xF8 + v % 8])] if v < 8 else [b"\x80"], 7 * v), True),
           ("counts of exactly 16385, 9999 and 10000", lambda v: _rare_in(b"e", 16385 + 9999 + 10000 + 2 * (v + 1), [b"x"] * 9999 + [b"yy"] * 5000 + [E_ACUTE] * (v + 1), 0), True),
           ("a code of 22 bits", _deep, True)]
    return out


@pytest.fixture(scope="module")
def shapes(mods):
    """every shape in RUNE_MID_GROUP_MIN copies with variation, shape-major: (datas, taken)"""
    huffman = mods[1]
    datas, taken = [], []
    for name, variant, takes in _shapes():
        for v in range(huffman.RUNE_MID_GROUP_MIN):
            d = variant(v)
            assert K16 < len(d) <= K64 and max(d) >= 0x80, (name, v, len(d))
            datas.append(d)
            taken.append(takes)
    assert len(set(datas)) == len(datas)
    return datas, taken


def test_the_shapes_are_what_they_say():
    from collections import Counter
    d = _uniform_256(3)
    c = Counter(d.decode())
    assert len(d) == K64 and len(c) == 256 and sorted(set(c.values())) == [170, 171]
    d = _deep(0)
    c = Counter(d.decode())
    assert sorted(c.values()) == sorted(DEEP) and len(d) == 65437
    assert max(len(x) for x in long_codes.codes({ord(r): k for r, k in c.items()}).values()) == 22
    c = Counter(_rare_in(b"a", K64, [b"b", b"\xff"], 5).decode("utf-8", "replace"))
    assert sorted(c.values()) == [1, 1, 65534]
    c = Counter(_shapes()[8][1](2).decode())
    assert c["e"] == 16385 and c["x"] == 9999 and c["y"] == 10000 and c["é"] == 3
    c = Counter(_shapes()[7][1](1).decode("utf-8", "replace"))
    assert sorted(c.values()) == [1, 65535]


def test_alphabet_limits_counts_and_depth(mods, want, shapes):
    _lib, huffman, _ = mods
    datas, taken = shapes
    prof, dprof = _both_forms(_lib, huffman, want, datas, taken)
    assert prof == {MID: 1, RUNE_MID: 1}, prof
    assert dprof.get(RUNE_MID) == 1 and dprof.get(MID) == 1 and RUNE not in dprof and _general(dprof), dprof     # (what the kernel handed back took the single call)
    n = huffman.RUNE_MID_GROUP_MIN
    for name, d in (("uniform", datas[5 * n]), ("deep", datas[9 * n])):
        assert len(want(d)) <= len(d) + HDR_MAX, name                     # the derived bound of the image: a byte a rune at most, and the header


def test_only_the_taken_shapes_leave_no_general_launch(mods, want, shapes):
    _lib, huffman, _ = mods
    datas = [d for d, t in zip(*shapes) if t]
    got, prof = _prof(_lib, lambda: huffman.CompressBatch(datas))[:2]
    assert got == [want(d) for d in datas]
    assert prof == {MID: 1, RUNE_MID: 1}, prof


# ---------------------------------------------------------------- 4: a mixed call, in index order
def test_mixed_call_keeps_index_order(mods, want):
    _lib, huffman, _ = mods
    datas = []
    for k in range(huffman.RUNE_MID_GROUP_MIN + 1):
        datas += [_ascii(50000 + k, 300 + 11 * k), _ascii(51000 + k, 20000 + k), _text(52000 + k, 900 + 100 * k), _text(53000 + k, 17000 + 2900 * k)]
        if k < huffman.BIG_GROUP_MIN + 1:
            datas.append(_ascii(54000 + k, 70000 + k))
        if k == 7:
            datas.append(_text(55000, 70000))
    taken = [len(d) != 70000 or max(d) < 0x80 for d in datas]
    assert taken.count(False) == 1
    prof, dprof = _both_forms(_lib, huffman, want, datas, taken)
    for p in (prof, dprof):
        assert all(p.get(name) == 1 for name in (SMALL, MID, RUNE, RUNE_MID) + BIG), p
    assert _general(dprof), dprof                                                   # the rune member of 70000 bytes


# ---------------------------------------------------------------- 5: the device form's contracts
def test_a_capacity_one_byte_short(mods, want):
    _lib, huffman, _ = mods
    datas = [_text(60000 + k, 16385 + 2000 * k) for k in range(huffman.RUNE_MID_GROUP_MIN + 1)]
    exp = [want(d) for d in datas]
    short = 5
    caps = [len(w) for w in exp]
    caps[short] -= 1
    pack, slots = Pack(datas, lambda i: b"\xac\xbf"), Slots(caps)
    (rc, lens, msg), prof, _ = _prof(_lib, lambda: _batch(_lib, ENC, [(pack.ptr(i), len(d), slots.ptr(i), caps[i]) for i, d in enumerate(datas)]))
    assert rc == E_CAP and msg.startswith("member %d: " % short), (rc, msg)
    assert prof.get(RUNE_MID) == 1 and not _general(prof), prof
    h = slots.host()
    for i, w in enumerate(exp):
        o = slots.offs[i]
        if i == short:
            assert lens[i] == _ru16(len(w)) + 32                           # the figure the single call reports (rsn.h)
            assert (h[o:o + _ru16(caps[i]) + 16] == 0xEE).all()              # nothing of it was written
        else:
            assert lens[i] == len(w) and bytes(h[o:o + len(w)]) == w, i
            assert (h[o + len(w):o + _ru16(caps[i]) + 16] == 0xEE).all(), i


def test_a_cut_rune_is_not_completed_by_what_lies_behind(mods, want):
    _lib, huffman, _ = mods
    datas = []
    for k in range(huffman.RUNE_MID_GROUP_MIN):
        body = _text(61000 + k, 16400 + 3001 * k)
        # an odd one fills whole 16-byte units and ends in a lone E2 (Pack puts 16 bytes of 82 AC .. behind it); an even one ends in E2 82, one byte short of a unit (AC)
        body += b"." * ((15 - len(body)) % 16 if k % 2 else (13 - len(body)) % 16)
        datas.append(body + (b"\xe2" if k % 2 else b"\xe2\x82"))
    assert all(len(d) % 16 == (0 if k % 2 else 15) for k, d in enumerate(datas))
    behind = lambda i: b"\x82\xac" if i % 2 else b"\xac"
    exp = [want(d) for d in datas]
    got, prof, _ = _run_slots(_lib, ENC, datas, [len(w) for w in exp], behind=behind)
    assert got == exp
    assert prof.get(RUNE_MID) == 1 and not _general(prof), prof
    pack = Pack(datas, behind)
    whole = bytes(pack.t.cpu().numpy())
    assert whole[pack.offs[1] + len(datas[1]) - 1:][:3] == EURO and whole[pack.offs[0] + len(datas[0]) - 2:][:3] == EURO    # what lies behind does complete them


# ---------------------------------------------------------------- 6: through the layers
def test_layered_forms(mods, oracle):
    import torch
    _lib, huffman, layers = mods
    names = [LZ, HU]
    datas = [_text(70000 + k, 40 << 10) for k in range(huffman.RUNE_MID_GROUP_MIN + 2)]
    mids = [oracle.lzss_compress(d, 4096) for d in datas]
    assert sum(K16 < len(m) <= K64 and max(m) >= 0x80 for m in mids) >= huffman.RUNE_MID_GROUP_MIN
    exp = [oracle.huffman_compress(m) for m in mids]
    got, prof = _prof(_lib, lambda: layers.CompressBatch(datas, names))[:2]
    assert got == exp
    assert prof.get(RUNE_MID) == 1 and not _general(prof), prof
    rows, prof = _prof(_lib, lambda: layers.RoundTripBatch(datas, names, hists=False))[:2]
    assert prof.get(RUNE_MID) == 1 and not any(any(f in k for f in GENERAL[:1] + GENERAL[2:]) for k in prof), prof
    for d, w, r in zip(datas, exp, rows):
        rt, _ = layers.RoundTrip(d, names)
        assert (r.original_n, r.compressed_n, r.decompressed_n, r.first_difference, r.lossless) == \
               (rt.original_n, rt.compressed_n, rt.decompressed_n, rt.first_difference, bool(rt.lossless)), d[:24]
        assert (r.original_n, r.compressed_n, r.decompressed_n, r.lossless) == (len(d), len(w), len(d), True), d[:24]
    torch.cuda.synchronize()
