"""GPU: the grouped Huffman encoder for members with bytes >= 0x80 (k_huff_batch_rune_enc, raisin_amd/csrc/huff_rune.hip): a
call that holds at least huffman.RUNE_GROUP_MIN members which the byte encoder hands back because of such a byte, of at most 16 KiB each,
runs them one launch per group, in the host form, the device form and the layered forms.  Every expected byte comes from the CPU oracle
(oracle.huffman_compress), never from the library; the instruments are tests/test_gpu_batch_dev.py's -- members back to back in ONE
allocation with hostile bytes between them, outputs with out_cap exactly the result size, the library's launch profile."""
import pytest

from test_gpu_batch_dev import E_CAP, OK, Pack, Slots, _batch, _prof, _ru16
from test_gpu_huffman_batch_dev import ENC, _run_slots

pytestmark = pytest.mark.gpu

GENERAL = ("huff_byte_hist", "huff_tile_bits", "huff_emit")     # name fragments of the single call's launches
RUNE = "huff_batch_rune_enc"
E_ACUTE, EURO, CLEF = "é".encode(), "€".encode(), "𝄞".encode()
INVALID = (b"\x80", b"\xbf", b"\xc0\x80", b"\xff", b"\xe2\x82", b"\xf0\x9f", b"\xed\xa0\x80", b"\xf4\x90\x80\x80")   # tests/test_gpu_dev_fences.py's forms
LZ, HU = "lzss", "huffman"


@pytest.fixture(scope="module")
def mods():
    from raisin_amd import _lib, huffman, layers
    _lib.check(_lib.lib().rsn_device_set(0))
    assert huffman.RUNE_GROUP_MIN >= 16 and huffman.RUNE_SYMS_MAX == 256
    return _lib, huffman, layers


_ENC = {}


def _want(oracle, d):
    """the oracle's stream, computed once per input"""
    if d not in _ENC:
        _ENC[d] = oracle.huffman_compress(d)
    return _ENC[d]


def _runes(first, count):
    """`count` distinct runes from U+`first` up, none a surrogate"""
    return "".join(chr(first + k) for k in range(count))


def _prefixed(base):
    """copies with variation: variant v has v + 1 more ASCII letters in front -- what the member ends in stays"""
    return lambda v: (bytes([0x41 + v % 26]) * (v + 1) if v else b"") + base


def _shapes():
    """[(name, variant(v) -> bytes, taken by the rune class)] -- the small shapes of the class and the two it hands back"""
    out = [("width %d" % len(r), _prefixed(b"a" + r), True) for r in (E_ACUTE, EURO, CLEF)]      # (the first is "aé": two runes)
    out.append(("text", _prefixed("héllo wörld, naïve café. ".encode() * 20), True))
    out += [("invalid " + f.hex(), _prefixed(b"some text " + f + b" and more of it"), True) for f in INVALID]
    out.append(("ends in E2 82", _prefixed("prix: 12 €, 13 ".encode() + b"\xe2\x82"), True))
    out.append(("literal EF BF BD and an invalid byte", _prefixed(b"ab \xef\xbf\xbd cd \xff ef \xef\xbf\xbd"), True))
    out.append(("every byte value, lossy", _prefixed(bytes(range(256)) * 3), True))
    out.append(("header's special bytes", _prefixed(b"line 1\nline 2 | 3 \\ 4 \\n 5566778899 " + E_ACUTE + b"\n"), True))
    # exact sizes of 2-byte runes: 8192 runes at 16384 bytes; at 16383 the last byte is a lone lead
    out.append(("16384 of 2-byte runes", lambda v: (_runes(0xC0 + v, 37) * 222).encode()[:16384], True))
    out.append(("16383 of 2-byte runes", lambda v: (_runes(0xC0 + v, 37) * 222).encode()[:16383], True))
    out.append(("256 distinct runes", lambda v: (_runes(0x100 + 7 * v, 256) + _runes(0x100 + 7 * v, 40 + v)).encode(), True))
    out.append(("257 distinct runes", lambda v: (_runes(0x100 + 7 * v, 257) + _runes(0x100 + 7 * v, 40 + v)).encode(), False))
    out.append(("one distinct rune", lambda v: E_ACUTE * (9 + v), False))
    return out


@pytest.fixture(scope="module")
def shapes(mods):
    """every shape in RUNE_GROUP_MIN copies with variation, shape-major: (datas, taken)"""
    huffman = mods[1]
    datas, taken = [], []
    for _, variant, takes in _shapes():
        for v in range(huffman.RUNE_GROUP_MIN):
            datas.append(variant(v))
            taken.append(takes)
    assert len(set(datas)) == len(datas) and max(map(len, datas)) == 16384
    assert all(max(d) >= 0x80 and len(d) >= 2 for d in datas)
    return datas, taken


def _utf8(k, n=0):
    """member k of a batch the class takes whole: UTF-8 text of about n bytes (0: a few dozen)"""
    line = ("naïve café n° %d: 12 € — déjà vu, señor. " % k).encode()
    return line * max(1, n // len(line))


# ---------------------------------------------------------------- 1: small shapes, host form and device form
def test_shapes_host_form(mods, oracle, shapes):
    _lib, huffman, _ = mods
    datas, _ = shapes
    got, prof = _prof(_lib, lambda: huffman.CompressBatch(datas))[:2]
    assert len(got) == len(datas)
    for d, g in zip(datas, got):
        assert g == _want(oracle, d), (len(d), d[:24])
    assert prof.get(RUNE) == 1 and prof.get("huff_batch_enc") == 1, prof
    for d in datas[::huffman.RUNE_GROUP_MIN] + datas[5::huffman.RUNE_GROUP_MIN]:
        assert huffman.Compress(d) == _want(oracle, d), (len(d), d[:24])


def test_shapes_device_form(mods, oracle, shapes):
    _lib, huffman, _ = mods
    datas, taken = shapes
    want = [_want(oracle, d) for d in datas]
    bound = _lib.lib().rsn_huffman_compress_bound
    caps = [len(w) if t else bound(len(d)) for d, w, t in zip(datas, want, taken)]       # exact sizes where the class takes the member
    loose = {i for i, t in enumerate(taken) if not t}
    got, prof, _ = _run_slots(_lib, ENC, datas, caps, behind=lambda i: b"\xac\xbf\x80", loose=loose)
    for d, w, g in zip(datas, want, got):
        assert g == w, (len(d), d[:24])
    assert prof.get(RUNE) == 1 and prof.get("huff_batch_enc") == 1, prof
    assert any(any(f in k for f in GENERAL) for k in prof), prof         # the members handed back took the single call


# ---------------------------------------------------------------- 2: profiles
def test_device_form_takes_the_minimum_and_not_one_fewer(mods, oracle):
    _lib, huffman, _ = mods
    n = huffman.RUNE_GROUP_MIN
    datas = [_utf8(k, 40 * k) for k in range(n)]
    want = [_want(oracle, d) for d in datas]
    got, prof, _ = _run_slots(_lib, ENC, datas, [len(w) for w in want])
    assert got == want
    assert prof.get(RUNE) == 1, prof
    assert not any(any(f in k for f in GENERAL) for k in prof), prof     # no member took the single call
    bound = _lib.lib().rsn_huffman_compress_bound
    got, prof, _ = _run_slots(_lib, ENC, datas[:n - 1], [bound(len(d)) for d in datas[:n - 1]], loose=set(range(n - 1)))
    assert got == want[:n - 1]
    assert RUNE not in prof and any(any(f in k for f in GENERAL) for k in prof), prof


def test_host_form_launches(mods, oracle):
    _lib, huffman, _ = mods
    n = huffman.RUNE_GROUP_MIN
    datas = [_utf8(k, 40 * k) for k in range(n)]
    got, prof = _prof(_lib, lambda: huffman.CompressBatch(datas))[:2]
    assert got == [_want(oracle, d) for d in datas]
    assert prof == {"huff_batch_enc": 1, RUNE: 1}, prof
    got, prof = _prof(_lib, lambda: huffman.CompressBatch(datas[:n - 1]))[:2]
    assert got == [_want(oracle, d) for d in datas[:n - 1]]
    assert prof == {"huff_batch_enc": 1}, prof
    datas = [b"%d a" % (k % 8) + E_ACUTE for k in range(4097)]             # SMALL_GROUP_MAX members a group (eight contents: the oracle runs eight times)
    got, prof = _prof(_lib, lambda: huffman.CompressBatch(datas))[:2]
    assert prof == {"huff_batch_enc": 2, RUNE: 2}, prof
    assert got == [_want(oracle, d) for d in datas]


def test_mixed_batch_keeps_index_order(mods, oracle):
    _lib, huffman, _ = mods
    datas = []
    for k in range(huffman.RUNE_GROUP_MIN + 3):
        datas += [b"plain ascii text number %d. " % k * (k + 1), _utf8(k, 100 * k), b"z" * (k + 1), _utf8(k, 20 << 10) + b"x" * k,
                  E_ACUTE * (k + 2), b"ascii of twenty KiB %d " % k * 900]
    want = [_want(oracle, d) for d in datas]
    got, prof = _prof(_lib, lambda: huffman.CompressBatch(datas))[:2]
    assert got == want
    assert prof.get(RUNE) == 1 and prof.get("huff_batch_enc") == 1 and prof.get("huff_batch_mid_enc") == 1, prof
    bound = _lib.lib().rsn_huffman_compress_bound
    got, prof, _ = _run_slots(_lib, ENC, datas, [bound(len(d)) for d in datas], loose=set(range(len(datas))))
    assert got == want
    assert prof.get(RUNE) == 1 and prof.get("huff_batch_enc") == 1 and prof.get("huff_batch_mid_enc") == 1, prof


# ---------------------------------------------------------------- 3: fences, device form
def _cut_members(n):
    """members that their neighbours in one allocation would complete: an even one fills whole 16-byte units and ends in a lone E2, the odd
    one behind it starts 82 AC (the rest of that euro sign) and ends in E2 82, and what follows it is AC AC ..."""
    out = []
    for k in range(n):
        if k % 2 == 0:
            body = _utf8(k, 50 + 30 * k)
            body += b"." * (15 - len(body) % 16)
            out.append(body + b"\xe2")
        else:
            out.append(b"\x82\xac" + _utf8(k, 50 + 30 * k) + b"\xe2\x82")
    return out


def test_a_cut_rune_is_not_completed_by_the_neighbours(mods, oracle):
    _lib, huffman, _ = mods
    datas = _cut_members(huffman.RUNE_GROUP_MIN + 2)
    assert all(len(d) % 16 == 0 for d in datas[0::2])
    want = [_want(oracle, d) for d in datas]
    got, prof, _ = _run_slots(_lib, ENC, datas, [len(w) for w in want], behind=lambda i: b"\xac")    # exact capacities; Slots checks what lies outside them
    for d, w, g in zip(datas, want, got):
        assert g == w, (len(d), d[-8:])
    assert prof.get(RUNE) == 1 and not any(any(f in k for f in GENERAL) for k in prof), prof
    pack = Pack(datas, lambda i: b"\xac")
    whole = bytes(pack.t.cpu().numpy())
    assert whole[pack.offs[1] - 1:pack.offs[1] + 2] == EURO and whole[pack.offs[1] + len(datas[1]) - 2:][:3] == EURO    # the neighbours do complete them


def test_a_capacity_one_byte_short(mods, oracle):
    _lib, huffman, _ = mods
    datas = [_utf8(k, 60 * k) for k in range(huffman.RUNE_GROUP_MIN + 1)]
    want = [_want(oracle, d) for d in datas]
    short = 5
    caps = [len(w) for w in want]
    caps[short] -= 1
    pack, slots = Pack(datas), Slots(caps)
    rc, lens, msg = _batch(_lib, ENC, [(pack.ptr(i), len(d), slots.ptr(i), caps[i]) for i, d in enumerate(datas)])
    assert rc == E_CAP and msg.startswith("member %d: " % short), (rc, msg)
    h = slots.host()
    for i, w in enumerate(want):
        o = slots.offs[i]
        if i == short:
            assert lens[i] == _ru16(len(w)) + 32
            assert (h[o:o + _ru16(caps[i]) + 16] == 0xEE).all()              # nothing of it was written
        else:
            assert lens[i] == len(w) and bytes(h[o:o + len(w)]) == w, i
            assert (h[o + len(w):o + _ru16(caps[i]) + 16] == 0xEE).all(), i


# ---------------------------------------------------------------- 4: layered
def test_layered_forms(mods, oracle):
    import torch
    _lib, huffman, layers = mods
    names = [LZ, HU]
    datas = [_utf8(k, 30 + 90 * k) for k in range(huffman.RUNE_GROUP_MIN)] + [b"lossy \xff member, with \xc0\x80 in it"]
    want = [_want(oracle, oracle.lzss_compress(d, 4096)) for d in datas]
    got, prof = _prof(_lib, lambda: layers.CompressBatch(datas, names))[:2]
    assert got == want
    assert prof.get(RUNE) == 1, prof
    pack = Pack(datas, lambda i: b"\xac")
    srcs = [pack.t[o:o + n] for o, n in zip(pack.offs, pack.lens)]
    got, prof = _prof(_lib, lambda: [bytes(t.cpu().numpy()) for t in layers.compress_tensors(srcs, names)])[:2]
    assert got == want
    assert prof.get(RUNE) == 1, prof
    rows, prof = _prof(_lib, lambda: layers.RoundTripBatch(datas, names, hists=False))[:2]
    assert prof.get(RUNE) == 1, prof
    for d, w, r in zip(datas, want, rows):
        rt, _ = layers.RoundTrip(d, names)
        assert (r.original_n, r.compressed_n, r.decompressed_n, r.first_difference, r.lossless) == \
               (rt.original_n, rt.compressed_n, rt.decompressed_n, rt.first_difference, bool(rt.lossless)), d[:24]
        assert r.compressed_n == len(w)
    assert [r.lossless for r in rows] == [True] * (len(datas) - 1) + [False]
    torch.cuda.synchronize()
