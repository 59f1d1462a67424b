"""GPU: every class of the Huffman batch calls in ONE call, at its minimum -- the rows (small, mid, big) and the class behind them (the rune
encoder, the rune decoder), in both directions, from host buffers and on device buffers (raisin_amd/csrc/codecs.h: BatchClass, BehindClass;
group_run.h: the one device-staging driver, the one host-over-device run; rsn_api.hip: batch_front, layer_batch_run).  Every result is held
against the single call's bytes, and the library's launch profile against what the contract in codecs.h says of each class: one launch a
group for the small, mid and rune classes, three for the tiled ones, one gather and one scatter a group on device buffers, one plan launch
a call and one more over the refused streams when there are at least the rune decoder's minimum of them.  Then a member that does not fit
its buffer, in a class of the rows and in the class behind them: the call's answer across both stages."""
import pytest

from test_gpu_batch_dev import E_CAP, _fenced_call, _out_bytes, _prof, _ru16
from test_gpu_huffman_batch_dev import DEC, ENC, _run_slots
from test_gpu_huffman_rune_batch import _runes
from test_gpu_lzss_mid import _text

pytestmark = pytest.mark.gpu

SMALL_GROUP_MIN = 2                                     # huff_small.hip: the small encoder's (the small decoder groups from one member on)
HB_OUT_MAX = 32768                                      # huff_small_body.h: what k_huff_batch_dec's workgroup decodes at most
RUNE_STREAM_MAX = 256 * 10 + 3 + 8 + 9 * 16384 // 8     # huff_parse_rune.h: HUFF_RUNE_STREAM_MAX
BIG = ("huff_batch_big_count", "huff_batch_big_plan", "huff_batch_big_emit")
BIG_DEC = ("huff_batch_big_dec_map", "huff_batch_big_dec_chain", "huff_batch_big_dec_emit")
GROUPED = ("huff_batch_enc", "huff_batch_mid_enc", "huff_batch_rune_enc", "huff_batch_dec", "huff_batch_mid_dec", "huff_batch_rune_dec",
           "group_gather", "group_scatter", "huff_dev_gather", "huff_dev_scatter", "huff_dev_plan", "huff_dev_rune_plan") + BIG + BIG_DEC
VARIANTS = ("at the minimums", "one rune member fewer", "fewer refused streams than the minimum")


@pytest.fixture(scope="module")
def mods():
    from raisin_amd import _lib, huffman
    _lib.check(_lib.lib().rsn_device_set(0))
    assert (huffman.MID_GROUP_MIN, huffman.BIG_GROUP_MIN, huffman.BIG_DEC_GROUP_MIN, huffman.RUNE_GROUP_MIN, huffman.RUNE_DEC_GROUP_MIN) == (4, 4, 4, 16, 16)
    assert huffman.BATCH_COMPRESS_INPUT_MAX == 16384 and huffman.MID_IN_MAX == 65536 and huffman.MID_OUT_MAX == 65536
    return _lib, huffman


def _rune_member(k):
    d = (b"file %02d, one accent:" % k).ljust(23) + "é".encode()
    assert len(d) == 25 and d.decode().count("é") == 1
    return d


def _members(huffman, variant):
    """-> [(data, class)] in a call's order, the classes interleaved.  class: "small", "mid", "big", "rune" -- what the compress batch runs it
    through -- "mid dec" (ASCII text of HB_OUT_MAX + 1 bytes: the smallest stream the mid DECODER takes; the mid encoder takes it too), or
    "single": handed back by every kernel it meets, or of a class that is below its minimum in this call."""
    n_rune = huffman.RUNE_GROUP_MIN - (0 if variant == VARIANTS[0] else 1)
    rune = "rune" if variant == VARIANTS[0] else "single"
    out = [(_rune_member(k), rune) for k in range(n_rune)]
    out[3:3] = [(b"ab", "small"), (_text(4100, huffman.BATCH_COMPRESS_INPUT_MAX + 1), "mid"), (_text(4200, huffman.MID_IN_MAX + 1), "big")]
    out[9:9] = [(_text(4101 + k, huffman.BATCH_COMPRESS_INPUT_MAX + 1), "mid") for k in range(huffman.MID_GROUP_MIN - 1)]
    out += [(_text(4201 + k, huffman.MID_IN_MAX + 1), "big") for k in range(huffman.BIG_GROUP_MIN - 1)] + [(b"cd", "small")]
    out += [(_text(4300 + k, HB_OUT_MAX + 1), "mid dec") for k in range(huffman.MID_GROUP_MIN)]
    assert SMALL_GROUP_MIN == 2
    many = _runes(0x100, 257) + _runes(0x100, 40)                         # more distinct runes than the rune kernels hold
    if variant == VARIANTS[0]:
        out[6:6] = [(b"a" * 100, "single"), (many.encode(), "single")]    # a single repeated byte; handed back by the byte kernel AND the rune kernel
    elif variant == VARIANTS[1]:
        # over the rune encoder's size: it never counts towards its minimum; its stream is the sixteenth the byte decoders' plan refuses
        out[6:6] = [(b"a" * 100, "single"), ((many * 30).encode(), "single")]
        assert len(out[7][0]) > 16384
    else:
        out[6:6] = [(b"aa", "single")]                                    # (its stream is shorter than any a plan looks at)
    return out


_SINGLE = {}


def _single_enc(huffman, d):
    if d not in _SINGLE:
        _SINGLE[d] = huffman.Compress(d)
    return _SINGLE[d]


def _want_counts(classes, device, refused=0):
    """the launch profile's grouped names: {name: count}, from the classes present (each in one group here) and the form"""
    want = {}
    enc = {"small": "huff_batch_enc", "mid": "huff_batch_mid_enc", "rune": "huff_batch_rune_enc"}
    dec = {"small dec": "huff_batch_dec", "mid dec": "huff_batch_mid_dec", "rune dec": "huff_batch_rune_dec"}
    for k in classes:
        for name in ([enc[k]] if k in enc else [dec[k]] if k in dec else BIG if k == "big" else BIG_DEC):
            want[name] = 1
    # one gather and one scatter a group on device staging: every class in the device form, and the tiled ones in the host form too
    staged = sum(1 for k in classes if k == "big" or (device and k in ("small", "mid", "rune", "rune dec")))    # the SmallMember family (group_dev.hip)
    planned = sum(1 for k in classes if k == "big dec" or (device and k in ("small dec", "mid dec")))          # the decoders' family (huff_dev.hip)
    if staged:
        want["group_gather"] = want["group_scatter"] = staged
    if planned:
        want["huff_dev_gather"] = want["huff_dev_scatter"] = planned
    if device and any(k.endswith("dec") for k in classes):
        want["huff_dev_plan"] = 1                                         # (the host form plans on the host)
    if device and refused >= 16:
        want["huff_dev_rune_plan"] = 1
    return want


def _grouped(prof):
    return {k: v for k, v in prof.items() if k in GROUPED}


@pytest.mark.parametrize("variant", VARIANTS)
def test_compress_every_class_in_one_call(mods, variant):
    _lib, huffman = mods
    members = _members(huffman, variant)
    datas = [d for d, _ in members]
    want = [_single_enc(huffman, d) for d in datas]
    classes = {"mid" if k == "mid dec" else k for _, k in members} - {"single"}
    assert classes == ({"small", "mid", "big", "rune"} if variant == VARIANTS[0] else {"small", "mid", "big"})
    got, prof = _prof(_lib, lambda: huffman.CompressBatch(datas))[:2]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, members[i][1], len(datas[i]))
    assert _grouped(prof) == _want_counts(classes, False), prof
    bound = _lib.lib().rsn_huffman_compress_bound
    caps = [bound(len(d)) if k == "single" else len(w) for (d, k), w in zip(members, want)]         # exact sizes wherever a class takes the member
    loose = {i for i, (_, k) in enumerate(members) if k == "single"}
    got, prof, _ = _run_slots(_lib, ENC, datas, caps, loose=loose)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, members[i][1], len(datas[i]))
    assert _grouped(prof) == _want_counts(classes, True), prof


@pytest.mark.parametrize("variant", VARIANTS)
def test_decompress_every_class_in_one_call(mods, variant):
    _lib, huffman = mods
    members = _members(huffman, variant)
    datas = [d for d, _ in members]
    streams = [_single_enc(huffman, d) for d in datas]
    # the decoders' classes: by what the stream promises, not by what encoded it -- 16 KiB + 1 of text is a stream the small decoder holds
    dec_class = {"small": "small dec", "mid": "small dec", "mid dec": "mid dec", "big": "big dec", "rune": "rune dec", "single": "single"}
    kinds = [dec_class[k] for _, k in members]
    classes = set(kinds) - {"single"}
    assert classes == {"small dec", "mid dec", "big dec"} | ({"rune dec"} if variant == VARIANTS[0] else set())
    want = [huffman.Decompress(s) for s in streams]                       # the single call: the member itself, but for a single symbol's stream
    assert all(w == d for w, d in zip(want, datas) if len(set(d)) > 1)
    # what k_huff_dev_plan refuses of these: a header that names a rune, or a single symbol -- when the plan looks at the stream at all
    refused = sum(1 for d, s in zip(datas, streams) if 8 <= len(s) <= RUNE_STREAM_MAX and (max(d) >= 0x80 or len(set(d)) == 1))
    assert (refused >= 16) == (variant != VARIANTS[2]) and (variant != VARIANTS[1] or refused >= 16 > sum(1 for k in kinds if k == "rune dec"))
    got, prof = _prof(_lib, lambda: huffman.DecompressBatch(streams))[:2]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, kinds[i], len(datas[i]))
    assert _grouped(prof) == _want_counts(classes, False), prof
    caps = [_ru16(len(w)) + 16 if k == "single" else len(w) for w, k in zip(want, kinds)]
    got, prof, _ = _run_slots(_lib, DEC, streams, caps)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, kinds[i], len(datas[i]))
    assert _grouped(prof) == _want_counts(classes, True, refused), prof


@pytest.mark.parametrize("short", ("rune", "big", "both"))
def test_a_member_that_does_not_fit_across_both_stages(mods, short):
    """device buffers: one member of the rune decoder's group (the class behind the rows, settled last) and / or one of the tiled decoder's (a
    row, settled first) has an out_cap one byte short -- RSN_ERR_CAPACITY with the lowest such member, its out_lens as the single call
    reports it (the size rounded up to 16, plus 16), and every other member complete"""
    _lib, huffman = mods
    members = _members(huffman, VARIANTS[0])
    datas = [d for d, k in members if k in ("rune", "big", "small")]
    kinds = [k for _, k in members if k in ("rune", "big", "small")]
    streams = [_single_enc(huffman, d) for d in datas]
    rune_at, big_at = [i for i, k in enumerate(kinds) if k == "rune"][5], [i for i, k in enumerate(kinds) if k == "big"][1]
    assert rune_at < big_at                                                # the lowest is the second stage's, though the rows settle first
    tight = {"rune": [rune_at], "big": [big_at], "both": [rune_at, big_at]}[short]
    caps = [len(d) - 1 if i in tight else len(d) for i, d in enumerate(datas)]
    (rc, lens, msg, outs), prof = _prof(_lib, lambda: _fenced_call(_lib, DEC, streams, caps))[:2]
    low = tight[0]
    assert rc == E_CAP and msg.startswith("member %d: huffman: output needs %d bytes, buffer holds %d" % (low, len(datas[low]), len(datas[low]) - 1)), msg
    assert prof.get("huff_batch_rune_dec") == 1 and all(prof.get(n) == 1 for n in BIG_DEC), prof    # both classes ran grouped
    for i, d in enumerate(datas):
        if i in tight:
            assert lens[i] == _ru16(len(d)) + 16, (i, lens[i])             # the single call's figure
        else:
            assert lens[i] == len(d) and _out_bytes(outs[i], lens[i]) == d, (i, kinds[i])
