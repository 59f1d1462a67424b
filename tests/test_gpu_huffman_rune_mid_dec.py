"""GPU: the grouped Huffman decoder for rune streams that promise more than 16384 and at most 65536 bytes (k_huff_mid_rune_dec,
raisin_amd/csrc/huff_rune_mid_dec.hip): a decompress batch that holds at least huffman.RUNE_MID_DEC_GROUP_MIN such streams
runs them one launch per group, in the host form, the device form (behind one more plan launch, k_huff_dev_rune_mid_plan) and the layered
forms.  Every expected byte comes from the CPU oracle (oracle.huffman_decompress), which the library's single call is held equal to on a
sample; the streams come from oracle.huffman_compress or are built by hand (tests/rune_mid_dec_cases.py), and whether the class takes a
member is the verdict of the CPU model of the lane maps there, which tests/test_huff_rune_mid_dec_host.py pins.  The instruments are
tests/test_gpu_batch_dev.py's: members back to back in ONE allocation with hostile bytes between and behind them, outputs with out_cap
exactly the result size, the library's launch profile."""
import pytest

import rune_mid_dec_cases as C
from test_gpu_batch_dev import E_CAP, E_FORMAT, OK, Pack, Slots, _batch, _fenced_call, _out_bytes, _prof, _ru16
from test_gpu_huffman_batch_dev import DEC, _run_slots
from test_gpu_huffman_rune_dec_batch import FFFD, RUNE, RUNE_PLAN, _build, _dec, _enc, _general, _spread
from test_gpu_huffman_rune_batch import _utf8
from test_gpu_huffman_rune_mid import _text
from test_gpu_lzss_mid import _text as _ascii_text

pytestmark = pytest.mark.gpu

MID, MID_PLAN = "huff_batch_rune_mid_dec", "huff_dev_rune_mid_plan"
# the device form's launches when this class takes every member: none of them is a candidate of the 16 KiB class's plan, whose limit on the
# stream's length (HUFF_RUNE_STREAM_MAX = 21003 bytes) every stream below that is shorter passes -- then that plan launches too, once
TAKEN_DEV = {"huff_dev_plan": 1, MID_PLAN: 1, "group_gather": 1, MID: 1, "group_scatter": 1}
SMALL_STREAM_MAX = 256 * 10 + 3 + 8 + 18432
LZ, HU = "lzss", "huffman"


@pytest.fixture(scope="module")
def mods():
    from raisin_amd import _lib, huffman, layers
    _lib.check(_lib.lib().rsn_device_set(0))
    assert huffman.RUNE_MID_DEC_GROUP_MIN == C.N >= 16 and huffman.RUNE_MID_OUT_MAX == C.OUT_MAX and huffman.RUNE_MID_PAY_MAX == C.PAY_MAX
    assert huffman.RUNE_OUT_MAX == C.OUT_MIN
    return _lib, huffman, layers


def _taken_dev(streams):
    """TAKEN_DEV, and the 16 KiB class's plan launch when at least its minimum of the streams are short enough to be its candidates"""
    small = sum(len(s) <= SMALL_STREAM_MAX for s in streams)
    return dict(TAKEN_DEV, **({RUNE_PLAN: 1} if small >= 16 else {}))


def _both_forms(mods, oracle, streams, names):
    """members the class takes, all of them (the CPU model's verdict, pinned by tests/test_huff_rune_mid_dec_host.py), through
    DecompressBatch and the device form on exact capacities: the bytes, and both profiles exactly -- nothing else runs"""
    _lib, huffman, _ = mods
    want = [_dec(oracle, s) for s in streams]
    got, host_prof = _prof(_lib, lambda: huffman.DecompressBatch(streams))[:2]
    for g, w, n in zip(got, want, names):
        assert g == w, n
    assert host_prof == {MID: 1}, host_prof
    got, dev_prof, _ = _run_slots(_lib, DEC, streams, [len(w) for w in want], behind=lambda i: b"\xac\xbf\x80")
    for g, w, n in zip(got, want, names):
        assert g == w, n
    assert dev_prof == _taken_dev(streams), dev_prof
    return want


# ---------------------------------------------------------------- 1: shapes, host form and device form
def test_shapes(mods, oracle):
    _lib, huffman, _ = mods
    rows = [r for v in range(C.N) for r in C.shapes(v)]
    streams, names = [r[1] for r in rows], [r[0] for r in rows]
    assert all(r[2] == (True, None) for r in rows), [(r[0], r[2]) for r in rows if r[2] != (True, None)]     # the model's verdict: every member is taken
    want = _both_forms(mods, oracle, streams, names)
    assert all(C.OUT_MIN < len(w) <= C.OUT_MAX for w in want)
    by = dict(zip(names, zip(streams, want)))
    assert len(by["largest expansion"][1]) == 65536 and C.payload(by["largest expansion"][0]) == 2048
    assert len(by["two runes at one bit"][1]) == 64373 and len(by["lossy, promises 16385"][1]) == 16385 and by["lossy, promises 16385"][1].endswith(FFFD.encode())
    assert "ж".encode() not in by["a zero count"][1] and b"0|" in by["a zero count"][0]
    assert len(by["promises more than it holds"][1]) < 24000 + 3000
    for s, w in list(zip(streams, want))[:len(C.shapes(0))]:
        assert huffman.Decompress(s) == w                               # the single call and the oracle are held equal


# ---------------------------------------------------------------- 2: not taken
def test_not_taken(mods, oracle):
    """what the class leaves to the single call, which decodes it.  A code of 33 bits shows only once the tree is built: those streams are
    planned, go through the one launch and are handed back; none of the others costs a launch of the class."""
    _lib, huffman, _ = mods
    rows = [r for v in range(C.N) for r in C.not_taken(v)]
    streams, names = [r[1] for r in rows], [r[0] for r in rows]
    want = [_dec(oracle, s) for s in streams]
    got, prof = _prof(_lib, lambda: huffman.DecompressBatch(streams))[:2]
    for g, w, n in zip(got, want, names):
        assert g == w, n
    assert prof.get(MID) == 1 and RUNE not in prof and _general(prof), prof
    got, prof, _ = _run_slots(_lib, DEC, streams, [_ru16(len(w)) + 16 for w in want], behind=lambda i: b"\xac\xbf\x80")
    for g, w, n in zip(got, want, names):
        assert g == w, n
    assert prof.get(MID) == 1 and prof.get(MID_PLAN) == 1 and RUNE not in prof and _general(prof), prof
    rest = [s for s, n in zip(streams, names) if n != "depth 33"]
    got, prof = _prof(_lib, lambda: huffman.DecompressBatch(rest))[:2]
    assert got == [w for w, n in zip(want, names) if n != "depth 33"]
    assert MID not in prof and RUNE not in prof and _general(prof), prof
    assert len(want[names.index("promises 65537")]) == 65537
    for s, w in list(zip(streams, want))[:len(C.not_taken(0))]:
        assert huffman.Decompress(s) == w


# ---------------------------------------------------------------- 3: the limits, taken
def test_limits_taken(mods, oracle):
    rows = [r for v in range(C.N) for r in C.limits_taken(v)]
    assert all(r[2] == (True, None) for r in rows), [(r[0], r[2]) for r in rows if r[2][0] is not True]
    assert {C.payload(r[1]) for r in rows if r[0].startswith("a payload")} == {C.PAY_MAX}
    _both_forms(mods, oracle, [r[1] for r in rows], [r[0] for r in rows])


# ---------------------------------------------------------------- 4: exactly the minimum, and one fewer
def _texts(n):
    return [_text(82000 + k, 16385 + 1031 * k) for k in range(n)]


def test_the_minimum_and_not_one_fewer(mods, oracle):
    _lib, huffman, _ = mods
    n = huffman.RUNE_MID_DEC_GROUP_MIN
    datas = _texts(n)
    streams = [_enc(oracle, d) for d in datas]
    assert [_dec(oracle, s) for s in streams] == datas
    got, prof = _prof(_lib, lambda: huffman.DecompressBatch(streams))[:2]
    assert got == datas
    assert prof == {MID: 1}, prof
    got, prof = _prof(_lib, lambda: huffman.DecompressBatch(streams[:n - 1]))[:2]
    assert got == datas[:n - 1]
    assert MID not in prof and _general(prof), prof
    got, prof, _ = _run_slots(_lib, DEC, streams, [len(d) for d in datas])
    assert got == datas
    assert prof == _taken_dev(streams), prof
    got, prof, _ = _run_slots(_lib, DEC, streams[:n - 1], [len(d) for d in datas[:n - 1]])
    assert got == datas[:n - 1]
    assert MID not in prof and MID_PLAN not in prof and _general(prof), prof


# ---------------------------------------------------------------- 5: more members than a group
def test_more_members_than_a_group(mods, oracle):
    _lib, huffman, _ = mods
    few = [_text(83000 + k, 65536 - 16 * k) for k in range(4)]
    enc = {d: _enc(oracle, d) for d in few}
    assert all(_dec(oracle, enc[d]) == d for d in few)
    datas = [few[(3 * i) % 4] for i in range(170)]                       # 170 x (37 KiB + 64 KiB) of slots: more than a group's 16 MiB
    streams = [enc[d] for d in datas]
    got, prof = _prof(_lib, lambda: huffman.DecompressBatch(streams))[:2]
    assert got == datas
    assert prof == {MID: 2}, prof
    got, prof, _ = _run_slots(_lib, DEC, streams, [len(d) for d in datas])
    assert got == datas
    assert prof == {"huff_dev_plan": 1, MID_PLAN: 1, "group_gather": 2, MID: 2, "group_scatter": 2}, prof


# ---------------------------------------------------------------- 6: a mixed call in index order
def test_mixed_call_in_index_order(mods, oracle):
    _lib, huffman, _ = mods
    datas = []
    for k in range(huffman.RUNE_MID_DEC_GROUP_MIN + 2):
        datas += [_ascii_text(3100 + k, 60 + 90 * k), _utf8(k, 100 * k), _text(84000 + k, 17000 + 2500 * k), _ascii_text(3200 + k, 32 << 10)]
    datas += [_ascii_text(3300 + k, 100 << 10) for k in range(4)]         # the tiled class's
    streams = [_enc(oracle, d) for d in datas]
    want = [_dec(oracle, s) for s in streams]
    assert want == datas
    got, prof = _prof(_lib, lambda: huffman.DecompressBatch(streams))[:2]
    assert got == want
    names = (RUNE, MID, "huff_batch_dec", "huff_batch_mid_dec")
    assert all(prof.get(k) == 1 for k in names) and any(k.startswith("huff_batch_big_dec") for k in prof) and not _general(prof), prof
    got, prof, _ = _run_slots(_lib, DEC, streams, [len(w) for w in want])
    assert got == want
    assert all(prof.get(k) == 1 for k in names + (RUNE_PLAN, MID_PLAN)) and not _general(prof), prof
    # a malformed member among them: the single call's code and words
    bad = streams[2][:streams[2].index(b"\\\n")]
    with pytest.raises(_lib.RsnError) as single:
        huffman.Decompress(bad)
    mixed = streams[:9] + [bad] + streams[9:]
    with pytest.raises(_lib.RsnError) as batch:
        huffman.DecompressBatch(mixed)
    assert batch.value.code == single.value.code == E_FORMAT and str(batch.value) == str(single.value).replace(": ", ": member 9: ", 1)


# ---------------------------------------------------------------- 7: contracts
def test_capacity_and_fences(mods, oracle):
    _lib, huffman, _ = mods
    datas = [_text(85000 + k, 16385 + 997 * k) + b"!" * (k % 16) for k in range(huffman.RUNE_MID_DEC_GROUP_MIN + 3)]
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


def test_hostile_neighbours(mods, oracle):
    """the header ends in E2 82: what lies behind the stream would complete a euro sign, were it not behind the separator; the members end
    on a payload byte, and what follows would add code bits"""
    _lib, huffman, _ = mods
    streams = []
    for v in range(huffman.RUNE_MID_DEC_GROUP_MIN):
        lossy = {"a": 9000 + v, FFFD: 3000, "b": 2000}
        streams.append(_build([(9000 + v, "a", None), (2000, "b", None), (3000, FFFD, b"\xe2\x82")], _spread(lossy, v)))
    want = [_dec(oracle, s) for s in streams]
    assert all(len(w) == 20000 + v and w.count(FFFD.encode()) == 3000 for v, w in enumerate(want))
    got, prof, _ = _run_slots(_lib, DEC, streams, [len(w) for w in want], behind=lambda i: b"\xac\xff\x00\x55")
    assert got == want
    assert prof == _taken_dev(streams), prof


# ---------------------------------------------------------------- 8: closure with the library's own encoder
def test_round_trip_through_the_library(mods, oracle):
    _lib, huffman, _ = mods
    datas = [_text(86000 + k, 16385 + 2900 * k) for k in range(huffman.RUNE_MID_DEC_GROUP_MIN + 1)] + [_text(86100, 65536)]
    comp, prof = _prof(_lib, lambda: huffman.CompressBatch(datas))[:2]
    assert comp == [_enc(oracle, d) for d in datas]
    assert prof.get("huff_batch_rune_mid_enc") == 1, prof
    back, prof = _prof(_lib, lambda: huffman.DecompressBatch(comp))[:2]
    assert back == datas
    assert prof == {MID: 1}, prof


# ---------------------------------------------------------------- 9: through the layers
def test_layered_forms(mods, oracle):
    import torch
    _lib, huffman, layers = mods
    names = [LZ, HU]
    datas = [_text(70000 + k, 40 << 10) for k in range(huffman.RUNE_MID_DEC_GROUP_MIN + 2)]   # test_gpu_huffman_rune_mid.py::test_layered_forms' inputs
    streams = [oracle.huffman_compress(oracle.lzss_compress(d, 4096)) for d in datas]
    want = [oracle.lzss_decompress(_dec(oracle, s)) for s in streams]
    got, prof = _prof(_lib, lambda: layers.DecompressBatch(streams, names))[:2]
    assert got == want
    assert prof.get(MID) == 1 and not _general(prof), prof
    pack = Pack(streams, lambda i: b"\xac")
    srcs = [pack.t[o:o + n] for o, n in zip(pack.offs, pack.lens)]
    got, prof = _prof(_lib, lambda: [bytes(t.cpu().numpy()) for t in layers.decompress_tensors(srcs, names)])[:2]
    assert got == want
    assert prof.get(MID) == 1 and not _general(prof), prof
    rows, prof = _prof(_lib, lambda: layers.RoundTripBatch(datas, names, hists=False))[:2]
    assert prof.get(MID) == 1 and not _general(prof), prof
    for d, s, r in zip(datas, streams, rows):
        rt, _ = layers.RoundTrip(d, names)
        assert (r.original_n, r.compressed_n, r.decompressed_n, r.first_difference, r.lossless) == \
               (rt.original_n, rt.compressed_n, rt.decompressed_n, rt.first_difference, bool(rt.lossless)), d[:24]
        assert (r.original_n, r.compressed_n, r.decompressed_n, r.lossless) == (len(d), len(s), len(d), True), d[:24]
    torch.cuda.synchronize()
