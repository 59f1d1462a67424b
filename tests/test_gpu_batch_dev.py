"""GPU: the batch calls on device buffers (include/rsn.h: rsn_*_batch_dev).  Expected bytes come from the CPU oracle (LZSS)
and from tests/arith_model.py (arithmetic), never from the library; the single *_dev call is held against the same bytes.  The
instruments: members packed back to back in ONE allocation with hostile bytes between them, outputs between the fences of
tests/test_gpu_dev_fences.py with out_cap exactly the result size, the library's launch profile and its count of copied bytes."""
import ctypes

import pytest

import arith_model as M
from test_gpu_arith import cases
from test_gpu_dev_fences import RESIDUES, fenced
from test_gpu_lzss_mid import _text

pytestmark = pytest.mark.gpu

OK, E_ARG, E_FORMAT, E_CAP = 0, -1, -3, -7
GROUP_MEMBERS, GROUP_BYTES = 4096, 16 << 20            # codecs.h: SMALL_GROUP_MAX, SMALL_GROUP_BYTES
AR_GROUP_MAX = 32768                                    # arith.hip
TABLE_UP, TABLE_DOWN = 64, 4                            # group_dev.hip: a member's two table entries go up, its answer comes down
SINGLE_WORDS = 4096                                     # what one single call may copy of its own (flags, counts, a descriptor): far below any member here
AR_UP = 48 + 16                                         # arith.hip: a member's descriptor and destination go up; a summary of 16 bytes comes down per look


def _ru16(x):
    return (x + 15) // 16 * 16


@pytest.fixture(scope="module")
def mods():
    from raisin_amd import _lib, arithmetic, lz
    _lib.check(_lib.lib().rsn_device_set(0))
    return _lib, lz, arithmetic


class Pack:
    """`datas` back to back in ONE allocation, member i at a 16-byte offset; what lies between a member's end and the next member's start,
    and behind the last, is behind(i) repeated (default: 0xA5) -- every second member gets a whole extra 16 bytes of it."""

    def __init__(self, datas, behind=None):
        import torch
        buf, self.offs = bytearray(), []
        for i, d in enumerate(datas):
            self.offs.append(len(buf))
            buf += d
            fill = _ru16(len(buf)) + (16 if i % 2 else 0) - len(buf)
            pat = behind(i) if behind else b"\xa5"
            buf += (pat * (fill // len(pat) + 1))[:fill]
        buf += bytes([0xA5]) * 64
        self.lens = [len(d) for d in datas]
        self.t = torch.frombuffer(buf, dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        assert self.t.data_ptr() % 16 == 0

    def ptr(self, i):
        return self.t.data_ptr() + self.offs[i]


class Slots:
    """output buffers of `caps` bytes at 16-byte offsets of ONE allocation, 0xEE all over"""

    def __init__(self, caps):
        import torch
        self.offs, at = [], 0
        for c in caps:
            self.offs.append(at)
            at += _ru16(c) + 16
        self.caps = list(caps)
        self.t = torch.full((at + 16,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def ptr(self, i):
        return self.t.data_ptr() + self.offs[i]

    def host(self):
        import torch
        torch.cuda.synchronize()
        return self.t.cpu().numpy()


def _batch(_lib, name, members, *extra):
    """-> (rc, out_lens, message)"""
    fn = getattr(_lib.lib(), name)
    k = len(members)
    arr = (_lib.DevMember * max(k, 1))(*[_lib.DevMember(*m) for m in members])
    olens = (ctypes.c_size_t * max(k, 1))(*[77] * max(k, 1))
    rc = fn(k, arr, *extra, olens, None)
    return rc, [int(olens[i]) for i in range(k)], _lib.lib().rsn_last_error().decode("utf-8", "replace")


def _prof(_lib, fn):
    _lib.prof_enable(True)
    _lib.prof_reset()
    try:
        res = fn()
        return res, {k: v[0] for k, v in _lib.prof_get().items() if v[0]}, _lib.prof_copied()
    finally:
        _lib.prof_enable(False)


def _single(_lib, name, data, cap, *extra):
    """the single *_dev call on a buffer of its own -> bytes"""
    import torch
    src = torch.frombuffer(bytearray(data) + bytearray(64), dtype=torch.uint8).cuda()
    dst = torch.zeros(_ru16(cap) + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    got = _lib.call_dev(getattr(_lib.lib(), name), src.data_ptr(), len(data), dst.data_ptr(), cap, None, *extra)
    return bytes(dst[:got].cpu().numpy())


def _run_slots(_lib, name, datas, caps, *extra, behind=None):
    """one call over Pack(datas) into Slots(caps) -> (results, prof, copied); asserts RSN_OK and that the slots' surroundings are untouched"""
    pack, slots = Pack(datas, behind), Slots(caps)
    members = [(pack.ptr(i), len(d), slots.ptr(i), caps[i]) for i, d in enumerate(datas)]
    (rc, lens, msg), prof, copied = _prof(_lib, lambda: _batch(_lib, name, members, *extra))
    assert rc == OK, msg
    h = slots.host()
    res = []
    for i, c in enumerate(caps):
        o = slots.offs[i]
        assert lens[i] <= c
        res.append(bytes(h[o:o + lens[i]]))
        assert (h[o + lens[i]:o + _ru16(c) + 16] == 0xEE).all(), "member %d of %d bytes: a byte behind its result changed" % (i, lens[i])
    return res, prof, copied


LENGTHS = (0, 1, 13, 15, 16, 17, 25, 31, 32, 33, 1023, 1024, 1025, 4096, 65535, 65536, 65537)


@pytest.fixture(scope="module")
def mid_pad(mods):
    """enough members of 6 to 26 KiB to fill the mid classes both ways (their streams are above the small decoder's 2 KiB)"""
    lz = mods[1]
    return [_text(700 + i, 6000 + 311 * i) for i in range(lz.MID_GROUP_MIN)]


_ORACLE = {}


def _enc(oracle, d, w):
    """the oracle's stream, computed once per (input, window)"""
    key = (d, w)
    if key not in _ORACLE:
        _ORACLE[key] = oracle.lzss_compress(d, w)
    return _ORACLE[key]


# ---------------------------------------------------------------- LZSS
@pytest.mark.parametrize("window", (4096, 50))
def test_lzss_lengths_and_slot_edges(mods, oracle, mid_pad, window):
    _lib, lz, _ = mods
    L = _lib.lib()
    datas = [_text(40 + n % 97, n) for n in LENGTHS] + mid_pad
    assert len(datas[-1]) <= lz.MID_IN_MAX
    want = [_enc(oracle, d, window) for d in datas]
    caps = [L.rsn_lzss_compress_bound(len(d)) for d in datas]
    got, prof, copied = _run_slots(_lib, "rsn_lzss_compress_batch_dev", datas, caps, window)
    grouped = sum(1 for d in datas if 0 < len(d) <= lz.MID_IN_MAX)
    singles = len(datas) - grouped
    assert singles == 2                                                   # the empty member and the one of 65537 bytes
    for d, w, g in zip(datas, want, got):
        assert g == w, (len(d), window)
    for d, w in zip(datas[:len(LENGTHS)], want):
        assert _single(_lib, "rsn_lzss_compress_dev", d, L.rsn_lzss_compress_bound(len(d)), window) == w, (len(d), window)
    assert prof.get("group_gather") == 2 and prof.get("group_scatter") == 2, prof
    assert prof.get("lzss_batch_enc") == 1 and prof.get("lzss_batch_mid_enc") == 1, prof
    assert set(prof) - {"group_gather", "group_scatter", "lzss_batch_enc", "lzss_batch_mid_enc"}, prof   # (the member of 65537 bytes: the single call's kernels)
    bound = grouped * (TABLE_UP + TABLE_DOWN) + 32 + singles * SINGLE_WORDS
    assert sum(copied) <= bound < sum(map(len, datas)) // 8, (copied, bound)
    # ... and back
    streams = want
    caps = [len(d) for d in datas]                                        # exactly the result sizes
    got, prof, copied = _run_slots(_lib, "rsn_lzss_decompress_batch_dev", streams, caps)
    for d, s, g in zip(datas, streams, got):
        assert g == d == oracle.lzss_decompress(s), (len(d), window)
    for d, s in zip(datas[:len(LENGTHS)], streams):
        if d:
            assert _single(_lib, "rsn_lzss_decompress_dev", s, len(d)) == d, len(d)
    assert prof.get("group_gather") == 2 and prof.get("group_scatter") == 2, prof
    assert prof.get("lzss_batch_dec") == 1 and prof.get("lzss_batch_mid_dec") == 1, prof
    grouped = sum(1 for s in streams if 0 < len(s) <= lz.MID_E_MAX)
    singles = len(streams) - grouped
    bound = grouped * (TABLE_UP + TABLE_DOWN) + 32 + singles * SINGLE_WORDS
    assert sum(copied) <= bound < sum(map(len, streams)) // 8, (copied, bound)


def test_lzss_hostile_neighbours(mods, oracle, mid_pad):
    """Back to back in one allocation.  An input ends in a copy of its own beginning and what lies behind it goes on with that beginning:
    a match that read on would be longer.  A stream is followed by tokens: a decoder that read on would produce more."""
    _lib, lz, _ = mods
    L = _lib.lib()
    datas, heads = [], []
    for n in (13, 17, 25, 33, 100, 1023, 1025, 4097, 65536 + 40):
        body = _text(900 + n, n + 64)
        k = max(1, min(n // 3, 40))
        body = body[:n - k]
        datas.append(body + body[:k])                                     # ends in a copy of its own first k bytes ...
        heads.append(body[k:k + 64])                                      # ... and what lies behind it goes on as the beginning does
    for d in mid_pad:
        datas.append(d)
        heads.append(d[:64])

    def behind(i):
        return heads[i]
    want = [_enc(oracle, d, 4096) for d in datas]
    got, _, _ = _run_slots(_lib, "rsn_lzss_compress_batch_dev", datas, [L.rsn_lzss_compress_bound(len(d)) for d in datas], 4096, behind=behind)
    assert got == want
    got, _, _ = _run_slots(_lib, "rsn_lzss_decompress_batch_dev", want, [len(d) for d in datas], behind=lambda i: b"<1,1><2,2>xy")
    assert got == datas


def _by_residue(cands, size):
    """members of `cands` whose size(member) covers every residue mod 16 of RESIDUES, one each, then the rest"""
    first, rest, seen = [], [], set()
    for c in cands:
        r = size(c) % 16
        if r in RESIDUES and r not in seen:
            seen.add(r)
            first.append(c)
        else:
            rest.append(c)
    assert seen == set(RESIDUES), seen
    return first, rest


@pytest.fixture(scope="module")
def fence_members(mods, oracle):
    """small and mid members whose streams AND whose lengths cover the residues 0, 1, 7, 8, 15 mod 16, a mid class's minimum of them, and one
    member for the single path"""
    lz = mods[1]
    small = [_text(1000 + i, 20 + 7 * i) for i in range(120)]
    mid = [_text(1200 + i, 3000 + 53 * i) for i in range(160)]
    out = []
    for cands, total in ((small, 12), (mid, lz.MID_GROUP_MIN + 4)):
        a, rest = _by_residue(cands, lambda d: len(_enc(oracle, d, 4096)))
        b, rest = _by_residue(rest, len)
        out += a + b + rest[:total - len(a) - len(b)]
    return out + [_text(1400, lz.MID_IN_MAX + 4097)]


def _fenced_call(_lib, name, datas, caps, *extra, null_out=()):
    """one call, every member's d_out a fenced buffer of exactly caps[i] bytes (None at the indexes of null_out) -> (rc, lens, msg, outs)"""
    pack = Pack(datas)
    outs = [None if i in null_out else fenced(c) for i, c in enumerate(caps)]
    members = [(pack.ptr(i), len(d), outs[i][1] if outs[i] else None, caps[i] if outs[i] else 0) for i, d in enumerate(datas)]
    rc, lens, msg = _batch(_lib, name, members, *extra)
    for i, o in enumerate(outs):
        if o:
            o[2]("member %d's output" % i)
    return rc, lens, msg, outs


def _out_bytes(o, k):
    return bytes(o[0][:k].cpu().numpy())


def test_lzss_fences_at_exact_capacity(mods, oracle, fence_members):
    _lib = mods[0]
    datas = fence_members
    want = [_enc(oracle, d, 4096) for d in datas]
    assert {len(w) % 16 for w in want} >= set(RESIDUES) and {len(d) % 16 for d in datas} >= set(RESIDUES)
    rc, lens, msg, outs = _fenced_call(_lib, "rsn_lzss_compress_batch_dev", datas, [len(w) for w in want], 4096)
    assert rc == OK, msg
    assert lens == [len(w) for w in want]
    assert [_out_bytes(o, k) for o, k in zip(outs, lens)] == want
    rc, lens, msg, outs = _fenced_call(_lib, "rsn_lzss_decompress_batch_dev", want, [len(d) for d in datas])
    assert rc == OK, msg
    assert [_out_bytes(o, k) for o, k in zip(outs, lens)] == datas


def test_lzss_capacity(mods, oracle, fence_members):
    _lib, lz, _ = mods
    datas = fence_members
    last = len(datas) - 1                                                 # the single path's member
    for name, extra, ins, want in (("rsn_lzss_compress_batch_dev", (4096,), datas, [_enc(oracle, d, 4096) for d in datas]),
                                   ("rsn_lzss_decompress_batch_dev", (), [_enc(oracle, d, 4096) for d in datas], datas)):
        tight = {3: "one byte short", 5: "null", 20: "one byte short", 21: "one byte short", last: "one byte short"}
        caps = [len(w) - 1 if i in tight else len(w) for i, w in enumerate(want)]
        rc, lens, msg, outs = _fenced_call(_lib, name, ins, caps, *extra, null_out=(5,))
        assert rc == E_CAP and msg.startswith("member 3: lzss: output needs %d bytes, buffer holds %d" % (len(want[3]), len(want[3]) - 1)), msg
        for i, w in enumerate(want):
            cap = 0 if i == 5 else caps[i]
            if i in tight:
                assert lens[i] > cap and lens[i] >= len(w), (i, lens[i], len(w))
            else:
                assert lens[i] == len(w) <= cap and _out_bytes(outs[i], lens[i]) == w, i
        caps2 = [lens[i] if i in tight else caps[i] for i in range(len(want))]
        rc, lens2, msg, outs = _fenced_call(_lib, name, ins, caps2, *extra)
        assert rc == OK, msg
        assert lens2 == [len(w) for w in want]
        assert [_out_bytes(o, k) for o, k in zip(outs, lens2)] == want


def test_lzss_group_cuts(mods, oracle):
    _lib, lz, _ = mods
    L = _lib.lib()
    # 4100 members of 13 bytes: more than a group's members
    few = [_text(1500 + i, 13) for i in range(4)]
    datas = [few[(i * 7 + i // 4096) % 4] for i in range(GROUP_MEMBERS + 4)]
    want = {d: _enc(oracle, d, 4096) for d in few}
    got, prof, _ = _run_slots(_lib, "rsn_lzss_compress_batch_dev", datas, [L.rsn_lzss_compress_bound(13)] * len(datas), 4096)
    assert got == [want[d] for d in datas]
    assert prof == {"group_gather": 2, "lzss_batch_enc": 2, "group_scatter": 2}, prof
    got, prof, _ = _run_slots(_lib, "rsn_lzss_decompress_batch_dev", got, [13] * len(datas))
    assert got == datas
    assert prof.get("lzss_batch_dec", 0) >= 2 and prof["group_gather"] == prof["lzss_batch_dec"] == prof["group_scatter"] and len(prof) == 3, prof
    # 130 members of 64 KiB: more than a group's bytes
    three = [_text(1600 + i, lz.MID_IN_MAX) for i in range(3)]
    need = TABLE_UP + lz.MID_IN_MAX + 32 + min(2 * lz.MID_IN_MAX, lz.MID_E_MAX) + 16 + 16
    per_group = GROUP_BYTES // need
    assert per_group < 130 <= 2 * per_group
    datas = [three[(i + i // per_group) % 3] for i in range(130)]
    want = {d: _enc(oracle, d, 4096) for d in three}
    got, prof, _ = _run_slots(_lib, "rsn_lzss_compress_batch_dev", datas, [L.rsn_lzss_compress_bound(lz.MID_IN_MAX)] * 130, 4096)
    assert got == [want[d] for d in datas]
    assert prof == {"group_gather": 2, "lzss_batch_mid_enc": 2, "group_scatter": 2}, prof
    got, prof, _ = _run_slots(_lib, "rsn_lzss_decompress_batch_dev", got, [lz.MID_IN_MAX] * 130)
    assert got == datas
    assert prof.get("lzss_batch_mid_dec", 0) >= 1 and "group_gather" in prof, prof


def test_lzss_handed_back(mods, oracle, mid_pad):
    _lib, lz, _ = mods
    L = _lib.lib()
    # every byte a 5C escapes to twice MID_IN_MAX: the mid encoder hands it back, the single call's codec writes the same bytes
    datas = mid_pad[:10] + [b"\\" * lz.MID_IN_MAX] + mid_pad[10:]
    want = [_enc(oracle, d, 4096) for d in datas]
    got, prof, _ = _run_slots(_lib, "rsn_lzss_compress_batch_dev", datas, [L.rsn_lzss_compress_bound(len(d)) for d in datas], 4096)
    assert got == want
    assert got[10] == _single(_lib, "rsn_lzss_compress_dev", datas[10], L.rsn_lzss_compress_bound(len(datas[10])), 4096)
    assert prof.get("lzss_batch_mid_enc") == 1 and len(prof) > 3, prof
    # a token that points in front of the data, among good streams: the single call's code and words, nothing handed out
    bad = want[0][:3000] + b"<60000,3>" + want[0][3000:3100]
    with pytest.raises(oracle.OracleError):
        oracle.lzss_decompress(bad)
    with pytest.raises(_lib.RsnError) as single:
        _single(_lib, "rsn_lzss_decompress_dev", bad, 1 << 17)
    streams = want[:7] + [bad] + want[7:]
    pack, slots = Pack(streams), Slots([1 << 17] * len(streams))
    rc, lens, msg = _batch(_lib, "rsn_lzss_decompress_batch_dev", [(pack.ptr(i), len(s), slots.ptr(i), 1 << 17) for i, s in enumerate(streams)])
    assert rc == single.value.code == E_FORMAT
    assert "librsn error %d: %s" % (rc, msg) == str(single.value).replace(": ", ": member 7: ", 1), (msg, str(single.value))
    assert lens == [0] * len(streams)


# ---------------------------------------------------------------- arithmetic
def _arith_names(A):
    S = A.SLICE_SYMBOLS
    return ["len%d" % n for n in (0, 1, 13, 64, 65, 16126, 16127, S, S + 1, 2 * S + 7)]


def test_arithmetic_lengths_both_ways(mods):
    _lib, _, A = mods
    c = cases()
    names = _arith_names(A)
    order = [names[k] for k in (9, 1, 7, 0, 5, 2, 8, 3, 6, 4)]           # short members sit finished through the long ones' later slices
    datas, encs = [c[n][0] for n in order], [c[n][1] for n in order]
    assert [len(d) for d in datas] == [int(n[3:]) for n in order]
    rc, lens, msg, outs = _fenced_call(_lib, "rsn_arithmetic_compress_batch_dev", datas, [len(e) for e in encs])
    assert rc == OK, msg
    assert [_out_bytes(o, k) for o, k in zip(outs, lens)] == encs
    for d, e in zip(datas[:4], encs):
        assert _single(_lib, "rsn_arithmetic_compress_dev", d, len(e)) == e
    # ... and back: the empty input's stream, 01 ff, does not decode (as in the reference and the single call) -- the others
    keep = [i for i, d in enumerate(datas) if d]
    rc, lens, msg, outs = _fenced_call(_lib, "rsn_arithmetic_decompress_batch_dev", [encs[i] for i in keep], [len(datas[i]) for i in keep])
    assert rc == OK, msg
    assert [_out_bytes(o, k) for o, k in zip(outs, lens)] == [datas[i] for i in keep]
    rc, lens, msg, _ = _fenced_call(_lib, "rsn_arithmetic_decompress_batch_dev", encs, [max(len(d), 16) for d in datas])
    with pytest.raises(_lib.RsnError) as single:
        _single(_lib, "rsn_arithmetic_decompress_dev", b"\x01\xff", 64)
    assert rc == single.value.code == E_FORMAT and lens == [0] * len(encs)
    assert "librsn error %d: %s" % (rc, msg) == str(single.value).replace(": ", ": member 3: ", 1), (msg, str(single.value))


def test_arithmetic_more_members_than_a_group(mods):
    _lib, _, A = mods
    L = _lib.lib()
    few = [b"a", b"\xff", b"ab", b"\x00\x00", b"abc", b"zzz", b"e\n "]
    want = {d: M.encode(d) for d in few}
    n = AR_GROUP_MAX + 2
    datas = [few[(i * 5 + i // AR_GROUP_MAX) % len(few)] for i in range(n)]
    (got, prof, copied) = _run_slots(_lib, "rsn_arithmetic_compress_batch_dev", datas, [L.rsn_arithmetic_compress_bound(len(d)) for d in datas])
    assert got == [want[d] for d in datas]
    assert prof.get("k_arith_enc") == 2 and prof.get("k_arith_pack_own") == 2 and "k_arith_pack" not in prof and "k_arith_dec" not in prof, prof
    assert sum(copied) <= n * (AR_UP + 16) + 2 * 64, copied
    (back, prof, copied) = _run_slots(_lib, "rsn_arithmetic_decompress_batch_dev", got, [len(d) for d in datas])
    assert back == datas
    assert prof == {"k_arith_dec": 2}, prof
    assert sum(copied) <= n * (48 + 16) + 2 * 64, copied


def test_arithmetic_decode_capacity_and_a_stream_without_an_end(mods):
    _lib, _, A = mods
    c = cases()
    names = ["len16127", "hello", "len%d" % (A.SLICE_SYMBOLS + 1), "abc", "len13"]
    datas, encs = [c[n][0] for n in names], [c[n][1] for n in names]
    caps = [len(d) for d in datas]
    caps[0], caps[2] = len(datas[0]) // 2, len(datas[2]) // 2
    rc, lens, msg, outs = _fenced_call(_lib, "rsn_arithmetic_decompress_batch_dev", encs, caps)
    assert rc == E_CAP and msg == "member 0: arithmetic: output needs %d bytes, buffer holds %d" % (len(datas[0]), caps[0]), msg
    assert lens == [len(d) for d in datas]                                # the exact need, the members that fit and those that do not
    for i in (1, 3, 4):
        assert _out_bytes(outs[i], lens[i]) == datas[i]
    rc, lens, msg, outs = _fenced_call(_lib, "rsn_arithmetic_decompress_batch_dev", encs, lens)
    assert rc == OK and [_out_bytes(o, k) for o, k in zip(outs, lens)] == datas, msg
    # the encoder's size query: a null d_out among members that fit
    rc, lens, msg, outs = _fenced_call(_lib, "rsn_arithmetic_compress_batch_dev", datas, [len(e) for e in encs], null_out=(1,))
    assert rc == E_CAP and msg.startswith("member 1: arithmetic: output needs %d bytes, buffer holds 0" % len(encs[1])), msg
    assert lens == [len(e) for e in encs] and [_out_bytes(outs[i], lens[i]) for i in (0, 2, 3, 4)] == [encs[i] for i in (0, 2, 3, 4)]
    # no end symbol within the tail rule's bits: RSN_ERR_FORMAT, the member named
    enc = M.encode(b"a" * 20000)
    bad = enc[:-40] + bytes(4000)
    with pytest.raises(M.FormatError):
        M.decode(bad)
    with pytest.raises(_lib.RsnError) as single:
        _single(_lib, "rsn_arithmetic_decompress_dev", bad, 1 << 16)
    streams = encs[:2] + [bad] + encs[2:]
    rc, lens, msg, _ = _fenced_call(_lib, "rsn_arithmetic_decompress_batch_dev", streams, [1 << 17] * len(streams))
    assert rc == single.value.code == E_FORMAT and lens == [0] * len(streams)
    assert "librsn error %d: %s" % (rc, msg) == str(single.value).replace(": ", ": member 2: ", 1), (msg, str(single.value))


# ---------------------------------------------------------------- Python, independence
def test_tensor_lists_round_trip(mods, oracle):
    import torch
    _lib, lz, A = mods
    datas = [_text(1700 + i, n) for i, n in enumerate((0, 1, 25, 1000, 5000, 70000, 33, 16))]
    pack = Pack(datas)
    srcs = [pack.t[o:o + n] for o, n in zip(pack.offs, pack.lens)]       # slices of one allocation
    comp = lz.compress_tensors(srcs, 4096)
    assert [bytes(t.cpu().numpy()) for t in comp] == [_enc(oracle, d, 4096) for d in datas]
    back = lz.decompress_tensors(comp)
    assert [bytes(t.cpu().numpy()) for t in back] == datas
    some = [d for d in datas if d]
    pack = Pack(some)
    srcs = [pack.t[o:o + n] for o, n in zip(pack.offs, pack.lens)]
    comp = A.compress_tensors(srcs)
    assert [bytes(t.cpu().numpy()) for t in comp] == [M.encode(d) for d in some]
    assert [bytes(t.cpu().numpy()) for t in A.decompress_tensors(comp)] == some
    # a guess that is too small: the members that did not fit are run once more, the others are kept
    tight = [torch.empty(max(len(d) // (2 if i % 2 else 1), 16), dtype=torch.uint8, device="cuda") for i, d in enumerate(some)]
    assert [bytes(t.cpu().numpy()) for t in A.decompress_tensors(comp, outs=tight)] == some
    assert lz.compress_tensors([]) == [] and A.decompress_tensors([]) == []


def test_calls_do_not_depend_on_what_earlier_calls_left(mods, oracle, mid_pad):
    _lib, lz, A = mods
    L = _lib.lib()
    datas = [_text(1800 + i, n) for i, n in enumerate((13, 700, 1024, 33))] + mid_pad
    caps = [L.rsn_lzss_compress_bound(len(d)) for d in datas]
    want = [_enc(oracle, d, 4096) for d in datas]
    first, _, _ = _run_slots(_lib, "rsn_lzss_compress_batch_dev", datas, caps, 4096)
    again, _, _ = _run_slots(_lib, "rsn_lzss_compress_batch_dev", datas[::-1], caps[::-1], 4096)   # other members in the same staging
    assert lz.CompressAsyncBatch([_text(1900 + i, 900 + 500 * i) for i in range(70)], 4096)       # a host-buffer batch on the same thread
    assert A.CompressBatch([b"abc" * 50, b"xyz" * 5000])
    third, _, _ = _run_slots(_lib, "rsn_lzss_compress_batch_dev", datas, caps, 4096)
    assert first == again[::-1] == third == want
    back, _, _ = _run_slots(_lib, "rsn_lzss_decompress_batch_dev", want, [len(d) for d in datas])
    back2, _, _ = _run_slots(_lib, "rsn_lzss_decompress_batch_dev", want, [len(d) for d in datas])
    assert back == back2 == datas
    small = [b"hello", b"abc" * 50, b"\xff" * 300, b"e" * 70000]
    encs = [M.encode(d) for d in small]
    a1, _, _ = _run_slots(_lib, "rsn_arithmetic_compress_batch_dev", small, [L.rsn_arithmetic_compress_bound(len(d)) for d in small])
    assert A.DecompressBatch(encs) == small
    a2, _, _ = _run_slots(_lib, "rsn_arithmetic_compress_batch_dev", small, [L.rsn_arithmetic_compress_bound(len(d)) for d in small])
    assert a1 == a2 == encs
    d1, _, _ = _run_slots(_lib, "rsn_arithmetic_decompress_batch_dev", encs, [len(d) for d in small])
    assert d1 == small
