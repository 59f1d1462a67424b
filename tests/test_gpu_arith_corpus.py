"""GPU: the arithmetic kernels (raisin_amd/csrc/arith.hip) on the corpus of tests/arith_cases.py -- all 256 symbols and every
(lane, register) position of the table, noise that expands, pending runs at every place of a word, every end of a stream -- through every
route, byte for byte against tests/arith_model.py; then what the corpus cannot hold: streams behind leading zero bytes (the decoder's
scan and its resume), host batches whose rounds resume at odd budgets, the reason of every refusal, and the size limits."""
import ctypes
import os
import random
import re

import pytest

import arith_cases as C
import arith_model as M
from test_gpu_arith import _dev, _fenced
from test_gpu_batch_dev import Pack, Slots, _batch, _fenced_call, _out_bytes, _prof, _single

pytestmark = pytest.mark.gpu

OK, E_FORMAT, E_LIMIT, E_CAP = 0, -3, -6, -7
_SRC = open(os.path.join(C.ROOT, "raisin_amd", "csrc", "arith.hip")).read()
AR_SCAN_CHUNKS = int(re.search(r"AR_SCAN_CHUNKS\s*=\s*(\d+)", _SRC).group(1))
AR_GROUP_MAX = int(re.search(r"AR_GROUP_MAX\s*=\s*(\d+)", _SRC).group(1))
AR_ARENA_BYTES = int(re.search(r"AR_ARENA_BYTES\s*=\s*\(size_t\)(\d+)\s*<<\s*20", _SRC).group(1)) << 20
MAX_BYTES = 64 << 20                                                       # include/rsn.h RSN_ARITH_MAX_BYTES
REASONS = ("no 1 bit", "fewer than 16 bits", "no end symbol within", "a code value outside the table")


@pytest.fixture(scope="module")
def mods():
    from raisin_amd import _lib, arithmetic
    _lib.check(_lib.lib().rsn_device_set(0))
    assert arithmetic.MAX_BYTES == MAX_BYTES and arithmetic.SLICE_SYMBOLS == C.SLICE_SYMBOLS
    return _lib, arithmetic


def _reason(text):
    found = [r for r in REASONS if r in text]
    assert len(found) == 1, text
    return found[0]


_VERDICTS = {}


def verdict(stream):
    """the model's: (bytes, None) or (None, the reason), once per stream"""
    if stream not in _VERDICTS:
        try:
            _VERDICTS[stream] = (M.decode(stream), None)
        except M.FormatError as e:
            _VERDICTS[stream] = (None, _reason(str(e)))
    return _VERDICTS[stream]


def host_verdict(mods, stream):
    _lib, A = mods
    try:
        return A.Decompress(stream), None
    except _lib.RsnError as e:
        assert e.code == E_FORMAT, e
        return None, _reason(str(e))


def dev_verdict(mods, stream):
    _lib, A = mods
    want = verdict(stream)[0]
    try:
        return _single(_lib, "rsn_arithmetic_decompress_dev", stream, max(len(want or b""), 64)), None
    except _lib.RsnError as e:
        assert e.code == E_FORMAT, e
        return None, _reason(str(e))


# ---------------------------------------------------------------- the corpus, every route
def test_corpus_single_host_calls(mods):
    _, A = mods
    for name, c in C.CASES.items():
        assert A.Compress(c.data) == c.enc, name
        assert A.Decompress(c.enc) == c.data, name


def test_corpus_in_one_host_batch(mods):
    _, A = mods
    order = list(C.NAMES)
    random.Random(0xC0DE).shuffle(order)
    assert order != C.NAMES
    assert A.CompressBatch([C.CASES[n].data for n in order]) == [C.CASES[n].enc for n in order]
    assert A.DecompressBatch([C.CASES[n].enc for n in order]) == [C.CASES[n].data for n in order]


def test_corpus_in_one_device_batch_between_fences(mods):
    _lib, _ = mods
    datas, encs = [c.data for c in C.CASES.values()], [c.enc for c in C.CASES.values()]
    rc, lens, msg, outs = _fenced_call(_lib, "rsn_arithmetic_compress_batch_dev", datas, [len(e) for e in encs])
    assert rc == OK, msg
    assert lens == [len(e) for e in encs]
    for n, o, e in zip(C.NAMES, outs, encs):
        assert _out_bytes(o, len(e)) == e, n
    del outs
    rc, lens, msg, outs = _fenced_call(_lib, "rsn_arithmetic_decompress_batch_dev", encs, [len(d) for d in datas])
    assert rc == OK, msg
    assert lens == [len(d) for d in datas]
    for n, o, d in zip(C.NAMES, outs, datas):
        assert _out_bytes(o, len(d)) == d, n


def test_corpus_as_tensor_lists(mods):
    _, A = mods
    datas = [c.data for c in C.CASES.values()]
    pack = Pack(datas)
    comp = A.compress_tensors([pack.t[o:o + n] for o, n in zip(pack.offs, pack.lens)])
    for n, t in zip(C.NAMES, comp):
        assert bytes(t.cpu().numpy()) == C.CASES[n].enc, n
    back = A.decompress_tensors(comp)
    for n, t in zip(C.NAMES, back):
        assert bytes(t.cpu().numpy()) == C.CASES[n].data, n


@pytest.mark.parametrize("name", C.dev_subset())
@pytest.mark.parametrize("enc", [True, False], ids=["compress", "decompress"])
def test_corpus_single_dev_calls_between_fences(mods, name, enc):
    L = mods[0].lib()
    c = C.CASES[name]
    src, want = (c.data, c.enc) if enc else (c.enc, c.data)
    fn = L.rsn_arithmetic_compress_dev if enc else L.rsn_arithmetic_decompress_dev
    d_in, check_in, _, keep_in = _fenced(len(src), src)
    rc, need = _dev(fn, d_in, len(src), None, 0)                          # the size query
    assert rc == E_CAP and need == len(want)
    d_out, check, read, keep_out = _fenced(need)
    rc, got = _dev(fn, d_in, len(src), d_out, need)                       # exact capacity
    assert rc == OK and got == len(want) and read(got) == want
    check()
    d_out, check, read, keep_out = _fenced(need - 1)
    rc, got = _dev(fn, d_in, len(src), d_out, need - 1)                   # one byte less
    assert rc == E_CAP and got == need
    check()
    check_in()


# ---------------------------------------------------------------- leading zero bytes: the scan for the first 1 bit
def _zero_counts():
    L = AR_SCAN_CHUNKS * 256
    return (1, 2, 3, 4, 5, 252, 255, 256, 257, 2047, 2048, L - 1, L, L + 1, 2 * L + 5)


def _behind_zeros():
    pend = C.first(lambda n, c: n.startswith("pending"), "a pending run")
    return [(n, z, bytes(z) + C.CASES[n].enc) for n in ("hello", "noise1000", pend) for z in _zero_counts()]


def _refused_behind_zeros():
    L = AR_SCAN_CHUNKS * 256
    return [(bytes(2 * L + 5), REASONS[0]), (bytes(L) + b"\x20\xff", REASONS[1]), (bytes(L + 3) + b"\x01", REASONS[1])]


def test_a_stream_behind_zero_bytes_decodes_as_the_stream(mods):
    _lib, A = mods
    streams = _behind_zeros()
    for n, z, s in streams:
        assert verdict(s) == (C.CASES[n].data, None), (n, z)             # as the model says
    for n, z, s in streams:
        assert A.Decompress(s) == C.CASES[n].data, (n, z)
    assert A.DecompressBatch([s for _, _, s in streams]) == [C.CASES[n].data for n, _, _ in streams]
    for n, z, s in streams:
        assert _single(_lib, "rsn_arithmetic_decompress_dev", s, len(C.CASES[n].data)) == C.CASES[n].data, (n, z)
    # ... and all of them in one batch on device buffers: members that are still scanning next to members that decode
    rc, lens, msg, outs = _fenced_call(_lib, "rsn_arithmetic_decompress_batch_dev", [s for _, _, s in streams], [len(C.CASES[n].data) for n, _, _ in streams])
    assert rc == OK, msg
    assert [_out_bytes(o, k) for o, k in zip(outs, lens)] == [C.CASES[n].data for n, _, _ in streams]


def test_zero_bytes_without_a_start_behind_them_are_refused(mods):
    L = AR_SCAN_CHUNKS * 256
    for s, why in _refused_behind_zeros():
        assert verdict(s) == (None, why)
        assert host_verdict(mods, s) == (None, why) and dev_verdict(mods, s) == (None, why), (len(s), why)
    s = bytes(L) + b"\x40\x00"                                            # 14 bits behind the 1: the decoder's own verdict
    assert verdict(s)[1] != REASONS[1]
    assert host_verdict(mods, s) == verdict(s) == dev_verdict(mods, s)


# ---------------------------------------------------------------- host batches whose rounds resume at odd budgets
def _many(n):
    """n members: 12 of noise (300 to 3000 bytes) at seeded places, the others cyclically from 16 inputs of 1 to 13 bytes"""
    rng = random.Random(0x0DD + n)
    few = [C.noise(rng.randrange(1, 14), 0x5EED00 + i) for i in range(16)]
    assert len(set(few)) == 16
    big = {p: C.noise(rng.randrange(300, 3001), 0xB16000 + p) for p in rng.sample(range(n), 12)}
    return [big.get(i) or few[i % 16] for i in range(n)]


@pytest.mark.parametrize("n", [20000, AR_GROUP_MAX + 3], ids=["budget384", "budget256-two-groups"])
def test_host_batch_resumes_at_odd_budgets(mods, n):
    _lib, A = mods
    first_group = min(n, AR_GROUP_MAX)
    assert AR_ARENA_BYTES == 8 << 20 and AR_ARENA_BYTES // first_group // 64 * 64 == (384 if n == 20000 else 256)
    datas = _many(n)
    want = {d: M.encode(d) for d in set(datas)}
    assert len(want) == 28
    encs, prof, _ = _prof(_lib, lambda: A.CompressBatch(datas))
    assert encs == [want[d] for d in datas]
    if n > AR_GROUP_MAX:                                                  # (the host form runs on the calling thread: its launches are in the profile)
        assert prof.get("k_arith_enc") == 2 and prof.get("k_arith_pack") == 2, prof
    assert A.DecompressBatch(encs) == datas


# ---------------------------------------------------------------- the reason of every refusal
CUT = ("noise4097", "reg3lane32", "all256x2")
PARTS = len(CUT) + 16


def _judged_streams(part):
    """Part `part` of the streams whose verdict is compared (the model needs seconds for those the tail rule ends, so each part judges
    its own).  Parts 0 to 2: a corpus stream cut at each of its last 8 bytes or followed by 600 zero bytes; part 0 has in front of them
    a good stream, every refused stream behind zero bytes and a stream that decodes behind more zero bytes than a launch scans, so that
    a refused member has a complete one before it and a scanning one behind it.  The other parts: 200 seeded random streams of 1 to 200
    bytes, dealt out."""
    if part >= len(CUT):
        rng = random.Random(0x2EA5)
        rand = [bytes(rng.randrange(256) for _ in range(rng.randrange(1, 201))) for _ in range(200)]
        return rand[part - len(CUT)::PARTS - len(CUT)]
    enc, hello = C.CASES[CUT[part]].enc, C.CASES["hello"].enc
    front = [hello] + [s for s, _ in _refused_behind_zeros()] + [bytes(AR_SCAN_CHUNKS * 256 + 1) + hello] if part == 0 else []
    return front + [enc[:len(enc) - k] for k in range(1, 9)] + [enc + bytes(600)]


@pytest.mark.parametrize("part", range(PARTS))
def test_refusals_carry_the_model_s_reason(mods, part):
    streams = _judged_streams(part)
    want = [verdict(s) for s in streams]
    if part == 0:                                                         # (the table's reason may be unreachable: it is not required)
        assert {w[1] for w in want} >= set(REASONS[:3]) and any(w[1] is None for w in want)
    for s, w in zip(streams, want):
        assert host_verdict(mods, s) == w, (len(s), s[:16].hex())
        assert dev_verdict(mods, s) == w, (len(s), s[:16].hex())


@pytest.mark.parametrize("part", range(PARTS))
def test_refusals_member_by_member_in_a_device_batch(mods, part):
    """the call over streams[i:] names its lowest failing member and leaves those in front of it complete; then on from behind that one"""
    _lib, _ = mods
    streams = _judged_streams(part)
    want = [verdict(s) for s in streams]
    if part == 0:                                                         # every reason goes through the device batch, the scan's resume too
        assert {w[1] for w in want} >= set(REASONS[:3]) and want[0][0] and want[1] == (None, REASONS[0]) and want[4][0]
    caps = [max(len(w[0] or b""), 64) for w in want]
    pack, slots = Pack(streams), Slots(caps)
    members = [(pack.ptr(i), len(s), slots.ptr(i), caps[i]) for i, s in enumerate(streams)]
    i, refused = 0, 0
    while i < len(streams):
        bad = next((k for k in range(i, len(streams)) if want[k][0] is None), len(streams))
        slots.t.fill_(0xEE)
        rc, lens, msg = _batch(_lib, "rsn_arithmetic_decompress_batch_dev", members[i:])
        h = slots.host()
        for k in range(i, bad):
            o = slots.offs[k]
            assert bytes(h[o:o + len(want[k][0])]) == want[k][0], k
        if bad == len(streams):
            assert rc == OK and lens == [len(w[0]) for w in want[i:]], msg
        else:
            assert rc == E_FORMAT and msg.startswith("member %d: arithmetic: " % (bad - i)) and _reason(msg) == want[bad][1], (bad, msg)
            assert lens == [0] * (len(streams) - i)
            refused += 1
        i = bad + 1
    assert refused == sum(1 for w in want if w[0] is None)


# ---------------------------------------------------------------- the size limits
def test_limits_of_the_single_calls(mods):
    import torch
    _lib, A = mods
    L = _lib.lib()
    bound = L.rsn_arithmetic_compress_bound(MAX_BYTES)
    n = ctypes.c_size_t(0)
    for fn, host, size in ((L.rsn_arithmetic_compress_dev, A.Compress, MAX_BYTES + 1), (L.rsn_arithmetic_decompress_dev, A.Decompress, bound + 1)):
        data = bytes(size)
        with pytest.raises(_lib.RsnError) as e:
            _prof(_lib, lambda: host(data))
        assert e.value.code == E_LIMIT and "arithmetic" in str(e.value)
        assert not any(v[0] for v in _lib.prof_get().values())            # nothing was launched
        src = torch.zeros(size + 15, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc, prof, _ = _prof(_lib, lambda: fn(src.data_ptr(), size, dst.data_ptr(), 4096, ctypes.byref(n), None))
        assert rc == E_LIMIT and prof == {}, (rc, prof)
        del src, data


def test_limits_in_the_batch_calls(mods):
    import torch
    _lib, A = mods
    L = _lib.lib()
    hello = C.CASES["hello"]
    for enc, size in ((True, MAX_BYTES + 1), (False, L.rsn_arithmetic_compress_bound(MAX_BYTES) + 1)):
        small, res = (hello.data, hello.enc) if enc else (hello.enc, hello.data)
        bufs = [small, bytes(size), small]
        ins = (ctypes.c_char_p * 3)(*bufs)
        lens = (ctypes.c_size_t * 3)(*[len(b) for b in bufs])
        outs = (ctypes.POINTER(ctypes.c_uint8) * 3)()
        olens = (ctypes.c_size_t * 3)()
        fn = L.rsn_arithmetic_compress_batch if enc else L.rsn_arithmetic_decompress_batch
        assert fn(3, ins, lens, outs, olens) == E_LIMIT
        assert L.rsn_last_error().startswith(b"member 1: arithmetic: ")
        assert all(not outs[i] for i in range(3)) and all(olens[i] == 0 for i in range(3))
        # on device buffers: the member in front of the one above the limit is complete
        big = torch.zeros(size + 15, dtype=torch.uint8, device="cuda")
        pack, slots = Pack([small, small]), Slots([len(res), 64, len(res)])
        members = [(pack.ptr(0), len(small), slots.ptr(0), len(res)), (big.data_ptr(), size, slots.ptr(1), 64), (pack.ptr(1), len(small), slots.ptr(2), len(res))]
        rc, lens2, msg = _batch(_lib, "rsn_arithmetic_%s_batch_dev" % ("compress" if enc else "decompress"), members)
        assert rc == E_LIMIT and msg.startswith("member 1: arithmetic: "), msg
        h = slots.host()
        assert bytes(h[:len(res)]) == res
        del big
