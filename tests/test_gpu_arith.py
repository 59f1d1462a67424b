"""The arithmetic codec on the device, byte for byte against tests/arith_model.py: single, batch and device-buffer calls, the
streams a decoder must refuse, and the independence of calls that share a thread's scratch.  Every expected byte and every verdict
on a damaged stream comes from the model, computed once per session."""
import ctypes
import random
import threading

import pytest

import arith_model as M

pytestmark = pytest.mark.gpu

OK, E_ARG, E_FORMAT, E_CAP = 0, -1, -3, -7
FENCE = 4096


def _skewed(n, seed):
    rng = random.Random(seed)
    return bytes(rng.choice(b"eeeeeeeetttttaaaaoooiinnsshhrrdlu \n\x00\xff") for _ in range(n))


def _lengths():
    from raisin_amd import arithmetic
    S = arithmetic.SLICE_SYMBOLS
    return [0, 1, 2, 3, 13, 25, 63, 64, 65, 127, 128, 129, 16124, 16125, 16126, 16127, 16128, S - 1, S, S + 1, 2 * S + 7]


_CASES = {}


def cases():
    """name -> (input, the model's stream)"""
    if not _CASES:
        inputs = {"len%d" % n: _skewed(n, 0xA000 + n) for n in _lengths()}
        g = M.greedy_input(400)
        for k in (40, 100, 200, 400):
            inputs["greedy%d" % k] = g[:k]
        inputs["a100000"] = b"a" * 100000
        assert M.stats(inputs["a100000"])["end_pending"] > 0           # ends with pending bits that are dropped
        inputs["ff20000"] = b"\xff" * 20000
        inputs["zero20000"] = bytes(20000)
        inputs["hello"] = b"Hello world!\n"
        inputs["abc"] = b"abc" * 8 + b"\n"
        inputs["alphabet"] = (b"abcdefghijklmnopqrstuvwxyz" * 3847)[:100000]
        for name, data in inputs.items():
            _CASES[name] = (data, M.encode(data))
    return _CASES


def _names():
    return ["len%d" % n for n in _lengths()] + ["greedy40", "greedy100", "greedy200", "greedy400", "a100000", "ff20000", "zero20000",
                                               "hello", "abc", "alphabet"]


@pytest.fixture(scope="module")
def A():
    from raisin_amd import _lib, arithmetic
    _lib.check(_lib.lib().rsn_device_set(0))
    return arithmetic


def _verdict(stream):
    try:
        return M.decode(stream)
    except M.FormatError:
        return None


def _lib_verdict(A, stream):
    from raisin_amd import RsnError
    try:
        return A.Decompress(stream)
    except RsnError as e:
        assert e.code == E_FORMAT, e
        return None


@pytest.mark.parametrize("name", _names())
def test_single_calls_match_the_model(A, name):
    data, enc = cases()[name]
    assert A.Compress(data) == enc
    assert _lib_verdict(A, enc) == (data if data else None)           # 01 ff, the empty input's stream, does not decode (as in the reference)


def test_published_sizes(A):
    c = cases()
    assert [len(A.Compress(c[k][0])) for k in ("hello", "abc", "a100000", "alphabet")] == [14, 21, 477, 59191]
    assert A.Compress(b"a").hex() == "01619d" and A.Compress(b"") == b"\x01\xff"


def test_streams_without_a_start_are_refused(A):
    for s in (b"", b"\x01", b"\x01\xff", b"\x00\x00\x00", bytes(5000)):
        assert _verdict(s) is None and _lib_verdict(A, s) is None


def test_damaged_streams_get_the_model_s_verdict(A):
    rng = random.Random(0xBAD5)
    data, enc = cases()["len16127"]
    streams = [enc[:len(enc) - k] for k in range(1, 9)] + [enc + bytes(600)]
    streams += [bytes(rng.randrange(256) for _ in range(rng.randrange(1, 201))) for _ in range(64)]
    want = [_verdict(s) for s in streams]                             # (the model applies the same 4096-bit rule: each of these ends)
    assert any(w is None for w in want) and any(w is not None for w in want)
    for s, w in zip(streams, want):
        assert _lib_verdict(A, s) == w
    # ... and in one batch, member by member, when none of them fails
    good = [s for s, w in zip(streams, want) if w is not None]
    assert A.DecompressBatch(good) == [w for w in want if w is not None]


def test_tail_rule_on_a_frozen_table(A):
    """one dominant symbol in a frozen table, then zeros: the longest a hostile stream can keep a decoder busy per bit"""
    enc = M.encode(b"a" * 20000)
    bad = enc[:-40] + bytes(4000)
    assert _verdict(bad) is None and _lib_verdict(A, bad) is None


def test_batch_equals_the_single_calls(A):
    c = cases()
    datas = [c[n][0] for n in _names()] + [b"", b""]
    encs = [c[n][1] for n in _names()] + [b"\x01\xff", b"\x01\xff"]
    assert A.CompressBatch(datas) == encs
    ok = [(d, e) for d, e in zip(datas, encs) if d]
    assert A.DecompressBatch([e for _, e in ok]) == [d for d, _ in ok]
    same = c["len16127"][0]
    assert A.CompressBatch([same, same]) == [c["len16127"][1]] * 2
    assert A.DecompressBatch([c["len16127"][1]] * 2) == [same] * 2
    assert A.CompressBatch([]) == [] and A.DecompressBatch([]) == []


def test_batch_of_4096_small_files(A):
    data, enc = cases()["hello"]
    assert A.CompressBatch([data] * 4096) == [enc] * 4096
    assert A.DecompressBatch([enc] * 4096) == [data] * 4096


def test_batch_of_random_lengths(A):
    rng = random.Random(0x300)
    datas = [_skewed(rng.randrange(0, 2001), 0x3000 + i) for i in range(300)]
    encs = A.CompressBatch(datas)
    for i in (0, 1, 17, 150, 299):
        assert encs[i] == M.encode(datas[i])
    assert encs == [A.Compress(d) for d in datas]
    full = [(d, e) for d, e in zip(datas, encs) if d]
    assert A.DecompressBatch([e for _, e in full]) == [d for d, _ in full]


def test_batch_with_a_bad_member_is_refused(A):
    from raisin_amd import _lib
    L = _lib.lib()
    c = cases()
    bufs = [c["hello"][1], c["abc"][1], b"\x00\x00\x00", c["len129"][1], b"\x01", c["len64"][1]]
    k = len(bufs)
    ins = (ctypes.c_char_p * k)(*bufs)
    lens = (ctypes.c_size_t * k)(*[len(b) for b in bufs])
    outs = (ctypes.POINTER(ctypes.c_uint8) * k)()
    olens = (ctypes.c_size_t * k)()
    assert L.rsn_arithmetic_decompress_batch(k, ins, lens, outs, olens) == E_FORMAT
    msg = L.rsn_last_error()
    assert msg.startswith(b"member 2: ") and b"no 1 bit" in msg
    assert all(not outs[i] for i in range(k)) and all(olens[i] == 0 for i in range(k))
    assert A.DecompressBatch(bufs[:2]) == [c["hello"][0], c["abc"][0]]


def _fenced(cap, data=None):
    """(device pointer of a 16-byte aligned buffer of cap bytes between two fences, check, read)"""
    import torch
    total = FENCE + (cap + 15) // 16 * 16 + FENCE
    host = torch.randint(0, 256, (total,), dtype=torch.uint8, generator=torch.Generator().manual_seed(cap + 1))
    if data:
        host[FENCE:FENCE + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    whole = host.cuda()
    assert whole.data_ptr() % 16 == 0
    keep = (whole[:FENCE].clone(), whole[FENCE + cap:].clone())
    torch.cuda.synchronize()

    def check():
        torch.cuda.synchronize()
        assert torch.equal(whole[:FENCE], keep[0]) and torch.equal(whole[FENCE + cap:], keep[1]), "a byte outside the buffer changed"

    def read(k):
        return bytes(whole[FENCE:FENCE + k].cpu().numpy())
    return whole.data_ptr() + FENCE, check, read, whole


def _dev(fn, d_in, n, d_out, cap):
    got = ctypes.c_size_t(0)
    rc = fn(d_in, n, d_out, cap, ctypes.byref(got), None)
    return rc, got.value


@pytest.mark.parametrize("name", ["hello", "len16127", "len65537", "greedy400"])
@pytest.mark.parametrize("enc", [True, False], ids=["compress", "decompress"])
def test_dev_calls_between_fences(A, name, enc):
    from raisin_amd import _lib
    L = _lib.lib()
    data, stream = cases()[name]
    src, want = (data, stream) if enc else (stream, data)
    fn = L.rsn_arithmetic_compress_dev if enc else L.rsn_arithmetic_decompress_dev
    d_in, check_in, _, keep_in = _fenced(len(src), src)
    rc, need = _dev(fn, d_in, len(src), None, 0)                      # the size query
    assert rc == E_CAP and need == len(want)
    d_out, check, read, keep_out = _fenced(need)
    rc, got = _dev(fn, d_in, len(src), d_out, need)                   # exact capacity
    assert rc == OK and got == len(want) and read(got) == want
    check()
    d_out, check, read, keep_out = _fenced(need - 1)
    rc, got = _dev(fn, d_in, len(src), d_out, need - 1)               # one byte less
    assert rc == E_CAP and got == need
    check()
    check_in()
    if enc:
        assert need <= L.rsn_arithmetic_compress_bound(len(src))


def test_dev_calls_check_their_arguments(A):
    from raisin_amd import _lib
    L = _lib.lib()
    data, stream = cases()["len129"]
    d_in, _, _, keep = _fenced(256, data)
    for fn in (L.rsn_arithmetic_compress_dev, L.rsn_arithmetic_decompress_dev):
        assert _dev(fn, d_in + 1, 100, d_in + 4096, 64)[0] == E_ARG
        assert _dev(fn, d_in, 100, d_in + 4096 + 4, 64)[0] == E_ARG
        assert _dev(fn, d_in, 128, d_in + 64, 512)[0] == E_ARG


def test_dev_decode_of_hostile_streams_stays_inside(A):
    from raisin_amd import _lib
    L = _lib.lib()
    enc = M.encode(b"a" * 20000)
    for s in (bytes(48), b"\x01\xff", enc[:-40] + bytes(4000)):
        assert _verdict(s) is None
        d_in, _, _, k1 = _fenced(len(s), s)
        d_out, check, _, k2 = _fenced(1000)
        assert _dev(L.rsn_arithmetic_decompress_dev, d_in, len(s), d_out, 1000)[0] == E_FORMAT
        check()


def test_tensor_forms(A):
    import torch
    data, stream = cases()["len16127"]
    src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    c = A.compress_tensor(src)
    assert bytes(c.cpu().numpy()) == stream
    assert bytes(A.decompress_tensor(c).cpu().numpy()) == data
    assert A.compress_bound(len(data)) == 2 * len(data) + 4


def test_calls_do_not_see_each_other_s_scratch(A):
    c = cases()
    a_data, a_enc = c["len65537"]
    b_data, b_enc = c["len129"]
    assert A.Compress(a_data) == a_enc
    assert A.Compress(b_data) == b_enc                                # a small call after a large one ...
    assert A.Decompress(a_enc) == a_data
    assert A.Decompress(b_enc) == b_data
    assert A.Compress(a_data) == a_enc                                # ... and the large one again
    errors = []

    def work(data, enc):
        try:
            for _ in range(4):
                assert A.Compress(data) == enc
                assert A.Decompress(enc) == data
        except Exception as e:                                        # noqa: BLE001
            errors.append(e)
    ts = [threading.Thread(target=work, args=c[n]) for n in ("len16127", "greedy400")]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
