"""CPU tests of the arithmetic codec: the checker (tests/arith_model.py) against the sizes the reference published, the bound, and
the new entry points' behaviour on a machine without a device."""
import ctypes
import os
import random
import re
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import arith_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rsn_arithmetic_compress_bound", "rsn_arithmetic_compress", "rsn_arithmetic_decompress", "rsn_arithmetic_compress_batch",
       "rsn_arithmetic_decompress_batch", "rsn_arithmetic_compress_dev", "rsn_arithmetic_decompress_dev"]
ALPHABET = (b"abcdefghijklmnopqrstuvwxyz" * 3847)[:100000]

# (input, bytes of the stream): the reference's README.md:154,166 and ai/data.json
PUBLISHED = [(b"Hello world!\n", 14), (b"abc" * 8 + b"\n", 21), (b"a", 3), (b"a" * 100000, 477), (ALPHABET, 59191)]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from raisin_amd import _lib
    return _lib


@pytest.mark.parametrize("k", range(len(PUBLISHED)))
def test_model_reproduces_the_published_sizes(k):
    data, size = PUBLISHED[k]
    enc = M.encode(data)
    assert len(enc) == size
    assert M.decode(enc) == data


def test_model_known_streams():
    assert M.encode(b"Hello world!\n").hex() == "1481d3b709d73fd1fb4b442b0cd7"
    assert M.encode(b"a").hex() == "01619d"
    assert M.encode(b"") == b"\x01\xff"


def test_model_reproduces_pi_txt():
    pytest.importorskip("mpmath")
    import make_pi
    pi = make_pi.pi_digits()
    enc = M.encode(pi)
    assert len(enc) == 418224                       # ai/data.json: 41.8224 % of 1 000 000
    assert M.decode(enc) == pi


def test_model_refuses_what_the_reference_panics_on():
    for s in (b"", b"\x00", b"\x00\x00\x00", b"\x01", b"\x01\xff", b"\x20\xff"):   # (the last: 13 bits behind the 1)
        with pytest.raises(M.FormatError):
            M.decode(s)
    # 14 bits behind the first 1 are enough to start: the verdict is then the decoder's own
    try:
        M.decode(b"\x40\x00")
    except M.FormatError as e:
        assert "16 bits" not in str(e)
    with pytest.raises(M.FormatError) as e:
        M.decode(b"\x20\xff")
    assert "16 bits" in str(e.value)


def test_model_tail_rule():
    """a frozen, one-symbol table and a stream of zeros never reach the end symbol: the tail rule ends it"""
    enc = M.encode(b"a" * 20000)
    with pytest.raises(M.FormatError) as e:
        M.decode(enc[:-40] + bytes(40))
    assert "end symbol" in str(e.value)
    assert M.decode(enc) == b"a" * 20000


def _inputs():
    rng = random.Random(0xA217)
    out = []
    for n in (1, 2, 3, 17, 255, 256, 257, 1000, 4097, 16125, 16126, 16127, 40000):
        out.append(bytes(rng.randrange(256) for _ in range(n)))
        out.append(bytes(rng.choice(b"ab") for _ in range(n)))
        out.append(bytes(rng.choice(b"aaaaaaaaaaaaaaaabbbc\x00\xff") for _ in range(n)))
    return out


def test_model_round_trips():
    for data in _inputs():
        enc = M.encode(data)
        assert M.decode(enc) == data
        assert len(enc) <= 2 * len(data) + 4


def test_greedy_input_piles_up_pending_bits():
    g = M.greedy_input(400)
    st = M.stats(g)
    assert st["max_pending"] >= 512
    assert [M.stats(g[:k])["max_pending"] for k in (40, 100, 200)] == [148, 598, 903]   # (the GPU suite's cases lean on these)
    assert M.decode(M.encode(g)) == g


@pytest.mark.parametrize("data", [b"a" * 16126 + bytes(range(256)) * 40, bytes(range(256)) * 64], ids=["frozen-then-all", "all-bytes"])
def test_bound_holds(data):
    assert len(M.encode(data)) <= 2 * len(data) + 4


def test_compress_bound_is_the_formula(built):
    L = built.lib()
    for n in (0, 1, 13, 4096, 1 << 20, (1 << 32) + 5):
        assert L.rsn_arithmetic_compress_bound(n) == 2 * n + 4


def test_new_symbols_are_declared_exported_and_bound(built):
    import subprocess
    hdr = open(os.path.join(ROOT, "include", "rsn.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rsn_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "raisin_amd", "librsn.so")], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW:
        assert name in declared and name in exported and name in built.SYMBOLS, name
    from raisin_amd import arithmetic
    assert arithmetic.SLICE_SYMBOLS == int(re.search(r"ARITH_SLICE_SYMBOLS\s*=\s*(\d+)", open(os.path.join(ROOT, "raisin_amd", "csrc", "codecs.h")).read()).group(1))
    assert arithmetic.TAIL_BITS == M.TAIL_BITS == int(re.search(r"#define RSN_ARITH_TAIL_BITS\s+(\d+)", open(os.path.join(ROOT, "include", "rsn.h")).read()).group(1))


def _batch_args(bufs):
    k = len(bufs)
    ins = (ctypes.c_char_p * k)(*bufs)
    lens = (ctypes.c_size_t * k)(*[len(b) for b in bufs])
    outs = (ctypes.POINTER(ctypes.c_uint8) * k)()
    olens = (ctypes.c_size_t * k)()
    return k, ins, lens, outs, olens


def test_arguments_are_checked_before_any_device(built):
    L = built.lib()
    k, ins, lens, outs, olens = _batch_args([b"abc", b"", b"xyz"])
    out, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t(0)
    for fn in (L.rsn_arithmetic_compress_batch, L.rsn_arithmetic_decompress_batch):
        assert fn(k, None, lens, outs, olens) == -1
        assert fn(k, ins, None, outs, olens) == -1
        assert fn(k, ins, lens, None, olens) == -1
        assert fn(k, ins, lens, outs, None) == -1
        ins[1] = None
        lens[1] = 5
        assert fn(k, ins, lens, outs, olens) == -1 and b"member 1" in L.rsn_last_error()
        assert all(not outs[i] for i in range(k))
        lens[1] = 0
        assert fn(0, None, None, None, None) == 0
    for fn in (L.rsn_arithmetic_compress, L.rsn_arithmetic_decompress):
        assert fn(None, 3, ctypes.byref(out), ctypes.byref(n)) == -1
        assert fn(b"abc", 3, None, ctypes.byref(n)) == -1
    for fn in (L.rsn_arithmetic_compress_dev, L.rsn_arithmetic_decompress_dev):
        assert fn(None, 16, None, 0, ctypes.byref(n), None) == -1
        assert fn(4096, 16, 8192, 64, None, None) == -1
        assert fn(4096 + 1, 16, 8192, 64, ctypes.byref(n), None) == -1 and b"aligned" in L.rsn_last_error()
        assert fn(4096, 16, 8192 + 8, 64, ctypes.byref(n), None) == -1 and b"aligned" in L.rsn_last_error()
        assert fn(4096, 64, 4096 + 32, 64, ctypes.byref(n), None) == -1 and b"overlap" in L.rsn_last_error()


def test_no_device_no_fallback(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = built.lib()
    from raisin_amd import RsnError, arithmetic
    for fn in (lambda: arithmetic.Compress(b"abc"), lambda: arithmetic.Decompress(M.encode(b"abc")), lambda: arithmetic.Compress(b""),
               lambda: arithmetic.CompressBatch([b"abc", b"d"]), lambda: arithmetic.DecompressBatch([M.encode(b"abc")])):
        with pytest.raises(RsnError) as e:
            fn()
        assert e.value.code == -4 and "no CPU fallback" in str(e.value)
    k, ins, lens, outs, olens = _batch_args([b"abc", b"", b"xyz"])
    assert L.rsn_arithmetic_compress_batch(k, ins, lens, outs, olens) == -4
    assert all(not outs[i] for i in range(k))
    n = ctypes.c_size_t(0)
    for fn in (L.rsn_arithmetic_compress_dev, L.rsn_arithmetic_decompress_dev):
        assert fn(4096, 16, 8192, 64, ctypes.byref(n), None) == -4 and b"no CPU fallback" in L.rsn_last_error()
