"""rsn_huffman_compress_bound / rsn_lzss_compress_bound against what the codecs can produce at most: plain arithmetic, no device.

lz.compress_tensor and every caller of the *_dev compress calls size their buffers by these two functions, so a bound below the
oracle's output on some input is an RSN_ERR_CAPACITY nobody expects.  The inputs are the ones that stretch the formats:
  LZSS     5C and FF double (lzss.go:373-379), '<' maps to one byte, a token is only written where it is shorter than its bytes;
  Huffman  every distinct rune costs a header entry (count, '|', the rune's bytes), a rune used once costs its entry and a long
           code, counts of many digits widen the entries, invalid bytes become U+FFFD (three bytes in the header, one symbol)."""
import random

import pytest

SIZES = (0, 1, 15, 16, 17, 4096, 65537)


@pytest.fixture(scope="module")
def L():
    from raisin_amd import _lib
    return _lib.lib()


def _lzss_inputs(n):
    rng = random.Random(n)
    yield "all backslashes", b"\\" * n
    yield "random over 5C FF", bytes(rng.choice(b"\\\xff") for _ in range(n))
    yield "random over 5C FF 3C", bytes(rng.choice(b"\\\xff<") for _ in range(n))
    yield "alternating 5C 3C", (b"\\<" * (n // 2 + 1))[:n]


@pytest.mark.parametrize("n", SIZES)
def test_lzss_bound_covers_the_oracle(L, oracle, n):
    bound = L.rsn_lzss_compress_bound(n)
    for name, data in _lzss_inputs(n):
        assert len(data) == n
        for w in (4096, 1000):
            out = oracle.lzss_compress(data, w)
            assert len(out) <= bound, (name, n, w, len(out), bound)
    assert len(oracle.lzss_escape(b"\\" * n)) <= bound                    # what the stream is before any token shortens it


def _distinct_runes(n, order):
    """n bytes in which every rune is a new one for as long as the code space lasts.  order "wide": 4-byte runes, then 3-byte ones;
    "dense": 1-, 2-, 3-, then 4-byte runes -- the most header bytes per input byte first.  What is left over is filled with 'a'."""
    four = range(0x10000, 0x110000)
    three = (r for r in range(0x800, 0x10000) if not 0xD800 <= r < 0xE000 and r != 0xFFFD)
    groups = [four, three] if order == "wide" else [range(1, 0x80), range(0x80, 0x800), three, four]
    out = bytearray()
    for g in groups:
        for r in g:
            b = chr(r).encode("utf-8")
            if len(out) + len(b) > n:
                break
            out += b
    out += b"a" * (n - len(out))
    return bytes(out)


def _huffman_inputs(n):
    rng = random.Random(n)
    yield "distinct runes, wide first", _distinct_runes(n, "wide")
    yield "distinct runes, dense first", _distinct_runes(n, "dense")
    yield "counts of many digits", (b"a" * (n - min(n, 40)) + bytes(rng.choice(b"bcdefghij") for _ in range(min(n, 40))))
    yield "many digits, rune alphabet", ("\U0001F600".encode() * (n // 4) + "é€x".encode())[:n]
    yield "all invalid bytes", bytes(rng.choice(b"\x80\xbf\xc0\xc1\xf5\xff\xfe") for _ in range(n))
    yield "a single symbol", b"a" * n


@pytest.mark.parametrize("n", SIZES[1:] + (1 << 20,))
def test_huffman_bound_covers_the_oracle(L, oracle, n):
    bound = L.rsn_huffman_compress_bound(n)
    for name, data in _huffman_inputs(n):
        assert len(data) == n, name
        out = oracle.huffman_compress(data)
        assert len(out) <= bound, (name, n, len(out), bound)
    if n == 1 << 20:
        counts = oracle.header_entries(oracle.huffman_compress(b"a" * (n - 40) + b"b" * 40))[0]
        assert max(len(f) for f, _ in counts) >= 7                         # the case's point: a count of seven digits


def test_huffman_of_nothing_has_no_stream_to_bound(L, oracle):
    with pytest.raises(oracle.OracleError):
        oracle.huffman_compress(b"")
    assert L.rsn_huffman_compress_bound(0) <= L.rsn_huffman_compress_bound(1)


def test_the_rune_heavy_mebibyte_outgrows_the_host_calls_first_buffer(oracle):
    """The input test_gpu_dev_fences.py sends through rsn_huffman_compress to reach host_call's retry on RSN_ERR_CAPACITY: the host
    calls first allocate n + n / 8 + 64 KiB, and a quarter of a million runes used once each need more than that."""
    n = 1 << 20
    data = _distinct_runes(n, "wide")
    assert len(oracle.huffman_compress(data)) > n + n // 8 + 65536


def test_bounds_are_monotone(L):
    for fn in (L.rsn_huffman_compress_bound, L.rsn_lzss_compress_bound):
        prev = fn(0)
        for n in range(1, 70001):
            cur = fn(n)
            assert cur >= prev, (fn.__name__, n)
            prev = cur
        assert fn(1 << 32) >= fn((1 << 32) - 1) >= prev
