"""CPU tests of the argument checks of every entry point of include/rsn.h that takes buffers: what a bad argument answers (code, a word
of rsn_last_error(), nothing handed out) and how far a good one gets.  The copies of these checks differ in small ways -- whether an
empty input is looked at before a null pointer, whether a null input of length 0 is a call, whether a NULL d_out makes out_cap count
as 0 -- and every difference is pinned here as it is.  Device pointers are integers where nothing can dereference them (a bad argument,
no device); where a device is present the calls that pass the checks get real memory."""
import ctypes

import pytest

U8P = ctypes.POINTER(ctypes.c_uint8)
DATA = b"abcabcabcabc\n"
GARBAGE = 0xDEAD0


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from raisin_amd import _lib
    return _lib


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def _err(L):
    return L.rsn_last_error()


def _host(fn, data, n, *extra, out=True, out_n=True, fill=False):
    """One (in, n, [extra,] out, out_n) call -> (rc, *out as an integer or None, *out_n); fill: both hold garbage before the call."""
    o = ctypes.cast(GARBAGE, U8P) if fill else U8P()
    k = ctypes.c_size_t(5 if fill else 0)
    rc = fn(data, n, *extra, ctypes.byref(o) if out else None, ctypes.byref(k) if out_n else None)
    return rc, ctypes.cast(o, ctypes.c_void_p).value, k.value


def _check_null_arguments(L, fn, *extra, null_in_with_length=True):
    """out == NULL, out_n == NULL, and in == NULL with a length: -1 "null argument", nothing handed out"""
    cases = [dict(out=False), dict(out_n=False)]
    for kw in cases:
        rc, p, k = _host(fn, DATA, len(DATA), *extra, **kw)
        assert rc == -1 and b"null argument" in _err(L) and p is None and k == 0
    if null_in_with_length:
        rc, p, k = _host(fn, None, 7, *extra)
        assert rc == -1 and b"null argument" in _err(L) and p is None and k == 0


def _check_good_call(L, fn, data, n, *extra, fill=True):
    """a call that passes the checks: without a device it fails loudly with everything zeroed; with one it is no argument error"""
    if _has_gpu():
        rc, p, k = _host(fn, data, n, *extra)
        assert rc not in (-1, -2)
        if p:
            L.rsn_free(p)
        return
    rc, p, k = _host(fn, data, n, *extra, fill=fill)
    assert rc == -4 and b"no CPU fallback" in _err(L) and p is None and k == 0


def test_huffman_compress_looks_at_the_length_first(built):
    L = built.lib()
    fn = L.rsn_huffman_compress
    for kw in (dict(), dict(out=False), dict(out_n=False), dict(out=False, out_n=False)):
        for data in (DATA, None):
            rc, p, k = _host(fn, data, 0, **kw)
            assert rc == -2 and b"empty" in _err(L) and p is None and k == 0
    _check_null_arguments(L, fn)


def test_huffman_compress_sharded_looks_at_the_pointers_first(built):
    L = built.lib()
    fn = L.rsn_huffman_compress_sharded
    _check_null_arguments(L, fn, 2)
    for kw in (dict(out=False), dict(out_n=False)):
        rc, p, k = _host(fn, DATA, 0, 2, **kw)
        assert rc == -1 and b"null argument" in _err(L)
    for data in (DATA, None):
        rc, p, k = _host(fn, data, 0, 2, fill=True)
        assert rc == -2 and b"empty" in _err(L) and p is None and k == 0
    _check_good_call(L, fn, DATA, len(DATA), 2)


def test_host_single_calls(built):
    L = built.lib()
    for fn, extra, null_empty_is_a_call in ((L.rsn_huffman_decompress, (), False), (L.rsn_lzss_compress, (4096,), True),
                                            (L.rsn_lzss_decompress, (), True), (L.rsn_arithmetic_compress, (), True),
                                            (L.rsn_arithmetic_decompress, (), True)):
        _check_null_arguments(L, fn, *extra)
        if null_empty_is_a_call:
            _check_good_call(L, fn, None, 0, *extra)
    _check_good_call(L, L.rsn_huffman_compress, DATA, len(DATA), fill=False)   # (its small-input path writes *out only on success)
    _check_good_call(L, L.rsn_lzss_compress, DATA, len(DATA), 4096)
    _check_good_call(L, L.rsn_arithmetic_compress, DATA, len(DATA))


def test_lzss_compress_legacy_is_host_code_with_a_bound(built):
    L = built.lib()
    fn = L.rsn_lzss_compress_legacy
    _check_null_arguments(L, fn, 4096)
    rc, p, k = _host(fn, DATA, len(DATA), 4096, fill=True)
    assert rc == 0 and p and k > 0                                       # no device needed
    L.rsn_free(p)
    rc, p, k = _host(fn, None, 0, 4096, fill=True)
    assert rc == 0 and p and k == 0
    L.rsn_free(p)
    big = bytes((1 << 20) + 1)
    rc, p, k = _host(fn, big, len(big), 0, fill=True)
    assert rc == -6 and b"bound" in _err(L) and p is None and k == 0     # RSN_ERR_LIMIT (rsn.h)


class _DevMem:
    """Device addresses for the calls that pass the argument checks: integers without a device (the call ends at "no device"), real
    memory with one (torch's blocks are 512-byte aligned and zero behind the data)."""

    def __init__(self):
        self.keep = []
        self.gpu = _has_gpu()

    def buf(self, data=b"", fake=4096):
        if not self.gpu:
            return fake
        import torch
        t = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        if data:
            t[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        self.keep.append(t)
        torch.cuda.synchronize()
        return t.data_ptr()


def _dev_calls(L):
    """(fn, extra, a NULL input of length 0 is a call, NULL d_out is the size query, alignment message or None)"""
    return [(L.rsn_huffman_compress_dev, (), False, True, None), (L.rsn_huffman_decompress_dev, (), False, False, None),
            (L.rsn_lzss_compress_dev, (4096,), True, True, None), (L.rsn_lzss_decompress_dev, (), True, False, None),
            (L.rsn_arithmetic_compress_dev, (), True, True, b"arithmetic: device buffers must be 16-byte aligned"),
            (L.rsn_arithmetic_decompress_dev, (), True, True, b"arithmetic: device buffers must be 16-byte aligned")]


def _dev(fn, extra, d_in, n, d_out, cap, got=True):
    k = ctypes.c_size_t(0)
    return fn(d_in, n, *extra, d_out, cap, ctypes.byref(k) if got else None, None)


def test_device_calls_bad_arguments(built):
    L = built.lib()
    for fn, extra, null_empty, _query, align in _dev_calls(L):
        assert _dev(fn, extra, None, 64, 8192, 4096) == -1 and b"null argument" in _err(L)
        assert _dev(fn, extra, 4096, 64, 8192, 4096, got=False) == -1 and b"null argument" in _err(L)
        assert _dev(fn, extra, 4096, 64, 4096 + 32, 64) == -1 and b"overlap" in _err(L)
        assert _dev(fn, extra, 4096 + 32, 64, 4096, 64) == -1 and b"overlap" in _err(L)
        if not null_empty:
            assert _dev(fn, extra, None, 0, 8192, 4096) == -1 and b"null argument" in _err(L)
        if align:
            assert _dev(fn, extra, 4100, 64, 8192, 4096) == -1 and align in _err(L)
            assert _dev(fn, extra, 4096, 64, 8200, 4096) == -1 and align in _err(L)


def test_device_calls_that_pass_the_checks(built):
    L = built.lib()
    mem = _DevMem()

    def passes(rc):
        if mem.gpu:
            assert rc not in (-1, -2)
        else:
            assert rc == -4 and b"no CPU fallback" in _err(L)
    for fn, extra, null_empty, query, align in _dev_calls(L):
        # (with a device only the LZSS calls get the NULL input: they return before a kernel could be handed it)
        if null_empty and not (mem.gpu and align):
            passes(_dev(fn, extra, None, 0, mem.buf(fake=8192), 4096))
        if query:                                                         # d_out NULL: out_cap counts as 0, whatever it says
            data = DATA * 4
            if mem.gpu and fn is L.rsn_arithmetic_decompress_dev:
                data = built.call_host(L.rsn_arithmetic_compress, data)
            passes(_dev(fn, extra, mem.buf(data), len(data), None, 1 << 40))


def _batch(fn, members, lens, *extra, arrays=True, n=None):
    """One (n, ins, lens, [extra,] outs, out_lens) call with outs / out_lens full of garbage -> (rc, outs as integers, out_lens)"""
    k = len(members)
    ins = (ctypes.c_char_p * max(k, 1))(*members)
    ln = (ctypes.c_size_t * max(k, 1))(*lens)
    outs = (U8P * max(k, 1))(*[ctypes.cast(GARBAGE, U8P)] * k)
    olens = (ctypes.c_size_t * max(k, 1))(*[5] * k)
    if not arrays:
        return fn(k if n is None else n, None, None, *extra, None, None), [], []
    rc = fn(k if n is None else n, ins, ln, *extra, outs, olens)
    return rc, [ctypes.cast(outs[i], ctypes.c_void_p).value for i in range(k)], [olens[i] for i in range(k)]


def _nothing_out(outs, olens):
    return all(p is None for p in outs) and all(v == 0 for v in olens)


def test_huffman_compress_batch(built):
    L = built.lib()
    fn = L.rsn_huffman_compress_batch
    rc, _, _ = _batch(fn, [], [], arrays=False)
    assert rc == -1 and b"null argument" in _err(L)                      # n_chunks == 0 does not return before the null check
    rc, _, _ = _batch(fn, [], [], arrays=False, n=2)
    assert rc == -1 and b"null argument" in _err(L)
    rc, outs, olens = _batch(fn, [DATA, None, DATA], [len(DATA), 7, len(DATA)])
    assert rc == -1 and _err(L) == b"null argument" and _nothing_out(outs, olens)
    rc, outs, olens = _batch(fn, [DATA, DATA, DATA], [len(DATA), 0, len(DATA)])
    assert rc == -2 and b"empty" in _err(L) and _nothing_out(outs, olens)
    rc, outs, olens = _batch(fn, [DATA, DATA], [len(DATA), len(DATA)])
    if _has_gpu():
        assert rc not in (-1, -2)
        for p in outs:
            L.rsn_free(p)
    else:
        assert rc == -4 and b"no CPU fallback" in _err(L) and _nothing_out(outs, olens)


def test_the_other_batch_calls(built):
    L = built.lib()
    for fn, extra in ((L.rsn_huffman_decompress_batch, ()), (L.rsn_lzss_compress_batch, (4096,)), (L.rsn_lzss_decompress_batch, ()),
                      (L.rsn_arithmetic_compress_batch, ()), (L.rsn_arithmetic_decompress_batch, ())):
        rc, _, _ = _batch(fn, [], [], *extra, arrays=False)
        assert rc == 0                                                    # n == 0 returns before the null check
        rc, _, _ = _batch(fn, [], [], *extra, arrays=False, n=2)
        assert rc == -1 and b"null argument" in _err(L)
        rc, outs, olens = _batch(fn, [DATA, DATA, None], [len(DATA), len(DATA), 7], *extra)
        assert rc == -1 and _err(L) == b"member 2: null argument" and _nothing_out(outs, olens)
    for fn, extra in ((L.rsn_lzss_compress_batch, (4096,)), (L.rsn_arithmetic_compress_batch, ())):
        rc, outs, olens = _batch(fn, [DATA, DATA], [len(DATA), len(DATA)], *extra)
        if _has_gpu():
            assert rc not in (-1, -2)
            for p in outs:
                L.rsn_free(p)
        else:
            assert rc == -4 and b"no CPU fallback" in _err(L) and _nothing_out(outs, olens)
